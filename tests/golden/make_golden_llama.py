"""Recipe of tests/golden/tiny_llama*.npz and tiny_mistral_window.npz: HF `LlamaModel` / `MistralModel` (transformers, CPU, fp32, eager
attention) on tiny random configs -- the reference forward of the Llama family (SGPT_ARCH_LLAMA), as make_golden_bert.py records
HF BertModel.

    python tests/golden/make_golden_llama.py          (needs torch + transformers; writes next to itself)

Weights: sgpt_amd.model.synthetic_llama_weights(cfg, seed) -- seeded numpy, under HF LlamaModel state-dict names -- loaded into the HF
module with load_state_dict(strict=True).  The file records cfg + seed and a sha256 over the tensors' bytes instead of the weights
(a committed file stays under 1 MiB), so a change of the generator stream fails the reader loudly.

Cases -- the smallest that reach every branch (grouped K / V with one, two and four query heads per key head, head_dim 64 and 128,
ffn != 4 d and no multiple of 256, the sliding window):
  tiny_llama           d 128, heads 2 / 1, head_dim 64,  ffn 256, 2 layers
  tiny_llama_dh128     d 256, heads 2 / 2, head_dim 128, ffn 384, 2 layers
  tiny_llama_g4        d 256, heads 4 / 1, head_dim 64,  ffn 384, 2 layers
  tiny_mistral_window  d 128, heads 2 / 1, head_dim 64,  ffn 256, 2 layers, sliding_window 16 (MistralModel)
Inputs: five sequences of 1, 7, 64, 70 and 130 seeded ids (a single token, odd, exactly one 64-key tile, across a tile, above the
128-row threshold of the attention kernel), one HF call per sequence (no padding, no mask arithmetic in the reference values);
max_position_embeddings 160.
Recorded: ids (flat) + seq_lens, all L + 1 hidden states per token (flat rows, HF numbering: entry i = input of layer i, entry L =
the final RMSNorm's output) and the mean / weightedmean / lasttoken pooled vectors of the last hidden state."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

LENS = [1, 7, 64, 70, 130]


def _cfg(model_type, d, H, kv, ffn, **kw):
    return dict(model_type=model_type, vocab_size=200, hidden_size=d, num_hidden_layers=2, num_attention_heads=H, num_key_value_heads=kv,
                intermediate_size=ffn, max_position_embeddings=160, rms_norm_eps=1e-5, rope_theta=10000.0, hidden_act="silu",
                attention_bias=False, mlp_bias=False, **kw)


FIXTURES = {
    "tiny_llama": dict(cfg=_cfg("llama", 128, 2, 1, 256), seed=21),
    "tiny_llama_dh128": dict(cfg=_cfg("llama", 256, 2, 2, 384), seed=22),
    "tiny_llama_g4": dict(cfg=_cfg("llama", 256, 4, 1, 384), seed=23),
    "tiny_mistral_window": dict(cfg=_cfg("mistral", 128, 2, 1, 256, sliding_window=16), seed=24),
}


def weights_digest(w) -> str:
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def main():
    import torch
    from transformers import LlamaConfig, LlamaModel, MistralConfig, MistralModel
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights
    for name, fx in FIXTURES.items():
        hf = dict(fx["cfg"])
        cfg = SGPTConfig.from_hf_dict(hf)
        w = synthetic_llama_weights(cfg, seed=fx["seed"])
        mistral = hf["model_type"] == "mistral"
        drop = {"model_type"} | ({"mlp_bias", "attention_bias"} if mistral else set())     # (MistralConfig has no bias switches)
        kw = {k: v for k, v in hf.items() if k not in drop}
        conf = (MistralConfig if mistral else LlamaConfig)(**kw, attention_dropout=0.0, attn_implementation="eager")
        model = (MistralModel if mistral else LlamaModel)(conf).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        rng = np.random.default_rng(fx["seed"] + 1000)
        seqs = [rng.integers(3, hf["vocab_size"], size=n).tolist() for n in LENS]
        hidden, pooled = [], {"mean": [], "weightedmean": [], "lasttoken": []}
        with torch.no_grad():
            for s in seqs:
                out = model(input_ids=torch.tensor([s]), output_hidden_states=True)
                hs = torch.stack(out.hidden_states)[:, 0]            # [L + 1, len, d]
                assert torch.equal(hs[-1], out.last_hidden_state[0])
                hidden.append(hs.numpy())
                last = hs[-1].double()
                wgt = torch.arange(1, len(s) + 1, dtype=torch.float64)
                pooled["mean"].append(last.mean(0).numpy())
                pooled["weightedmean"].append(((last * wgt[:, None]).sum(0) / wgt.sum()).numpy())
                pooled["lasttoken"].append(last[-1].numpy())
        np.savez_compressed(os.path.join(HERE, name + ".npz"), cfg=json.dumps(hf), seed=fx["seed"], weights_sha256=weights_digest(w),
                            seq_lens=np.asarray(LENS, np.int64), ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
                            hidden=np.concatenate(hidden, axis=1).astype(np.float32),
                            **{f"emb_{m}": np.stack(v).astype(np.float32) for m, v in pooled.items()})
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
