"""Recipe of tests/golden/tiny_qwen2.npz, tiny_qwen3.npz and tiny_qwen3_dh64.npz: HF `Qwen2Model` / `Qwen3Model` (transformers, CPU, fp32,
eager attention) on tiny random configs -- the reference forward of the Qwen members of the Llama family (SGPT_ARCH_LLAMA), as
make_golden_llama.py records HF LlamaModel / MistralModel.

    python tests/golden/make_golden_qwen.py          (needs torch + transformers; writes next to itself)

Weights: sgpt_amd.model.synthetic_qwen_weights(cfg, seed, qkv_bias, qk_norm) -- seeded numpy, under HF state-dict names -- loaded into
the HF module with load_state_dict(strict=True).  The file records cfg + seed and a sha256 over the tensors' bytes instead of the
weights (a committed file stays under 1 MiB), so a change of the generator stream fails the reader loudly.

Cases -- the smallest that reach every branch the two models add:
  tiny_qwen2        Qwen2Model  d 128, heads 2 / 1, head_dim 64,  ffn 256, 2 layers   the q / k / v bias (V's through the V^T epilogue)
  tiny_qwen3        Qwen3Model  d 128, heads 2 / 1, head_dim 128, ffn 256, 2 layers   q / k norm; query width 256 > d
  tiny_qwen3_dh64   Qwen3Model  d 256, heads 2 / 2, head_dim 64,  ffn 384, 2 layers   q / k norm on a half-wave head; query width 128 < d
Inputs and recorded values as make_golden_llama.py: five sequences of 1, 7, 64, 70 and 130 seeded ids, one HF call per sequence,
max_position_embeddings 160; ids (flat) + seq_lens, all L + 1 hidden states per token and the mean / weightedmean / lasttoken pooled
vectors of the last hidden state."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)

from make_golden_llama import LENS, weights_digest  # noqa: E402


def _cfg(model_type, d, H, kv, ffn, **kw):
    return dict(model_type=model_type, vocab_size=200, hidden_size=d, num_hidden_layers=2, num_attention_heads=H, num_key_value_heads=kv,
                intermediate_size=ffn, max_position_embeddings=160, rms_norm_eps=1e-6, rope_theta=10000.0, hidden_act="silu",
                use_sliding_window=False, **kw)


FIXTURES = {
    "tiny_qwen2": dict(cfg=_cfg("qwen2", 128, 2, 1, 256), seed=31, qkv_bias=True, qk_norm=False),
    "tiny_qwen3": dict(cfg=_cfg("qwen3", 128, 2, 1, 256, head_dim=128, attention_bias=False), seed=32, qkv_bias=False, qk_norm=True),
    "tiny_qwen3_dh64": dict(cfg=_cfg("qwen3", 256, 2, 2, 384, head_dim=64, attention_bias=False), seed=33, qkv_bias=False, qk_norm=True),
}


def main():
    import torch
    from transformers import Qwen2Config, Qwen2Model, Qwen3Config, Qwen3Model
    from sgpt_amd.model import SGPTConfig, synthetic_qwen_weights
    for name, fx in FIXTURES.items():
        hf = dict(fx["cfg"])
        cfg = SGPTConfig.from_hf_dict(hf)
        w = synthetic_qwen_weights(cfg, seed=fx["seed"], qkv_bias=fx["qkv_bias"], qk_norm=fx["qk_norm"])
        q3 = hf["model_type"] == "qwen3"
        kw = {k: v for k, v in hf.items() if k != "model_type"}
        conf = (Qwen3Config if q3 else Qwen2Config)(**kw, attention_dropout=0.0, attn_implementation="eager")
        model = (Qwen3Model if q3 else Qwen2Model)(conf).eval()
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
        np.savez_compressed(os.path.join(HERE, name + ".npz"), cfg=json.dumps(hf), seed=fx["seed"], qkv_bias=fx["qkv_bias"],
                            qk_norm=fx["qk_norm"], weights_sha256=weights_digest(w), seq_lens=np.asarray(LENS, np.int64),
                            ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
                            hidden=np.concatenate(hidden, axis=1).astype(np.float32),
                            **{f"emb_{m}": np.stack(v).astype(np.float32) for m, v in pooled.items()})
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
