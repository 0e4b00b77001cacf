"""Recipe of tests/golden/tiny_*_long*.npz: HF `LlamaModel` / `MistralModel` / `Qwen3Model` (transformers, CPU, fp32, eager attention) on
sequences LONGER than 2048 tokens -- the reference values of tests/test_long_ref.py and tests/test_gpu_long_sequences.py, as
make_golden_llama.py / make_golden_qwen.py record the short ones.

    python tests/golden/make_golden_long.py          (needs torch + transformers; writes next to itself)

Weights: sgpt_amd.model.synthetic_llama_weights / synthetic_qwen_weights(cfg, seed), loaded with load_state_dict(strict=True); the file
records cfg + seed and a sha256 over the tensors' bytes instead of the weights.

Cases (max_position_embeddings 4352 everywhere):
  tiny_llama_long           d 128, heads 2 / 1, head_dim 64,  ffn 256, 2 layers         sequences of 2049, 4100 and 7 tokens
  tiny_llama_long_dh128     d 256, heads 2 / 2, head_dim 128, ffn 384, 2 layers         2049, 4100, 7
  tiny_mistral_long_window  tiny_llama_long's shape with sliding_window 100             2049, 4100, 7
  tiny_qwen3_long           make_golden_qwen.py's tiny_qwen3 (head_dim 128, q / k norm)   2049, 7
2049 is the first length past the old limit of 2048 tokens; 4100 spans two full 2048-key chunks of the fp32 attention plus a 4-key
tail; the 7-token sequence is a short one riding in a long call.  One HF call per sequence (no padding, no mask arithmetic).
Recorded: ids (flat) + seq_lens, the mean / weightedmean / lasttoken pooled vectors of the last hidden state of every sequence, and
all L + 1 hidden states ONLY at the token rows {0, 2047, 2048, last} of each sequence longer than 2048 tokens (`hidden_rows`: the flat
row numbers in `ids`; `hidden` [L + 1, len(hidden_rows), d]) -- every row of a 4100-token sequence would be 6 MB, and a committed file
stays under 1 MiB."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)

from make_golden_llama import _cfg as _llama_cfg, weights_digest  # noqa: E402
from make_golden_qwen import _cfg as _qwen_cfg  # noqa: E402

MAX_POS = 4352
LENS = [2049, 4100, 7]


def _long(cfg):
    return dict(cfg, max_position_embeddings=MAX_POS)


FIXTURES = {
    "tiny_llama_long": dict(cfg=_long(_llama_cfg("llama", 128, 2, 1, 256)), seed=41, lens=LENS),
    "tiny_llama_long_dh128": dict(cfg=_long(_llama_cfg("llama", 256, 2, 2, 384)), seed=42, lens=LENS),
    "tiny_mistral_long_window": dict(cfg=_long(_llama_cfg("mistral", 128, 2, 1, 256, sliding_window=100)), seed=43, lens=LENS),
    "tiny_qwen3_long": dict(cfg=_long(_qwen_cfg("qwen3", 128, 2, 1, 256, head_dim=128, attention_bias=False)), seed=44, lens=[2049, 7],
                            qk_norm=True),
}


def hidden_rows(lens):
    """Flat row numbers of the recorded hidden states: rows 0, 2047, 2048 and the last of every sequence longer than 2048 tokens."""
    rows, start = [], 0
    for n in lens:
        if n > 2048:
            rows += [start + r for r in (0, 2047, 2048, n - 1)]
        start += n
    return sorted(set(rows))


def main():
    import torch
    from transformers import LlamaConfig, LlamaModel, MistralConfig, MistralModel, Qwen3Config, Qwen3Model
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights, synthetic_qwen_weights
    for name, fx in FIXTURES.items():
        hf, lens = dict(fx["cfg"]), fx["lens"]
        cfg = SGPTConfig.from_hf_dict(hf)
        mt = hf["model_type"]
        if mt == "qwen3":
            w = synthetic_qwen_weights(cfg, seed=fx["seed"], qkv_bias=False, qk_norm=True)
        else:
            w = synthetic_llama_weights(cfg, seed=fx["seed"])
        drop = {"model_type"} | ({"mlp_bias", "attention_bias"} if mt == "mistral" else set())     # (MistralConfig has no bias switches)
        kw = {k: v for k, v in hf.items() if k not in drop}
        Conf, Model = {"llama": (LlamaConfig, LlamaModel), "mistral": (MistralConfig, MistralModel), "qwen3": (Qwen3Config, Qwen3Model)}[mt]
        model = Model(Conf(**kw, attention_dropout=0.0, attn_implementation="eager")).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        rng = np.random.default_rng(fx["seed"] + 1000)
        seqs = [rng.integers(3, hf["vocab_size"], size=n).tolist() for n in lens]
        keep = hidden_rows(lens)
        hidden, pooled, start = [], {"mean": [], "weightedmean": [], "lasttoken": []}, 0
        with torch.no_grad():
            for s in seqs:
                out = model(input_ids=torch.tensor([s]), output_hidden_states=True)
                hs = torch.stack(out.hidden_states)[:, 0]            # [L + 1, len, d]
                assert torch.equal(hs[-1], out.last_hidden_state[0])
                local = [r - start for r in keep if start <= r < start + len(s)]
                if local:
                    hidden.append(hs[:, local].numpy())
                last = hs[-1].double()
                wgt = torch.arange(1, len(s) + 1, dtype=torch.float64)
                pooled["mean"].append(last.mean(0).numpy())
                pooled["weightedmean"].append(((last * wgt[:, None]).sum(0) / wgt.sum()).numpy())
                pooled["lasttoken"].append(last[-1].numpy())
                start += len(s)
        extra = {"qkv_bias": False, "qk_norm": True} if mt == "qwen3" else {}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), cfg=json.dumps(hf), seed=fx["seed"], weights_sha256=weights_digest(w),
                            seq_lens=np.asarray(lens, np.int64), ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
                            hidden_rows=np.asarray(keep, np.int64), hidden=np.concatenate(hidden, axis=1).astype(np.float32),
                            **extra, **{f"emb_{m}": np.stack(v).astype(np.float32) for m, v in pooled.items()})
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
