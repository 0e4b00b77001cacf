"""Encode time of a Llama-family decoder with causal and with bidirectional attention (SGPTModel.set_attention), same model, same
batch, one process: what the non-causal attention launch costs next to the causal one at a shape a user would run.

    python scripts/bidir_bench.py [--layers 4] [--docs 64] [--seq 512] [--iters 20] [--windows 5]

Shape: `--layers` blocks of Mistral-7B (d 4096, 32 query heads on 8 key / value heads, head_dim 128, ffn 14336), bf16, random-init weights
(sgpt_amd.model.synthetic_llama_weights), `--docs` sequences of `--seq` tokens, mean pooling.
Timing as scripts/bert_bench.py: 3 warm-up calls, then `--iters` back-to-back sgpt_encode calls between two events on one stream, one
synchronisation at the end = one window.  The two modes ALTERNATE, `--windows` windows each, so that drift of the box lands on both;
per mode: every window's ms per call, their median and their spread (max - min) / median.  The attention's share is the difference of
the two medians (nothing else differs between the modes).  Prints one JSON line per mode and one for the difference."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sgpt_amd import SGPTConfig, SGPTModel  # noqa: E402
from sgpt_amd.model import synthetic_llama_weights  # noqa: E402


def window(m, pb, out, iters):
    for _ in range(3):
        m.encode_packed(pb, mode="mean", normalize=True, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        m.encode_packed(pb, mode="mean", normalize=True, out=out)
    e1.record()
    e1.synchronize()
    assert torch.isfinite(out).all()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--docs", type=int, default=64)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    cfg = SGPTConfig.from_hf_dict(dict(model_type="mistral", vocab_size=4096, hidden_size=4096, num_hidden_layers=a.layers,
                                       num_attention_heads=32, num_key_value_heads=8, intermediate_size=14336,
                                       max_position_embeddings=32768, sliding_window=None, rms_norm_eps=1e-5, rope_theta=10000.0))
    m = SGPTModel(cfg, synthetic_llama_weights(cfg, 0), device="cuda:0", dtype="bf16")
    rng = np.random.default_rng(0)
    pb = m.pack(rng.integers(3, cfg.vocab_size, size=(a.docs, a.seq)).tolist())
    out = torch.empty((pb.B, cfg.hidden_size), dtype=torch.float32, device=m.device)
    ms = {"causal": [], "bidirectional": []}
    for _ in range(a.windows):
        for mode in ms:
            m.set_attention(mode)
            ms[mode].append(window(m, pb, out, a.iters))
    shape = dict(layers=a.layers, d=4096, heads="32/8", ffn=14336, dtype="bf16", docs=a.docs, seq=a.seq, token_rows=pb.T_pad, iters=a.iters)
    med = {}
    for mode, v in ms.items():
        med[mode] = statistics.median(v)
        print(json.dumps(dict(attention=mode, **shape, ms_per_call=[round(x, 3) for x in v], median_ms=round(med[mode], 3),
                              spread=round((max(v) - min(v)) / med[mode], 4))), flush=True)
    diff = med["bidirectional"] - med["causal"]
    print(json.dumps(dict(bidirectional_minus_causal_ms=round(diff, 3), per_layer_ms=round(diff / max(a.layers, 1), 3),
                          relative=round(diff / med["causal"], 4))), flush=True)
    m.close()


if __name__ == "__main__":
    main()
