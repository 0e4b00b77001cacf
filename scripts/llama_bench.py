"""Encode rate of the Llama / Mistral block at Mistral-7B shape (32 layers, d 4096, 32 query / 8 key-value heads of 128, ffn 14336) in
bf16, and what the UNFUSED SwiGLU costs: the fc1 launch (N = 2 ffn, plain store) with and without the row kernel behind it.

    python scripts/llama_bench.py [--docs 256] [--seq 128] [--iters 5]

Timing as scripts/bert_bench.py: warm-up calls, then `iters` back-to-back sgpt_encode calls between two events on one stream, one
synchronisation at the end; mean pooling.  Random-init weights: ONE layer's tensors (sgpt_amd.model.synthetic_llama_weights at one
layer) are handed to all 32 layers -- the rate does not depend on the values, and 7 G random floats take minutes to draw.
roofline_share = projection FLOPs / time / 2.5 PFLOP/s (the dense 16-bit MFMA peak): per token and layer
2 (d (d + 2 d_kv) + d d + 3 d ffn) -- the grouped K / V widths and the three MLP matrices; the attention's own FLOPs are not counted.
Prints one JSON line for the model and one for the MLP pieces."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sgpt_amd import SGPTConfig, SGPTModel, get_context  # noqa: E402
from sgpt_amd.model import synthetic_llama_weights  # noqa: E402

PEAK_16BIT_TFLOPS = 2500.0


def timed(fn, iters):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=256)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    hf = dict(model_type="mistral", vocab_size=32000, hidden_size=4096, num_hidden_layers=a.layers, num_attention_heads=32,
              num_key_value_heads=8, intermediate_size=14336, max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=10000.0,
              sliding_window=None, hidden_act="silu")
    cfg = SGPTConfig.from_hf_dict(hf)
    one = synthetic_llama_weights(SGPTConfig.from_hf_dict(dict(hf, num_hidden_layers=1)), 0)
    w = {k: v for k, v in one.items() if not k.startswith("layers.")}
    for i in range(cfg.num_layers):
        w.update({k.replace("layers.0.", f"layers.{i}."): v for k, v in one.items() if k.startswith("layers.0.")})
    m = SGPTModel(cfg, w, device="cuda:0", dtype="bf16")
    del w, one
    rng = np.random.default_rng(0)
    seqs = rng.integers(3, 32000, size=(a.docs, a.seq)).tolist()
    pb = m.pack(seqs)
    out = torch.empty((pb.B, cfg.hidden_size), dtype=torch.float32, device=m.device)
    ms = timed(lambda: m.encode_packed(pb, mode="mean", normalize=True, out=out), a.iters)
    assert torch.isfinite(out).all()
    d, ffn, dkv = cfg.hidden_size, cfg.intermediate_size, cfg.num_kv_heads * (cfg.hidden_size // cfg.num_heads)
    flops = 2.0 * (d * (d + 2 * dkv) + d * d + 3 * d * ffn) * cfg.num_layers * pb.T_pad
    print(json.dumps(dict(model="mistral-7b-shape", layers=cfg.num_layers, docs=a.docs, seq=a.seq, dtype="bf16", token_rows=pb.T_pad,
                          ms_per_call=round(ms, 2), sentences_per_s=round(a.docs / ms * 1e3, 1),
                          projection_tflops=round(flops / ms / 1e9, 1),
                          roofline_share=round(flops / ms / 1e9 / PEAK_16BIT_TFLOPS, 4))), flush=True)
    m.close()
    # the MLP's first half alone, at the same token rows: fc1 (store epilogue) and fc1 + the SwiGLU row kernel
    ctx = get_context("cuda:0")
    T = pb.T_pad
    x = (torch.randn((T, d), device="cuda:0") * 0.5).to(torch.bfloat16)
    wgu = (torch.randn((2 * ffn, d), device="cuda:0") * 0.02).to(torch.bfloat16)
    fc1 = timed(lambda: ctx.linear(x, wgu, None, epi="store"), 10)
    both = timed(lambda: ctx.swiglu(ctx.linear(x, wgu, None, epi="store")), 10)
    gu = ctx.linear(x, wgu, None, epi="store")
    row = timed(lambda: ctx.swiglu(gu), 10)
    print(json.dumps(dict(piece="mlp-first-half", token_rows=T, fc1_ms=round(fc1, 3), fc1_plus_swiglu_ms=round(both, 3),
                          swiglu_alone_ms=round(row, 3), swiglu_gbytes_per_s=round(T * ffn * 2 * 3 / row / 1e6, 1))), flush=True)


if __name__ == "__main__":
    main()
