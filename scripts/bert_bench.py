"""Encode rate of the BERT block at bert-base shape (12 layers, d 768, 12 heads, ffn 3072, sequences of 128 tokens) next to the
SGPT-125M block on the same box -- the two share every GEMM shape; the bidirectional attention sums twice the keys.

    python scripts/bert_bench.py [--docs 1024] [--iters 20]

Timing as scripts/gemm_bench.py: warm-up calls, then `iters` back-to-back sgpt_encode calls between two events on one stream,
one synchronisation at the end; random-init weights (sgpt_amd.model.synthetic_bert_weights / synthetic_weights), f16 operands,
mean pooling.  Prints one JSON line per model."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sgpt_amd import SGPTConfig, SGPTModel  # noqa: E402
from sgpt_amd.model import synthetic_bert_weights, synthetic_weights  # noqa: E402


def rate(m, seqs, iters):
    pb = m.pack(seqs)
    out = torch.empty((pb.B, m.cfg.hidden_size), dtype=torch.float32, device=m.device)
    for _ in range(3):
        m.encode_packed(pb, mode="mean", normalize=True, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        m.encode_packed(pb, mode="mean", normalize=True, out=out)
    e1.record()
    e1.synchronize()
    assert torch.isfinite(out).all() and m.range_flags() == 0
    ms = e0.elapsed_time(e1) / iters
    return dict(ms_per_call=round(ms, 3), sentences_per_s=round(len(seqs) / ms * 1e3, 1), token_rows=pb.T_pad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1024)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    bert = SGPTConfig.from_hf_dict(dict(model_type="bert", vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                        intermediate_size=3072, max_position_embeddings=512, layer_norm_eps=1e-12, type_vocab_size=2))
    neo = SGPTConfig(vocab_size=50257, max_position_embeddings=2048, hidden_size=768, num_layers=12, num_heads=12)
    for name, cfg, w in (("bert-base", bert, synthetic_bert_weights(bert, 0)), ("sgpt-125m", neo, synthetic_weights(neo, 0))):
        m = SGPTModel(cfg, w, device="cuda:0", dtype="f16", precision="plain")
        seqs = rng.integers(3, 30000, size=(a.docs, a.seq)).tolist()
        print(json.dumps(dict(model=name, docs=a.docs, seq=a.seq, dtype="f16", **rate(m, seqs, a.iters))), flush=True)
        m.close()


if __name__ == "__main__":
    main()
