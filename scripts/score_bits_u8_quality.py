#!/usr/bin/env python3
"""Ranking quality of the two-stage search over a binary corpus with each second stage, on clustered anisotropic rows: numpy and the
CPU references under tests/ only -- no device is used, and nothing here is a speed.

Corpus (tests/scorebits_u8_ref.py::clustered_anisotropic, seed 5): 1 000 cluster centres N(0, 1)^768, each repeated 20 times plus
0.5 N(0, 1); columns 0 .. 2 scaled by 30; a common offset 4 mu added, mu = N(0, 1)^768; rows normalised.  Queries: 32 corpus rows plus
0.3 N(0, 1) / sqrt(d), renormalised.  Printed: the recall of stage 1 (the share of the float64 top-10 among the kp Hamming candidates) and
the top-10 overlap with the float64 ranking for bits centred on the corpus mean or not, the stores sign / fp8 / uint8 and
kp in {40, 100, 400}; and the overlap of the full fp8 and uint8 scans.  Synthetic rows: the ordering of the pipelines is what the
figures show, not what real embeddings would give.

  python scripts/score_bits_u8_quality.py [--out profiles/score_bits_u8_quality.txt]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import score8_ref as R8  # noqa: E402
import scorebits_ref as B  # noqa: E402
import scorebits_u8_ref as BU  # noqa: E402
import scoreu8_ref as U  # noqa: E402


def top_of(vals, cand, k):
    """The k best candidates of every query by value descending, ties to the lowest index."""
    cv = np.take_along_axis(vals, cand, axis=1)
    order = np.lexsort((cand, -cv), axis=1)[:, :k]
    return np.take_along_axis(cand, order, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    k = a.k
    x, q = BU.clustered_anisotropic()
    N, d = x.shape
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    _, gold = R8.topk_lowest_index(exact, k)
    start, step = U.ranges(x)
    codes = U.quantize_rows(x, start, step)
    v_u8 = BU.values64(q, codes, start, step)
    c8, s8 = R8.quantize_rows(x)
    v_fp8 = R8.scores64(q, R8.dequantize(c8, s8))
    lines = [f"# scripts/score_bits_u8_quality.py: {N} x {d} clustered anisotropic unit rows, {q.shape[0]} queries, top-{k} overlap with the float64 "
             "ranking; numpy on the CPU references, no device",
             f"full scan: fp8 {BU.overlap(R8.topk_lowest_index(v_fp8, k)[1], gold):.4f}, uint8 {BU.overlap(R8.topk_lowest_index(v_u8, k)[1], gold):.4f}"]
    for name, center in (("centred", x.astype(np.float64).mean(axis=0).astype(np.float32)), ("uncentred", None)):
        bits = B.pack(x, center)
        qc = BU.centred(q, center)
        v_sign = B.sign_values(qc, bits, d)
        for kp in (40, 100, 400):
            _, cand = B.stage1(qc, bits, d, kp)
            recall = BU.overlap(cand, gold)
            ov = {s: BU.overlap(top_of(v, cand, k), gold) for s, v in (("sign", v_sign), ("fp8", v_fp8), ("uint8", v_u8))}
            lines.append(f"bits {name:9s} kp = {kp:3d}: stage-1 recall {recall:.4f}; top-{k} overlap: sign {ov['sign']:.4f}, fp8 {ov['fp8']:.4f}, "
                         f"uint8 {ov['uint8']:.4f}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
