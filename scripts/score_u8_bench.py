#!/usr/bin/env python3
"""The search pass over an f16 corpus, over its fp8 (e4m3fn, one scale per row) quantisation and over its uint8 (one range per
dimension) quantisation: 1 M x 768 unit rows, cosine top-11, nq in {1, 16, 64, 1000}, the three corpora in one process on one card,
timed in alternating order.

Per (nq, format): REPEATS windows of REPS passes each between two device events (a window of ~0.1 s or more), the windows of the
formats interleaved and their order rotated; the median window and the min .. max spread are printed, with the corpus bytes one pass
reads (N d 2 for f16, N d + 4 N for fp8, N d + 8 d for uint8: whatever the schedule re-reads for its threshold sample is not counted;
nq > 64 re-streams the uint8 codes once per group of 64 queries, counted) and the stream rate they imply.  The top-k overlap of each
format with the f16 corpus and the overflow count of the last pass (filtered chunks recomputed by the fallback) are reported.

  python scripts/score_u8_bench.py [--n 1000000] [--d 768] [--k 11] [--nq 1,16,64,1000] [--out profiles/score_u8_corpus.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import get_context  # noqa: E402

FORMATS = ("f16", "fp8", "uint8")


def corpus_bytes(fmt, N, d, nq):
    if fmt == "f16":
        return N * d * 2
    if fmt == "fp8":
        return N * d + 4 * N
    return ((nq + 63) // 64) * (N * d + 8 * d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--nq", default="1,16,64,1000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=150.0, help="target length of one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_u8_bench.py measures on the GPU: no HIP device visible")
    ctx = get_context("cuda:0")
    N, d, k = a.n, a.d, a.k
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randn(1, d, device="cuda", generator=g) * 3          # anisotropic: shared dominant direction (scripts/score_bench.py)
    c32 = torch.nn.functional.normalize(base + torch.randn(N, d, device="cuda", generator=g), dim=1)
    c16 = c32.to(torch.float16)
    c8 = ctx.quantize_corpus(c32, normalize=True)
    cu = ctx.scalar_quantize_corpus(c32, normalize=True)
    del c32
    lines = [f"# scripts/score_u8_bench.py: N = {N} x d = {d} unit rows, k = {k}; {torch.cuda.get_device_name(0)}",
             f"# corpus bytes: f16 {N * d * 2 / 1e9:.3f} GB, fp8 {c8.nbytes / 1e9:.3f} GB (codes + one fp32 scale per row), "
             f"uint8 {cu.nbytes / 1e9:.3f} GB (codes + two fp32 per dimension)",
             "# time = median of the windows (min .. max), each window REPS passes between two device events, formats alternating"]
    print("\n".join(lines), flush=True)
    for nq in [int(x) for x in a.nq.split(",")]:
        q32 = torch.nn.functional.normalize(base + torch.randn(nq, d, device="cuda", generator=g), dim=1)
        q16 = q32.to(torch.float16)
        run = {"f16": lambda: ctx.score_topk(q16, c16, k, dtype=torch.float16), "fp8": lambda: ctx.score_topk(q16, c8, k),
               "uint8": lambda: ctx.score_topk(q32, cu, k)}
        # results first: overlap with the unquantised f16 corpus, overflow counts
        res, over = {}, {}
        for name in FORMATS:
            res[name] = run[name]()
            over[name] = ctx.score_overflow_count()
        i16 = res["f16"][1].tolist()
        overlap = {n_: sum(len(set(x) & set(y)) for x, y in zip(res[n_][1].tolist(), i16)) / (nq * k) for n_ in FORMATS}
        dmax = {n_: float((res[n_][0][:, 0] - res["f16"][0][:, 0]).abs().max()) for n_ in FORMATS}
        # warm-up and window length
        for f in run.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        reps = {}
        for name, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                f()
            e1.record()
            torch.cuda.synchronize()
            reps[name] = max(5, int(a.window_ms / (e0.elapsed_time(e1) / 5)))
        times = {n_: [] for n_ in FORMATS}
        for r in range(a.repeats):
            for name in FORMATS[r % 3:] + FORMATS[:r % 3]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps[name]):
                    run[name]()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps[name])
        med = {n_: statistics.median(t) for n_, t in times.items()}
        for name in FORMATS:
            b = corpus_bytes(name, N, d, nq)
            line = (f"nq={nq:5d} {name:5s}: {med[name]:.4f} ms per pass ({min(times[name]):.4f} .. {max(times[name]):.4f}, {a.repeats} windows x "
                    f"{reps[name]} passes); corpus {b / 1e9:.3f} GB per pass -> {b / (med[name] * 1e-3) / 1e12:.2f} TB/s; top-{k} overlap with the "
                    f"f16 corpus {overlap[name]:.4f}, max |d best score| {dmax[name]:.2e}; filtered chunks {over[name][0]}, overflowed {over[name][1]}")
            lines.append(line)
            print(line, flush=True)
        line = (f"nq={nq:5d} uint8 / fp8 time = {med['uint8'] / med['fp8']:.3f}, uint8 / f16 = {med['uint8'] / med['f16']:.3f}, "
                f"fp8 / f16 = {med['fp8'] / med['f16']:.3f}")
        lines.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
