#!/usr/bin/env python3
"""The two-stage search over a binary corpus with each of its second stages, and the full uint8 scan, in one process on one card: unit
rows of width 768, cosine top-11, nq in {16, 1000}, corpora of 1 M and 16 M documents, timed in alternating order.

Passes: bits0 = Hamming only (kp = k); sign = sign re-scoring, fp8 = fp8 re-scoring, uint8 = uint8 re-scoring (sgpt_score_topk_bits_u8)
of kp = k * multiplier candidates; u8scan = sgpt_score_topk_u8 over all codes.  The yardstick of the uint8 re-scoring is the fp8
re-scoring measured here, in the same windows: both stores hold 768 bytes per candidate row.  Per (nq, pass): REPEATS windows of REPS
passes each between two device events on a warmed-up context, the windows of the passes interleaved; the median window and the
min .. max spread are printed.  The last line per nq states uint8 against fp8 and the spread of both.  The corpus is built block by
block: the fp32 rows of 16 M documents never exist whole.  The uint8 ranges come from the first block.

  python scripts/score_bits_u8_bench.py [--n 1000000,16000000] [--d 768] [--k 11] [--mult 4] [--nq 16,1000] [--out profiles/score_bits_u8_corpus.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import BinaryCorpus, QuantizedCorpus, Uint8Corpus, get_context  # noqa: E402

PASSES = ("bits0", "sign", "fp8", "uint8", "u8scan")


def build(ctx, N, d, base, g, block=1_000_000):
    ld = (d + 127) // 128 * 128
    codes8 = torch.empty((N, d), dtype=torch.uint8, device="cuda")
    scale = torch.empty((N,), dtype=torch.float32, device="cuda")
    codes = torch.empty((N, ld), dtype=torch.uint8, device="cuda")
    bits = torch.empty((N, 4 * ((d + 31) // 32)), dtype=torch.uint8, device="cuda")
    start = step = None
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        c32 = torch.nn.functional.normalize(base + torch.randn(n, d, device="cuda", generator=g), dim=1)
        if start is None:                                        # ranges of the first block; later rows outside them clamp
            mn, mx = ctx.u8_col_minmax(c32)
            start = torch.zeros((ld,), dtype=torch.float32, device="cuda")
            step = torch.zeros((ld,), dtype=torch.float32, device="cuda")
            start[:d] = mn
            step[:d] = (mx - mn) / torch.full_like(mx, 255.0)
        cb, sb = ctx.fp8_quantize_rows(c32)
        codes8[r0:r0 + n], scale[r0:r0 + n] = cb, sb
        ctx.u8_quantize_rows(c32, start, step, out=codes[r0:r0 + n])
        ctx.pack_sign_bits(c32, out=bits[r0:r0 + n])
        del c32, cb, sb
    c8 = QuantizedCorpus(codes8, scale, True, d)
    cu = Uint8Corpus(codes, start, step, True, d)
    return cu, BinaryCorpus(bits, d, fp8=c8, u8=cu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,16000000")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--mult", type=float, default=4.0)
    ap.add_argument("--nq", default="16,1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="target length of one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bits_u8_bench.py measures on the GPU: no HIP device visible")
    ctx = get_context("cuda:0")
    d, k, mult = a.d, a.k, a.mult
    kp = min(1024, max(k, int(round(k * mult))))
    lines = [f"# scripts/score_bits_u8_bench.py: d = {d} unit rows, k = {k}, re-scoring of kp = {kp} candidates; {torch.cuda.get_device_name(0)}",
             "# time = median of the windows (min .. max), each window REPS passes between two device events, passes alternating",
             "# bits0 = Hamming only, sign / fp8 / uint8 = + that re-scoring, u8scan = the full uint8 scan (sgpt_score_topk_u8)"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:                                                # kept current: a run cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for N in [int(x) for x in a.n.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(0)
        base = torch.randn(1, d, device="cuda", generator=g) * 3      # anisotropic: shared dominant direction (scripts/score_bench.py)
        cu, cb = build(ctx, N, d, base, g)
        emit(f"== N = {N}: bits {cb.bits.numel() / 1e9:.4f} GB, fp8 copy {cb.fp8.nbytes / 1e9:.3f} GB, uint8 copy {cu.nbytes / 1e9:.3f} GB")
        for nq in [int(x) for x in a.nq.split(",")]:
            q32 = torch.nn.functional.normalize(base + torch.randn(nq, d, device="cuda", generator=g), dim=1)
            run = {"bits0": lambda: ctx.score_topk(q32, cb, k, rescore="none"),
                   "sign": lambda: ctx.score_topk(q32, cb, k, rescore="sign", rescore_multiplier=mult),
                   "fp8": lambda: ctx.score_topk(q32, cb, k, rescore="fp8", rescore_multiplier=mult),
                   "uint8": lambda: ctx.score_topk(q32, cb, k, rescore="uint8", rescore_multiplier=mult),
                   "u8scan": lambda: ctx.score_topk(q32, cu, k)}
            _, iscan, _ = run["u8scan"]()
            overlap = {}
            for name in PASSES[:4]:
                _, ib, _ = run[name]()
                overlap[name] = sum(len(set(x) & set(y)) for x, y in zip(ib.tolist(), iscan.tolist())) / (nq * k)
            reps = {}
            for name, f in run.items():                              # warm-up and window length (a pass of seconds is not repeated much)
                f()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                reps[name] = max(1, int(a.window_ms / e0.elapsed_time(e1)))
                for _ in range(min(3, reps[name])):
                    f()
            torch.cuda.synchronize()
            times = {n_: [] for n_ in PASSES}
            for r in range(a.repeats):
                for name in (PASSES if r % 2 == 0 else PASSES[::-1]):
                    if reps[name] == 1 and r >= 3:                   # a pass longer than a window: three windows
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps[name]):
                        run[name]()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / reps[name])
            med = {n_: statistics.median(t) for n_, t in times.items()}
            for name in PASSES:
                line = (f"nq={nq:5d} {name:6s}: {med[name]:.4f} ms per pass ({min(times[name]):.4f} .. {max(times[name]):.4f}, {len(times[name])} windows x "
                        f"{reps[name]} passes)")
                if name in overlap:
                    line += f"; top-{k} overlap with the full uint8 scan {overlap[name]:.4f}"
                emit(line)
            sp8, spu = max(times["fp8"]) - min(times["fp8"]), max(times["uint8"]) - min(times["uint8"])
            emit(f"nq={nq:5d} uint8 re-scoring against fp8 re-scoring: {med['uint8']:.4f} vs {med['fp8']:.4f} ms ({med['uint8'] - med['fp8']:+.4f} ms, "
                 f"x{med['uint8'] / med['fp8']:.3f}); spread of the windows (max - min): fp8 {sp8:.4f} ms, uint8 {spu:.4f} ms; over the Hamming-only pass "
                 f"(stage 1 keeping kp instead of k, plus the second stage): sign {med['sign'] - med['bits0']:+.4f}, fp8 {med['fp8'] - med['bits0']:+.4f}, "
                 f"uint8 {med['uint8'] - med['bits0']:+.4f} ms")
        del cu, cb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
