#!/usr/bin/env python3
"""The search pass over a binary (1-bit) corpus against the same pass over f16 rows and over the fp8 (e4m3fn) quantisation: unit rows
of width 768, cosine top-11, nq in {1, 16, 64, 1000}, corpora of 1 M and 16 M documents, all formats in one process on one card,
timed in alternating order.

Formats: f16 (sgpt_score_topk), fp8 (sgpt_score_topk_q8), and sgpt_score_topk_bits in its three modes -- bits0 = Hamming only (kp = k),
bits1 = sign re-scoring and bits2 = fp8 re-scoring of kp = 40 candidates.  Per (nq, format): REPEATS windows of REPS passes each between
two device events on a warmed-up context, the windows of the formats interleaved; the median window and the min .. max spread are
printed, with the corpus bytes one pass reads (what the schedule re-reads for its threshold sample, and the rows the re-scoring
gathers, are not counted; nq > 64 streams the bits once per group of 64 queries, which IS counted) and the stream rate they imply.
After the passes of every bits mode the overflow fallback of its last pass is read back (filtered chunks / chunks that overflowed
their candidate lists and were recomputed; for nq > 64 that is the last group of 64 queries only), and the top-k overlap with the f16 result is reported.  The corpus is built block by block:
the fp32 rows of 16 M documents never exist whole.

  python scripts/score_bits_bench.py [--n 1000000,16000000] [--d 768] [--k 11] [--kp 40] [--nq 1,16,64,1000] [--out profiles/score_bits_corpus.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import BinaryCorpus, QuantizedCorpus, get_context  # noqa: E402

FORMATS = ("f16", "fp8", "bits0", "bits1", "bits2")


def build(ctx, N, d, base, g, block=1_000_000):
    c16 = torch.empty((N, d), dtype=torch.float16, device="cuda")
    codes = torch.empty((N, d), dtype=torch.uint8, device="cuda")
    scale = torch.empty((N,), dtype=torch.float32, device="cuda")
    bits = torch.empty((N, 4 * ((d + 31) // 32)), dtype=torch.uint8, device="cuda")
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        c32 = torch.nn.functional.normalize(base + torch.randn(n, d, device="cuda", generator=g), dim=1)
        c16[r0:r0 + n] = c32.to(torch.float16)
        cb, sb = ctx.fp8_quantize_rows(c32)
        codes[r0:r0 + n], scale[r0:r0 + n] = cb, sb
        ctx.pack_sign_bits(c32, out=bits[r0:r0 + n])
        del c32, cb, sb
    c8 = QuantizedCorpus(codes, scale, True, d)
    return c16, c8, BinaryCorpus(bits, d, fp8=c8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,16000000")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--kp", type=int, default=40)
    ap.add_argument("--nq", default="1,16,64,1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="target length of one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bits_bench.py measures on the GPU: no HIP device visible")
    ctx = get_context("cuda:0")
    d, k, kp = a.d, a.k, a.kp
    mult = max(1.0, kp / k)
    lines = [f"# scripts/score_bits_bench.py: d = {d} unit rows, k = {k}, re-scoring of kp = {min(1024, max(k, int(round(k * mult))))} candidates; "
             f"{torch.cuda.get_device_name(0)}",
             "# time = median of the windows (min .. max), each window REPS passes between two device events, formats alternating",
             "# bits0 = Hamming only, bits1 = + sign re-scoring, bits2 = + fp8 re-scoring; fallback = filtered chunks of the last pass / "
             "chunks whose candidate lists overflowed (nq > 64: of the last group of 64 queries only -- every group reuses the flags)"]
    print("\n".join(lines), flush=True)
    for N in [int(x) for x in a.n.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(0)
        base = torch.randn(1, d, device="cuda", generator=g) * 3      # anisotropic: shared dominant direction (scripts/score_bench.py)
        c16, c8, cb = build(ctx, N, d, base, g)
        nbytes = {"f16": N * d * 2, "fp8": c8.nbytes, "bits": cb.bits.numel()}
        line = (f"== N = {N}: corpus bytes f16 {nbytes['f16'] / 1e9:.3f} GB, fp8 {nbytes['fp8'] / 1e9:.3f} GB, bits {nbytes['bits'] / 1e9:.4f} GB "
                f"({cb.bits.shape[1]} bytes per document)")
        lines.append(line)
        print(line, flush=True)
        for nq in [int(x) for x in a.nq.split(",")]:
            q32 = torch.nn.functional.normalize(base + torch.randn(nq, d, device="cuda", generator=g), dim=1)
            q16 = q32.to(torch.float16)
            run = {"f16": lambda: ctx.score_topk(q16, c16, k, dtype=torch.float16),
                   "fp8": lambda: ctx.score_topk(q16, c8, k),
                   "bits0": lambda: ctx.score_topk(q32, cb, k, rescore="none"),
                   "bits1": lambda: ctx.score_topk(q32, cb, k, rescore="sign", rescore_multiplier=mult),
                   "bits2": lambda: ctx.score_topk(q32, cb, k, rescore="fp8", rescore_multiplier=mult)}
            _, i16, _ = run["f16"]()
            overlap, fallback = {}, {}
            for name in FORMATS[2:]:
                _, ib, _ = run[name]()
                overlap[name] = sum(len(set(x) & set(y)) for x, y in zip(ib.tolist(), i16.tolist())) / (nq * k)
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
            times = {n_: [] for n_ in FORMATS}
            for r in range(a.repeats):
                for name in (FORMATS if r % 2 == 0 else FORMATS[::-1]):
                    if reps[name] == 1 and r >= 3:                   # a pass longer than a window: three windows
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps[name]):
                        run[name]()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / reps[name])
                    if name.startswith("bits"):
                        fallback[name] = ctx.score_overflow_count()
            med = {n_: statistics.median(t) for n_, t in times.items()}
            for name in FORMATS:
                b = nbytes["bits"] * ((nq + 63) // 64) if name.startswith("bits") else nbytes[name]
                line = (f"nq={nq:5d} {name:5s}: {med[name]:.4f} ms per pass ({min(times[name]):.4f} .. {max(times[name]):.4f}, {len(times[name])} windows x "
                        f"{reps[name]} passes); corpus {b / 1e9:.4f} GB per pass -> {b / (med[name] * 1e-3) / 1e12:.2f} TB/s")
                if name.startswith("bits"):
                    line += f"; fallback {fallback[name][0]} / {fallback[name][1]}; top-{k} overlap with f16 {overlap[name]:.4f}"
                lines.append(line)
                print(line, flush=True)
            line = (f"nq={nq:5d} time relative to fp8: bits0 {med['bits0'] / med['fp8']:.3f}, bits1 {med['bits1'] / med['fp8']:.3f}, "
                    f"bits2 {med['bits2'] / med['fp8']:.3f}; relative to f16: bits0 {med['bits0'] / med['f16']:.3f}")
            lines.append(line)
            print(line, flush=True)
        del c16, c8, cb
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
