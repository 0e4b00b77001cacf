#!/usr/bin/env python3
"""The IVF corpus over uint8 lists against the IVF corpus over f16 lists, in one process on one card: clustered unit rows of width 768,
cosine top-11, 1 / 16 / 1000 queries, corpora of 1 M (nlist 1024) and 16 M (nlist 4096) documents, nprobe 8 / 32 / 128.

Rows and queries are those of scripts/ivf_bench.py.  Both indices are built by Context.ivf_index from the same rows and the same seed (timed:
wall clock around a synchronised call), so their centroids, ids and offsets are the same bits and a query probes the same lists in both.
Passes: f16P = sgpt_ivf_search at nprobe P (the f16-list scan, code this change does not touch: a valid same-process baseline); u8P =
sgpt_ivf_search_u8 at nprobe P; u8scan = the full uint8 scan sgpt_score_topk_u8 over a uint8 corpus of the same rows in their original
order; f16scan = the exact f16 scan sgpt_score_topk(SGPT_F16) over those rows.  Per (nq, pass): REPEATS windows of REPS passes each
between two device events on a warmed-up context, the windows of the passes interleaved; the median window and the min .. max spread are
printed.  recall@10 = the overlap of a pass's ten best with the exact f16 scan's ten best over the 1000 queries.  The A/B bar for a speed
claim: the u8P median below the f16P median of the same run by more than three times the larger of the two window spreads.

  python scripts/ivf_u8_bench.py [--n 1000000,16000000] [--nlist 1024,4096] [--nprobe 8,32,128] [--nq 1,16,1000] [--out profiles/ivf_u8_corpus.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ivf_bench import make_rows  # noqa: E402
from sgpt_amd import get_context  # noqa: E402

# read off the gfx950 ISA of csrc/ivf.hip (hipcc --offload-arch=gfx950 -O3 --save-temps), by hand: the compiler's own figures per kernel
ISA_NOTES = [
    "# ISA of ivf_scan_u8_kernel (gfx950, -O3), per 16-byte piece per lane: 16 v_cvt_f32_ubyte{0..3} + 8 v_pk_add_f32 (code - 128) + 8 v_pk_fma_f32",
    "#   = 32 VALU instructions (32 per wavefront per KB of codes at ld % 1024 == 0; 16 of 64 lanes idle at ld = 768); a row's sum adds 3 v_add_f32",
    "#   and log2(G) ds_bpermute_b32 + v_add_f32.  <G, NR, RB>: VGPRs, waves per SIMD: <8,1,8> 72, 7; <16,1,8> 78, 6; <32,1,8> 98, 4;",
    "#   <64,1,8> (d = 768) 84, 5; <64,2,4> 90, 5; <64,4,2> 118, 4; no scratch.  For comparison ivf_scan_kernel<2,8> (f16 lists, d = 768): 113 VGPRs,",
    "#   4 waves per SIMD; its 16 pieces of a round take 80 v_cvt_f32_f16 + 40 v_pk_fma_f32 + 48 v_fma_mix_f32 = 10.5 VALU instructions per piece.",
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,16000000")
    ap.add_argument("--nlist", default="1024,4096")
    ap.add_argument("--nprobe", default="8,32,128")
    ap.add_argument("--nq", default="1,16,1000")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--n-iter", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0, help="target length of one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_u8_bench.py measures on the GPU: no HIP device visible")
    ctx = get_context("cuda:0")
    d, k = a.d, a.k
    probes = [int(x) for x in a.nprobe.split(",")]
    passes = tuple(f"{kind}{p}" for p in probes for kind in ("f16", "u8")) + ("u8scan", "f16scan")
    lines = [f"# scripts/ivf_u8_bench.py: d = {d} clustered unit rows ({a.clusters} clusters), k = {k}; {torch.cuda.get_device_name(0)}",
             "# time = median of the windows (min .. max), each window REPS passes between two device events, passes alternating",
             "# f16P = sgpt_ivf_search at nprobe P (f16 lists), u8P = sgpt_ivf_search_u8 at nprobe P (uint8 lists, the same lists), u8scan = the full",
             "# uint8 scan (sgpt_score_topk_u8), f16scan = the exact f16 scan (sgpt_score_topk); rows of both scans in their original order",
             "# recall@10 = overlap of the ten best with the exact f16 scan's, over 1000 queries (perturbed corpus rows); synthetic rows: quality on",
             "# real embeddings is not measured here"] + ISA_NOTES
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:                                                # kept current: a run cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    for N, nlist in zip([int(x) for x in a.n.split(",")], [int(x) for x in a.nlist.split(",")]):
        g = torch.Generator(device="cuda").manual_seed(0)
        emb = make_rows(N, d, a.clusters, g)
        built = []
        for precision in ("f16", "uint8"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index = ctx.ivf_index(emb, nlist=nlist, n_iter=a.n_iter, precision=precision)
            torch.cuda.synchronize()
            built.append((index, time.perf_counter() - t0))
        (ix, t16), (ix8, t8) = built
        del built
        same = all(torch.equal(getattr(ix, n_), getattr(ix8, n_)) for n_ in ("centroids", "ids", "offsets"))
        qall = torch.nn.functional.normalize(emb[torch.randperm(N, device="cuda", generator=g)[:1000]].float()
                                             + 0.3 * torch.randn(1000, d, device="cuda", generator=g) / d ** 0.5, dim=1)
        sizes = (ix.offsets[1:] - ix.offsets[:-1]).cpu()
        ld = ix8.codes.shape[1]
        emit(f"== N = {N}, nlist = {nlist} ({a.n_iter} Lloyd iterations on {min(N, 256 * nlist)} rows); lists: max {ix.max_list}, median "
             f"{int(sizes.median())}, empty {int((sizes == 0).sum())}; the two builds share centroids, ids and offsets bit for bit: {same}")
        emit(f"f16 lists: built in {t16:.3f} s; index {ix.nbytes / 1e9:.3f} GB, rows {N} x 2 d = {N * 2 * d / 1e9:.3f} GB")
        emit(f"uint8 lists: built in {t8:.3f} s; index {ix8.nbytes / 1e9:.3f} GB, rows {N} x ld = {N * ld / 1e9:.3f} GB (ld = {ld})")
        rows0 = torch.empty((N, d), dtype=torch.float16, device="cuda")
        for r0 in range(0, N, 1_000_000):
            rows0[r0:r0 + 1_000_000] = ctx.l2_normalize(emb[r0:r0 + 1_000_000], out_dtype=torch.float16)
        del emb
        torch.cuda.empty_cache()
        cu = ctx.scalar_quantize_corpus(rows0)
        q16all = qall.half()
        _, iex, _ = ctx.score_topk(q16all, rows0, 10, dtype=torch.float16)
        exact = iex.tolist()

        def recall(idx):
            return sum(len(set(x) & set(y)) for x, y in zip(idx.tolist(), exact)) / (1000 * 10)
        for p in sorted(set([1, 2, 4] + probes)):
            if p > ix.nlist:
                continue
            r16, r8 = recall(ctx.score_topk(qall, ix.with_nprobe(p), 10)[1]), recall(ctx.score_topk(qall, ix8.with_nprobe(p), 10)[1])
            emit(f"recall@10 nprobe {p}: f16 lists {r16:.4f}, uint8 lists {r8:.4f} (difference {r8 - r16:+.4f})")
        emit(f"recall@10 u8scan: {recall(ctx.score_topk(qall, cu, 10)[1]):.4f}")
        for nq in [int(x) for x in a.nq.split(",")]:
            q32, q16 = qall[:nq].contiguous(), q16all[:nq].contiguous()
            run = {}
            for p in probes:
                run[f"f16{p}"] = lambda v=ix.with_nprobe(p): ctx.score_topk(q32, v, k)
                run[f"u8{p}"] = lambda v=ix8.with_nprobe(p): ctx.score_topk(q32, v, k)
            run["u8scan"] = lambda: ctx.score_topk(q32, cu, k)
            run["f16scan"] = lambda: ctx.score_topk(q16, rows0, k, dtype=torch.float16)
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
            times = {n_: [] for n_ in passes}
            for r in range(a.repeats):
                for name in (passes if r % 2 == 0 else passes[::-1]):
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
            spread = {n_: max(t) - min(t) for n_, t in times.items()}
            for name in passes:
                emit(f"nq={nq:5d} {name:7s}: {med[name]:.4f} ms per pass ({min(times[name]):.4f} .. {max(times[name]):.4f}, {len(times[name])} windows x "
                     f"{reps[name]} passes)")
            for p in probes:
                u, f = f"u8{p}", f"f16{p}"
                bar = 3 * max(spread[u], spread[f])
                emit(f"nq={nq:5d} {u} against {f}: {med[u]:.4f} vs {med[f]:.4f} ms (x{med[f] / med[u]:.2f}); three times the larger spread "
                     f"{bar:.4f} ms: {'below the f16 lists by more than the bar' if med[f] - med[u] > bar else 'NOT below the f16 lists by the bar'}")
        del ix, ix8, cu, rows0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
