#!/usr/bin/env python3
"""The IVF corpus against the exact f16 scan and the binary + uint8-rescore search, in one process on one card: clustered unit rows of
width 768, cosine top-11, 1 / 16 / 1000 queries, corpora of 1 M (nlist 1024) and 16 M (nlist 4096) documents, nprobe 8 / 32 / 128.

Rows: `--clusters` Gaussian clusters (unit-variance centres, unit per-element noise), L2-normalised; queries are perturbed corpus rows.
The index is built by Context.ivf_index (timed: wall clock around a synchronised call).  Passes: ivf8 / ivf32 / ivf128 = sgpt_ivf_search
at that nprobe; f16 = the exact scan sgpt_score_topk(SGPT_F16) over the same f16 rows in their original order (code the IVF change does
not touch: a valid same-process baseline); bits+u8 = sgpt_score_topk_bits_u8 over a binary copy with a uint8 copy (kp = 4 k).  Per (nq, pass): REPEATS
windows of REPS passes each between two device events on a warmed-up context, the windows of the passes interleaved; the median window
and the min .. max spread are printed.  recall@10 = the overlap of a pass's ten best with the exact f16 scan's ten best, over the 1000
queries, also at nprobe 1, 2 and 4.  The A/B bar for a speed claim: the IVF median below the f16 median by more than three times the larger window spread.

  python scripts/ivf_bench.py [--n 1000000,16000000] [--nlist 1024,4096] [--nprobe 8,32,128] [--nq 1,16,1000] [--out profiles/ivf_corpus.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import get_context  # noqa: E402


def make_rows(N, d, clusters, g, block=1_000_000):
    """(f16 rows [N, d] on the device, the cluster centres): built block by block, the fp32 rows never exist whole."""
    centres = torch.randn(clusters, d, device="cuda", generator=g)
    out = torch.empty((N, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, N, block):
        n = min(block, N - r0)
        lab = torch.randint(0, clusters, (n,), device="cuda", generator=g)
        out[r0:r0 + n] = torch.nn.functional.normalize(centres[lab] + torch.randn(n, d, device="cuda", generator=g), dim=1).half()
    return out


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
        raise SystemExit("ivf_bench.py measures on the GPU: no HIP device visible")
    ctx = get_context("cuda:0")
    d, k = a.d, a.k
    probes = [int(x) for x in a.nprobe.split(",")]
    passes = tuple(f"ivf{p}" for p in probes) + ("f16", "bits+u8")
    lines = [f"# scripts/ivf_bench.py: d = {d} clustered unit rows ({a.clusters} clusters), k = {k}; {torch.cuda.get_device_name(0)}",
             "# time = median of the windows (min .. max), each window REPS passes between two device events, passes alternating",
             "# ivfP = sgpt_ivf_search at nprobe P, f16 = the exact f16 scan (sgpt_score_topk), bits+u8 = binary search + uint8 re-scoring (kp = 4 k)",
             "# recall@10 = overlap of the ten best with the exact f16 scan's, over 1000 queries (perturbed corpus rows); synthetic rows"]
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
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix = ctx.ivf_index(emb, nlist=nlist, n_iter=a.n_iter)
        torch.cuda.synchronize()
        t_build = time.perf_counter() - t0
        qall = torch.nn.functional.normalize(emb[torch.randperm(N, device="cuda", generator=g)[:1000]].float()
                                             + 0.3 * torch.randn(1000, d, device="cuda", generator=g) / d ** 0.5, dim=1)
        sizes = (ix.offsets[1:] - ix.offsets[:-1]).cpu()
        emit(f"== N = {N}, nlist = {nlist}: built in {t_build:.3f} s ({a.n_iter} Lloyd iterations on {min(N, 256 * nlist)} rows); index "
             f"{ix.nbytes / 1e9:.3f} GB; lists: max {ix.max_list}, median {int(sizes.median())}, empty {int((sizes == 0).sum())}")
        # the baselines scan the rows in their ORIGINAL order: list-major order is sorted by content, which the sampled thresholds of
        # the streaming scorers are not built for (a drifting score distribution overflows their candidate lists)
        rows0 = torch.empty((N, d), dtype=torch.float16, device="cuda")
        for r0 in range(0, N, 1_000_000):
            rows0[r0:r0 + 1_000_000] = ctx.l2_normalize(emb[r0:r0 + 1_000_000], out_dtype=torch.float16)
        del emb
        torch.cuda.empty_cache()
        cb = ctx.binarize_corpus(rows0, keep_uint8=True)
        q16all = qall.half()
        _, iex, _ = ctx.score_topk(q16all, rows0, 10, dtype=torch.float16)
        exact = iex.tolist()
        for p in sorted(set([1, 2, 4] + probes)):
            if p > ix.nlist:
                continue
            _, ii, _ = ctx.score_topk(qall, ix.with_nprobe(p), 10)
            rec = sum(len(set(x) & set(y)) for x, y in zip(ii.tolist(), exact)) / (1000 * 10)
            emit(f"recall@10 ivf{p}: {rec:.4f}")
        _, ib, _ = ctx.score_topk(qall, cb, 10, rescore="uint8")
        rec = sum(len(set(x) & set(y)) for x, y in zip(ib.tolist(), exact)) / (1000 * 10)
        emit(f"recall@10 bits+u8: {rec:.4f}")
        for nq in [int(x) for x in a.nq.split(",")]:
            q32, q16 = qall[:nq].contiguous(), q16all[:nq].contiguous()
            run = {f"ivf{p}": (lambda v=ix.with_nprobe(p): ctx.score_topk(q32, v, k)) for p in probes}
            run["f16"] = lambda: ctx.score_topk(q16, rows0, k, dtype=torch.float16)
            run["bits+u8"] = lambda: ctx.score_topk(q32, cb, k, rescore="uint8")
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
                name = f"ivf{p}"
                bar = 3 * max(spread[name], spread["f16"])
                emit(f"nq={nq:5d} {name} against f16: {med[name]:.4f} vs {med['f16']:.4f} ms (x{med['f16'] / med[name]:.2f}); three times the larger spread "
                     f"{bar:.4f} ms: {'below the exact scan by more than the bar' if med['f16'] - med[name] > bar else 'NOT below the exact scan by the bar'}")
        del ix, cb, rows0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
