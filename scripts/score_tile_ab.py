#!/usr/bin/env python3
"""Same-process A/B of two builds of the library on the short-batch search pass (nq <= 64): parent A / new / parent B, three contexts
in ONE process.  Every build is loaded through its own dlopen handle and gets its own Context; parent B is a second instance of the
parent build (a COPY of its file: its own code object, context and workspace), so |A - B| holds what a context alone moves.  Timing loop
of scripts/score_u8_bench.py: windows of ~0.15 s between two device events, 7 windows per series, order A / new / B per repeat.  Cases:
1 M x 768 unit rows, k = 11, nq = 1, 16, 64 over f16 / fp8 / uint8 corpora, then a ragged second shard behind the running list of a
first one.  The results of the two builds must be torch.equal before a case is timed.  Criterion: |new - mean(A, B)| <= |A - B|.

  SGPT_LIB_TAG=parent python -m sgpt_amd.build      # at the parent commit; then copy libsgpt_hip_parent.so to a second name
  python scripts/score_tile_ab.py PARENT_LIB NEW_LIB OUT [PARENT_LIB_COPY]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import QuantizedCorpus, Uint8Corpus, _lib, runtime  # noqa: E402

FORMATS = ("f16", "fp8", "uint8")
REPEATS = 7
WINDOW_MS = 150.0


def ctx_for(path):
    _lib._lib = None
    _lib.LIB_PATH = path
    ctx = runtime.Context(0)
    assert ctx.lib._name == path
    return ctx


def window(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(name, run_parent, run_new, lines, run_parent_b=None):
    """run_*: zero-argument callables of one pass.  Returns (parent A median, new median, parent B median)."""
    run_parent_b = run_parent_b or run_parent
    for f in (run_parent, run_new, run_parent_b):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    reps = max(5, int(WINDOW_MS / window(run_parent, 5)))
    t = {"A": [], "new": [], "B": []}
    for r in range(REPEATS):
        t["A"].append(window(run_parent, reps))
        t["new"].append(window(run_new, reps))
        t["B"].append(window(run_parent_b, reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    pm = (med["A"] + med["B"]) / 2
    spread = abs(med["A"] - med["B"])
    allp = t["A"] + t["B"]
    diff = med["new"] - pm
    verdict = "within the parent's spread" if abs(diff) <= spread else ("FASTER than the parent beyond its spread" if diff < 0 else
                                                                        ("SLOWER than the parent beyond its spread" if med["new"] > max(allp) else
                                                                         "above the two parent medians' gap, inside the parent windows' min .. max"))
    line = (f"{name}: parent A {med['A']:.4f} ms ({min(t['A']):.4f} .. {max(t['A']):.4f}), new {med['new']:.4f} ms ({min(t['new']):.4f} .. {max(t['new']):.4f}), "
            f"parent B {med['B']:.4f} ms ({min(t['B']):.4f} .. {max(t['B']):.4f}); {REPEATS} windows x {reps} passes each; "
            f"new - parent = {diff * 1e3:+.2f} us ({diff / pm * 100:+.2f} %), |A - B| = {spread * 1e3:.2f} us, parent windows {min(allp):.4f} .. {max(allp):.4f}: {verdict}")
    lines.append(line)
    print(line, flush=True)


def main():
    parent_lib, new_lib, out = sys.argv[1:4]
    cp, cn = ctx_for(parent_lib), ctx_for(new_lib)
    cb = ctx_for(sys.argv[4]) if len(sys.argv) > 4 else cp      # parent B: a second instance of the parent's library (a copy of the file)
    lines = [f"# parent = {os.path.basename(parent_lib)}, new = {os.path.basename(new_lib)}; one process, parent B = {'a second instance of the parent library (its own context)' if len(sys.argv) > 4 else 'the same context as A'}, "
             f"order per repeat: parent A, new, parent B; median of {REPEATS} windows (min .. max)"]
    print(lines[0], flush=True)
    N, d, k = 1_000_000, 768, 11
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randn(1, d, device="cuda", generator=g) * 3
    c32 = torch.nn.functional.normalize(base + torch.randn(N, d, device="cuda", generator=g), dim=1)
    c16 = c32.to(torch.float16)
    c8 = cn.quantize_corpus(c32, normalize=True)
    cu = cn.scalar_quantize_corpus(c32, normalize=True)
    del c32
    lines.append(f"# search pass, {N} x {d} unit rows, k = {k}")
    for nq in (1, 16, 64):
        q32 = torch.nn.functional.normalize(base + torch.randn(nq, d, device="cuda", generator=g), dim=1)
        q16 = q32.to(torch.float16)

        def runs(ctx):
            return {"f16": lambda: ctx.score_topk(q16, c16, k, dtype=torch.float16), "fp8": lambda: ctx.score_topk(q16, c8, k),
                    "uint8": lambda: ctx.score_topk(q32, cu, k)}
        rp, rn, rb = runs(cp), runs(cn), runs(cb)
        for fmt in FORMATS:
            a, b = rp[fmt](), rn[fmt]()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (fmt, nq)
            ab(f"nq={nq:3d} {fmt:5s}", rp[fmt], rn[fmt], lines, rb[fmt])
    # one filtered shard behind a running list: shard 1 gives the list, shard 2 (one filtered launch with appends, ragged) is timed
    lines.append("# running list from shard 1 (250 000 documents), then shard 2 (749 923 documents, ragged; timed with the list restored per pass), nq = 16")
    N1, N2 = 250_000, 749_923         # (shard 2: 2929 whole tiles + 99 documents)
    for fmt in FORMATS:
        def shard(ctx):
            q = q16 if fmt != "uint8" else q32
            if fmt == "f16":
                s1, s2 = c16[:N1], c16[N1:N1 + N2]
            elif fmt == "fp8":
                s1, s2 = QuantizedCorpus(c8.codes[:N1], c8.scale[:N1], True), QuantizedCorpus(c8.codes[N1:N1 + N2], c8.scale[N1:N1 + N2], True)
            else:
                s1 = Uint8Corpus(cu.codes[:N1], cu.start, cu.step, True, d)
                s2 = Uint8Corpus(cu.codes[N1:N1 + N2], cu.start, cu.step, True, d)
            v0, i0, n0 = ctx.score_topk(q, s1, k, idx_base=0)
            keep = (v0.clone(), i0.clone())

            def one():
                v0.copy_(keep[0])
                i0.copy_(keep[1])
                return ctx.score_topk(q, s2, k, idx_base=N1, run=(v0, i0, n0))
            return one
        nq = 16
        q32 = torch.nn.functional.normalize(base + torch.randn(nq, d, device="cuda", generator=g), dim=1)
        q16 = q32.to(torch.float16)
        fp, fn, fb = shard(cp), shard(cn), shard(cb)
        a = fp()
        a = (a[0].clone(), a[1].clone())
        over_p = cp.score_overflow_count()
        b = fn()
        over_n = cn.score_overflow_count()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), fmt
        lines.append(f"# {fmt}: filtered chunks / overflowed: parent {over_p}, new {over_n}; results identical")
        ab(f"shard 2 after shard 1, nq= 16 {fmt:5s}", fp, fn, lines, fb)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
