#!/usr/bin/env python3
"""score_samebits.py save FILE | check FILE: seeded score_topk results (values, indices, n, filtered-chunk and overflow counts) over
f16 / fp8 / uint8 corpora at nq = 1, 16, 64, fresh and with a running list, at a materialised size (N = 1000) and the smallest filtered
one (N = 262 144 + 77), d = 128, k = 11: 36 results; and over the binary corpus at the same two sizes, nq = 16 and 70 (two stage-1 query
groups), fresh and running, with rescore none / sign / fp8 on an uncentred corpus and rescore uint8 on one centred on its mean: 32
more.  `save` writes them (run with SGPT_HIP_LIB = the build to compare against), `check`
requires torch.equal on every one from the library now selected.  For refactors of the scorer that must not change a bit."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sgpt_amd import BinaryCorpus, QuantizedCorpus, Uint8Corpus, _lib, get_context  # noqa: E402


def results():
    ctx = get_context("cuda:0")
    out = {}
    d, k = 128, 11
    for N in (1000, 262_144 + 77):
        g = torch.Generator(device="cuda").manual_seed(1000 + N % 997)
        q32 = torch.nn.functional.normalize(torch.randn(64, d, device="cuda", generator=g), dim=1)
        base = torch.randn(1, d, device="cuda", generator=g) * 2
        c32 = torch.nn.functional.normalize(base + torch.randn(N + 700, d, device="cuda", generator=g), dim=1)
        c16 = c32.to(torch.float16)
        c8 = ctx.quantize_corpus(c32, normalize=True)
        cu = ctx.scalar_quantize_corpus(c32, normalize=False)
        corp = {
            "f16": (lambda a, b: c16[a:b], lambda nq: q32[:nq].to(torch.float16).contiguous()),
            "fp8": (lambda a, b: QuantizedCorpus(c8.codes[a:b], c8.scale[a:b], True), lambda nq: q32[:nq].to(torch.float16).contiguous()),
            "uint8": (lambda a, b: Uint8Corpus(cu.codes[a:b].contiguous(), cu.start, cu.step, False, d), lambda nq: q32[:nq].contiguous()),
        }
        for fmt, (part, qf) in corp.items():
            for nq in (1, 16, 64):
                q = qf(nq)
                val, idx, n = ctx.score_topk(q, part(700, 700 + N), k, idx_base=700)
                over = ctx.score_overflow_count()
                out[f"{fmt} N={N} nq={nq} fresh"] = (val.cpu().clone(), idx.cpu().clone(), n, over)
                v0, i0, n0 = ctx.score_topk(q, part(0, 700), k, idx_base=0)
                val, idx, n = ctx.score_topk(q, part(700, 700 + N), k, idx_base=700, run=(v0, i0, n0))
                over = ctx.score_overflow_count()
                out[f"{fmt} N={N} nq={nq} running"] = (val.cpu().clone(), idx.cpu().clone(), n, over)
        q70 = torch.nn.functional.normalize(torch.randn(70, d, device="cuda", generator=g), dim=1)
        cb = ctx.binarize_corpus(c32, keep_fp8=True)
        cc = ctx.binarize_corpus(c32, center="mean", keep_uint8=True)
        plain = lambda a, b: BinaryCorpus(cb.bits[a:b], d, fp8=QuantizedCorpus(cb.fp8.codes[a:b], cb.fp8.scale[a:b], True, d))  # noqa: E731
        centred = lambda a, b: BinaryCorpus(cc.bits[a:b], d, center=cc.center,  # noqa: E731
                                            u8=Uint8Corpus(cc.u8.codes[a:b].contiguous(), cc.u8.start, cc.u8.step, True, d))
        for rescore, part in (("none", plain), ("sign", plain), ("fp8", plain), ("uint8", centred)):
            for nq in (16, 70):
                q = q70[:nq].contiguous()
                val, idx, n = ctx.score_topk(q, part(700, 700 + N), k, idx_base=700, rescore=rescore)
                over = ctx.score_overflow_count()
                out[f"bits {rescore} N={N} nq={nq} fresh"] = (val.cpu().clone(), idx.cpu().clone(), n, over)
                run = ctx.score_topk(q, part(0, 700), k, idx_base=0, rescore=rescore)
                val, idx, n = ctx.score_topk(q, part(700, 700 + N), k, idx_base=700, run=run, rescore=rescore)
                over = ctx.score_overflow_count()
                out[f"bits {rescore} N={N} nq={nq} running"] = (val.cpu().clone(), idx.cpu().clone(), n, over)
    return out


def main():
    mode, path = sys.argv[1], sys.argv[2]
    print(f"samebits {mode}: library {_lib.LIB_PATH}", flush=True)
    res = results()
    if mode == "save":
        torch.save(res, path)
        print(f"saved {len(res)} results")
        return
    want = torch.load(path)
    assert sorted(want) == sorted(res)
    bad = 0
    for name in sorted(res):
        (v, i, n, over), (wv, wi, wn, wover) = res[name], want[name]
        ok = torch.equal(v, wv) and torch.equal(i, wi) and n == wn and over == wover
        bad += not ok
        print(f"{'same' if ok else 'DIFFERENT'}: {name}: n = {n}, filtered chunks / overflowed = {over}, best {v[0, 0].item():.6f}")
    print(f"compared {len(res)} results (values and indices, torch.equal): {len(res) - bad} identical, {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
