"""-m gpu: the binary corpus with a uint8 second stage -- sgpt_u8_rescore and sgpt_score_topk_bits_u8 (the query prologue and the gather
kernel of csrc/scoreu8.hip), Context.binarize_corpus(keep_uint8=True) / score_topk(rescore="uint8") / rescore_u8,
util.quantize_embeddings("ubinary", keep_uint8=True) / semantic_search.

Stage 1 is integer arithmetic and is compared index for index with tests/scorebits_ref.py on q - center.  The re-scored values are held
to the bound of include/sgpt_hip.h (tests/scorebits_u8_ref.py::bound) against float64; wherever two runs see the same (query,
document), their values are compared bit for bit: the order of the arithmetic does not depend on the launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import score8_ref as R8
import scorebits_ref as B
import scorebits_u8_ref as BU
import scoreu8_ref as U

pytestmark = pytest.mark.gpu

N_DOCS = 256 * 5 + 37


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


_cases = {}


def _case(d, N=N_DOCS, nq=65):
    """Unit rows around a common offset (so that the corpus mean changes the bits), unit queries; the uint8 codes, both sets of bits and
    the float64 values and bounds of every (query, document) -- built once per shape, never written to."""
    if (d, N) not in _cases:
        q, c = R8.unit_corpus(2317 + d, N, d, nq)
        q, c = q.numpy(), c.numpy()
        center = c.astype(np.float64).mean(axis=0).astype(np.float32)
        start, step = U.ranges(c)
        codes = U.quantize_rows(c, start, step)
        vals = BU.values64(q, codes, start, step)
        _cases[(d, N)] = dict(q=q, c=c, center=center, start=start, step=step, codes=codes, vals=vals,
                              bound=BU.bound(q, codes, start, step, vals), bits={False: B.pack(c), True: B.pack(c, center)})
    return _cases[(d, N)]


def _u8(cs, rows=slice(None)):
    from sgpt_amd import Uint8Corpus
    d = cs["q"].shape[1]
    return Uint8Corpus(torch.from_numpy(np.ascontiguousarray(cs["codes"][rows])).cuda(), torch.from_numpy(cs["start"]).cuda(),
                       torch.from_numpy(cs["step"]).cuda(), True, d)


def _corpus(cs, centred, rows=slice(None)):
    from sgpt_amd import BinaryCorpus
    d = cs["q"].shape[1]
    return BinaryCorpus(torch.from_numpy(np.ascontiguousarray(cs["bits"][centred][rows])).cuda(), d,
                        center=torch.from_numpy(cs["center"]).cuda() if centred else None, u8=_u8(cs, rows))


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("d", [100, 128, 768, 1100])
def test_rescore_alone(ctx, d, nq):
    """1. sgpt_u8_rescore, m = 44 slots of N = 300 documents, idx_base = 3, index rows 50 apart: every valid slot within the header's bound
    of float64 (pad columns at d = 100, one exact round at 128, the workload's width, a second 16-byte round at 1100); slots with idx = -1,
    idx < idx_base and idx - idx_base >= N give (-inf, -1); a NaN in a query row gives -1 in that query's valid slots; the outputs sit in
    sentinel-filled buffers and are written in every slot and nowhere else."""
    cs = _case(d, 300, 5)
    q, m, N, base, ld_idx = cs["q"][:nq].copy(), 44, 300, 3, 50
    rng = np.random.default_rng(d + nq)
    idx = np.full((nq, ld_idx), 123456, dtype=np.int64)
    idx[:, :m] = base + rng.integers(0, N, (nq, m))
    idx[:, 0], idx[:, 1] = base, base + N - 1
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 43] = -1, base - 1, base + N, base + N + 1000
    bad = np.zeros((nq, m), dtype=bool)
    bad[:, [5, 6, 7, 43]] = True
    u8 = _u8(cs)
    qd, idxd = torch.from_numpy(q).cuda(), torch.from_numpy(idx).cuda()
    guard = 64
    val = torch.full((nq * m + 2 * guard,), 7.0, device="cuda")
    out = torch.full((nq * m + 2 * guard,), -7, dtype=torch.int64, device="cuda")

    def call(qt):
        st = ctx.lib.sgpt_u8_rescore(ctx.handle, qt.data_ptr(), u8.codes.data_ptr(), u8.start.data_ptr(), u8.step.data_ptr(), nq, N, d,
                                     u8.codes.shape[1], idxd.data_ptr(), ld_idx, m, base, val[guard:].data_ptr(), out[guard:].data_ptr(), None)
        torch.cuda.synchronize()
        assert st == 0
        return val[guard:guard + nq * m].reshape(nq, m).cpu().numpy(), out[guard:guard + nq * m].reshape(nq, m).cpu().numpy()
    gv, gi = call(qd)
    assert (val[:guard] == 7.0).all() and (val[-guard:] == 7.0).all() and (out[:guard] == -7).all() and (out[-guard:] == -7).all()
    assert np.all(np.isneginf(gv[bad])) and np.all(gi[bad] == -1)
    assert np.array_equal(gi[~bad], idx[:, :m][~bad])
    rows = np.where(bad, 0, idx[:, :m] - base)
    want, bnd = np.take_along_axis(cs["vals"][:nq], rows, axis=1), np.take_along_axis(cs["bound"][:nq], rows, axis=1)
    err = np.abs(gv.astype(np.float64) - want)[~bad]
    print(f"d = {d}, nq = {nq}: max |value - float64| = {err.max():.3e}, smallest bound {bnd[~bad].min():.3e}")
    assert np.all(err <= bnd[~bad])
    # the wrapper gives the same bits; a NaN in the last query row: -1 in its valid slots, the other rows as before
    wv, wi = ctx.rescore_u8(qd, u8, idxd[:, :m], idx_base=base)
    assert np.array_equal(wv.cpu().numpy(), gv) and np.array_equal(wi.cpu().numpy(), gi)
    q[nq - 1, d // 2] = np.nan
    nv, ni = call(torch.from_numpy(q).cuda())
    assert np.all(nv[nq - 1][~bad[0]] == -1.0) and np.all(np.isneginf(nv[nq - 1][bad[0]]))
    assert np.array_equal(ni, gi) and np.array_equal(nv[:nq - 1], gv[:nq - 1])


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("nq", [1, 16, 64, 65])
@pytest.mark.parametrize("d", [128, 768])
def test_two_stage_against_the_reference(ctx, d, nq, centred):
    """2. k = 11 of kp = 44 candidates of 1 317 documents, idx_base = 3, bits centred on the corpus mean or not (65 queries: a second
    group of stage 1): indices inside the reference's candidates stage1(q - center), values within the bound of float64, the float64
    top-k of the candidates up to twice the bound, descending."""
    cs = _case(d)
    q = cs["q"][:nq]
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(cs, centred), 11, idx_base=3, rescore="uint8", rescore_multiplier=4)
    assert n == 11
    _, cand = B.stage1(BU.centred(q, cs["center"] if centred else None), cs["bits"][centred], d, 44, idx_base=3)
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, cs["vals"][:nq], cs["bound"][:nq], 11, idx_base=3)


@pytest.mark.parametrize("d", [128, 768])
def test_candidates_equal_those_of_score_topk_bits(ctx, d):
    """3. kp = k = 44 returns every candidate: as sets of indices per query they equal what sgpt_score_topk_bits (mode 1) returns for the
    matrix q - center on the same bits, and the reference's."""
    from sgpt_amd import BinaryCorpus
    cs = _case(d)
    q = cs["q"]
    _, iu, n = ctx.score_topk(torch.from_numpy(q), _corpus(cs, True), 44, idx_base=3, rescore="uint8", rescore_multiplier=1)
    plain = BinaryCorpus(torch.from_numpy(cs["bits"][True]).cuda(), d)
    _, isg, _ = ctx.score_topk(torch.from_numpy(q - cs["center"][None, :]), plain, 44, idx_base=3, rescore="sign", rescore_multiplier=1)
    _, cand = B.stage1(q - cs["center"][None, :], cs["bits"][True], d, 44, idx_base=3)
    assert n == 44
    assert np.array_equal(np.sort(iu.cpu().numpy(), axis=1), np.sort(isg.cpu().numpy(), axis=1))
    assert np.array_equal(np.sort(iu.cpu().numpy(), axis=1), np.sort(cand, axis=1))


def test_kp_1024_over_300_documents(ctx):
    """4. kp = 1024 > N = 300 (k = 320): all 300 documents come back ranked by value, n_out = min(k, N), the tail is (-inf, -1)."""
    cs = _case(128, 300, 5)
    q = cs["q"]
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(cs, True), 320, idx_base=3, rescore="uint8", rescore_multiplier=4)
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    assert n == 300 and np.all(np.isneginf(val[:, 300:])) and np.all(idx[:, 300:] == -1)
    cand = np.tile(np.arange(3, 303), (5, 1))
    B.check_rescored(val[:, :300], idx[:, :300], cand, cs["vals"], cs["bound"], 300, idx_base=3)
    assert np.all(np.sort(idx[:, :300], axis=1) == cand)


@pytest.mark.parametrize("centred", [False, True])
def test_running_list(ctx, centred):
    """5. The corpus in two calls, split at 700, idx_base advanced, the running list chained.
    a) 1 000 documents, k = 256, kp = 1024: every document is a candidate of both searches, and the two-call result equals the one-call
       result -- indices, and values bit for bit.
    b) 1 317 documents, k = 11, kp = 44: a two-stage search in two calls re-scores the 44 Hamming-best of EACH part, the one call the 44
       best of the whole, so the lists themselves differ (on the CPU reference too).  What holds, and is asserted: each result is exactly
       the top-k -- value descending, ties to the lowest index -- of its own candidates (the reference's, per part), taken on the values
       sgpt_u8_rescore gives for those documents, bit for bit: a document's value does not depend on the call that computed it."""
    d, base, split = 768, 3, 700
    cs = _case(d)
    q = torch.from_numpy(cs["q"][:16])
    sub = _corpus(cs, centred, slice(0, 1000))
    v1, i1, n1 = ctx.score_topk(q, sub, 256, idx_base=base, rescore="uint8", rescore_multiplier=4)
    va, ia, na = ctx.score_topk(q, _corpus(cs, centred, slice(0, split)), 256, idx_base=base, rescore="uint8", rescore_multiplier=4)
    vb, ib, nb = ctx.score_topk(q, _corpus(cs, centred, slice(split, 1000)), 256, idx_base=base + split, run=(va, ia, na), rescore="uint8",
                                rescore_multiplier=4)
    assert n1 == na == nb == 256
    assert torch.equal(i1, ib) and torch.equal(v1.view(torch.int32), vb.view(torch.int32))
    # b)
    every = torch.arange(base, base + N_DOCS, device="cuda").repeat(16, 1)
    allv, _ = ctx.rescore_u8(q, _u8(cs), every, idx_base=base)
    allv = allv.cpu().numpy()
    center = cs["center"] if centred else None
    qc, bits = BU.centred(cs["q"][:16], center), cs["bits"][centred]

    def top(cand):
        cv = np.take_along_axis(allv, cand - base, axis=1)
        o = np.lexsort((cand, -cv.astype(np.float64)), axis=1)[:, :11]
        return np.take_along_axis(cv, o, axis=1), np.take_along_axis(cand, o, axis=1)
    v1, i1, _ = ctx.score_topk(q, _corpus(cs, centred), 11, idx_base=base, rescore="uint8")
    va, ia, na = ctx.score_topk(q, _corpus(cs, centred, slice(0, split)), 11, idx_base=base, rescore="uint8")
    v2, i2, n2 = ctx.score_topk(q, _corpus(cs, centred, slice(split, None)), 11, idx_base=base + split, run=(va, ia, na), rescore="uint8")
    assert n2 == 11
    _, c_all = B.stage1(qc, bits, d, 44, idx_base=base)
    _, c_a = B.stage1(qc, bits[:split], d, 44, idx_base=base)
    _, c_b = B.stage1(qc, bits[split:], d, 44, idx_base=base + split)
    for (gv, gi), cand in (((v1, i1), c_all), ((v2, i2), np.concatenate([c_a, c_b], axis=1))):
        wv, wi = top(cand)
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gv.cpu().numpy().view(np.int32), wv.view(np.int32))


def test_calibration_ranges_narrower_than_the_data(ctx):
    """6. ranges= from the first 40 rows: later rows clamp at both ends, on the device as in the reference, and the search still matches
    the reference pipeline on those codes."""
    d = 128
    cs = _case(d)
    rows = ctx.l2_normalize(torch.from_numpy(cs["c"])).cpu().numpy()          # the rows binarize_corpus quantises
    rng = np.stack([rows[:40].min(axis=0), rows[:40].max(axis=0)])
    corpus = ctx.binarize_corpus(torch.from_numpy(cs["c"]), center="mean", keep_uint8=True, ranges=rng, block_rows=500)
    start, step = corpus.u8.start.cpu().numpy(), corpus.u8.step.cpu().numpy()
    assert np.array_equal(start[:d], rng[0]) and np.array_equal(step[:d], (rng[1] - rng[0]) / np.float32(255))
    codes = U.quantize_rows(rows, start, step)
    assert np.array_equal(corpus.u8.codes.cpu().numpy(), codes)
    outside = (rows < rng[0][None, :]) | (rows > rng[1][None, :])
    assert outside[40:].mean() > 0.01 and np.all(np.isin(codes[:, :d][outside], (0, 255)))
    center = corpus.center.cpu().numpy()
    bits = corpus.bits.cpu().numpy()
    assert np.array_equal(bits, B.pack(rows, center))
    q = cs["q"][:16]
    val, idx, n = ctx.score_topk(torch.from_numpy(q), corpus, 11, idx_base=3, rescore="uint8")
    _, cand = B.stage1(BU.centred(q, center), bits, d, 44, idx_base=3)
    vals = BU.values64(q, codes, start, step)
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, vals, BU.bound(q, codes, start, step, vals), 11, idx_base=3)


def test_python_layer_and_semantic_search(ctx):
    """7. binarize_corpus(keep_uint8=True, center="mean") round-trips (bits, codes and ranges equal the separate builders'; a calibration
    set and keep_fp8 beside it are accepted); semantic_search over it re-scores with the uint8 copy and equals
    score_topk(rescore="uint8"); a corpus without the copy refuses rescore="uint8" naming keep_uint8, and searches through
    semantic_search with the same `rescore` as before."""
    from sgpt_amd import BinaryCorpus, util
    d = 100
    cs = _case(d, 300, 5)
    emb, q = torch.from_numpy(cs["c"]), torch.from_numpy(cs["q"])
    corpus = util.quantize_embeddings(emb, precision="ubinary", center="mean", keep_uint8=True)
    assert isinstance(corpus, BinaryCorpus) and corpus.fp8 is None and corpus.u8 is not None and corpus.u8.dim == d and corpus.u8.normalized
    plain, u8 = ctx.binarize_corpus(emb, center="mean"), ctx.scalar_quantize_corpus(emb)
    assert torch.equal(corpus.bits, plain.bits) and torch.equal(corpus.center, plain.center)
    assert torch.equal(corpus.u8.codes, u8.codes) and torch.equal(corpus.u8.start, u8.start) and torch.equal(corpus.u8.step, u8.step)
    assert corpus.u8.codes.shape == (300, 128) and corpus.nbytes == plain.nbytes + u8.nbytes
    blocks = ctx.binarize_corpus(emb, center="mean", keep_uint8=True, block_rows=77)
    assert torch.equal(blocks.bits, corpus.bits) and torch.equal(blocks.u8.codes, corpus.u8.codes)
    cal = util.quantize_embeddings(emb, precision="ubinary", keep_uint8=True, keep_fp8=True, calibration_embeddings=emb[:50])
    want = ctx.scalar_quantize_corpus(emb, calibration_embeddings=emb[:50])
    assert cal.center is None and cal.fp8 is not None and torch.equal(cal.u8.codes, want.codes) and torch.equal(cal.u8.step, want.step)
    assert [util._binary_rescore(c) for c in (corpus, cal, plain)] == ["uint8", "uint8", "sign"]
    # semantic_search == score_topk(rescore="uint8") on the normalised queries, and follows the reference
    hits = util.semantic_search(q, corpus, top_k=10)
    val, idx, n = ctx.score_topk(ctx.l2_normalize(q), corpus, 10, rescore="uint8")
    assert n == 10 and [[e["corpus_id"] for e in h] for h in hits] == idx.cpu().tolist()
    assert [[e["score"] for e in h] for h in hits] == val.cpu().tolist()
    qn, rows = ctx.l2_normalize(q).cpu().numpy(), ctx.l2_normalize(emb).cpu().numpy()
    center, start, step = corpus.center.cpu().numpy(), corpus.u8.start.cpu().numpy(), corpus.u8.step.cpu().numpy()
    codes = corpus.u8.codes.cpu().numpy()
    assert np.array_equal(corpus.bits.cpu().numpy(), B.pack(rows, center)) and np.array_equal(codes, U.quantize_rows(rows, start, step))
    _, cand = B.stage1(BU.centred(qn, center), corpus.bits.cpu().numpy(), d, 40)
    vals = BU.values64(qn, codes, start, step)
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, vals, BU.bound(qn, codes, start, step, vals), 10)
    # a corpus as it is built today
    with pytest.raises(ValueError, match="keep_uint8"):
        ctx.score_topk(q, plain, 10, rescore="uint8")
    with pytest.raises(ValueError, match="rescore must be.*'uint8'"):
        ctx.score_topk(q, corpus, 10, rescore="int8")
    vs, is_, _ = ctx.score_topk(ctx.l2_normalize(q), plain, 10, rescore="sign")
    hp = util.semantic_search(q, plain, top_k=10)
    assert [[e["corpus_id"] for e in h] for h in hp] == is_.cpu().tolist() and [[e["score"] for e in h] for h in hp] == vs.cpu().tolist()
    with pytest.raises(ValueError, match="keep_uint8"):
        ctx.binarize_corpus(emb, ranges=np.zeros((2, d), dtype=np.float32))
    with pytest.raises(ValueError, match="embedding dims differ"):
        ctx.rescore_u8(q[:, :64], corpus.u8, torch.zeros((5, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="idx must be"):
        ctx.rescore_u8(q, corpus.u8, torch.zeros((4, 3), dtype=torch.int64))


def test_refusals_leave_the_outputs_untouched(ctx):
    """8. Every refusal of the two C entry points returns SGPT_ERR_INVALID with nothing launched -- sentinel-filled outputs stay as they
    were -- then one well-formed call of each goes through."""
    nq, N, d, ld, k, kp, m = 4, 300, 100, 128, 5, 20, 7
    q = torch.ones((nq, d), device="cuda")
    center = torch.zeros((d,), device="cuda")
    bits = torch.zeros((N, 16), dtype=torch.uint8, device="cuda")
    codes = torch.full((N + 1, ld), 128, dtype=torch.uint8, device="cuda")
    start, step = torch.zeros((ld,), device="cuda"), torch.zeros((ld,), device="cuda")
    cand = torch.zeros((nq, m), dtype=torch.int64, device="cuda")
    val = torch.full((nq, 8), 7.0, device="cuda")
    idx = torch.full((nq, 8), -7, dtype=torch.int64, device="cuda")
    n_out = C.c_int32(-3)

    def two(ctx_=ctx.handle, q_=q.data_ptr(), center_=center.data_ptr(), bits_=bits.data_ptr(), ldb=16, codes_=codes.data_ptr(),
            start_=start.data_ptr(), step_=step.data_ptr(), ld_=ld, d_=d, k_=k, kp_=kp, val_=val.data_ptr(), idx_=idx.data_ptr(), n_run=0):
        return ctx.lib.sgpt_score_topk_bits_u8(ctx_, q_, center_, bits_, ldb, codes_, start_, step_, ld_, nq, N, d_, k_, kp_, 0, val_, idx_,
                                               n_run, C.byref(n_out), None)

    def one(ctx_=ctx.handle, q_=q.data_ptr(), codes_=codes.data_ptr(), start_=start.data_ptr(), step_=step.data_ptr(), nq_=nq, N_=N, d_=d,
            ld_=ld, cand_=cand.data_ptr(), ld_idx=m, m_=m, val_=val.data_ptr(), idx_=idx.data_ptr()):
        return ctx.lib.sgpt_u8_rescore(ctx_, q_, codes_, start_, step_, nq_, N_, d_, ld_, cand_, ld_idx, m_, 0, val_, idx_, None)
    shared = [dict(ctx_=None), dict(q_=None), dict(codes_=None), dict(start_=None), dict(step_=None), dict(val_=None), dict(idx_=None),
              dict(ld_=100), dict(ld_=0), dict(ld_=192), dict(d_=129), dict(d_=0), dict(codes_=codes.data_ptr() + 8),
              dict(codes_=codes.data_ptr() + 1)]
    for kw in shared + [dict(bits_=None), dict(ldb=12), dict(ldb=18), dict(ldb=0), dict(k_=0), dict(k_=-1), dict(kp_=k - 1), dict(kp_=1025),
                        dict(k_=1025, kp_=1025), dict(n_run=-1), dict(n_run=k + 1)]:
        assert two(**kw) == -1, kw                           # SGPT_ERR_INVALID
    for kw in shared + [dict(cand_=None), dict(nq_=0), dict(N_=0), dict(m_=0), dict(m_=-1), dict(ld_idx=m - 1)]:
        assert one(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (val == 7.0).all() and (idx == -7).all() and n_out.value == -3
    assert two() == 0 and two(center_=None) == 0             # (the centre may be null)
    torch.cuda.synchronize()
    got_v, got_i = val.reshape(-1)[:nq * k].reshape(nq, k), idx.reshape(-1)[:nq * k].reshape(nq, k)     # (the call's lists are [nq, k])
    assert n_out.value == k and (got_v == 0).all() and got_i.tolist() == [list(range(k))] * nq               # code 128 under step 0: value 0
    assert one() == 0
    torch.cuda.synchronize()
    assert (val.reshape(-1)[:nq * m] == 0).all() and (idx.reshape(-1)[:nq * m] == 0).all()
