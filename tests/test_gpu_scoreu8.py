"""-m gpu: score and rank against a uint8 corpus with one range per dimension -- sgpt_score_topk_u8, score64c_kernel with the uint8 codec and the prologue /
row kernels (csrc/scoreu8.hip), Context.scalar_quantize_corpus / score_topk(Uint8Corpus), util.quantize_embeddings(precision="uint8")
/ semantic_search.

Score MATRICES are compared (k = N, scattered back by index), not lists, so that the ties the fma makes cannot hide behind tie order.
Exact where the arithmetic is exact (the integer probe, equality with the f16 scorer on the rows codes - 128 followed by the same fma,
the row kernels); the two derived bounds of tests/scoreu8_ref.py elsewhere."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import score8_ref as R8
import scoreu8_ref as R
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _uc(codes, start, step, dim, normalized=True):
    from sgpt_amd import Uint8Corpus
    return Uint8Corpus(torch.as_tensor(codes).cuda().contiguous(), torch.as_tensor(start).float().cuda().contiguous(),
                       torch.as_tensor(step).float().cuda().contiguous(), normalized, dim)


def _all_scores(ctx, q, corpus, **kw):
    """The materialised score matrix [nq, N] through the public call: k = N, scattered back by index."""
    N = len(corpus)
    val, idx, n = ctx.score_topk(q, corpus, N, **kw)
    assert n == N and sorted(idx[0].tolist()) == list(range(N))
    return torch.zeros_like(val).scatter_(1, idx, val), val, idx


@pytest.mark.parametrize("nq", [1, 33, 64])
@pytest.mark.parametrize("d", [128, 384])
def test_layout_probe_is_exact(ctx, d, nq):
    """1. Small-integer codes in an ASYMMETRIC pattern against integer-valued queries, step = 1 and start = -128 (so x^ = code - 128 and
    qbias = 0): every product and sum is exact and qscale is a power of two, so a swapped byte / lane / k-chunk / document of the
    conversion, the fragment or the epilogue map fails bit for bit."""
    N = 512
    ci = (torch.arange(N)[:, None] * 7 + torch.arange(d)[None, :] * 11) % 13 - 6
    qi = (torch.arange(nq)[:, None] * 5 + torch.arange(d)[None, :] * 3) % 9 - 4
    corpus = _uc((ci + 128).to(torch.uint8), torch.full((d,), -128.0), torch.ones(d), d, normalized=False)
    got, _, _ = _all_scores(ctx, qi.float().cuda(), corpus)
    assert torch.equal(got.cpu(), qi.float() @ ci.float().T)
    # and every one of the 256 codes, in every byte position (sums stay below 2^24: still exact)
    ca = (torch.arange(N)[:, None] * 7 + torch.arange(d)[None, :] * 11) % 256 - 128
    corpus = _uc((ca + 128).to(torch.uint8), torch.full((d,), -128.0), torch.ones(d), d, normalized=False)
    got, _, _ = _all_scores(ctx, qi.float().cuda(), corpus)
    assert torch.equal(got.cpu(), qi.float() @ ca.float().T)


_cases = {}


def _case(ctx, N, d):
    """Unit rows around a common offset (tests/score8_ref.py), quantised on the device; 64 unit queries; the prologue's outputs; the
    uint8 scorer's score matrices for nq = 1 and 64.  Built once per shape and left unchanged."""
    if (N, d) not in _cases:
        q, c = R8.unit_corpus(N + d, max(N, 300), d, 64)
        corpus = ctx.scalar_quantize_corpus(c, normalize=False)      # (ranges of all max(N, 300) rows: one row alone has none)
        from sgpt_amd import Uint8Corpus
        corpus = Uint8Corpus(corpus.codes[:N].contiguous(), corpus.start, corpus.step, False, d)
        q = q.cuda()
        prep = {nq: ctx.u8_prepare_queries(q[:nq], corpus.start, corpus.step) for nq in (1, 64)}
        got = {nq: _all_scores(ctx, q[:nq], corpus)[0] for nq in (1, 64)}
        _cases[(N, d)] = (corpus, q, prep, got)
    return _cases[(N, d)]


SHAPES = [(N, d) for d in (128, 768) for N in (1, 255, 256, 257, 1000)] + [(257, 200)]      # (d = 200: 56 pad columns)


@pytest.mark.parametrize("nq", [1, 64])
@pytest.mark.parametrize("N,d", SHAPES)
def test_equals_the_f16_scorer_then_the_fma(ctx, N, d, nq):
    """2. The f16 scorer on the f16 rows codes - 128 against the prologue's q'', then val * qscale + qbias in fp32 (the product is exact,
    the sum rounds once: the kernel's fma): equal to the uint8 scorer's matrix bit for bit -- whole tiles, ragged tiles, one document."""
    corpus, q, prep, got = _case(ctx, N, d)
    q2, qscale, qbias = prep[nq]
    rows16 = (corpus.codes.to(torch.int16) - 128).to(torch.float16)
    val, idx, n = ctx.score_topk(q2[:nq].contiguous(), rows16, N, dtype=torch.float16)
    assert n == N
    raw = torch.zeros_like(val).scatter_(1, idx, val)
    want = raw * qscale[:nq, None] + qbias[:nq, None]
    assert torch.equal(got[nq], want)
    # the prologue itself: q'' and qscale are the reference's bit for bit, qbias within its fp32 accumulation (d roundings)
    w2, ws, wb = R.prepare_queries(q[:nq].cpu().numpy(), corpus.start.cpu().numpy(), corpus.step.cpu().numpy())
    assert np.array_equal(q2[:nq].cpu().numpy().view(np.uint16), w2.view(np.uint16)) and (q2[nq:] == 0).all()
    assert np.array_equal(qscale[:nq].cpu().numpy(), ws) and (qscale[nq:] == 1).all() and (qbias[nq:] == 0).all()
    mid = corpus.start.double() + 128 * corpus.step.double()
    lim = d * 2.0 ** -24 * (q[:nq].double().abs() @ mid[:d].abs()).cpu().numpy() + 1e-30
    assert np.all(np.abs(qbias[:nq].cpu().numpy().astype(np.float64) - wb) <= lim)


@pytest.mark.parametrize("nq", [1, 64])
@pytest.mark.parametrize("N,d", SHAPES)
def test_arithmetic_bound_against_float64(ctx, N, d, nq):
    """3. Independent of the f16 kernel: every score within d 2^-23 qscale sum|q''_j c_j| + 2^-23 |score| of the float64 score of the
    same q'', qscale, qbias and codes."""
    corpus, q, prep, got = _case(ctx, N, d)
    q2, qscale, qbias = (t[:nq].cpu().numpy() for t in prep[nq])
    codes = corpus.codes.cpu().numpy()
    exact = R.exact_scores(q2, qscale, qbias, codes)
    err = np.abs(got[nq].cpu().numpy().astype(np.float64) - exact)
    bound = R.arithmetic_bound(q2, qscale, codes, exact, d)
    print(f"N={N} d={d} nq={nq}: max |score - float64| = {err.max():.3e}, smallest bound = {bound.min():.3e}")
    assert np.all(err <= bound)


_big = {}


def _big_case(ctx):
    """262 144 + 77 documents x 128, 16 queries: the smallest shard the planner filters at nq = 16 (tests/test_score_plan_u8.py)."""
    if not _big:
        N, d = 262_144 + 77, 128
        g = torch.Generator(device="cuda").manual_seed(4)
        q = torch.nn.functional.normalize(torch.randn(16, d, device="cuda", generator=g), dim=1)
        base = torch.randn(1, d, device="cuda", generator=g) * 2
        c = torch.nn.functional.normalize(base + torch.randn(N + 700, d, device="cuda", generator=g), dim=1)
        every = ctx.scalar_quantize_corpus(c, normalize=False)
        from sgpt_amd import Uint8Corpus
        _big["prev"] = Uint8Corpus(every.codes[:700].contiguous(), every.start, every.step, False, d)
        _big["corpus"] = Uint8Corpus(every.codes[700:].contiguous(), every.start, every.step, False, d)
        _big["q"] = q
    return _big["corpus"], _big["prev"], _big["q"]


def _sliced(ctx, q, corpus, k, idx_base, run):
    """The materialise-and-select route (test 2's) over the same documents: calls short enough that the planner filters none."""
    from sgpt_amd import Uint8Corpus
    for s in range(0, len(corpus), 100_000):
        part = Uint8Corpus(corpus.codes[s:s + 100_000], corpus.start, corpus.step, corpus.normalized, corpus.dim)
        run = ctx.score_topk(q, part, k, idx_base=idx_base + s, run=run)
    return run


@pytest.mark.parametrize("running", [False, True], ids=["fresh", "running"])
def test_filtered_route_equals_the_materialised_one(ctx, running):
    """4. N = 262 144 + 77, d = 128, k = 11, nq = 16: sampled thresholds, filtered launches, the 77-document tail riding in the last of
    them -- values and indices equal to the materialise-and-select route's, fresh and with a running list; no list overflowed; and the
    values are within the arithmetic bound of float64."""
    corpus, prev, q = _big_case(ctx)
    k, N = 11, len(corpus)
    run, base = None, 5
    if running:
        v0, i0, n0 = ctx.score_topk(q, prev, k, idx_base=0)
        run, base = (v0.clone(), i0.clone(), n0), 700
        val, idx, n = ctx.score_topk(q, corpus, k, idx_base=base, run=(v0, i0, n0))
    else:
        val, idx, n = ctx.score_topk(q, corpus, k, idx_base=base)
    chunks, over = ctx.score_overflow_count()
    assert chunks >= 1 and over == 0
    wv, wi, wn = _sliced(ctx, q, corpus, k, base, run)
    assert n == wn == k
    assert torch.equal(val, wv) and torch.equal(idx, wi)
    if not running:
        q2, qscale, qbias = (t[:16].cpu().numpy() for t in ctx.u8_prepare_queries(q, corpus.start, corpus.step))
        got_idx = idx.cpu().numpy() - base
        assert got_idx.min() >= 0 and got_idx.max() < N
        for r in range(16):
            codes = corpus.codes[torch.as_tensor(got_idx[r]).cuda()].cpu().numpy()
            exact = R.exact_scores(q2[r:r + 1], qscale[r:r + 1], qbias[r:r + 1], codes)
            bound = R.arithmetic_bound(q2[r:r + 1], qscale[r:r + 1], codes, exact, 128)
            assert np.all(np.abs(val[r].cpu().numpy().astype(np.float64) - exact[0]) <= bound[0])


def test_tail_documents_are_found_by_the_filtered_launch(ctx):
    """4b. The same shard with its best documents placed in the ragged tail: the filtered launch that carries the tail appends them."""
    corpus, prev, q = _big_case(ctx)
    from sgpt_amd import Uint8Corpus
    k, N = 11, len(corpus)
    v0, i0, _ = ctx.score_topk(q[:1], corpus, k)
    codes = corpus.codes.clone()
    best = codes[i0[0, :5]].clone()
    codes[N - 5:] = best                                      # copies of query 0's five best documents, at the very end
    moved = Uint8Corpus(codes, corpus.start, corpus.step, False, corpus.dim)
    val, idx, n = ctx.score_topk(q, moved, k)
    wv, wi, wn = _sliced(ctx, q, moved, k, 0, None)
    assert torch.equal(val, wv) and torch.equal(idx, wi)
    assert set(range(N - 5, N)) <= set(idx[0].tolist())


@pytest.mark.parametrize("running", [False, True], ids=["fresh", "running"])
def test_overflow_fallback(ctx, running):
    """5. One row repeated 262 221 times: every score of a query ties, every document passes the inclusive threshold, the candidate lists
    overflow and the predicated materialise + select recomputes the chunk -- the reference order (ties to the lowest index), and
    sgpt_score_overflow_count reports it."""
    nq, d, k, N = 16, 128, 10, 262_144 + 77
    g = torch.Generator(device="cpu").manual_seed(21)
    row = torch.randint(0, 256, (1, d), generator=g).to(torch.uint8)
    start, step = torch.randn(d, generator=g) * 0.1, torch.rand(d, generator=g) * 1e-3 + 1e-4
    corpus = _uc(row.expand(N, d), start, step, d, normalized=False)
    q = torch.randn(nq, d, generator=g).cuda()
    one = _all_scores(ctx, q, _uc(row.expand(4, d), start, step, d, normalized=False))[0][:, 0]
    if running:
        lower = _uc((row.to(torch.int16).clamp(1, 255) - 1).to(torch.uint8).expand(300, d), start, step, d, normalized=False)
        v0, i0, n0 = ctx.score_topk(q, lower, k, idx_base=0)
        val, idx, n = ctx.score_topk(q, corpus, k, idx_base=300, run=(v0.clone(), i0.clone(), n0))
        chunks, over = ctx.score_overflow_count()            # (of the last pass: read before the reference's passes)
        wv, wi, wn = _sliced(ctx, q, corpus, k, 300, (v0, i0, n0))
    else:
        val, idx, n = ctx.score_topk(q, corpus, k)
        chunks, over = ctx.score_overflow_count()
        wv, wi, wn = None, None, k
    assert chunks >= 1 and over >= 1
    assert n == wn == k
    if running:
        assert torch.equal(val, wv) and torch.equal(idx, wi)
    else:
        assert torch.equal(idx.cpu(), torch.arange(k).expand(nq, k)) and torch.equal(val, one[:, None].expand(nq, k))


@pytest.mark.parametrize("nq", [65, 130])
def test_query_groups_equal_the_per_group_calls(ctx, nq):
    """6. More than 64 queries run in groups of 64, each re-streaming the codes: the groups' lists are the per-group calls' lists, with a
    running list chained per group."""
    N, d, k = 1000, 128, 11
    corpus, _, _, _ = _case(ctx, N, d)
    g = torch.Generator(device="cpu").manual_seed(nq)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1).cuda()
    from sgpt_amd import Uint8Corpus
    head = Uint8Corpus(corpus.codes[:300].contiguous(), corpus.start, corpus.step, False, d)
    tail = Uint8Corpus(corpus.codes[300:].contiguous(), corpus.start, corpus.step, False, d)
    val, idx, n = ctx.score_topk(q, corpus, k, idx_base=3)
    v1, i1, n1 = ctx.score_topk(q, head, k, idx_base=3)
    v2, i2, n2 = ctx.score_topk(q, tail, k, idx_base=303, run=(v1, i1, n1))
    assert n == n2 == k and torch.equal(v2, val) and torch.equal(i2, idx)
    for g0 in range(0, nq, 64):
        wv, wi, wn = ctx.score_topk(q[g0:g0 + 64].contiguous(), corpus, k, idx_base=3)
        assert wn == k and torch.equal(val[g0:g0 + 64], wv) and torch.equal(idx[g0:g0 + 64], wi)
    # any float dtype is upcast; a dtype argument is refused
    v16, i16, _ = ctx.score_topk(q.to(torch.float16), corpus, k, idx_base=3)
    w16, j16, _ = ctx.score_topk(q.to(torch.float16).float(), corpus, k, idx_base=3)
    assert torch.equal(v16, w16) and torch.equal(i16, j16)
    with pytest.raises(ValueError, match="dtype must be None"):
        ctx.score_topk(q, corpus, k, dtype=torch.float16)
    with pytest.raises(ValueError, match="embedding dims differ"):
        ctx.score_topk(q[:, :64], corpus, k)


def test_row_kernels(ctx):
    """7. Column min / max exact (blocks chained, NaN-propagating); the quantiser against the float64 rule -- where the float64 quotient
    is within 1e-4 of a half-integer either neighbour is accepted, and such elements are at most 0.1 % of all (a uniform fraction gives
    0.02 %); clamps, a constant column, a NaN element, pad columns; de-quantise exact in fp32 and one rounding more in f16 / bf16."""
    n, d = 3000, 200
    x = R.row_kernel_case(11, n, d)                           # (column 17 is constant: step == 0)
    xt = torch.from_numpy(x).cuda()
    run = ctx.u8_col_minmax(xt[:1000])
    run = ctx.u8_col_minmax(xt[1000:1001], run)
    mn, mx = ctx.u8_col_minmax(xt[1001:], run)
    assert np.array_equal(mn.cpu().numpy(), x.min(axis=0)) and np.array_equal(mx.cpu().numpy(), x.max(axis=0))
    xn = xt.clone()
    xn[5, 3] = float("nan")
    xn[2999, 199] = float("nan")
    mn2, mx2 = ctx.u8_col_minmax(xn)
    nan_cols = torch.zeros(d, dtype=torch.bool)
    nan_cols[[3, 199]] = True
    assert torch.equal(torch.isnan(mn2).cpu(), nan_cols) and torch.equal(torch.isnan(mx2).cpu(), nan_cols)
    assert torch.equal(mn2[~nan_cols.cuda()], mn[~nan_cols.cuda()]) and torch.equal(mx2[~nan_cols.cuda()], mx[~nan_cols.cuda()])
    with pytest.raises(ValueError, match="not finite"):
        ctx.scalar_quantize_corpus(xn, normalize=False)
    with pytest.raises(ValueError, match="not finite"):
        ctx.scalar_quantize_corpus(xt, normalize=False, ranges=np.stack([np.full(d, -np.inf), np.ones(d)]))
    # ranges from every third row: the rest clamps
    corpus = ctx.scalar_quantize_corpus(xn, normalize=False, calibration_embeddings=xt[::3], block_rows=1024)
    start, step = R.ranges(x[::3])
    assert corpus.codes.shape == (n, 256) and np.array_equal(corpus.start.cpu().numpy(), start) and np.array_equal(corpus.step.cpu().numpy(), step)
    codes = corpus.codes.cpu().numpy()
    t64 = R.quotient64(xn.cpu().numpy(), start, step)
    live = np.isfinite(t64)
    want = np.where(live, np.clip(np.rint(np.where(live, t64, 0)), 0, 255), 128).astype(np.uint8)
    near = R.near_half(t64)
    other = np.where(live, np.clip(np.where(np.rint(np.where(live, t64, 0)) > np.where(live, t64, 0), np.floor(np.where(live, t64, 0)),
                                            np.ceil(np.where(live, t64, 0))), 0, 255), 128).astype(np.uint8)
    print(f"quantiser: {near.sum()} of {near.size} elements within 1e-4 of a half step, {(codes[:, :d] != want).sum()} codes take the other neighbour")
    assert near.mean() <= 1e-3
    ok = (codes[:, :d] == want) | (near & (codes[:, :d] == other))
    assert ok.all()
    assert (codes[:, 17] == 128).all() and codes[5, 3] == 128 and codes[2999, 199] == 128 and (codes[:, d:] == 128).all()
    assert (codes[:, :d] == 0).any() and (codes[:, :d] == 255).any()
    assert np.array_equal(codes, R.quantize_rows(xn.cpu().numpy(), start, step))         # (and numpy's fp32 gives the same codes)
    deq = corpus.dequantize(torch.float32)
    w32 = R.dequantize32(codes, start, step)
    assert np.array_equal(deq.cpu().numpy(), w32)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(corpus.dequantize(dt).cpu(), torch.from_numpy(w32).to(dt))
    assert corpus.nbytes == n * 256 + 2 * 256 * 4 and len(corpus) == n and corpus.dim == d
    assert torch.equal(corpus.codes_int8().cpu(), torch.from_numpy(codes[:, :d].astype(np.int16) - 128).to(torch.int8))


def test_refusals_leave_the_outputs_untouched(ctx):
    """8. Every refusal of the C entry point returns SGPT_ERR_INVALID with nothing launched: sentinel-filled outputs stay as they were."""
    nq, N, d, ld, k = 4, 300, 100, 128, 5
    q = torch.zeros((65, d), device="cuda")
    codes = torch.full((N * ld + 16,), 128, dtype=torch.uint8, device="cuda")
    start, step = torch.zeros(ld, device="cuda"), torch.zeros(ld, device="cuda")
    val = torch.full((65, k), 7.0, device="cuda")
    idx = torch.full((65, k), -7, dtype=torch.int64, device="cuda")
    n_out = C.c_int32(-3)

    def call(q_=q.data_ptr(), codes_=codes.data_ptr(), start_=start.data_ptr(), step_=step.data_ptr(), nq_=nq, d_=d, ld_=ld, k_=k,
             val_=val.data_ptr(), idx_=idx.data_ptr(), n_run=0):
        return ctx.lib.sgpt_score_topk_u8(ctx.handle, q_, codes_, start_, step_, nq_, N, d_, ld_, k_, 0, val_, idx_, n_run, C.byref(n_out), None)
    bad = [dict(nq_=65), dict(nq_=0), dict(ld_=120), dict(ld_=64), dict(d_=129), dict(d_=0), dict(codes_=codes.data_ptr() + 4),
           dict(codes_=codes.data_ptr() + 8), dict(n_run=k + 1), dict(n_run=-1), dict(k_=0), dict(q_=None), dict(codes_=None), dict(start_=None),
           dict(step_=None), dict(val_=None), dict(idx_=None)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # SGPT_ERR_INVALID
    torch.cuda.synchronize()
    assert (val == 7.0).all() and (idx == -7).all() and n_out.value == -3
    assert call() == 0                                       # (and the well-formed call goes through)
    torch.cuda.synchronize()
    assert n_out.value == k and (val[:nq] == 0).all() and (val[nq:] == 7.0).all()
    assert torch.equal(idx[:nq].cpu(), torch.arange(k).expand(nq, k))
    # the stand-alone entries refuse the same shapes
    out = torch.full((N, ld), 9, dtype=torch.uint8, device="cuda")
    x = torch.zeros((N, d), device="cuda")
    assert ctx.lib.sgpt_u8_quantize_rows(ctx.handle, x.data_ptr(), N, d, 120, start.data_ptr(), step.data_ptr(), out.data_ptr(), None) == -1
    assert ctx.lib.sgpt_u8_quantize_rows(ctx.handle, x.data_ptr(), N, 129, ld, start.data_ptr(), step.data_ptr(), out.data_ptr(), None) == -1
    assert ctx.lib.sgpt_u8_dequantize_rows(ctx.handle, out.data_ptr(), N, 120, start.data_ptr(), step.data_ptr(), x.data_ptr(), 0, None) == -1
    assert ctx.lib.sgpt_u8_prepare_queries(ctx.handle, q.data_ptr(), start.data_ptr(), step.data_ptr(), 65, d, ld, out.data_ptr(),
                                           val.data_ptr(), val.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (out == 9).all()


def test_quantisation_bound_against_the_unquantised_fixture(ctx):
    """9. The embeddings of tests/golden/scoring.npz (700 x 96 corpus, 13 queries, anisotropic), through the public call: every cosine
    score from the uint8 corpus within sum |q_j| step_j / 2 of the fp32 rows' score.  Reported beside the fp8 corpus's figures on the same
    rows (CPU references: uint8 max |dcos| 5.8e-3, top-10 overlap 0.97; fp8 4.2e-2, 0.80)."""
    fx = np.load(f"{GOLDEN}/scoring.npz")
    meta = json.loads(str(fx["es_json"]))
    cn = torch.nn.functional.normalize(torch.from_numpy(fx["es_corpus_emb"]), dim=1)
    qn = torch.nn.functional.normalize(torch.from_numpy(fx["es_query_emb"]), dim=1)
    uc = ctx.scalar_quantize_corpus(cn, normalize=False)      # (the rows are unit rows already: these are the rows the bound speaks of)
    assert uc.codes.shape == (700, 128) and uc.dim == 96
    s32 = qn.numpy().astype(np.float64) @ cn.numpy().astype(np.float64).T
    want = meta["results"]["cos_sim"]

    def report(name, corpus, q):
        got, val, idx = _all_scores(ctx, q, corpus)
        err = np.abs(got.cpu().numpy().astype(np.float64) - s32)
        overlap = []
        for r, qid in enumerate(meta["queries"]):
            mine = [f"d{i}" for i in idx[r].tolist() if f"d{i}" != qid][:10]
            ref10 = sorted(want[qid], key=want[qid].get, reverse=True)[:10]
            overlap.append(len(set(mine) & set(ref10)) / len(ref10))
        print(f"{name} corpus vs fp32: max |dcos| = {err.max():.3e}, top-10 overlap with the fixture's ranking = {np.mean(overlap):.4f}")
        return err
    err = report("uint8", uc, qn.cuda())
    report("fp8", ctx.quantize_corpus(cn, normalize=True), qn.cuda().to(torch.float16))
    assert np.all(err <= R.quantisation_bound(qn.numpy(), cn.numpy(), uc.start.cpu().numpy(), uc.step.cpu().numpy()))


def test_semantic_search_with_a_uint8_corpus(ctx):
    """10. util.semantic_search over util.quantize_embeddings(docs, precision="uint8"): the reference's result contract (per query a list
    of {'corpus_id', 'score'} by decreasing score), the index set of the float64 reference on the same q'', qscale, qbias and codes
    outside score gaps smaller than the arithmetic bound, every score within that bound; the overlap with the fp32 golden lists is
    reported.  The fixture's width, 100, is no multiple of 128: the codes carry 28 pad columns."""
    from sgpt_amd import Uint8Corpus, util
    fx = np.load(f"{GOLDEN}/scoring.npz")
    q, docs = torch.from_numpy(fx["ss_q"]), torch.from_numpy(fx["ss_docs"])
    corpus = util.quantize_embeddings(docs, precision="uint8")
    assert isinstance(corpus, Uint8Corpus) and len(corpus) == 1000 and corpus.codes.shape == (1000, 128) and corpus.dim == 100 and corpus.normalized
    assert (corpus.codes[:, 100:] == 128).all() and (corpus.start[100:] == 0).all() and (corpus.step[100:] == 0).all()
    hits = util.semantic_search(q, corpus, top_k=10, query_chunk_size=5, corpus_chunk_size=17)
    assert len(hits) == 20 and all(len(h) == 10 for h in hits)
    assert all(h[i]["score"] >= h[i + 1]["score"] for h in hits for i in range(9))
    q2, qscale, qbias = (t[:20].cpu().numpy() for t in ctx.u8_prepare_queries(ctx.l2_normalize(q), corpus.start, corpus.step))
    codes = corpus.codes.cpu().numpy()
    ref = R.exact_scores(q2, qscale, qbias, codes)
    bound = R.arithmetic_bound(q2, qscale, codes, ref, 100)
    _, wi = R.topk_lowest_index(ref, 10)
    for r in range(20):
        got, want = [h["corpus_id"] for h in hits[r]], set(wi[r].tolist())
        for h in hits[r]:
            assert abs(h["score"] - ref[r, h["corpus_id"]]) <= bound[r, h["corpus_id"]]
        for a in set(got) - want:                            # a swap is allowed only between scores closer than twice the bound
            assert all(abs(ref[r, a] - ref[r, b]) < 2 * max(bound[r, a], bound[r, b]) for b in want - set(got))
    same = np.mean([len(set(h["corpus_id"] for h in a) & set(b)) / 10 for a, b in zip(hits, fx["ss_idx"].tolist())])
    print(f"semantic_search, uint8 corpus: top-10 overlap with the fp32 golden lists = {same:.4f}")
    # ranges given as sentence-transformers gives them ([2, d]: min row, max row) reproduce the corpus; dot scores need normalize=False
    dn = ctx.l2_normalize(docs)
    again = util.quantize_embeddings(docs, precision="uint8", ranges=torch.stack([dn.min(dim=0).values, dn.max(dim=0).values]).cpu().numpy())
    assert torch.equal(again.codes, corpus.codes) and torch.equal(again.start, corpus.start) and torch.equal(again.step, corpus.step)
    cd = util.quantize_embeddings(docs, precision="uint8", normalize=False, calibration_embeddings=docs[:500])
    hd = util.semantic_search(q, cd, top_k=3, score_function=util.dot_score)
    dv, di, _ = ctx.score_topk(q.cuda(), cd, 3)
    assert [[h["corpus_id"] for h in r] for r in hd] == di.cpu().tolist() and [[h["score"] for h in r] for r in hd] == dv.cpu().tolist()
