"""-m gpu: score and rank against an fp8 (e4m3fn) corpus -- sgpt_score_topk_q8, score64c_kernel with the fp8 codec (csrc/score8.hip), the composed
route, Context.quantize_corpus / score_topk(QuantizedCorpus), util.quantize_embeddings / semantic_search.

Exact where the arithmetic is exact (integer probes, subnormal / NaN codes, equality with the f16 scorer on the de-quantised rows);
the two derived bounds of tests/score8_ref.py elsewhere."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import score8_ref as R
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _qc(codes, scale, normalized=True):
    from sgpt_amd import QuantizedCorpus
    return QuantizedCorpus(torch.as_tensor(codes).cuda().contiguous(), torch.as_tensor(scale).float().cuda().contiguous(), normalized)


def _all_scores(ctx, q, corpus, **kw):
    """The materialised score matrix [nq, N] through the public call: k = N, scattered back by index."""
    N = len(corpus)
    val, idx, n = ctx.score_topk(q, corpus, N, **kw)
    assert n == N and sorted(idx[0].tolist()) == list(range(N))
    return torch.zeros_like(val).scatter_(1, idx, val), val, idx


_corpora = {}


def _unit_case(ctx, N, d):
    """(fp8 corpus, its f16 de-quantisation, 64 f16 unit queries) of unit rows around a common offset, built once per shape."""
    if (N, d) not in _corpora:
        if N < 10_000:
            q, c = R.unit_corpus(N + d, N, d, 64)
            q, c = q.cuda(), c.cuda()
        else:
            g = torch.Generator(device="cuda").manual_seed(N + d)
            q = torch.nn.functional.normalize(torch.randn(64, d, device="cuda", generator=g), dim=1)
            base = torch.randn(1, d, device="cuda", generator=g) * 2
            c = torch.nn.functional.normalize(base + torch.randn(N, d, device="cuda", generator=g), dim=1)
        qc = ctx.quantize_corpus(c, normalize=True)
        _corpora[(N, d)] = (qc, qc.dequantize(torch.float16), q.to(torch.float16))
    return _corpora[(N, d)]


@pytest.mark.parametrize("nq", [1, 33, 64])
@pytest.mark.parametrize("d", [128, 384])
def test_layout_probe_is_exact(ctx, d, nq):
    """1. Small-integer codes in an ASYMMETRIC pattern against integer-valued f16 queries, scales 1: every product and sum is exact, so a
    swapped byte / lane / k-chunk / document of the fragment or epilogue map fails bit for bit."""
    N = 256 * 3
    ci = (torch.arange(N)[:, None] * 7 + torch.arange(d)[None, :] * 11) % 13 - 6
    qi = (torch.arange(nq)[:, None] * 5 + torch.arange(d)[None, :] * 3) % 9 - 4
    corpus = _qc(ci.float().to(torch.float8_e4m3fn).view(torch.uint8), torch.ones(N))
    got, _, _ = _all_scores(ctx, qi.to(torch.float16).cuda(), corpus)
    assert torch.equal(got.cpu(), qi.float() @ ci.float().T)


def test_subnormal_and_nan_codes_are_exact(ctx):
    """2. Rows of e4m3 SUBNORMAL codes only, a row with a NaN code, a zero row -- in the streamed tiles and in the ragged tail -- among
    small-integer rows, under scales 1, 2^-3 and 4; queries are multiples of 2^-6.  Every product and sum is exact: scores equal the
    float64 reference, the NaN rows score -1 and rank where -1 ranks (ties to the lowest index)."""
    d, nq, N = 128, 5, 256 * 2 + 5
    g = torch.Generator(device="cpu").manual_seed(2)
    codes = torch.randint(-6, 7, (N, d), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
    sub = torch.randint(1, 8, (N, d), generator=g).to(torch.uint8) | (torch.randint(0, 2, (N, d), generator=g).to(torch.uint8) << 7)
    for r in (3, 100, 300, 511, 513):                        # subnormal codes 0x01 .. 0x07, either sign
        codes[r] = sub[r]
    for r, col, code in ((7, 5, 0x7f), (260, 127, 0xff), (515, 0, 0x7f)):
        codes[r, col] = code
    codes[9] = 0
    codes[514] = 0
    scale = torch.tensor([1.0, 0.125, 4.0])[torch.arange(N) % 3]
    q = (torch.randint(-256, 257, (nq, d), generator=g).float() / 64).to(torch.float16)
    want = R.scores64(q.numpy(), R.dequantize(codes.numpy(), scale.numpy()))
    wv, wi = R.topk_lowest_index(want, N, idx_base=10)
    got, val, idx = _all_scores(ctx, q.cuda(), _qc(codes, scale, normalized=False), idx_base=0)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
    assert (got[:, [7, 260, 515]] == -1).all() and (got[:, [9, 514]] == 0).all()
    val, idx, _ = ctx.score_topk(q.cuda(), _qc(codes, scale, normalized=False), N, idx_base=10)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy().astype(np.float64), wv)


@pytest.mark.parametrize("N", [256 * 5 + 37, 300_005])
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("nq", [1, 16, 64])
def test_equals_the_f16_scorer_on_the_dequantised_corpus(ctx, nq, d, N):
    """3. The streaming kernel against the f16 scorer on corpus.dequantize(f16): values and indices torch.equal -- one chunk + ragged
    tail (small N), sampled thresholds + filtered chunks (large N), and a two-call running merge."""
    k = 11
    qc, deq, q = _unit_case(ctx, N, d)
    q = q[:nq].contiguous()
    val, idx, n = ctx.score_topk(q, qc, k, idx_base=3)
    wv, wi, wn = ctx.score_topk(q, deq, k, idx_base=3, dtype=torch.float16)
    assert n == wn == k
    assert torch.equal(val, wv) and torch.equal(idx, wi)
    from sgpt_amd import QuantizedCorpus
    cut = 70_000 if N > 70_000 else 700
    v1, i1, n1 = ctx.score_topk(q, QuantizedCorpus(qc.codes[:cut], qc.scale[:cut]), k, idx_base=3)
    v2, i2, n2 = ctx.score_topk(q, QuantizedCorpus(qc.codes[cut:], qc.scale[cut:]), k, idx_base=3 + cut, run=(v1, i1, n1))
    assert n2 == k and torch.equal(v2, val) and torch.equal(i2, idx)


@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("nq", [1, 16, 64])
def test_arithmetic_bound_against_float64(ctx, nq, d):
    """4. Independent of the f16 kernel: every returned value within d 2^-23 sum|q_i c_i| of the float64 score of the returned index,
    and the returned set is the float64 top-k except where the float64 scores in question differ by less than twice that bound."""
    N, k = 256 * 5 + 37, 11
    q, c = R.unit_corpus(nq, N, d, nq)
    qc = ctx.quantize_corpus(c.cuda(), normalize=True)
    q16 = q.to(torch.float16)
    rows = R.dequantize(qc.codes.cpu().numpy(), qc.scale.cpu().numpy())
    ref, bound = R.scores64(q16.numpy(), rows), R.arithmetic_bound(q16.numpy(), rows)
    val, idx, n = ctx.score_topk(q16.cuda(), qc, k)
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    err = np.abs(val - np.take_along_axis(ref, idx, axis=1))
    lim = np.take_along_axis(bound, idx, axis=1)
    print(f"nq={nq} d={d}: max |score - float64| = {err.max():.3e}, smallest bound = {lim.min():.3e}")
    assert n == k and np.all(err <= lim)
    _, wi = R.topk_lowest_index(ref, k)
    for r in range(nq):
        got, want = set(idx[r].tolist()), set(wi[r].tolist())
        for a in got - want:                                 # a swap is allowed only between scores closer than twice the bound
            assert all(abs(ref[r, a] - ref[r, b]) < 2 * max(bound[r, a], bound[r, b]) for b in want - got)


@pytest.mark.parametrize("running", [False, True], ids=["fresh", "running"])
def test_overflow_fallback(ctx, running):
    """5. Scores ascending with the index: every filtered chunk overflows its candidate lists and is recomputed by the predicated
    materialise + select -- on the quantised corpus, fresh and with a running list, the sliced materialise-and-select answer on the
    de-quantised corpus."""
    nq, d, k, N = 16, 128, 10, 300_005
    g = torch.Generator(device="cpu").manual_seed(21)
    u = torch.randn(d, generator=g)
    q = (torch.randn(nq, d, generator=g).abs() * u.sign()).cuda().to(torch.float16)
    c = (torch.arange(1, N + 1).float() / N)[:, None] * u[None, :]
    qc = ctx.quantize_corpus(c, normalize=False)
    deq = qc.dequantize(torch.float16)
    run, base = None, 0
    if running:
        prev = torch.randn(3000, d, generator=g).cuda().to(torch.float16)
        v0, i0, n0 = ctx.score_topk(q, prev, k, idx_base=0, dtype=torch.float16)
        run, base = (v0.clone(), i0.clone(), n0), 3000
        val, idx, n = ctx.score_topk(q, qc, k, idx_base=base, run=(v0, i0, n0))
    else:
        val, idx, n = ctx.score_topk(q, qc, k)
    for s in range(0, N, 100_000):                           # short calls: the materialise-and-select path
        run = ctx.score_topk(q, deq[s:s + 100_000], k, idx_base=base + s, run=run, dtype=torch.float16)
    wv, wi, wn = run
    assert n == wn == k
    assert torch.equal(val, wv) and torch.equal(idx, wi)
    if not running:
        assert (idx >= N - 64).all()


@pytest.mark.parametrize("nq,d", [(65, 128), (8, 72)], ids=["nq65", "d72"])
def test_composed_route_equals_the_f16_scorer(ctx, nq, d):
    """6. More than 64 queries (the 256-row path) and a width the streaming tile does not serve: blocks de-quantised to f16 and scored
    by the f16 path -- the f16 scorer's answer on the de-quantised corpus."""
    N, k = 1000, 11
    q, c = R.unit_corpus(nq + d, N, d, nq)
    qc = ctx.quantize_corpus(c, normalize=True)
    q16 = q.cuda().to(torch.float16)
    val, idx, n = ctx.score_topk(q16, qc, k, idx_base=3)
    wv, wi, wn = ctx.score_topk(q16, qc.dequantize(torch.float16), k, idx_base=3, dtype=torch.float16)
    assert n == wn == k and torch.equal(val, wv) and torch.equal(idx, wi)


def test_quantisation_bound_against_the_unquantised_fixture(ctx):
    """7. The embeddings of tests/golden/scoring.npz (700 x 96 corpus, 13 queries, anisotropic): every cosine score from the fp8 corpus
    within 2^-4 sum|q_i c_i| + 2^-10 scale sum|q_i| of the fp32 score.  Reported, not gated (measured on an MI355X):
    max |dcos| = 4.2e-2, top-10 overlap with the fixture's ranking = 0.80 -- these embeddings are built anisotropic (a few channels
    carry the row), which is where three mantissa bits under one scale per row cost most; the semantic_search fixture's isotropic
    rows (test 10) keep 0.96 of the fp32 top-10."""
    fx = np.load(f"{GOLDEN}/scoring.npz")
    meta = json.loads(str(fx["es_json"]))
    cn = torch.nn.functional.normalize(torch.from_numpy(fx["es_corpus_emb"]), dim=1)
    qn = torch.nn.functional.normalize(torch.from_numpy(fx["es_query_emb"]), dim=1)
    qc = ctx.quantize_corpus(cn, normalize=True)
    got, val, idx = _all_scores(ctx, qn.cuda(), qc)
    s32 = qn.numpy().astype(np.float64) @ cn.numpy().astype(np.float64).T
    err = np.abs(got.cpu().numpy().astype(np.float64) - s32)
    want = meta["results"]["cos_sim"]
    overlap = []
    for r, qid in enumerate(meta["queries"]):
        mine = [f"d{i}" for i in idx[r].tolist() if f"d{i}" != qid][:10]
        ref10 = sorted(want[qid], key=want[qid].get, reverse=True)[:10]
        overlap.append(len(set(mine) & set(ref10)) / len(ref10))
    print(f"fp8 corpus vs fp32: max |dcos| = {err.max():.3e}, top-10 overlap with the fixture's ranking = {np.mean(overlap):.4f}")
    assert np.all(err <= R.quantisation_bound(qn.numpy(), cn.numpy(), qc.scale.cpu().numpy()))


def test_refusals_leave_the_outputs_untouched(ctx):
    """8. Every refusal of the C entry point returns SGPT_ERR_INVALID with nothing launched -- sentinel-filled outputs stay as they
    were -- and the Python surface refuses what it documents."""
    from sgpt_amd import QuantizedCorpus, util
    nq, N, d, k = 4, 300, 128, 5
    q = torch.zeros(nq * d + 8, dtype=torch.float16, device="cuda")
    codes = torch.zeros((N, d), dtype=torch.uint8, device="cuda")
    scale = torch.ones(N, device="cuda")
    val = torch.full((nq, k), 7.0, device="cuda")
    idx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    n_out = C.c_int32(-3)

    def call(q_=q.data_ptr(), codes_=codes.data_ptr(), scale_=scale.data_ptr(), d_=d, k_=k, val_=val.data_ptr(), idx_=idx.data_ptr(), n_run=0):
        return ctx.lib.sgpt_score_topk_q8(ctx.handle, q_, codes_, scale_, nq, N, d_, k_, 0, val_, idx_, n_run, C.byref(n_out), None)
    bad = [dict(q_=None), dict(codes_=None), dict(scale_=None), dict(val_=None), dict(idx_=None), dict(d_=124), dict(k_=0), dict(k_=-1),
           dict(n_run=k + 1), dict(q_=q.data_ptr() + 2), dict(q_=q.data_ptr() + 8)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # SGPT_ERR_INVALID
    assert ctx.lib.sgpt_score_topk_q8(None, q.data_ptr(), codes.data_ptr(), scale.data_ptr(), nq, N, d, k, 0, val.data_ptr(), idx.data_ptr(),
                                      0, C.byref(n_out), None) == -1
    torch.cuda.synchronize()
    assert (val == 7.0).all() and (idx == -7).all() and n_out.value == -3
    assert call() == 0                                       # (and the well-formed call goes through)
    torch.cuda.synchronize()
    assert n_out.value == k and (val == 0).all()
    corpus = QuantizedCorpus(codes, scale)
    q2 = torch.zeros((nq, d), dtype=torch.float16, device="cuda")
    for dt in (torch.bfloat16, torch.float32):
        with pytest.raises(ValueError, match="dtype must be None or torch.float16"):
            ctx.score_topk(q2, corpus, k, dtype=dt)
    with pytest.raises(ValueError, match="embedding dims differ"):
        ctx.score_topk(q2[:, :64], corpus, k)
    with pytest.raises(ValueError, match="'int8'"):
        util.quantize_embeddings(torch.zeros(4, 16), precision="int8")
    with pytest.raises(ValueError, match="normalize=False"):
        util.semantic_search(q2, corpus, score_function=util.dot_score)
    with pytest.raises(ValueError, match="arbitrary score function"):
        util.semantic_search(q2, corpus, score_function=lambda a, b: a @ b.T)


def test_memory_and_the_quantiser_on_many_rows(ctx):
    """9. nbytes == N d + 4 N; the row blocks of quantize_corpus give what one call over all rows gives, and the quantiser's launcher
    takes a million rows."""
    N, d = 1_000_003, 16
    g = torch.Generator(device="cuda").manual_seed(9)
    emb = torch.randn(N, d, device="cuda", generator=g)
    qc = ctx.quantize_corpus(emb, normalize=False, block_rows=300_000)
    assert len(qc) == N and qc.nbytes == N * d + 4 * N and qc.dim == d and not qc.normalized
    codes, scale = ctx.fp8_quantize_rows(emb)
    assert torch.equal(qc.codes, codes) and torch.equal(qc.scale, scale)
    tail = emb[-5:].cpu().numpy()
    wc, ws = R.quantize_rows(tail)
    assert np.array_equal(codes[-5:].cpu().numpy(), wc) and np.array_equal(scale[-5:].cpu().numpy(), ws)


def test_semantic_search_with_a_quantised_corpus(ctx):
    """10. util.semantic_search over util.quantize_embeddings(docs): the reference's result contract (per query a list of
    {'corpus_id', 'score'} by decreasing score, tests/test_gpu_search.py's fixture), and the lists of the f16 scorer on the
    de-quantised corpus.  The fixture's width, 100, is no multiple of 8: the codes carry four zero columns."""
    from sgpt_amd import util
    fx = np.load(f"{GOLDEN}/scoring.npz")
    q, docs = torch.from_numpy(fx["ss_q"]), torch.from_numpy(fx["ss_docs"])
    corpus = util.quantize_embeddings(docs, precision="fp8")
    assert len(corpus) == 1000 and corpus.codes.shape == (1000, 104) and corpus.dim == 100 and corpus.normalized
    hits = util.semantic_search(q, corpus, top_k=10, query_chunk_size=5, corpus_chunk_size=17)
    assert len(hits) == 20 and all(len(h) == 10 for h in hits)
    qn = torch.nn.functional.pad(ctx.l2_normalize(q), (0, 4))
    deq = corpus.dequantize(torch.float32)
    wv, wi, wn = ctx.score_topk(ctx.to_16(qn, torch.float16), ctx.to_16(deq, torch.float16), 10, dtype=torch.float16)
    assert [[h["corpus_id"] for h in r] for r in hits] == wi.cpu().tolist()
    assert [[h["score"] for h in r] for r in hits] == wv.cpu().tolist()
    same = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(wi.cpu().tolist(), fx["ss_idx"].tolist())])
    print(f"semantic_search, fp8 corpus: top-10 overlap with the fp32 golden lists = {same:.4f}")
    # dot scores need a corpus quantised without normalisation
    cd = util.quantize_embeddings(docs, normalize=False)
    hd = util.semantic_search(q, cd, top_k=3, score_function=util.dot_score)
    dv, di, _ = ctx.score_topk(ctx.to_16(torch.nn.functional.pad(q, (0, 4)), torch.float16), cd.dequantize(torch.float16), 3, dtype=torch.float16)
    assert [[h["corpus_id"] for h in r] for r in hd] == di.cpu().tolist()
