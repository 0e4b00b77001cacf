"""-m gpu: the IVF corpus over uint8 lists -- sgpt_u8_gather_quantize_rows, sgpt_ivf_search_u8 (csrc/ivf.hip), IVFUint8Corpus,
Context.ivf_index(precision="uint8"), util.build_ivf_index / semantic_search -- against tests/ivf_u8_ref.py.

Codes are integers and compared exactly.  Values over integer-patterned codes, steps and queries are exact in fp32 whatever the order, so
they are compared bit for bit; over random unit rows they are held to the derived bound of the reference.

Widths and the instantiation of the scan kernel <lanes per row G, rounds NR, rows in flight RB> each one reaches (launch_ivf_scan_u8):
    d =    8 -> ld =  128: <8, 1, 8>        d =  768 -> ld =  768: <64, 1, 8>
    d =  136 -> ld =  256: <16, 1, 8>       d = 1032 -> ld = 1152: <64, 2, 4>
    d =  264 -> ld =  384: <32, 1, 8>       d = 2056 -> ld = 2176: <64, 4, 2>"""
import ctypes as C

import numpy as np
import pytest
import torch

import ivf_ref as R
import ivf_u8_ref as R8
import scoreu8_ref as U

pytestmark = pytest.mark.gpu

CH = R.CHUNK
DIMS = [8, 136, 264, 768, 1032, 2056]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _index(centroids, codes, start, step, ids, offsets, nprobe):
    from sgpt_amd import IVFUint8Corpus
    return IVFUint8Corpus(_t(np.asarray(centroids, dtype=np.float32)), _t(codes), _t(start), _t(step), _t(ids), _t(offsets),
                          int(np.diff(offsets).max()), nprobe, _t(R.f16(centroids)))


# ---- 1. gather-quantise ----
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_gather_quantize_equals_the_row_quantiser_of_the_gathered_rows(ctx, dtype):
    x = _unit(700, 136, 1).astype(dtype)
    x32 = x.astype(np.float32)
    perm = np.random.default_rng(2).permutation(700)[:611].astype(np.int64)
    start, step = U.ranges(x32)
    got = ctx.gather_quantize_rows(_t(x), _t(perm), _t(start), _t(step)).cpu().numpy()
    assert got.shape == (611, 256) and got.dtype == np.uint8 and (got[:, 136:] == 128).all()
    assert np.array_equal(got, ctx.u8_quantize_rows(_t(x32[perm]), _t(start), _t(step)).cpu().numpy())
    want = U.quantize_rows(x32[perm], start, step)
    edge = U.near_half(U.quotient64(x32[perm], start, step))
    assert edge.mean() < 1e-3 and np.array_equal(got[:, :136][~edge], want[:, :136][~edge])
    assert (np.abs(got[:, :136].astype(np.int64) - want[:, :136].astype(np.int64)) <= 1).all() and got[:, :136].min() == 0 and got[:, :136].max() == 255
    bad = perm.copy()
    bad[[0, 300, 610]] = [-1, 700, 2 ** 40]                                    # out of range: rows of 128s
    got2 = ctx.gather_quantize_rows(_t(x), _t(bad), _t(start), _t(step)).cpu().numpy()
    assert (got2[[0, 300, 610]] == 128).all() and np.array_equal(np.delete(got2, [0, 300, 610], axis=0), np.delete(got, [0, 300, 610], axis=0))


# ---- 2. exact search over hand-made lists ----
LIST_LENS = [0, 1, 5, CH - 1, CH, CH + 1, 2 * CH + 3, 15, 25]          # the last two hold 40 identical code rows between them


def _int_ranges(d):
    """step cycles through 1, 0.5, 0.25; start = m - 128 step with integer |m| <= 3: the mid-points are the integers m."""
    j = np.arange(d)
    ld = U.ld_of(d)
    start, step = np.zeros(ld, np.float32), np.zeros(ld, np.float32)
    step[:d] = np.array([1.0, 0.5, 0.25], np.float32)[j % 3]
    start[:d] = ((j * 5) % 7 - 3).astype(np.float32) - 128 * step[:d]
    return start, step


def _int_codes(N, d):
    """An integer pattern over 0 .. 255 that reaches both ends; pad columns 128."""
    n, i = np.arange(N, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    codes = np.full((N, U.ld_of(d)), 128, np.uint8)
    codes[:, :d] = (n * 37 + i * 11 + (n * i) % 5 + n // 64) % 256
    codes[0, 0], codes[0, min(1, d - 1)] = 0, 255
    return codes


def _int_queries(nq, d):
    m, i = np.arange(nq, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    return ((m * 5 + i * 3 + (m * i) % 7 + i // 32) % 9 - 4).astype(np.float32)


def _int_centroids(nlist, d):
    i, c = np.arange(d, dtype=np.int64)[None, :], np.arange(nlist, dtype=np.int64)[:, None]
    return ((c * 3 + i * 5 + (c * i) % 4) % 7 - 3).astype(np.float32)


def _handmade(d, seed=0):
    """(centroids [9, d], codes list-major, start, step, ids, offsets): lists of LIST_LENS, the code rows of the last two lists all equal
    (their original ids interleaved) and the best of all for query 0 of _int_queries."""
    rng = np.random.default_rng(seed + d)
    a = rng.permutation(np.repeat(np.arange(9), LIST_LENS))
    docs = _int_codes(len(a), d)
    start, step = _int_ranges(d)
    twins = np.flatnonzero(a >= 7)
    docs[twins, :d] = np.where(_int_queries(1, d)[0] > 0, 255, 0)               # the best row there is for query 0: forty equal best scores
    offsets, perm = R.lists(a, 9)
    # every product q_j step_j c_j, every term q_j mid_j and every partial sum is a multiple of 0.25; in units of 0.25 their magnitudes add
    # up to less than 2.6e6 < 2^24 (|q| <= 4, |c| <= 128, |mid| <= 3): fp32 holds every partial sum exactly, in any order
    mid = start[:d] + 128 * step[:d]
    assert np.array_equal(mid, np.rint(mid)) and np.abs(mid).max() <= 3
    assert (step[:d] * 4 * 128).sum() * 4 + np.abs(mid).sum() * 4 * 4 < 2.6e6 < 2 ** 24
    assert docs[:, :d].min() == 0 and docs[:, :d].max() == 255
    return _int_centroids(9, d), docs[perm], start, step, perm, offsets


@pytest.mark.parametrize("nq", [1, 3, 65])
@pytest.mark.parametrize("d", DIMS)
def test_search_equals_the_reference_exactly(ctx, d, nq):
    from sgpt_amd import IVFCorpus
    centroids, codes, start, step, ids, offsets = _handmade(d)
    q = _int_queries(nq, d)
    N = len(ids)
    rows16 = _t(np.zeros((N, d), np.float16))
    for nprobe in (1, 3, 9):
        ix = _index(centroids, codes, start, step, ids, offsets, nprobe)
        f16 = IVFCorpus(ix.centroids, rows16, ix.ids, ix.offsets, ix.max_list, nprobe, ix.centroids16)
        want_probe = f16.search(ctx, _t(q), 1, return_probes=True)[3].cpu().numpy()       # the f16 index over the same centroids
        for k in (1, 10, 1024):
            val, idx, n, probes = ix.search(ctx, _t(q), k, return_probes=True)
            probes = probes.cpu().numpy()
            assert n == min(k, N)
            assert np.array_equal(probes, want_probe) and np.array_equal(probes, R.probe_sets(q, R.f16(centroids), nprobe))
            rv, ri, _ = R8.search_u8(q, codes, start, step, ids, offsets, probes, k)
            assert np.array_equal(idx.cpu().numpy(), ri), (nprobe, k)
            assert np.array_equal(val.cpu().numpy(), rv.astype(np.float32)), (nprobe, k)
    # nprobe = 9, k = 1024: the forty twins of query 0 tie at the top, and stand in ascending id order across their two lists
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    twins = np.sort(np.concatenate([ids[offsets[7]:offsets[8]], ids[offsets[8]:offsets[9]]]))
    at = np.flatnonzero(np.isin(idx[0], twins))
    assert np.array_equal(at, np.arange(40)) and np.array_equal(idx[0, at], twins) and (val[0, at] == val[0, 0]).all()


@pytest.mark.parametrize("d", DIMS)
def test_a_nan_query_scores_minus_one_on_every_probed_row(ctx, d):
    centroids, codes, start, step, ids, offsets = _handmade(d)
    q = _int_queries(2, d)
    q[1, d // 2] = np.nan
    ix = _index(centroids, codes, start, step, ids, offsets, 3)
    val, idx, n, probes = ix.search(ctx, _t(q), 1024, return_probes=True)
    probes, val, idx = probes.cpu().numpy(), val.cpu().numpy(), idx.cpu().numpy()
    want = np.sort(np.concatenate([ids[offsets[c]:offsets[c + 1]] for c in probes[1]]))
    assert len(want) >= 1 and np.array_equal(idx[1, :len(want)], want) and (val[1, :len(want)] == -1.0).all()
    assert (idx[1, len(want):] == -1).all() and np.isinf(val[1, len(want):]).all()
    rv, ri, _ = R8.search_u8(q, codes, start, step, ids, offsets, probes, 1024)
    assert np.array_equal(idx, ri) and np.array_equal(val, rv.astype(np.float32))


# ---- 3. idx_base and a running list ----
@pytest.mark.parametrize("d", [8, 768])
def test_search_merges_idx_base_and_a_running_list(ctx, d):
    centroids, codes, start, step, ids, offsets = _handmade(d, seed=1)
    nq, k = 3, 10
    q = _int_queries(nq, d)
    ix = _index(centroids, codes, start, step, ids, offsets, 3)
    base = 5000
    plain_v, plain_i, _, probes = ix.search(ctx, _t(q), k, return_probes=True)
    probes, plain_v = probes.cpu().numpy(), plain_v.cpu().numpy()
    # the running list: a score above everything, a tie with this call's best under a LOWER index, one under a HIGHER index, a low one
    run_v = np.stack([np.array([plain_v[i, 0] + 8, plain_v[i, 0], plain_v[i, 0], -1e6], dtype=np.float32) for i in range(nq)])
    run_i = np.tile(np.array([17, 3, 9_000_000, 5], dtype=np.int64), (nq, 1))
    pad_v = np.concatenate([run_v, np.zeros((nq, k - 4), np.float32)], axis=1)
    pad_i = np.concatenate([run_i, np.zeros((nq, k - 4), np.int64)], axis=1)
    val, idx, n = ix.search(ctx, _t(q), k, idx_base=base, run=(_t(pad_v), _t(pad_i), 4))
    rv, ri, _ = R8.search_u8(q, codes, start, step, ids, offsets, probes, k, idx_base=base, run=(pad_v, pad_i, 4))
    assert n == k and np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))
    assert (ri[:, 0] == 17).all() and (ri[:, 1] == 3).all() and (ri[:, 2] == plain_i.cpu().numpy()[:, 0] + base).all()


# ---- 4. random unit rows ----
def _unit_index(N, d, nlist, seed):
    x16 = _unit(N, d, seed).astype(np.float16)
    centroids = _unit(nlist, d, seed + 1)
    offsets, perm = R.lists(R.assign(x16, centroids), nlist)
    rows16 = x16[perm]
    start, step = U.ranges(rows16.astype(np.float32))
    return centroids, U.quantize_rows(rows16.astype(np.float32), start, step), start, step, perm, offsets, rows16


@pytest.mark.parametrize("d", [136, 768])
def test_random_rows_stay_within_the_bound(ctx, d):
    centroids, codes, start, step, ids, offsets, rows16 = _unit_index(3000, d, 12, d)
    q = _unit(3, d, 99)
    k = 10
    ix = _index(centroids, codes, start, step, ids, offsets, 4)
    val, idx, n, probes = ix.search(ctx, _t(q), k, return_probes=True)
    assert n == k
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    _, _, cands = R8.search_u8(q, codes, start, step, ids, offsets, probes.cpu().numpy(), k)
    s, b = R8.values64(q, codes, start, step), R8.score_bound(q, codes, start, step)
    s16, qb = R.scores64(q, rows16), U.quantisation_bound(q, rows16.astype(np.float32), start, step)
    pos_of = np.full(int(ids.max()) + 1, -1)
    pos_of[ids] = np.arange(len(ids))
    worst = 0.0
    for i in range(len(q)):
        assert len(cands[i]) >= k and (idx[i] >= 0).all()
        pos = pos_of[idx[i]]
        assert np.isin(pos, cands[i]).all() and len(set(pos.tolist())) == k
        err = np.abs(val[i].astype(np.float64) - s[i, pos])
        worst = max(worst, float((err / b[i, pos]).max()))
        assert (err <= b[i, pos]).all()
        assert (np.diff(val[i]) <= 0).all()
        out = np.setdiff1d(cands[i], pos)
        assert (s[i, out] <= val[i, k - 1] + 2 * b[i, out]).all()
        assert (np.abs(val[i].astype(np.float64) - s16[i, pos]) <= b[i, pos] + qb[i, pos]).all()
    print(f"d={d}: max |value - float64| / bound = {worst:.3f} (n = {R8.score_roundings(d)} roundings)")


# ---- 5. place independence ----
@pytest.mark.parametrize("d", [136, 768, 1032])
def test_a_value_does_not_depend_on_nq_or_nprobe(ctx, d):
    centroids, codes, start, step, ids, offsets, _ = _unit_index(3000, d, 12, d + 1)
    q = _unit(65, d, 98)

    def values(nq, nprobe):
        val, idx, _ = _index(centroids, codes, start, step, ids, offsets, nprobe).search(ctx, _t(q[:nq]), 1024)
        val, idx = val[0].cpu().numpy(), idx[0].cpu().numpy()
        return {int(j): v.tobytes() for j, v in zip(idx, val) if j >= 0}
    alone, among = values(1, 3), values(65, 3)
    assert len(alone) >= 100 and alone == among
    wide = values(1, 9)
    both = set(alone) & set(wide)
    assert len(both) >= 100 and all(alone[j] == wide[j] for j in both)


# ---- 6. build, end to end ----
@pytest.fixture(scope="module")
def built(ctx):
    x, q = R.clustered_fixture()
    kw = dict(nlist=32, n_iter=8)
    return x, q, ctx.ivf_index(_t(x), **kw), ctx.ivf_index(_t(x), precision="uint8", **kw), ctx.ivf_index(_t(x), precision="uint8", **kw)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_two_builds_are_bit_identical_and_share_the_f16_lists(ctx, built):
    from sgpt_amd import IVFUint8Corpus
    x, _, f16, a, b = built
    assert type(a) is IVFUint8Corpus
    for name in ("centroids", "centroids16", "codes", "start", "step", "ids", "offsets"):
        assert _same_bits(getattr(a, name), getattr(b, name)), name
    assert a.max_list == b.max_list and a.nprobe == b.nprobe == 32 and a.dim == 128
    for name in ("centroids", "centroids16", "ids", "offsets"):
        assert _same_bits(getattr(a, name), getattr(f16, name)), name
    assert a.max_list == f16.max_list
    # the codes: the rule applied to the f16 index's rows, with the column min / max of those rows
    rows32 = f16.rows.float()
    mn, mx = ctx.u8_col_minmax(rows32)
    assert torch.equal(a.start, mn) and torch.equal(a.step, (mx - mn) / torch.full_like(mx, 255.0))
    assert torch.equal(a.codes, ctx.u8_quantize_rows(rows32, a.start, a.step))
    rows = rows32.cpu().numpy()
    start, step = U.ranges(rows)
    assert np.array_equal(a.start.cpu().numpy(), start) and np.array_equal(a.step.cpu().numpy(), step)
    edge = U.near_half(U.quotient64(rows, start, step))
    assert edge.mean() < 1e-3 and np.array_equal(a.codes.cpu().numpy()[~edge], U.quantize_rows(rows, start, step)[~edge])
    # de-quantised: the documented arithmetic bit for bit, and within half a step and an fp32 ulp of the rows.  The ulp: the fp32 quotient
    # is off by at most 255 * 2^-23 of a step (one subtraction, one division), so a code may stand that much further than half a step
    # from its element; start + code * step rounds its product (at most 255 step) and its sum (at most the column's largest magnitude)
    # once each, half an ulp of those.
    deq32 = a.dequantize().cpu().numpy()
    assert deq32.shape == rows.shape and np.array_equal(deq32, U.dequantize32(a.codes.cpu().numpy(), start, step))
    st = step[None, :].astype(np.float64)
    ulp = (np.spacing(255 * step) + np.spacing(np.maximum(np.abs(start), np.abs(start + 255 * step))))[None, :].astype(np.float64) / 2
    assert (np.abs(deq32.astype(np.float64) - rows) <= st / 2 + 255 * 2.0 ** -23 * st + ulp).all()
    N, ld = 4096, 128
    assert a.codes.shape == (N, ld) and a.nbytes == N * ld + 2 * ld * 4 + 32 * 128 * 4 + 32 * 128 * 2 + N * 8 + 33 * 8
    assert f16.nbytes - a.nbytes == N * 128 * 2 - N * ld - 2 * ld * 4
    u8 = a.as_uint8_corpus()
    assert u8.codes.data_ptr() == a.codes.data_ptr() and len(u8) == N


def test_ranges_and_calibration_rows_change_the_codes_as_the_rule_says(ctx, built):
    from sgpt_amd import util
    x, _, f16, a, _ = built
    kw = dict(nlist=32, n_iter=8, precision="uint8")
    rows32 = f16.rows.float()
    ranges = torch.stack([torch.full((128,), -0.25), torch.full((128,), 0.5)])
    r = util.build_ivf_index(_t(x), ranges=ranges, **kw)
    assert _same_bits(r.ids, a.ids) and _same_bits(r.centroids, a.centroids)
    assert torch.equal(r.start.cpu(), ranges[0]) and torch.equal(r.step.cpu(), (ranges[1] - ranges[0]) / torch.full((128,), 255.0))
    assert torch.equal(r.codes, ctx.u8_quantize_rows(rows32, r.start, r.step)) and not torch.equal(r.codes, a.codes)
    cal = x[::7]
    c = ctx.ivf_index(_t(x), calibration_embeddings=_t(cal), **kw)
    mn, mx = ctx.u8_col_minmax(ctx.l2_normalize(_t(cal), out_dtype=torch.float16).float())
    assert torch.equal(c.start, mn) and torch.equal(c.step, (mx - mn) / torch.full_like(mx, 255.0))
    assert torch.equal(c.codes, ctx.u8_quantize_rows(rows32, c.start, c.step)) and not torch.equal(c.codes, a.codes)
    codes = c.codes.cpu().numpy()
    assert (codes == 0).any() and (codes == 255).any()                          # rows outside the sample's ranges clamp
    with pytest.raises(ValueError, match="not both"):
        ctx.ivf_index(_t(x), ranges=ranges, calibration_embeddings=_t(cal), **kw)
    with pytest.raises(ValueError, match=r"ranges must be \[2, 128\]"):
        ctx.ivf_index(_t(x), ranges=ranges[:, :64], **kw)


# ---- 7. ranking ----
def test_ranking_follows_the_reference_and_the_f16_index(ctx, built):
    from sgpt_amd import util
    x, q, f16, a, _ = built
    codes, start, step = a.codes.cpu().numpy(), a.start.cpu().numpy(), a.step.cpu().numpy()
    ids, offsets = a.ids.cpu().numpy(), a.offsets.cpu().numpy()
    qd = ctx.l2_normalize(_t(q))
    qn = qd.cpu().numpy()
    s, b = R8.values64(qn, codes, start, step), R8.score_bound(qn, codes, start, step)
    pos_of = np.empty(len(ids), np.int64)
    pos_of[ids] = np.arange(len(ids))
    for p in (1, 2, 4, 8, 32):
        view = a.with_nprobe(p)
        val, idx, n, probes = view.search(ctx, qd, 10, return_probes=True)
        assert n == 10
        idx = idx.cpu().numpy()
        fv, fi, _, fprobes = f16.with_nprobe(p).search(ctx, qd, 10, return_probes=True)
        assert torch.equal(probes, fprobes)
        rv, ri, _ = R8.search_u8(qn, codes, start, step, ids, offsets, probes.cpu().numpy(), 10)
        # positions whose reference value stands further than twice the bound from both neighbours: the device must agree there
        gap = np.abs(np.diff(rv, axis=1))
        bb = np.take_along_axis(b, pos_of[np.maximum(ri, 0)], axis=1)
        clear = np.ones_like(ri, dtype=bool)
        clear[:, 1:] &= gap > 2 * np.maximum(bb[:, 1:], bb[:, :-1])
        clear[:, :-1] &= gap > 2 * np.maximum(bb[:, 1:], bb[:, :-1])
        clear &= ri >= 0
        assert clear.mean() >= 0.95 and np.array_equal(idx[clear], ri[clear])
        overlap = R.recall_at(idx, fi.cpu().numpy())
        print(f"nprobe {p}: clear positions {clear.mean():.4f}, top-10 overlap with the f16 index {overlap:.4f}")
        assert overlap >= 0.97
        hits = util.semantic_search(_t(q), view, top_k=10)
        tv, ti, _ = ctx.score_topk(qd, view, 10)
        assert [[h["corpus_id"] for h in row] for row in hits] == [[j for j in row if j >= 0] for row in ti.cpu().tolist()]
        assert torch.equal(ti.cpu(), torch.from_numpy(idx))


# ---- 8. skew ----
def test_one_list_holds_most_of_the_rows(ctx):
    N, d, nlist = 70_001, 32, 100
    rng = np.random.default_rng(7)
    a = np.where(rng.random(N) < 0.6, 50, rng.integers(0, nlist, N))
    offsets, perm = R.lists(a, nlist)
    assert (np.diff(offsets)[50] + CH - 1) // CH == 165
    docs = _int_codes(N, d)
    start, step = _int_ranges(d)
    q = _int_queries(2, d)
    centroids = _int_centroids(nlist, d)
    centroids[50] = q[0]                                                        # query 0 probes the long list first
    codes = docs[perm]
    ix = _index(centroids, codes, start, step, perm, offsets, 4)
    val, idx, n, probes = ix.search(ctx, _t(q), 10, return_probes=True)
    probes = probes.cpu().numpy()
    assert n == 10 and probes[0, 0] == 50 and np.array_equal(probes, R.probe_sets(q, R.f16(centroids), 4))
    rv, ri, _ = R8.search_u8(q, codes, start, step, perm, offsets, probes, 10)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))


# ---- 9. refusals through the ABI ----
def test_the_abi_refuses_bad_shapes_and_leaves_the_outputs(ctx):
    from sgpt_amd.corpus import _p, _stream_ptr
    d, ld, N, nlist, k = 16, 128, 40, 4, 10
    q, c16 = _t(_unit(2, d, 0)), _t(_unit(nlist, d, 1).astype(np.float16))
    buf = torch.full((N * 256 + 16,), 128, dtype=torch.uint8, device="cuda")
    start, step = torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")
    ids, offsets = torch.arange(N, device="cuda"), _t(np.array([0, 10, 20, 30, 40], dtype=np.int64))

    def call(codes=None, d=d, ld=ld, nprobe=2, k=k, start=start, step=step):
        codes = buf if codes is None else codes
        val = torch.full((2, max(k, 1)), 7.0, device="cuda")
        idx = torch.full((2, max(k, 1)), 7, dtype=torch.int64, device="cuda")
        probes = torch.full((2, 8), 7, dtype=torch.int64, device="cuda")
        n_out = C.c_int32(77)
        st = ctx.lib.sgpt_ivf_search_u8(ctx.handle, _p(q), _p(c16), _p(codes), _p(start), _p(step), _p(ids), _p(offsets), 2, N, d, ld, nlist, 10,
                                        nprobe, k, 0, _p(val), _p(idx), 0, C.byref(n_out), _p(probes), _stream_ptr(ctx.device))
        torch.cuda.synchronize()
        untouched = bool((val == 7.0).all()) and bool((idx == 7).all()) and bool((probes == 7).all()) and n_out.value == 77
        return st, untouched
    assert call() == (0, False)                                                # (the same arguments in range are served)
    assert call(ld=100) == (-1, True)
    assert call(d=136) == (-1, True)                                           # d > ld
    assert call(nprobe=5) == (-1, True)                                        # nprobe > nlist
    assert call(k=1025) == (-1, True)
    assert call(codes=buf[1:]) == (-1, True)                                   # a view offset by one byte
    assert call(start=None) == (-1, True) and call(step=None) == (-1, True)
    # the row entry
    x = _t(_unit(8, d, 2))
    perm = torch.arange(8, device="cuda")

    def gather(x=x, d=d, ld=ld, out=None, dtype=0):
        out = torch.full((8 * 256 + 16,), 9, dtype=torch.uint8, device="cuda") if out is None else out
        st = ctx.lib.sgpt_u8_gather_quantize_rows(ctx.handle, _p(x), dtype, 8, _p(perm), 8, d, ld, _p(start), _p(step), _p(out),
                                                  _stream_ptr(ctx.device))
        torch.cuda.synchronize()
        return st, bool((out == 9).all())
    assert gather() == (0, False)
    keep = torch.full((8 * 256 + 16,), 9, dtype=torch.uint8, device="cuda")
    assert gather(ld=100) == (-1, True) and gather(d=136) == (-1, True) and gather(d=12) == (-1, True) and gather(dtype=1) == (-1, True)
    assert gather(out=keep[1:]) == (-1, True) and gather(x=x.view(-1)[1:]) == (-1, True)
