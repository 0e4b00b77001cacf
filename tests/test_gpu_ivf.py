"""-m gpu: the IVF corpus -- sgpt_ivf_lists, sgpt_ivf_centroids, sgpt_gather_rows, sgpt_ivf_search (csrc/ivf.hip), IVFCorpus,
Context.ivf_index, util.build_ivf_index / kmeans / semantic_search -- against tests/ivf_ref.py.

Lists are integer arithmetic and compared exactly.  Sums and scores over integer-patterned data are exact in fp32 whatever the order, so
they are compared bit for bit; over random unit rows they are held to the derived bounds of the reference."""
import numpy as np
import pytest
import torch

import ivf_ref as R

pytestmark = pytest.mark.gpu

CH = R.CHUNK


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _patterned(nq, N, d):
    """Asymmetric small integers (exact in f16, their fp32 dot products exact in any order): queries in [-4, 4], documents in [-6, 6]."""
    n, i = np.arange(N, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    docs = ((n * 7 + i * 11 + (n * i) % 5 + n // 64) % 13 - 6).astype(np.float32)
    m = np.arange(nq, dtype=np.int64)[:, None]
    q = ((m * 5 + i * 3 + (m * i) % 7 + i // 32) % 9 - 4).astype(np.float32)
    return q, docs


def _unit(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _index(centroids, rows16, ids, offsets, nprobe):
    from sgpt_amd import IVFCorpus
    return IVFCorpus(_t(np.asarray(centroids, dtype=np.float32)), _t(rows16), _t(ids), _t(offsets), int(np.diff(offsets).max()), nprobe,
                     _t(R.f16(centroids)))


# ---- 1. lists ----
@pytest.mark.parametrize("N, nlist", [(1, 1), (257, 7), (5000, 64), (70000, 300)])
def test_lists_equal_the_stable_argsort(ctx, N, nlist):
    rng = np.random.default_rng(N)
    a = rng.integers(1, nlist - 1, N) if nlist >= 3 else rng.integers(0, nlist, N)       # (first and last list empty)
    offsets, perm = ctx.ivf_lists(_t(a), nlist)
    ro, rp = R.lists(a, nlist)
    assert np.array_equal(offsets.cpu().numpy(), ro) and np.array_equal(perm.cpu().numpy(), rp)
    assert np.array_equal(ro[1:] - ro[:-1], np.bincount(a, minlength=nlist))
    if nlist >= 3:
        assert ro[1] == 0 and ro[-2] == N


def test_lists_clamp_assignments_out_of_range(ctx):
    a = np.random.default_rng(3).integers(-4, 12, 3000)
    a[:3] = [-2 ** 40, 2 ** 40, 7]
    offsets, perm = ctx.ivf_lists(_t(a), 8)
    ro, rp = R.lists(a, 8)
    assert np.array_equal(offsets.cpu().numpy(), ro) and np.array_equal(perm.cpu().numpy(), rp)
    assert ro[1] == (a <= 0).sum() and ro[-1] - ro[-2] == (a >= 7).sum()


# ---- 2. centroids ----
LENS = [0, 1, 255, 256, 257, 1000]


def _centroid_case(d, seed):
    rng = np.random.default_rng(seed)
    a = rng.permutation(np.repeat(np.arange(len(LENS)), LENS))
    offsets, perm = R.lists(a, len(LENS))
    assert np.diff(offsets).tolist() == LENS
    return a, offsets, perm


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [8, 136, 768])
def test_centroid_sums_of_integer_rows_are_exact(ctx, d, dtype):
    a, offsets, perm = _centroid_case(d, d)
    x = _patterned(1, len(a), d)[1].astype(dtype)
    prev = np.random.default_rng(d + 1).standard_normal((len(LENS), d)).astype(np.float32)
    got = ctx.ivf_centroids(_t(x), _t(perm), _t(offsets), prev=_t(prev), normalize=False).cpu().numpy()
    want = R.centroids(x, perm, offsets, prev=prev, normalize=False)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(got[0], prev[0])                                      # the empty list returns prev
    bare = ctx.ivf_centroids(_t(x), _t(perm), _t(offsets), normalize=False).cpu().numpy()
    assert not bare[0].any() and np.array_equal(bare[1:], got[1:])              # (zeros without prev)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [8, 136, 768])
def test_normalised_centroids_stay_within_the_bound_and_do_not_depend_on_the_place(ctx, d, dtype):
    a, offsets, perm = _centroid_case(d, d + 7)
    x = _unit(len(a), d, d).astype(dtype)
    if d >= 136:
        x[:, 0] += dtype(0.25)                                                  # (a common direction: sums that do not cancel)
    prev = _unit(len(LENS), d, 5)
    got = ctx.ivf_centroids(_t(x), _t(perm), _t(offsets), prev=_t(prev)).cpu().numpy()
    want, bound = R.centroids(x, perm, offsets, prev=prev), R.centroid_bound(x, perm, offsets)
    err = np.abs(got.astype(np.float64) - want)
    print(f"d={d} {np.dtype(dtype).name}: max err / bound = {np.nanmax(err[1:] / bound[1:]):.3f}, max err = {err.max():.3e}")
    assert np.array_equal(got[0], prev[0]) and (err[1:] <= bound[1:]).all()
    assert np.allclose(np.linalg.norm(got[1:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the rows of the 1000-row list and of the 257-row list as lists 1 and 0 of another index, behind other rows of the same matrix
    l5, l4 = perm[offsets[5]:offsets[6]], perm[offsets[4]:offsets[5]]
    perm2 = np.concatenate([np.arange(3), l4, l5, np.arange(9)]).astype(np.int64)
    off2 = np.array([3, 3 + 257, 3 + 1257, 3 + 1257, 3 + 1257 + 9], dtype=np.int64)
    got2 = ctx.ivf_centroids(_t(x), _t(perm2), _t(off2)).cpu().numpy()
    assert np.array_equal(got2[0].view(np.uint32), got[4].view(np.uint32)) and np.array_equal(got2[1].view(np.uint32), got[5].view(np.uint32))
    assert not got2[2].any()


def test_gather_rows_rounds_to_f16(ctx):
    x = _unit(700, 136, 1)
    perm = np.random.default_rng(2).permutation(700)[:611].astype(np.int64)
    assert np.array_equal(ctx.gather_rows(_t(x), _t(perm)).cpu().numpy(), x[perm].astype(np.float16))
    x16 = x.astype(np.float16)
    assert np.array_equal(ctx.gather_rows(_t(x16), _t(perm)).cpu().numpy(), x16[perm])


# ---- 3. search over hand-made indices ----
LIST_LENS = [0, 1, 5, CH - 1, CH, CH + 1, 2 * CH + 3, 15, 25]          # the last two hold 40 identical rows between them


def _handmade(d, seed=0):
    """(centroids [9, d], rows f16 list-major, ids, offsets, docs in original order): integer patterns, lists of LIST_LENS, the rows of the
    last two lists all equal (their original ids interleaved), one NaN element in the 5-row list."""
    rng = np.random.default_rng(seed + d)
    a = rng.permutation(np.repeat(np.arange(9), LIST_LENS))
    N = len(a)
    _, docs = _patterned(1, N, d)
    twins = np.flatnonzero(a >= 7)
    docs[twins] = docs[twins[0]]
    docs[np.flatnonzero(a == 2)[3], d // 2] = np.nan
    offsets, perm = R.lists(a, 9)
    i, c = np.arange(d, dtype=np.int64)[None, :], np.arange(9, dtype=np.int64)[:, None]
    centroids = ((c * 3 + i * 5 + (c * i) % 4) % 7 - 3).astype(np.float32)
    return centroids, docs.astype(np.float16)[perm], perm, offsets, docs


@pytest.mark.parametrize("nq", [1, 3, 65])
@pytest.mark.parametrize("d", [8, 136, 768, 1032])
def test_search_equals_the_reference_exactly(ctx, d, nq):
    centroids, rows16, ids, offsets, docs = _handmade(d)
    q = _patterned(nq, 1, d)[0]
    q[0] = docs[ids[offsets[7]]]                                                # query 0 is the twin row: forty equal best scores in two lists
    N = len(ids)
    for nprobe in (1, 3, 9):
        ix = _index(centroids, rows16, ids, offsets, nprobe)
        _, want_probe, _ = ctx.score_topk(_t(q).half(), ix.centroids16, nprobe, dtype=torch.float16)
        for k in (1, 10, 1024):
            val, idx, n, probes = ix.search(ctx, _t(q), k, return_probes=True)
            probes = probes.cpu().numpy()
            assert n == min(k, N)
            assert np.array_equal(probes, want_probe.cpu().numpy()) and np.array_equal(probes, R.probe_sets(q, R.f16(centroids), nprobe))
            rv, ri, _ = R.search(q, rows16, ids, offsets, probes, k)
            assert np.array_equal(idx.cpu().numpy(), ri), (nprobe, k)
            assert np.array_equal(val.cpu().numpy(), rv.astype(np.float32)), (nprobe, k)
    # nprobe = 9, k = 1024: the forty twins of query 0 tie, and stand in ascending id order across their two lists
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    twins = np.sort(np.concatenate([ids[offsets[7]:offsets[8]], ids[offsets[8]:offsets[9]]]))
    at = np.flatnonzero(np.isin(idx[0], twins))
    assert len(at) == 40 and np.array_equal(idx[0, at], twins) and (val[0, at] == val[0, at[0]]).all()
    # the 5-row list on its own: all five rows come back, the NaN row with -1
    lo, hi = offsets[2], offsets[3]
    five = _index(centroids[2:3], rows16[lo:hi], ids[lo:hi], np.array([0, 5], dtype=np.int64), 1)
    v5, i5, n5 = five.search(ctx, _t(q), 5)
    v5, i5 = v5.cpu().numpy(), i5.cpu().numpy()
    nan_id = ids[lo + 3]
    assert n5 == 5 and np.isnan(docs[nan_id]).any() and (np.sort(i5, axis=1) == ids[lo:hi]).all() and (v5[i5 == nan_id] == -1.0).all()


@pytest.mark.parametrize("d", [8, 768])
def test_search_merges_idx_base_and_a_running_list(ctx, d):
    centroids, rows16, ids, offsets, docs = _handmade(d, seed=1)
    nq, k = 3, 10
    q = _patterned(nq, 1, d)[0]
    ix = _index(centroids, rows16, ids, offsets, 3)
    base = 5000
    plain_v, plain_i, _, probes = ix.search(ctx, _t(q), k, return_probes=True)
    probes, plain_v = probes.cpu().numpy(), plain_v.cpu().numpy()
    # the running list: a score above everything, a tie with this call's best under a LOWER index, one under a HIGHER index, a low one
    run_v = np.stack([np.array([plain_v[i, 0] + 8, plain_v[i, 0], plain_v[i, 0], -1e6], dtype=np.float32) for i in range(nq)])
    run_i = np.tile(np.array([17, 3, 9_000_000, 5], dtype=np.int64), (nq, 1))
    pad_v = np.concatenate([run_v, np.zeros((nq, k - 4), np.float32)], axis=1)
    pad_i = np.concatenate([run_i, np.zeros((nq, k - 4), np.int64)], axis=1)
    val, idx, n = ix.search(ctx, _t(q), k, idx_base=base, run=(_t(pad_v), _t(pad_i), 4))
    rv, ri, _ = R.search(q, rows16, ids, offsets, probes, k, idx_base=base, run=(pad_v, pad_i, 4))
    assert n == k and np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))
    assert (ri[:, 0] == 17).all() and (ri[:, 1] == 3).all() and (ri[:, 2] == plain_i.cpu().numpy()[:, 0] + base).all()


# ---- 4. / 5. random unit rows ----
def _unit_index(N, d, nlist, seed):
    x16 = _unit(N, d, seed).astype(np.float16)
    centroids = _unit(nlist, d, seed + 1)
    a = R.assign(x16, centroids)
    offsets, perm = R.lists(a, nlist)
    return centroids, x16[perm], perm, offsets


def _check_within_bounds(q, rows16, ids, cands, val, idx, k):
    """Values within the bound of float64; every returned document among the candidates; no candidate left out beats the k-th value by
    more than twice the bound."""
    s, b = R.scores64(q, rows16), R.score_bound(q, rows16)
    pos_of = np.full(int(ids.max()) + 1, -1)
    pos_of[ids] = np.arange(len(ids))
    worst = 0.0
    for i in range(len(q)):
        n = min(k, len(cands[i]))
        assert (idx[i, :n] >= 0).all() and (idx[i, n:] == -1).all() and np.isinf(val[i, n:]).all()
        pos = pos_of[idx[i, :n]]
        assert np.isin(pos, cands[i]).all() and len(set(pos.tolist())) == n
        err = np.abs(val[i, :n].astype(np.float64) - s[i, pos])
        worst = max(worst, float((err / b[i, pos]).max()))
        assert (err <= b[i, pos]).all()
        assert (np.diff(val[i, :n]) <= 0).all()
        out = np.setdiff1d(cands[i], pos)
        if n == k and len(out):
            assert (s[i, out] <= val[i, n - 1] + 2 * b[i, out]).all()
    print(f"max |value - float64| / bound = {worst:.3f}")


@pytest.mark.parametrize("d", [136, 768])
def test_random_rows_stay_within_the_bound(ctx, d):
    centroids, rows16, ids, offsets = _unit_index(3000, d, 12, d)
    q = _unit(3, d, 99)
    ix = _index(centroids, rows16, ids, offsets, 4)
    val, idx, n, probes = ix.search(ctx, _t(q), 10, return_probes=True)
    assert n == 10
    _, _, cands = R.search(q, rows16, ids, offsets, probes.cpu().numpy(), 10)
    _check_within_bounds(q, rows16, ids, cands, val.cpu().numpy(), idx.cpu().numpy(), 10)


def test_every_list_probed_equals_the_exact_search_on_integer_rows(ctx):
    centroids, rows16, ids, offsets, docs = _handmade(136, seed=2)
    keep = ~np.isnan(rows16.astype(np.float32)).any(axis=1)                      # (the fp32 scorer has its own NaN path: leave the row out)
    docs16 = np.zeros((len(ids), 136), np.float16)
    docs16[ids] = rows16
    docs16[ids[~keep]] = 0
    rows16 = docs16[ids]
    q = _patterned(5, 1, 136)[0]
    ix = _index(centroids, rows16, ids, offsets, 9)
    for k in (1, 10, 1024):
        val, idx, n = ctx.score_topk(_t(q), ix, k)
        ev, ei, en = ctx.score_topk(_t(q), _t(docs16.astype(np.float32)), k, dtype=torch.float32)
        assert n == en and torch.equal(idx, ei) and torch.equal(val, ev)


def test_every_list_probed_equals_the_exact_search_on_unit_rows(ctx):
    centroids, rows16, ids, offsets = _unit_index(2000, 136, 7, 11)
    q = _unit(4, 136, 12)
    val, idx, n = ctx.score_topk(_t(q), _index(centroids, rows16, ids, offsets, 7), 10)
    cands = [np.arange(2000)] * 4
    _check_within_bounds(q, rows16, ids, cands, val.cpu().numpy(), idx.cpu().numpy(), 10)


# ---- 6. build, end to end ----
@pytest.fixture(scope="module")
def built(ctx):
    x, q = R.clustered_fixture()
    return x, q, ctx.ivf_index(_t(x), nlist=32, n_iter=8), ctx.ivf_index(_t(x), nlist=32, n_iter=8)


def test_two_builds_are_bit_identical(built):
    _, _, a, b = built
    for name in ("centroids", "centroids16", "rows", "ids", "offsets"):
        assert torch.equal(getattr(a, name).view(torch.uint8), getattr(b, name).view(torch.uint8)), name
    assert a.max_list == b.max_list and a.nprobe == b.nprobe == 32


def test_built_lists_partition_the_rows_by_the_f16_scorer(ctx, built):
    x, _, ix, _ = built
    ids, offsets = ix.ids.cpu().numpy(), ix.offsets.cpu().numpy()
    sizes = np.diff(offsets)
    assert offsets[0] == 0 and offsets[-1] == len(x) and (sizes >= 0).all() and ix.max_list == sizes.max()
    assert np.array_equal(np.sort(ids), np.arange(len(x)))                       # every row in exactly one list
    for c in range(32):
        assert (np.diff(ids[offsets[c]:offsets[c + 1]]) > 0).all()
    x16 = ctx.l2_normalize(_t(x), out_dtype=torch.float16)
    assert torch.equal(ix.rows, x16[ix.ids])
    assert torch.equal(ix.centroids16, ix.centroids.half())
    assert np.allclose(np.linalg.norm(ix.centroids.cpu().numpy().astype(np.float64), axis=1), 1.0, atol=1e-6)
    _, best, _ = ctx.score_topk(ix.rows, ix.centroids16, 1, dtype=torch.float16)
    assert np.array_equal(best[:, 0].cpu().numpy(), np.repeat(np.arange(32), sizes))


def test_recall_grows_with_nprobe_and_semantic_search_agrees(ctx, built):
    from sgpt_amd import util
    x, q, ix, _ = built
    rows16, ids = ix.rows.cpu().numpy(), ix.ids.cpu().numpy()
    s = R.scores64(q, rows16)
    exact = np.stack([ids[R.library_order(r, ids)[:10]] for r in s])
    rec = []
    for p in (1, 2, 4, 8, 32):
        view = ix.with_nprobe(p)
        val, idx, n = ctx.score_topk(ctx.l2_normalize(_t(q)), view, 10)
        assert n == 10
        rec.append(R.recall_at(idx.cpu().numpy(), exact))
        hits = util.semantic_search(_t(q), view, top_k=10)
        want = [[j for j in row if j >= 0] for row in idx.cpu().tolist()]
        assert [[h["corpus_id"] for h in row] for row in hits] == want
    print("recall@10 at nprobe 1, 2, 4, 8, 32:", rec)
    assert rec == sorted(rec) and rec[-1] == 1.0 and rec[2] >= 0.90


def test_util_builders_wrap_the_same_steps(ctx, built):
    from sgpt_amd import util
    x, _, ix, _ = built
    again = util.build_ivf_index(_t(x), nlist=32, n_iter=8)
    assert torch.equal(again.rows.view(torch.int16), ix.rows.view(torch.int16)) and torch.equal(again.ids, ix.ids)
    cent, labels = util.kmeans(_t(x), 32, n_iter=8)
    assert torch.equal(cent, ix.centroids)
    want = torch.empty_like(labels)
    want[ix.ids] = torch.repeat_interleave(torch.arange(32, device=labels.device), ix.offsets[1:] - ix.offsets[:-1])
    assert torch.equal(labels, want)


# ---- 7. skew and size ----
def test_one_list_holds_most_of_a_million_rows(ctx):
    N, d, nlist = 1_000_003, 32, 1000
    rng = np.random.default_rng(7)
    a = np.where(rng.random(N) < 0.6, 500, rng.integers(0, nlist, N))
    offsets, perm = ctx.ivf_lists(_t(a), nlist)
    ro, rp = R.lists(a, nlist)
    assert np.array_equal(offsets.cpu().numpy(), ro) and np.array_equal(perm.cpu().numpy(), rp)
    q, docs = _patterned(2, N, d)
    rows = ctx.gather_rows(_t(docs), perm)
    rows16 = docs.astype(np.float16)[rp]
    assert np.array_equal(rows.cpu().numpy(), rows16)
    i, c = np.arange(d, dtype=np.int64)[None, :], np.arange(nlist, dtype=np.int64)[:, None]
    centroids = ((c * 3 + i * 5 + (c * i) % 4) % 7 - 3).astype(np.float32)
    centroids[500] = q[0]                                                        # query 0 probes the long list first
    from sgpt_amd import IVFCorpus
    ix = IVFCorpus(_t(centroids), rows, perm, offsets, int(np.diff(ro).max()), 4, _t(R.f16(centroids)))
    val, idx, n, probes = ix.search(ctx, _t(q), 10, return_probes=True)
    probes = probes.cpu().numpy()
    assert n == 10 and probes[0, 0] == 500 and np.array_equal(probes, R.probe_sets(q, R.f16(centroids), 4))
    rv, ri, _ = R.search(q, rows16, rp, ro, probes, 10)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(val.cpu().numpy(), rv.astype(np.float32))
