"""CPU tests of tests/topk_ref.py (the reference order of the top-k select), and the condition on the inputs of tests/test_gpu_topk.py:
every case reaches the exit of topk_select_kernel it names, and the table reaches every exit."""
import numpy as np
import pytest

import topk_ref as R
import test_gpu_topk as G

INF = np.float32(np.inf)


@pytest.mark.parametrize("n,k", [(1, 1), (17, 5), (300, 300), (5000, 64), (100, 250)])
def test_select_ref_is_the_stable_argsort_on_finite_rows(n, k):
    x = np.random.default_rng(n + k).standard_normal(n).astype(np.float32)
    x[::7] = x[0]                                                    # ties: the lower index first
    order = np.argsort(-x, kind="stable")[:k]
    ov, oi = R.select_ref(x, 100, None, None, k, 1)
    kk = min(k, n)
    assert np.array_equal(ov[:kk], x[order]) and np.array_equal(oi[:kk], order + 100)
    assert np.all(ov[kk:] == -INF) and np.all(oi[kk:] == -1)


def test_select_ref_on_the_rows_of_the_short_row_merge_test():
    """The literal inputs of test_gpu_kernels.py::test_topk_merge_duplicate_pairs_and_nan_same_order_on_both_short_row_paths."""
    rng = np.random.default_rng(11)
    nq, m, k = 4, 60, 16
    val = rng.standard_normal((nq, m)).astype(np.float32)
    idx = np.stack([rng.permutation(500)[:m] for _ in range(nq)]).astype(np.int64)
    val[0, 7] = val[0, 3] = 9.0; idx[0, 7] = idx[0, 3] = 77
    val[1, 10] = val[1, 20] = val[1, 30] = float(val[1].max()) + 1.0; idx[1, [10, 20, 30]] = [5, 5, 4]
    val[2, 2] = np.nan; val[2, 9] = np.inf
    val[3, 4] = -0.0; val[3, 5] = 0.0; idx[3, 4], idx[3, 5] = 9, 8; val[3, 6:] = -np.abs(val[3, 6:]) - 1.0; val[3, :4] = -5.0
    idx[:, -3:] = -1
    out = [R.select_ref(None, 0, val[r], idx[r], k, 0) for r in range(nq)]
    ov = np.stack([o[0] for o in out]); oi = np.stack([o[1] for o in out])
    assert oi[0, :2].tolist() == [77, 77] and ov[0, :2].tolist() == [9.0, 9.0]
    assert oi[1, :3].tolist() == [4, 5, 5]
    assert np.isnan(ov[2, 0]) and oi[2, 0] == idx[2, 2] and ov[2, 1] == np.inf
    assert oi[3, :2].tolist() == [8, 9] and (oi >= 0).all()
    # one far-away id (the comparator variant of that test) changes nothing
    out2 = [R.select_ref(None, 0, np.append(val[r], np.float32(-1e30)), np.append(idx[r], (1 << 33) + 5), k, 0) for r in range(nq)]
    for a, b in zip(out, out2):
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


def test_select_ref_exclusion_empty_slots_and_tails():
    pv = np.array([3.0, 9.0, 1.0, 7.0, 5.0], np.float32)
    pi = np.array([30, -1, 10, 70, -4], np.int64)
    ov, oi = R.select_ref(None, 0, pv, pi, 4, 0, exclude=70)        # 9.0 and 5.0 sit in empty slots, 7.0 is excluded
    assert ov.tolist() == [3.0, 1.0, -INF, -INF] and oi.tolist() == [30, 10, -1, -1]
    ov, oi = R.select_ref(np.array([2.0, np.nan, -INF], np.float32), 1000, pv, pi, 6, 1, exclude=None)
    assert ov.tolist() == [7.0, 3.0, 2.0, 1.0, -1.0, -INF] and oi.tolist() == [70, 30, 1000, 10, 1001, -1]      # a -inf score: (-inf, -1)
    ov, oi = R.select_ref(np.array([1.0, 1.0], np.float32), 5, np.array([1.0], np.float32), np.array([2], np.int64), 2, 0)
    assert oi.tolist() == [2, 5]                                     # the previous leg holds the lower id: it wins the tie


def test_key32_is_monotone_and_folds_the_zeros():
    pos = np.array([0x00000000, 0x00000001, 0x00000002, 0x007fffff, 0x00800000, 0x00800001, 0x3f800000, 0x7f7fffff, 0x7f800000],
                   np.uint32)
    sweep = np.concatenate([(pos[::-1] | np.uint32(0x80000000)).view(np.float32), pos.view(np.float32)])    # -inf ... -0, +0 ... +inf
    rnd = np.sort(np.random.default_rng(0).standard_normal(1000).astype(np.float32) * np.float32(1e-38))     # subnormals among them
    for xs in (sweep, rnd):
        assert np.all(np.diff(xs.astype(np.float64)) >= 0)
        key = R.key32(xs).astype(np.int64)
        d = np.diff(key)
        assert np.all(d >= 0) and np.array_equal(d == 0, np.diff(xs.astype(np.float64)) == 0)             # equal keys exactly where the floats are equal
    assert R.key32(np.float32(-0.0)) == R.key32(np.float32(0.0))
    nan_pos, nan_neg = np.array([0x7fc00000, 0xffc00000], np.uint32).view(np.float32)
    assert R.key32(nan_pos) > R.key32(INF) and R.key32(nan_neg) < R.key32(-INF)


def test_gathered_to_rows_is_the_rank_major_to_row_major_transpose():
    world, nq, k = 3, 2, 4
    gv = np.arange(world * nq * k, dtype=np.float32).reshape(world, nq, k)
    rv, ri = R.gathered_to_rows(gv, gv.astype(np.int64))
    for q in range(nq):
        for j in range(world * k):
            assert rv[q, j] == gv[j // k, q, j % k] == ri[q, j]


def test_constants_come_from_the_kernel_source():
    c = R.constants()
    assert c["TK_THREADS"] == 256 and c["TK_THREADS"] * c["SAMPLES_PER_THREAD"] == c["TK_FAST_MIN_ROW"]
    assert c["TK_FAST_KMAX"] <= 64 and c["CAND_KEYS_MAX"] < c["TK_SORT_MAX"]


_exits = {}


def _exits_of(case):
    if case["id"] not in _exits:
        _exits[case["id"]] = G.exits_of(case)
    return _exits[case["id"]]


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c["id"])
def test_every_gpu_case_reaches_the_exit_it_names(case):
    got = set(_exits_of(case))
    assert case["exit"] in R.EXITS and case["exit"] in got, got
    assert got <= {case["exit"], *case["others"]}, got


def test_the_gpu_case_table_reaches_every_exit():
    assert len({c["id"] for c in G.CASES}) == len(G.CASES)
    named = {c["exit"] for c in G.CASES}
    reached = set().union(*[set(_exits_of(c)) & {c["exit"]} for c in G.CASES])
    assert named == reached == set(R.EXITS), set(R.EXITS) - reached
