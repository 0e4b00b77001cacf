"""-m gpu: topk_select_kernel (csrc/topk.hip) on every exit, against the full sort of tests/topk_ref.py.  The kernel moves bits and does
no arithmetic on scores: every comparison is exact equality of values and of indices.

CASES is plain data (numpy inputs made from fixed seeds); tests/test_topk_ref.py checks on the CPU that every case reaches the exit
it names and that the table reaches every exit."""
import numpy as np
import pytest

import topk_ref as R

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
NAN = np.float32(np.nan)
NEG_NAN = np.array([0xffc00000], np.uint32).view(np.float32)[0]
SENT_V, SENT_I = 12345.0, -777                                   # what every output buffer holds before the launch

CASES = []


def _case(cid, api, exit_, make, others=()):
    """exit_: the exit the case is there for (at least one row takes it); others: exits its remaining rows may take."""
    CASES.append({"id": cid, "api": api, "exit": exit_, "others": tuple(others), "make": make})


def _rng(*seed):
    return np.random.default_rng(list(seed))


# ------------------------------------------------------------------ Context.topk: fresh leg only, NaN -> -1 -----------------------
def _layout(rows, layout):
    """The rows inside a parent whose other columns hold +inf (never to be selected): "aligned" = every row base 16-byte aligned,
    ld > n; "off1" = the same 4 bytes off (scores[:, 1:]); "oddld" = odd ld, the row bases take all four alignments in turn."""
    nq, n = rows.shape
    if layout == "aligned":
        ld, col0 = (n + 3) // 4 * 4 + 4, 0
    elif layout == "off1":
        ld, col0 = (n + 1 + 3) // 4 * 4 + 4, 1
    else:
        ld, col0 = n + 1 + (n % 2), 0
    parent = np.full((nq, ld), INF, np.float32)
    parent[:, col0:col0 + n] = rows
    return parent, col0


def _topk(cid, exit_, n, k, gen, nq=5, layout="aligned", idx_base=0, others=()):
    def make():
        rows = np.ascontiguousarray(gen(_rng(n, k, nq), nq, n), dtype=np.float32)
        parent, col0 = _layout(rows, layout)
        return {"parent": parent, "col0": col0, "n": n, "k": k, "idx_base": idx_base}
    _case(cid, "topk", exit_, make, others)


def g_normal(rng, nq, n):
    return rng.standard_normal((nq, n))


def g_ascending(rng, nq, n):
    return np.sort(rng.standard_normal((nq, n)), axis=1)


def g_descending(rng, nq, n):
    return -np.sort(rng.standard_normal((nq, n)), axis=1)


def g_sawtooth(rng, nq, n):
    return np.tile(((np.arange(n) * 7) % 256).astype(np.float32), (nq, 1)) + np.arange(nq, dtype=np.float32)[:, None]


def g_planted(n_high, last_high=False):
    """A row whose candidate count is known: noise in [0, 0.1); thread t's first sample (position t * stride) holds 0.2 + t / 10^4, so
    tau is wave 3's k-th best of those; n_high scores in [1, 2) at positions the sample skips.  Count = k + n_high."""
    def gen(rng, nq, n):
        stride = n // 4096
        x = (0.1 * rng.random((nq, n))).astype(np.float32)
        x[:, np.arange(256) * stride] = np.float32(0.2) + np.arange(256, dtype=np.float32) / np.float32(1e4)
        skipped = np.setdiff1d(np.arange(n), np.arange(4096) * stride)
        for r in range(nq):
            x[r, rng.permutation(skipped)[:n_high]] += 1.0
        if last_high:
            x[:, -1] = 50.0                                          # the row's best sits on the highest index
        return x
    return gen


def g_const(rng, nq, n):
    return np.full((nq, n), 1.25, np.float32) + np.arange(nq, dtype=np.float32)[:, None]


def g_two_valued(n_high):
    def gen(rng, nq, n):
        x = np.zeros((nq, n), np.float32)
        for r in range(nq):
            x[r, rng.permutation(n)[:n_high]] = 1.0
        return x
    return gen


def g_minus_inf_but_last_20(rng, nq, n):
    x = np.full((nq, n), -INF, np.float32)
    x[:, -20:] = rng.standard_normal((nq, 20))
    return x


def g_nan_mixed(rng, nq, n):
    """Scores in (-3, -0.5): a NaN (-> -1) lands inside the top-k; NaNs at even (sampled at n = 8192) and odd positions."""
    x = (-0.5 - 2.5 * rng.random((nq, n))).astype(np.float32)
    for r in range(nq):
        x[r, rng.permutation(n)[:40 + r]] = NAN
    x[0, 0::2][:8] = NAN
    x[1, 1::2][:8] = NAN
    return x


def g_all_nan(rng, nq, n):
    return np.full((nq, n), NAN, np.float32)


def g_adjacent_floats(rng, nq, n):
    base = np.float32(1.5).view(np.uint32)
    return (base + rng.integers(0, 300, (nq, n)).astype(np.uint32)).view(np.float32)    # only the last key byte (and a bit) differs


def g_around_zero(rng, nq, n):
    """40 scores above zero (subnormals, the smallest normal), 1000 zeros of either sign -- the k-th place for 40 < k <= 1040, where
    -0.0 and +0.0 tie on the index -- and subnormals / the smallest normal below zero for the rest."""
    pos = np.array([0x00000001, 0x00000002, 0x007fffff, 0x00800000], np.uint32)
    x = (pos | np.uint32(0x80000000))[rng.integers(0, 4, (nq, n))]
    for r in range(nq):
        p = rng.permutation(n)
        x[r, p[:40]] = np.repeat(pos, 10)
        x[r, p[40:1040]] = np.where(rng.random(1000) < 0.5, np.uint32(0), np.uint32(0x80000000))
    return x.view(np.float32)


def g_inf_classes(n_pos, n_neg_from):
    """n_pos times +inf, -inf from position n_neg_from on (the k-th place falls into the one or the other class)."""
    def gen(rng, nq, n):
        x = rng.standard_normal((nq, n)).astype(np.float32)
        for r in range(nq):
            p = rng.permutation(n)
            x[r, p[:n_pos]] = INF
            x[r, p[n_neg_from:]] = -INF
        return x
    return gen


for _n in (4096, 4099, 8191, 8193, 70_001):
    for _k in (1, 10, 64):
        for _lay in ("aligned", "off1", "oddld"):
            # (k = 64 on random scores: tau is the LEAST of a wave's 64 thread maxima, about a quarter of the row is a candidate)
            _exit, _others = ("one_pass_keys", ()) if _k < 64 or _n < 8000 else \
                (("one_pass_bitonic", ("one_pass_overflow_radix",)) if _n < 9000 else ("one_pass_overflow_radix", ()))
            _topk(f"topk-onepass-n{_n}-k{_k}-{_lay}", _exit, _n, _k, g_normal, layout=_lay, others=_others)
_topk("topk-band-keys-1024", "one_pass_keys", 8192, 64, g_planted(1024 - 64))
_topk("topk-band-bitonic-1025", "one_pass_bitonic", 8192, 64, g_planted(1025 - 64))
_topk("topk-band-bitonic-2048", "one_pass_bitonic", 8192, 64, g_planted(2048 - 64))
_topk("topk-band-overflow-2049", "one_pass_overflow_radix", 8192, 64, g_planted(2049 - 64))
_topk("topk-band-overflow-n12000", "one_pass_overflow_radix", 12_000, 64, g_planted(3000))
_topk("topk-all-equal-6000", "one_pass_overflow_radix", 6000, 16, g_const)
_topk("topk-two-valued-6000", "one_pass_overflow_radix", 6000, 64, g_two_valued(30))
_topk("topk-two-valued-half", "one_pass_overflow_radix", 6000, 10, g_two_valued(3000))
for _k in (10, 64):
    _topk(f"topk-minus-inf-but-20-k{_k}", "radix" if _k == 10 else "radix_index_select", 5000, _k, g_minus_inf_but_last_20)
    _topk(f"topk-maxima-unsampled-k{_k}", "one_pass_keys", 8192, _k, g_planted(20))
    _topk(f"topk-ascending-k{_k}", "one_pass_keys", 8192, _k, g_ascending)
    _topk(f"topk-descending-k{_k}", "one_pass_keys", 8192, _k, g_descending)
    _topk(f"topk-sawtooth-k{_k}", "one_pass_bitonic" if _k == 10 else "one_pass_overflow_radix", 8192, _k, g_sawtooth)
    _topk(f"topk-nan-mixed-k{_k}", "one_pass_keys" if _k == 10 else "one_pass_bitonic", 8192, _k, g_nan_mixed)
    _topk(f"topk-all-nan-k{_k}", "one_pass_overflow_radix", 5000, _k, g_all_nan)
    for _base in ((1 << 32) - 70_000, 1 << 33):
        _topk(f"topk-big-ids-base{_base}-k{_k}", "one_pass_comparator", 70_001, _k, g_planted(200, last_high=True), idx_base=_base)
    for _n in (2049, 3000, 4095):
        _topk(f"topk-radix-gap-n{_n}-k{_k}", "radix", _n, _k, g_normal)
for _k in (65, 1001, 2048):
    for _n in (5000, 100_003):
        _topk(f"topk-radix-n{_n}-k{_k}", "radix", _n, _k, g_normal, nq=3)
_topk("topk-adjacent-floats", "radix_index_select", 5000, 100, g_adjacent_floats, others=("radix",))
_topk("topk-around-zero-gap", "radix_index_select", 3000, 64, g_around_zero)
_topk("topk-around-zero-k500", "radix_index_select", 5000, 500, g_around_zero)
_topk("topk-around-zero-onepass-k64", "one_pass_bitonic", 5000, 64, g_around_zero)       # (tau = 0: both zeros are candidates)
_topk("topk-around-zero-onepass-k10", "one_pass_keys", 5000, 10, g_around_zero)
_topk("topk-plus-inf-at-threshold", "radix_index_select", 3000, 64, g_inf_classes(100, 2000))
_topk("topk-minus-inf-at-threshold", "radix_index_select", 3000, 64, g_inf_classes(5, 40))
_topk("topk-minus-inf-short-row", "short", 300, 64, g_inf_classes(5, 40))
_topk("topk-minus-inf-everything-survives", "all_survive", 50, 64, g_inf_classes(5, 40))
_topk("topk-k3000-n10000", "radix_unsorted", 10_000, 3000, g_normal, nq=3)
_topk("topk-k3000-n10000-minus-inf", "radix_unsorted", 10_000, 3000, g_inf_classes(5, 2000), nq=3)
_topk("topk-k3000-n2500", "all_survive", 2500, 3000, g_normal, nq=3)


# ------------------------------------------------------------------ Context.topk_merge: previous leg only, exclusion --------------
def _merge(cid, exit_, make, others=()):
    _case(cid, "merge", exit_, make, others)


def _unique_ids(rng, nq, m, hi=1_000_000):
    return np.stack([rng.permutation(hi)[:m] for _ in range(nq)]).astype(np.int64)


def _merge_random(m, k):
    def make():
        rng, nq = _rng(m, k), 4
        val = rng.standard_normal((nq, m)).astype(np.float32)
        idx = _unique_ids(rng, nq, m)
        idx[rng.random((nq, m)) < 0.05] = -1                         # ~5 % empty slots (their values must not matter)
        ex = np.array([idx[r, np.argmax(np.where(idx[r] >= 0, val[r], -INF))] for r in range(nq)], np.int64)   # the row's best
        ex[nq - 1] = 2_000_000                                       # one row whose excluded id is absent
        return {"val": val, "idx": idx, "k": k, "exclude": ex}
    return make


for _m in (2048, 2049, 4095, 4096, 9000):
    for _k in (11, 64, 65, 300):
        _exit = "radix" if _k > 64 or 2048 < _m < 4096 else ("short" if _m <= 2048 else "one_pass_keys")
        if (_m, _k) == (9000, 64):
            _exit = "one_pass_bitonic"                              # (stride 2: half the row sampled, a quarter of it above tau)
        _merge(f"merge-m{_m}-k{_k}", _exit, _merge_random(_m, _k))


def _merge_index_byte(b):
    """60 clear winners, then a 3000-way tie for the last 40 of k = 100 places.  The tied ids spread over 64 digits of byte b and 47 of
    byte (b + 3) % 8: the second radix select narrows in both, so every one of its eight passes sees many bins in one case or another."""
    def make():
        rng, nq, k = _rng(77, b), 3, 100
        j = np.arange(3000, dtype=np.int64)
        tied = 3 + ((j % 64) << (8 * b)) + ((j // 64) << (8 * ((b + 3) % 8)))
        assert tied.max() < (1 << 62) and len(set(tied.tolist())) == 3000
        ids = np.concatenate([tied, (1 << 40) + np.arange(100, dtype=np.int64) * 3 + 1])
        base = np.concatenate([np.full(3000, 0.5, np.float32), np.full(60, 2.0, np.float32) + np.arange(60, dtype=np.float32),
                               np.full(40, -1.0, np.float32)])
        val, idx = [], []
        for _ in range(nq):
            p = rng.permutation(len(ids))
            val.append(base[p]); idx.append(ids[p])
        return {"val": np.stack(val), "idx": np.stack(idx), "k": k, "exclude": None}
    return make


for _b in range(8):
    _merge(f"merge-index-radix-byte{_b}", "radix_index_select", _merge_index_byte(_b))


def _nan_head():
    """300 candidates: a positive NaN, +inf, a negative NaN among ordinary scores."""
    rng = _rng(300, 16)
    val = rng.standard_normal((4, 300)).astype(np.float32)
    idx = _unique_ids(rng, 4, 300, hi=100_000)
    for r in range(4):
        val[r, 10 + r], val[r, 100 + r], val[r, 200 + r] = NAN, INF, NEG_NAN
    return val, idx


def _merge_nan(m):
    def make():
        val, idx = _nan_head()
        if m > 300:                                                  # filler below every score of the head, ids above them
            rng = _rng(m)
            fill = (-100.0 - rng.random((4, m - 300))).astype(np.float32)
            fid = 100_000 + _unique_ids(rng, 4, m - 300)
            val, idx = np.concatenate([val, fill], axis=1), np.concatenate([idx, fid], axis=1)
            p = rng.permutation(m)
            val, idx = val[:, p], idx[:, p]
        return {"val": val, "idx": idx, "k": 16, "exclude": None}
    return make


for _m, _exit in ((300, "short"), (3000, "radix"), (5000, "one_pass_keys")):
    _merge(f"merge-nan-m{_m}", _exit, _merge_nan(_m))


def _merge_repeated_pairs(k):
    def make():
        rng, nq, m = _rng(5000, k), 4, 5000
        val = rng.standard_normal((nq, m)).astype(np.float32)
        idx = _unique_ids(rng, nq, m)
        for r in range(nq):
            order = np.argsort(-val[r])
            top, kth = order[0], order[k - 2]                       # (the copy moves the original k-th down one place)
            val[r, order[-1]], idx[r, order[-1]] = val[r, top], idx[r, top]          # the best pair twice
            val[r, order[-2]], idx[r, order[-2]] = val[r, kth], idx[r, kth]          # a pair twice, across the k-th place
            val[r, order[-3]], idx[r, order[-3]] = val[r, kth], idx[r, kth]
        return {"val": val, "idx": idx, "k": k, "exclude": None}
    return make


_merge("merge-repeated-pairs-k16", "one_pass_keys", _merge_repeated_pairs(16))
_merge("merge-repeated-pairs-k100", "radix_index_select", _merge_repeated_pairs(100))


def _merge_minus_inf_real_ids():
    """Fewer than k scores above -inf: documents that scored -inf and empty slots alike come back as (-inf, -1)."""
    rng, nq, m = _rng(3000, 1), 3, 3000
    val = np.full((nq, m), -INF, np.float32)
    idx = _unique_ids(rng, nq, m)
    val[:, :30] = rng.standard_normal((nq, 30))
    idx[:, 40:60] = -1
    p = rng.permutation(m)
    return {"val": val[:, p], "idx": idx[:, p], "k": 64, "exclude": idx[:, 0].copy()}


_merge("merge-minus-inf-real-ids", "radix_index_select", _merge_minus_inf_real_ids)


# ------------------------------------------------------------------ Context.fold_gathered_topk: the gathered address map ----------
def _fold(world, k, k_out, exit_, others=()):
    def make():
        rng, nq = _rng(world, k, k_out), 4
        gv = rng.standard_normal((world, nq, k)).astype(np.float32)
        gi = np.stack([w * 1_000_000 + _unique_ids(rng, nq, k) for w in range(world)])        # rank w holds shard w's ids
        live = [w for w in range(world) if w != 1]
        tie = np.float32(np.sort(gv[live, 2, :].ravel())[::-1][k_out - 1])
        gv[:, 2, :3] = tie                                           # row 2: the k_out-th place tied across every rank
        gv[1, :, :] = INF; gi[1, :, :] = -1                          # rank 1: all empty slots (whatever the values say)
        ex = np.full(nq, -1, np.int64)
        ex[0] = gi[0, 0, np.argmax(gv[0, 0])]                        # row 0: rank 0 holds the excluded id (its best)
        ex[1] = gi[world - 1, 1, np.argmax(gv[world - 1, 1])]        # row 1: the last rank does
        return {"gv": gv, "gi": gi, "k_out": k_out, "exclude": ex}
    _case(f"fold-w{world}-k{k}-kout{k_out}", "fold", exit_, make, others)


_fold(8, 11, 11, "short")
_fold(3, 64, 64, "short")
_fold(8, 300, 300, "radix", others=("radix_index_select",))         # (row 2, the tie across the ranks: the index select)
_fold(16, 300, 64, "one_pass_keys", others=("one_pass_bitonic",))
_fold(5, 1000, 10, "one_pass_keys")


# ------------------------------------------------------------------ both legs in one launch: score_topk(run=...), fp32 corpus ------
def _score(cid, exit_, k, n1, base2=None, tie=True, others=()):
    """Query r = unit vector e_r, document i = s[:, i]: the fp32 score of (r, i) is s[r, i] exactly, so the select's fresh leg IS s.
    First call: n1 documents from index 0; second call: 5003 documents from base2 on top of the first call's list."""
    def make():
        rng, nq, n2 = _rng(k, n1), 4, 5003
        s1 = rng.standard_normal((nq, n1)).astype(np.float32)
        s2 = rng.standard_normal((nq, n2)).astype(np.float32)
        if tie:                                                      # the k-th place: a tie between both legs, the lower ids in the first
            for r in range(nq):
                t = np.float32(np.sort(np.concatenate([s1[r], s2[r]]))[::-1][max(k - 3, 0)])
                s1[r, rng.permutation(n1)[:min(3, n1)]] = t
                s2[r, rng.permutation(n2)[:6]] = t
        return {"s1": s1, "s2": s2, "k": k, "base2": n1 if base2 is None else base2}
    _case(cid, "score", exit_, make, others)


for _k, _exit in ((8, "one_pass_keys"), (64, "one_pass_keys"), (100, "radix_index_select")):
    _score(f"score-two-legs-k{_k}", _exit, _k, 4001, others=("one_pass_bitonic",) if _k == 64 else ())
_score("score-short-previous-list-k8", "one_pass_keys", 8, 5)
_score("score-short-previous-list-k64", "one_pass_keys", 64, 5, others=("one_pass_bitonic",))
_score("score-second-call-at-2^32-k8", "one_pass_comparator", 8, 4001, base2=1 << 32)
_score("score-second-call-at-2^32-k100", "radix_index_select", 100, 4001, base2=1 << 32)


# ------------------------------------------------------------------ the rows of a case, as select_ref takes them -------------------
def rows_of(case, inp):
    """-> [(fresh, idx_base, prev_val, prev_idx, k, nan_to_m1, exclude)] of the launch the case is there for."""
    api = case["api"]
    if api == "topk":
        rows = inp["parent"][:, inp["col0"]:inp["col0"] + inp["n"]]
        return [(r, inp["idx_base"], None, None, inp["k"], 1, None) for r in rows]
    if api == "merge":
        ex = inp["exclude"]
        return [(None, 0, v, i, inp["k"], 0, None if ex is None else ex[q]) for q, (v, i) in enumerate(zip(inp["val"], inp["idx"]))]
    if api == "fold":
        rv, ri = R.gathered_to_rows(inp["gv"], inp["gi"])
        return [(None, 0, v, i, inp["k_out"], 0, inp["exclude"][q]) for q, (v, i) in enumerate(zip(rv, ri))]
    k = inp["k"]
    out = []
    for s1, s2 in zip(inp["s1"], inp["s2"]):
        pv, pi = R.select_ref(s1, 0, None, None, k, 0)               # the first call's list; its first min(k, n1) columns are handed on
        n_run = min(k, len(s1))
        out.append((s2, inp["base2"], pv[:n_run], pi[:n_run], k, 0, None))
    return out


def exits_of(case, inp=None):
    inp = case["make"]() if inp is None else inp
    got = []
    for fresh, base, pv, pi, k, nan1, ex in rows_of(case, inp):
        vals, ids = R.virtual_row(fresh, base, pv, pi, nan1, ex)
        got.append(R.path_of(0 if fresh is None else len(fresh), 0 if pv is None else len(pv), k, vals, ids))
    return got


# ------------------------------------------------------------------ the launches ------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _outputs(nq, k):
    import torch
    return (torch.full((nq, k), SENT_V, dtype=torch.float32, device="cuda:0"), torch.full((nq, k), SENT_I, dtype=torch.int64, device="cuda:0"))


def _launch(ctx, case, inp):
    """-> [(values [nq, k], indices [nq, k])] numpy: the C entry point on sentinel-filled outputs, then the Context method the case
    names (which allocates its own)."""
    from sgpt_amd.runtime import _p, _stream_ptr
    st = _stream_ptr(ctx.device)
    api = case["api"]
    if api == "topk":
        view = _dev(inp["parent"])[:, inp["col0"]:inp["col0"] + inp["n"]]      # a row-sliced tensor, passed straight through
        nq, n = view.shape
        ov, oi = _outputs(nq, inp["k"])
        ctx._chk(ctx.lib.sgpt_topk(ctx.handle, _p(view), nq, n, view.stride(0), inp["k"], inp["idx_base"], _p(ov), _p(oi), st), "sgpt_topk")
        outs = [(ov, oi), ctx.topk(view, inp["k"], idx_base=inp["idx_base"])]
    elif api == "merge":
        val, idx = _dev(inp["val"]), _dev(inp["idx"])
        ex = None if inp["exclude"] is None else _dev(inp["exclude"])
        nq, m = val.shape
        ov, oi = _outputs(nq, inp["k"])
        ctx._chk(ctx.lib.sgpt_topk_merge(ctx.handle, _p(val), _p(idx), nq, m, inp["k"], _p(ex), _p(ov), _p(oi), st), "sgpt_topk_merge")
        outs = [(ov, oi), ctx.topk_merge(val, idx, inp["k"], exclude_idx=ex)]
    elif api == "fold":
        gv, gi, ex = _dev(inp["gv"]), _dev(inp["gi"]), _dev(inp["exclude"])
        world, nq, k = gv.shape
        ov, oi = _outputs(nq, inp["k_out"])
        ctx._chk(ctx.lib.sgpt_fold_gathered_topk(ctx.handle, _p(gv), _p(gi), world, nq, k, inp["k_out"], _p(ex), _p(ov), _p(oi), st),
                 "sgpt_fold_gathered_topk")
        outs = [(ov, oi), ctx.fold_gathered_topk(gv, gi, inp["k_out"], exclude_idx=ex)]
    else:
        raise AssertionError(api)
    return [(v.cpu().numpy(), i.cpu().numpy()) for v, i in outs]


def _assert_rows(got_v, got_i, want, sorted_output=True):
    for q, (wv, wi) in enumerate(want):
        gv, gi = got_v[q], got_i[q]
        if not sorted_output:                                        # k > 2048: the same multiset of (value, index) pairs
            go, wo = np.lexsort((gi, R.key32(gv))), np.lexsort((wi, R.key32(wv)))
            gv, gi, wv, wi = gv[go], gi[go], wv[wo], wi[wo]
        assert np.array_equal(gi, wi), f"row {q}: indices"
        assert np.array_equal(gv, wv, equal_nan=True), f"row {q}: values"


@pytest.mark.parametrize("case", [c for c in CASES if c["api"] != "score"], ids=lambda c: c["id"])
def test_select_equals_the_sorted_row(ctx, case):
    inp = case["make"]()
    rows = rows_of(case, inp)
    want = [R.select_ref(*row) for row in rows]
    k = rows[0][4]
    for got_v, got_i in _launch(ctx, case, inp):
        _assert_rows(got_v, got_i, want, sorted_output=k <= R.constants()["TK_SORT_MAX"])


@pytest.mark.parametrize("case", [c for c in CASES if c["api"] == "score"], ids=lambda c: c["id"])
def test_both_legs_in_one_launch(ctx, case):
    import torch
    inp = case["make"]()
    k, s1, s2 = inp["k"], inp["s1"], inp["s2"]
    nq = s1.shape[0]
    q = torch.eye(4, dtype=torch.float32, device="cuda:0")[:nq]
    val, idx = _outputs(nq, k)
    val, idx, n_run = ctx.score_topk(q, _dev(s1.T), k, idx_base=0, run=(val, idx, 0))
    assert n_run == min(k, s1.shape[1])
    _assert_rows(val.cpu().numpy(), idx.cpu().numpy(), [R.select_ref(r, 0, None, None, k, 0) for r in s1])
    val, idx, n = ctx.score_topk(q, _dev(s2.T), k, idx_base=inp["base2"], run=(val, idx, n_run))
    assert n == k
    _assert_rows(val.cpu().numpy(), idx.cpu().numpy(), [R.select_ref(*row) for row in rows_of(case, inp)])


def test_big_index_bases_give_the_order_of_base_zero(ctx):
    """The comparator finish (an index >= 2^32 - 1 among the candidates) against the register-key finish on the same rows."""
    by_id = {c["id"]: c for c in CASES}
    for k in (10, 64):
        got = {}
        for base in (0, (1 << 32) - 70_000, 1 << 33):
            inp = by_id[f"topk-big-ids-base{1 << 33}-k{k}"]["make"]()
            inp["idx_base"] = base
            got[base] = _launch(ctx, by_id[f"topk-big-ids-base{1 << 33}-k{k}"], inp)[0]
        for base in got:
            assert np.array_equal(got[base][0], got[0][0]) and np.array_equal(got[base][1] - base, got[0][1])


def test_nan_candidates_rank_the_same_at_every_row_length(ctx):
    """A positive NaN first, then +inf, on the short-row, the radix and the one-pass path alike; the negative NaN nowhere in the list."""
    by_id = {c["id"]: c for c in CASES}
    got = {m: _launch(ctx, by_id[f"merge-nan-m{m}"], by_id[f"merge-nan-m{m}"]["make"]())[0] for m in (300, 3000, 5000)}
    head_v, head_i = _nan_head()
    for m, (gv, gi) in got.items():
        assert np.array_equal(gi, got[300][1]) and np.array_equal(gv, got[300][0], equal_nan=True), m
        for r in range(4):
            assert np.isnan(gv[r, 0]) and gi[r, 0] == head_i[r, 10 + r] and gv[r, 1] == INF and gi[r, 1] == head_i[r, 100 + r]
            assert head_i[r, 200 + r] not in gi[r].tolist()


def test_filtered_scorer_merges_candidates_with_ids_above_2_32(ctx):
    """cand_merge_kernel's comparator rounds (its key rounds need ids < 2^32 - 1): the filtered schedule at idx_base = 2^33 returns
    the lists of idx_base = 0, shifted."""
    import torch
    nq, d, N, k = 16, 128, 300_000, 10
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randn(nq, d, generator=g).cuda().to(torch.float16)
    c = (torch.randn(N, d, generator=g) * 0.1).cuda().to(torch.float16)
    v0, i0, n0 = ctx.score_topk(q, c, k)
    v1, i1, n1 = ctx.score_topk(q, c, k, idx_base=1 << 33)
    assert n0 == n1 == k
    assert torch.equal(v0, v1) and torch.equal(i1 - (1 << 33), i0)
    assert (i0 >= 0).all() and (i0 < N).all()
