"""CPU tests of tests/score_ref.py, the float64 reference of tests/test_gpu_score_f64.py: (1) the reference checks itself -- the three
properties of the exact operands, the filler / signal separation of leg D, the cap on ambiguous rows of leg F; (2) every shape of the
table reaches the launch it is listed for -- the plans of tests/score_plan_dump.cpp, the launch rule mirrored in tests/gemm_ref.py;
(3) the checkers can fail: six defects applied to the float64 reference, as if a kernel had produced it, are each rejected."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gemm_ref as G
import score_ref as S
import test_score_plan as TP

TOPK_CASES = S.CASES + S.CASES_F


# ---------------------------------------------------------------- 1. the reference checks itself ---------------------------------
def _shifted(x):
    """Every aligned 8-element k-slice of the rows replaced by its neighbour: the next one, or the one before where the next is
    missing or shorter."""
    d = x.shape[1]
    y = x.copy()
    for k0 in range(0, d if d > 8 else 0, 8):         # (one slice: it has no neighbour)
        n = min(8, d - k0)
        src = k0 + 8 if min(8, d - k0 - 8) >= n else k0 - 8
        y[:, k0:k0 + n] = x[:, src:src + n]
    return y


@pytest.mark.parametrize("name", [c.name for c in S.CASES + S.CASES_G])
def test_exact_operands_have_their_three_properties(name):
    c = S.case(name)
    leg_d = getattr(c, "leg", "") == "D"
    nq, N = (c.na, c.nb) if isinstance(c, S.CaseG) else (c.nq, c.N)
    q, rows = S.exact_operands(nq, N, c.d, S.FILLER if leg_d else 0)
    # asymmetric: the query and document patterns differ
    m = min(nq, N)
    assert m == 1 or not np.array_equal(q[:m], rows[:m])
    # (a) every operand is a bf16 and an f16 value
    for x in (q, rows):
        for fmt in S.F16:
            assert np.array_equal(S.rounded(x, fmt)[1], x.astype(np.float64)), fmt
    if leg_d:       # the signal documents and a piece of the filler (the parity argument is the same for every row)
        rows = np.concatenate([rows[:1024], rows[S.FILLER:]])
    q64, c64 = q.astype(np.float64), rows.astype(np.float64)
    # (b) every partial sum, in any order, stays below 2^24
    assert (np.abs(q64) @ np.abs(c64).T).max() < 2 ** 24
    # (c) dropping / doubling a slice changes the score by the slice's sum: never zero; a slice read from the neighbouring k offset,
    # in either operand, changes the slice's sum: never by zero
    qs, cs = _shifted(q64), _shifted(c64)
    for k0 in range(0, c.d, 8):
        sl = slice(k0, min(k0 + 8, c.d))
        part = q64[:, sl] @ c64[:, sl].T
        assert (part != 0).all(), f"slice at {k0}: a zero sum"
        if c.d > 8:
            assert (qs[:, sl] @ c64[:, sl].T != part).all() and (q64[:, sl] @ cs[:, sl].T != part).all(), f"slice at {k0}: a shift goes unseen"


@pytest.mark.parametrize("kind,fmt", [("exact", "f16"), ("gauss", "f16"), ("gauss", "bf16")])
@pytest.mark.parametrize("name", [c.name for c in S.CASES if c.leg == "D"])
def test_leg_d_filler_scores_lie_below_every_signal_score(name, kind, fmt):
    """The k returned entries of a leg D call are exactly the documents of the folded launch: the highest filler score plus its bound
    is below the lowest signal score minus its bound, from the float64 reference alone."""
    c = S.case(name)
    _, _, q64, c64 = S.operands(name, fmt, kind)
    hi_filler, lo_signal = -np.inf, np.inf
    ct, act = np.ascontiguousarray(c64.T), np.ascontiguousarray(np.abs(c64).T)
    for r0 in range(0, c.nq, 100):      # (S.scores64 and S.bound without their NaN handling: these operands have none)
        s, b = q64[r0:r0 + 100] @ ct, G.bound_from(np.abs(q64[r0:r0 + 100]) @ act, None, None, c.d)
        hi_filler = max(hi_filler, float((s + b)[:, :S.FILLER].max()))
        lo_signal = min(lo_signal, float((s - b)[:, S.FILLER:].min()))
    print(f"{name} {kind} {fmt}: highest filler score + bound = {hi_filler:.6g}, lowest signal score - bound = {lo_signal:.6g}")
    assert hi_filler < lo_signal
    assert c.N - S.FILLER == c.k


@pytest.mark.parametrize("fmt", S.F16)
@pytest.mark.parametrize("name", [c.name for c in S.CASES_F])
def test_leg_f_ambiguous_rows_stay_under_the_cap(name, fmt):
    """Condition, not a measurement: at most 5 % of a case's rows have their float64 k-th and (k + 1)-th scores closer than twice the
    larger of their bounds (computed from the reference alone, for the seed the GPU test uses)."""
    c = S.case(name)
    _, _, q64, c64, top_v, top_i = S.filtered_case(c.nq, c.N, c.d, fmt)
    assert c.k < S.F_KMAX
    assert (top_v[:, 1:] <= top_v[:, :-1]).all()
    share = float(S.ambiguous_rows(q64, c64, top_v, top_i, c.k).mean())
    print(f"{name} {fmt}: share of ambiguous rows = {100 * share:.2f} %")
    assert share <= 0.05


# ---------------------------------------------------------------- 2. every shape reaches its leg ---------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++) to build tests/score_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("score_ref_plan") / "score_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", TP.SRC, "-o", exe], check=True)
    return exe


def test_every_topk_shape_reaches_its_leg(dump):
    lines = "".join(f"{c.nq} {c.N} {c.d} {c.k} {'f32' if c.fmts == ('fp32',) else '16'} 0 0\n" for c in TOPK_CASES)
    r = subprocess.run([dump], input=lines, capture_output=True, text=True, check=True)
    plans = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(plans) == len(TOPK_CASES)
    for c, p in zip(TOPK_CASES, plans):
        assert set(c.plan) >= {"fast", "nq_pad", "filt", "sampled", "top2", "chunk", "first", "chunks", "rest"}, c.name
        for field, want in c.plan.items():
            assert p[field] == want, (c.name, field, p[field], want)
        n256, tail = c.N // 256 * 256, c.N % 256
        if c.leg in "ABC":
            # one materialised tile: whole 256-document tiles on the tile kernels, a tail that does NOT fold (na + 256 > the score
            # rows of `chunk` floats) on the register-staged kernel
            assert p["rest"] == c.N == c.k and n256 == 768 and tail == 37 and n256 + 256 > p["chunk"], c.name
        if c.leg == "A":
            assert c.nq <= 64 and p["nq_pad"] == 64, c.name
        if c.leg == "B":
            assert p["nq_pad"] % 256 == 0 and p["nq_pad"] < 768, c.name                 # deep_a = M >= N is false
        if c.leg == "C":
            assert p["nq_pad"] % 256 == 0 and p["nq_pad"] >= 768, c.name                # deep_a is true
        if c.leg == "D":
            # two chunks, the second of nc = k documents; tile_folds (score_plan.h) recomputed: na + 256 <= ld = chunk, the predicate
            nc = c.N - p["chunk"]
            na = nc // 256 * 256
            assert p["chunk"] == S.FILLER and 0 < nc == c.k < p["chunk"] and 0 < na < nc, c.name
            assert na + 256 <= p["chunk"] and TP._foldable(p["nq_pad"], na + 256, c.d), c.name
        if c.leg == "E":
            assert not p["fast"] and (c.fmts == ("fp32",) or c.d < 128 or c.d % 64), c.name
        if c.leg == "F":
            assert p["filt"] and p["rest"] == 0 and bool(p["sampled"]) == (c.k <= 64) == (p["first"] == 0), c.name
    f10, f100, f16 = (S.case(n).plan for n in ("F-nq2048-k10", "F-nq2048-k100", "F-nq16-k10"))
    assert f10["top2"] and f10["chunks"][-1][2] and f100["chunks"][-1][2] and len(f100["chunks"]) == 2      # the sample in the GEMM; folds
    assert f16["nq_pad"] == 64 and f16["chunks"][-1][4]                                                       # the 64-row tile's tail launch


def test_every_scores_shape_stays_on_the_register_staged_kernel():
    """sgpt_scores is EPI_STORE with an fp32 output through launch_gemm16 / launch_gemm (csrc/gemm.hip), mirrored by
    gemm_ref.linear_variant: no shape of leg G takes the 256x256 kernel, and the table reaches one-tile and many-tile launches of the
    64x64 tile in the run order and the 128x128 tile in the supertile order."""
    seen = set()
    for c in S.CASES_G:
        for fmt in c.fmts:
            kernel, order = G.linear_variant(fmt, G.EPI_STORE, False, c.na, c.nb, c.d)
            assert kernel in ("rs64-deep", "rs128"), (c.name, kernel)
            t = G.tile_of(kernel)
            seen.add((fmt == "fp32", t, order, 1 if (-(-c.na // t)) * (-(-c.nb // t)) == 1 else 2))
            assert c.d % (4 if fmt == "fp32" else 8) == 0
    for f32 in (False, True):
        assert {(f32, 64, "run", 1), (f32, 64, "run", 2), (f32, 128, "supertile", 2)} <= seen


# ---------------------------------------------------------------- 3. the checks can fail -----------------------------------------
def _as_kernel(scores, k, first_idx):
    """What a correct select returns for a score tile: fp32 values, the lowest-index order."""
    val, idx = S.topk(scores.astype(np.float32), k, first_idx)
    return val, idx, k


def _both(name, fmt="f16", nan_docs=()):
    """{kind: (ref, bnd, q64, c64)} over the checked documents of a case, exact and Gaussian."""
    c, out = S.case(name), {}
    for kind in ("exact", "gauss"):
        qt, ct, _, _ = S.operands(name, fmt, kind)
        ct = ct[S.doc0_of(c):]
        if nan_docs:
            ct = S.with_nan(ct, nan_docs)
        q64, c64 = qt.double().numpy(), ct.double().numpy()
        out[kind] = (S.scores64(q64, c64, True), S.bound(q64, c64), q64, c64)
    return out


def _rejected(kind, scores, ref, bnd, k, first_idx=S.BIG_BASE):
    val, idx, n = _as_kernel(scores, k, first_idx)
    with pytest.raises(AssertionError):
        if kind == "exact":
            S.check_exact(val, idx, n, ref, k, first_idx)
        else:
            S.check_bounded(val, idx, n, ref, bnd, k, first_idx)


def _accepted(kind, ref, bnd, k, first_idx=S.BIG_BASE):
    val, idx, n = _as_kernel(ref, k, first_idx)
    if kind == "exact":
        return S.check_exact(val, idx, n, ref, k, first_idx)
    return S.check_bounded(val, idx, n, ref, bnd, k, first_idx)


A_CASE, D_CASE = "A-nq33-d192", "D-nq100-nc549"


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_the_checkers_accept_the_reference_and_reject_each_defect(kind):
    ref, bnd, q64, c64 = _both(A_CASE)[kind]
    k = ref.shape[1]
    assert _accepted(kind, ref, bnd, k) < 0.02          # (the fp32 rounding of the float64 score is far inside the bound)
    # a dropped 8-element k-slice in one lane's rows: documents 256 + 16 j + 3 of the second tile lose k = 16 .. 23
    lane = np.arange(256 + 3, 512, 16)
    bad = ref.copy()
    bad[:, lane] -= q64[:, 16:24] @ c64[lane, 16:24].T
    _rejected(kind, bad, ref, bnd, k)
    # two documents of a tile swapped
    bad = ref.copy()
    bad[:, [260, 300]] = ref[:, [300, 260]]
    _rejected(kind, bad, ref, bnd, k)
    # the tail's columns shifted by one
    bad = ref.copy()
    bad[:, 768:k - 1] = ref[:, 769:k]
    _rejected(kind, bad, ref, bnd, k)
    # leg G's checker, the same three defects
    ldo = k + 7
    for cols, val in ((lane, ref[:, lane] - q64[:, 16:24] @ c64[lane, 16:24].T), ([260, 300], ref[:, [300, 260]]), (np.arange(768, k - 1), ref[:, 769:k])):
        bad = ref.copy()
        bad[:, cols] = val
        for scores, ok in ((ref, True), (bad, False)):
            bits = np.full((ref.shape[0], ldo), S.SENT32, np.int32)
            bits[:, :k] = scores.astype(np.float32).view(np.int32)
            if ok:
                assert S.check_scores(bits, k, ref, bnd, kind == "exact") < 0.02
            else:
                with pytest.raises(AssertionError):
                    S.check_scores(bits, k, ref, bnd, kind == "exact")
    bits = np.full((ref.shape[0], ldo), S.SENT32, np.int32)
    bits[:, :k + 1] = np.concatenate([ref, ref[:, -1:]], axis=1).astype(np.float32).view(np.int32)
    with pytest.raises(AssertionError, match="pad columns"):          # a store past nb
        S.check_scores(bits, k, ref, bnd, kind == "exact")


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_the_fold_mask_off_by_one_is_rejected(kind):
    """Leg D: document n_valid (one past the last) scored from the clamped row -- a copy of the last document's score under the
    next index.  It enters the k best of every query whose last document is not its lowest."""
    ref, bnd, _, _ = _both(D_CASE)[kind]
    k = ref.shape[1]
    first = S.BIG_BASE + S.FILLER
    assert _accepted(kind, ref, bnd, k, first) < 0.02
    _rejected(kind, np.concatenate([ref, ref[:, -1:]], axis=1), ref, bnd, k, first)


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_a_nan_left_as_nan_is_rejected(kind):
    docs = (300, 790)
    ref, bnd, _, _ = _both(A_CASE, nan_docs=docs)[kind]
    k = ref.shape[1]
    assert (ref[:, docs] == -1).all()
    val, idx, n = _as_kernel(ref, k, 0)
    check = (lambda v: S.check_exact(v, idx, n, ref, k, 0)) if kind == "exact" else (lambda v: S.check_bounded(v, idx, n, ref, bnd, k, 0))
    check(val)
    bad = val.copy()
    bad[np.isin(idx, docs)] = np.nan
    with pytest.raises(AssertionError):
        check(bad)


def test_a_tie_returned_highest_index_first_is_rejected():
    ref, bnd, _, _ = _both(A_CASE)["exact"]
    k = ref.shape[1]
    assert sum(len(np.unique(row)) < k for row in ref) == ref.shape[0]           # ties are plentiful with integer operands
    order = np.lexsort((-np.broadcast_to(np.arange(k), ref.shape), -ref), axis=1)
    val, idx = np.take_along_axis(ref, order, axis=1).astype(np.float32), order.astype(np.int64)
    with pytest.raises(AssertionError, match="lowest-index order"):
        S.check_exact(val, idx, k, ref, k, 0)
    with pytest.raises(AssertionError, match="ascending index order"):
        S.check_bounded(val, idx, k, ref, bnd, k, 0)


def test_the_filtered_checker_rejects_a_wrong_document_and_a_wrong_value():
    """Leg F's checker on a small corpus of the same law: the float64 top-k passes; the (k + 5)-th document in place of the k-th of a
    non-ambiguous row, a value 3 bounds off and a document returned twice are each rejected."""
    nq, N, d, k = 64, 4096, 128, 10
    q, c = S.topical_corpus(3, N, d, nq)
    (_, q64), (_, c64) = S.rounded(q, "f16"), S.rounded(c, "f16")
    top_v, top_i = S.filtered_reference(q64, c64, k + 6)
    full = S.scores64(q64, c64, True)
    wv, wi = S.topk(full, k + 6)
    assert np.array_equal(wi, top_i) and np.array_equal(wv, top_v)              # the blocked reference is the plain one
    val, idx = top_v[:, :k].astype(np.float32), top_i[:, :k] + S.BIG_BASE
    ratio, share = S.check_filtered(val, idx, k, q64, c64, top_v, top_i, k, S.BIG_BASE)
    assert ratio < 0.02 and share <= 0.05
    amb = S.ambiguous_rows(q64, c64, top_v, top_i, k)
    r = int(np.flatnonzero(~amb)[0])
    bad_i, bad_v = idx.copy(), val.copy()
    bad_i[r, k - 1], bad_v[r, k - 1] = top_i[r, k + 4] + S.BIG_BASE, top_v[r, k + 4]
    with pytest.raises(AssertionError, match="not ambiguous"):
        S.check_filtered(bad_v, bad_i, k, q64, c64, top_v, top_i, k, S.BIG_BASE)
    bad_v = val.copy()
    bad_v[r, 0] += 3 * S.pair_ref(q64, c64, top_i[:, :1])[1][r, 0]
    with pytest.raises(AssertionError, match="outside the bound"):
        S.check_filtered(bad_v, idx, k, q64, c64, top_v, top_i, k, S.BIG_BASE)
    bad_i, bad_v = idx.copy(), val.copy()
    bad_i[r, 1], bad_v[r, 1] = idx[r, 0], val[r, 0]
    with pytest.raises(AssertionError, match="twice"):
        S.check_filtered(bad_v, bad_i, k, q64, c64, top_v, top_i, k, S.BIG_BASE)


def test_the_gaussian_operands_are_rounded_once_and_deterministic():
    qt, ct, q64, c64 = S.operands("B-nq65-d128", "bf16", "gauss")
    assert qt.dtype == torch.bfloat16 and np.array_equal(qt.double().numpy(), q64) and np.array_equal(ct.double().numpy(), c64)
    S.operands.cache_clear()
    assert torch.equal(S.operands("B-nq65-d128", "bf16", "gauss")[1], ct)
    assert abs(float(np.linalg.norm(c64, axis=1).mean()) - 1) < 1e-2
