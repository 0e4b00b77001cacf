"""-m gpu: the f16, bf16 and fp32 scorers -- sgpt_scores, sgpt_score_topk (csrc/score.hip) -- against float64, tile by tile.

Every launch the scorer makes over 16-bit and fp32 rows (tests/score_ref.py: legs A to G; tests/test_score_ref.py asserts on the CPU that each
shape reaches its launch) is compared with the float64 product of the same rounded operands:
  exact operands     small integers whose sums are exact in any order: values bit-equal, indices in the lowest-index order;
  Gaussian operands  every element within gemm_ref.bound = (K + 4) 2^-23 |q| |c|^T, the derived bound of an fp32 chain of any order.
With N <= 1024 and k = N the materialise-and-select path returns every score of the launch, so legs A to E check every element of
every tile; leg G reads the score matrix itself; leg F (the filtered schedule) checks what comes back and that it is the float64 top-k.
The equality chains of the other scorer suites (filtered = materialised, 64-row tile = 256-row tile, fp8 / uint8 = f16 on de-quantised
rows) end here.  Each case prints "scoref64: <case>: worst error / bound = ..."."""
import numpy as np
import pytest
import torch

import gemm_gpu_util as U
import score_ref as S

pytestmark = pytest.mark.gpu

TOPK = [(c.name, fmt) for c in S.CASES for fmt in c.fmts]
FILTERED = [(c.name, fmt) for c in S.CASES_F for fmt in c.fmts]
SCORES = [(c.name, fmt, kind) for c in S.CASES_G for fmt in c.fmts for kind in ("exact", "gauss")]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _topk(ctx, qt, ct, k, idx_base, fmt):
    val, idx, n = ctx.score_topk(qt.cuda(), ct.cuda(), k, idx_base=idx_base, dtype=S.TORCH[fmt])
    assert val.shape == idx.shape == (qt.shape[0], k) and val.dtype == torch.float32 and idx.dtype == torch.int64
    return val.cpu().numpy(), idx.cpu().numpy(), n


def _reference(c, qt, ct):
    """(ref, bnd) float64 [nq, documents the leg checks] of the operands as the kernel reads them."""
    q64, c64 = qt.double().numpy(), ct[S.doc0_of(c):].double().numpy()
    return S.scores64(q64, c64, True), S.bound(q64, c64)


def _report(what, ratio, more=""):
    print(f"scoref64: {what}: worst error / bound = {ratio:.3f}{more}")


@pytest.mark.parametrize("name,fmt", TOPK)
def test_exact_operands_are_bit_equal_in_the_lowest_index_order(ctx, name, fmt):
    """Legs A to E, integer operands: val equals the float64 score bit for bit, idx the value-descending, lowest-index-first order (ties
    are plentiful), n == k."""
    c = S.case(name)
    qt, ct, _, _ = S.operands(name, fmt, "exact")
    base = S.idx_base_of(c, "exact")
    val, idx, n = _topk(ctx, qt, ct, c.k, base, fmt)
    ref, _ = _reference(c, qt, ct)
    _report(f"{name}-{fmt}-exact", S.check_exact(val, idx, n, ref, c.k, base + S.doc0_of(c)))


@pytest.mark.parametrize("name,fmt", TOPK)
def test_gaussian_operands_are_within_the_bound_everywhere(ctx, name, fmt):
    """Legs A to E, unit rows: every row of idx a permutation of the documents, every value within the bound of its document's float64
    score, values non-increasing with equal neighbours in ascending index order.  No element is excluded."""
    c = S.case(name)
    qt, ct, _, _ = S.operands(name, fmt, "gauss")
    base = S.idx_base_of(c, "gauss")
    val, idx, n = _topk(ctx, qt, ct, c.k, base, fmt)
    ref, bnd = _reference(c, qt, ct)
    _report(f"{name}-{fmt}-gauss", S.check_bounded(val, idx, n, ref, bnd, c.k, base + S.doc0_of(c)))


@pytest.mark.parametrize("kind", ["exact", "gauss"])
@pytest.mark.parametrize("name,fmt,docs,qrow", S.NAN_VARIANTS, ids=[f"{v[0]}-{v[1]}-{'docs' if v[2] else 'query'}" for v in S.NAN_VARIANTS])
def test_nan_rows_score_minus_one(ctx, name, fmt, docs, qrow, kind):
    """A NaN document in a whole tile and another in the tail score exactly -1.0 against every query and sit where -1 sorts; a NaN query
    row returns -1.0 everywhere with the indices idx_base .. idx_base + k - 1."""
    c = S.case(name)
    qt, ct, _, _ = S.operands(name, fmt, kind)
    d0 = S.doc0_of(c)
    if docs:
        ct = S.with_nan(ct, [d0 + j for j in docs])
    if qrow is not None:
        qt = S.with_nan(qt, [qrow])
    base = S.idx_base_of(c, kind)
    val, idx, n = _topk(ctx, qt, ct, c.k, base, fmt)
    ref, bnd = _reference(c, qt, ct)
    first = base + d0
    ratio = S.check_exact(val, idx, n, ref, c.k, first) if kind == "exact" else S.check_bounded(val, idx, n, ref, bnd, c.k, first)
    for j in docs:
        assert (ref[:, j] == -1.0).all() and (val[idx == first + j] == -1.0).all() and (idx == first + j).sum() == c.nq
    if qrow is not None:
        assert (val[qrow] == -1.0).all() and np.array_equal(idx[qrow], first + np.arange(c.k))
        assert not (val[np.arange(c.nq) != qrow] == -1.0).all(axis=1).any()
    _report(f"{name}-{fmt}-{kind}-nan-{'docs' if docs else 'query'}", ratio)


def _scores(ctx, c, fmt, at, bt):
    """sgpt_scores with ldo > nb into a guarded buffer: the int32 image [na, ldo] of the output rows (pad columns included)."""
    ldo = (c.nb + 3) // 4 * 4 + 4
    n = c.na * ldo
    a_d, b_d = at.cuda(), bt.cuda()
    buf, body = U.guarded(n, torch.float32)
    st = ctx.lib.sgpt_scores(ctx.handle, a_d.data_ptr(), b_d.data_ptr(), U.CODE[fmt], c.na, c.nb, c.d, body.data_ptr(), ldo, None)
    ctx._chk(st, f"sgpt_scores {c.name}")
    torch.cuda.synchronize()
    rows = buf[U.GUARD:U.GUARD + n].view(c.na, ldo)
    bits = rows.cpu().numpy()
    assert bool((rows[:, c.nb:] == U.SENT32).all()), f"{c.name}: a store into the pad columns"
    rows[:, c.nb:] = 0                                   # (check_guards takes every sentinel between the guards for an unwritten element)
    U.check_guards(buf, n, c.name)
    return bits


@pytest.mark.parametrize("name,fmt,kind", SCORES)
def test_scores_every_element(ctx, name, fmt, kind):
    """Leg G: every element of sgpt_scores within the bound (exact operands: bit-equal), the pad columns and the guards unwritten."""
    c = S.case(name)
    at, bt, a64, b64 = S.operands(name, fmt, kind)
    bits = _scores(ctx, c, fmt, at, bt)
    _report(f"{name}-{fmt}-{kind}", S.check_scores(bits, c.nb, S.scores64(a64, b64, False), S.bound(a64, b64), kind == "exact"))


@pytest.mark.parametrize("name,fmt", [("G-50x37-d72", "f16"), ("G-130x257-d768", "bf16"), ("G-fp32-130x257-d768", "fp32")])
def test_scores_keep_nan_in_its_row_and_column(ctx, name, fmt):
    """Leg G: a NaN in one row of a and one row of b gives NaN in exactly that row and that column; every other element stays within
    the bound."""
    c = S.case(name)
    at, bt, _, _ = S.operands(name, fmt, "gauss")
    at, bt = S.with_nan(at, [c.na - 2]), S.with_nan(bt, [c.nb - 1])
    a64, b64 = at.double().numpy(), bt.double().numpy()
    ref = S.scores64(a64, b64, False)
    assert np.isnan(ref).sum() == c.na + c.nb - 1
    _report(f"{name}-{fmt}-gauss-nan", S.check_scores(_scores(ctx, c, fmt, at, bt), c.nb, ref, S.bound(a64, b64), False))


@pytest.mark.parametrize("name,fmt", FILTERED)
def test_filtered_schedule_returns_the_float64_top_k(ctx, name, fmt):
    """Leg F: every returned value within the bound of the float64 score of its index; the returned set of a non-ambiguous row is the
    float64 top-k, an ambiguous row (k-th and (k + 1)-th float64 scores closer than twice the larger bound; at most 5 % of the rows,
    tests/test_score_ref.py) may swap documents that close.  The float64 reference is computed in blocks of 256 query rows."""
    c = S.case(name)
    qt, ct, q64, c64, top_v, top_i = S.filtered_case(c.nq, c.N, c.d, fmt)
    base = S.idx_base_of(c, "gauss")
    val, idx, n = _topk(ctx, qt, ct, c.k, base, fmt)
    ratio, share = S.check_filtered(val, idx, n, q64, c64, top_v, top_i, c.k, base)
    assert share <= 0.05
    _report(f"{name}-{fmt}", ratio, f", ambiguous rows = {100 * share:.2f} %")
