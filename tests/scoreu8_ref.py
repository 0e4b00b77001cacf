"""CPU reference of the uint8 corpus scorer, sgpt_score_topk_u8: numpy, float64.

A uint8 corpus is `codes` uint8 [N, ld], ld = ceil(d / 128) * 128 (pad columns hold 128), with `start`, `step` fp32 [ld] (pad columns 0):
document n is x^[n][j] = start[j] + codes[n][j] * step[j], exactly (float64 here).  This is sentence-transformers' precision="uint8";
codes - 128 are its "int8" codes.  Quantiser (fp32, IEEE subtraction and division, round-half-even):
codes = clamp(rint((x - start) / step), 0, 255), 128 where step == 0 or x is NaN; ranges: start = column min, step = (max - min) / 255.

The scorer folds the per-dimension scale into the query.  With mid = start + 128 step and c = code - 128 (an integer in [-128, 127]):
    <q, x^_n> = sum_j q_j mid_j + sum_j (q_j step_j) c[n][j] = qbias + qscale * <q'', c_n>
    q'_j = fp32(q_j * step_j);  e: max_j |q'_j| * 2^-e in [1, 2) (0 for a zero row);  q''_j = RNE_f16(q'_j * 2^-e);  qscale = 2^e;
    qbias = sum_j q_j * mid_j (fp32 on the device, float64 of the fp32 products here).
The kernel multiplies the f16 values q'' and c in the f16 MFMA (an 11-bit by an 8-bit significand: every product is exact in fp32),
accumulates in fp32 and applies one fma, score = fmaf(acc, qscale, qbias).  Two bounds:

arithmetic_bound    |kernel score - float64 score of the same q'', qscale, qbias, codes|
                    <= d * 2^-23 * qscale * sum_j |q''_j c_j| + 2^-23 * |score|:
                    at most d fp32 roundings of relative 2^-24 on partial sums bounded by sum_j |q''_j c_j| (the products are exact),
                    with a factor 2 for the MFMA's internal summation order -- the bound of score8_ref.py, scaled by the exact power
                    of two qscale; then the fma rounds acc * qscale + qbias once, relative 2^-24 of the result, again with a factor 2.
quantisation_bound  |<q, x^_n> - <q, x_n>| <= sum_j |q_j| (step_j / 2 + clamp distance of x[n][j]):
                    inside [start, start + 255 step] the nearest of 256 uniform levels is at most half a step away; outside, the code
                    is 0 or 255 and the element is off by its distance to that end.  (Stated for the exact quotient.  The fp32
                    subtraction and division move the quotient by at most 255 * 2^-22 of a step, which matters only for an element
                    within that of a half step; a sum over d elements that ALL sit there does not occur, so the bound is kept as
                    stated.)
"""
import numpy as np

from score8_ref import topk_lowest_index  # noqa: F401  (the order of every scorer: descending, ties to the lowest index)


def ld_of(d) -> int:
    return (int(d) + 127) // 128 * 128


def ranges(x):
    """fp32 rows [n, d] -> (start, step) fp32 [ld]: column min and (max - min) / 255 in fp32, pad columns 0."""
    x = np.asarray(x, dtype=np.float32)
    d = x.shape[1]
    start, step = np.zeros(ld_of(d), dtype=np.float32), np.zeros(ld_of(d), dtype=np.float32)
    mn, mx = x.min(axis=0), x.max(axis=0)
    start[:d] = mn
    step[:d] = (mx - mn) / np.float32(255)
    return start, step


def quotient64(x, start, step) -> np.ndarray:
    """(x - start) / step in float64 for the d true columns (inf / nan where step == 0)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x - np.asarray(start, dtype=np.float64)[None, :d]) / np.asarray(step, dtype=np.float64)[None, :d]


def quantize_rows(x, start, step) -> np.ndarray:
    """fp32 rows [n, d] -> codes uint8 [n, ld] by the rule, in numpy's fp32 (IEEE, np.rint rounds half to even)."""
    x = np.asarray(x, dtype=np.float32)
    start, step = np.asarray(start, dtype=np.float32), np.asarray(step, dtype=np.float32)
    n, d = x.shape
    codes = np.full((n, start.shape[0]), 128, dtype=np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.rint((x - start[None, :d]) / step[None, :d])
    t = np.where(np.isnan(t) | (step[None, :d] == 0), np.float32(128), np.clip(t, 0, 255))
    codes[:, :d] = t.astype(np.uint8)
    return codes


def dequantize(codes, start, step) -> np.ndarray:
    """float64 [N, ld]: the exact rows of the quantised corpus."""
    return np.asarray(start, dtype=np.float64)[None, :] + np.asarray(codes, dtype=np.float64) * np.asarray(step, dtype=np.float64)[None, :]


def dequantize32(codes, start, step) -> np.ndarray:
    """fp32 [N, ld] as sgpt_u8_dequantize_rows computes it: the product rounded to fp32, then the sum rounded to fp32."""
    prod = np.asarray(codes, dtype=np.float32) * np.asarray(step, dtype=np.float32)[None, :]
    return np.asarray(start, dtype=np.float32)[None, :] + prod


def prepare_queries(q, start, step):
    """q fp32 [nq, d] -> (q'' f16 [nq, ld], qscale fp32 [nq], qbias float64 [nq]) by the prologue's rule."""
    q = np.asarray(q, dtype=np.float32)
    start, step = np.asarray(start, dtype=np.float32), np.asarray(step, dtype=np.float32)
    nq, d = q.shape
    qp = q * step[None, :d]                                   # fp32, one rounding
    amax = np.abs(qp).max(axis=1)
    m, ex = np.frexp(amax.astype(np.float64))                 # amax = m 2^ex, 0.5 <= m < 1
    e = np.where((amax > 0) & np.isfinite(amax), ex - 1, 0).astype(np.int64)
    q2 = np.zeros((nq, start.shape[0]), dtype=np.float16)
    q2[:, :d] = np.ldexp(qp.astype(np.float64), -e[:, None]).astype(np.float16)      # (the scaling is exact: one rounding, to f16)
    mid = start + np.float32(128) * step
    qbias = (q * mid[None, :d]).astype(np.float64).sum(axis=1)
    return q2, np.ldexp(1.0, e).astype(np.float32), qbias


def exact_scores(q2, qscale, qbias, codes) -> np.ndarray:
    """float64 [nq, N]: qbias + qscale * <q'', codes - 128>."""
    c = np.asarray(codes, dtype=np.float64) - 128.0
    return np.asarray(qbias, dtype=np.float64)[:, None] + np.asarray(qscale, dtype=np.float64)[:, None] * (np.asarray(q2, dtype=np.float64) @ c.T)


def kernel_model(q2, qscale, qbias, codes) -> np.ndarray:
    """fp32 [nq, N] by the kernel's arithmetic, modelled: exact products, k slices of 32 summed (here in float64, rounded once) and
    accumulated in fp32 with k ascending, then one fma with the fp32 qscale / qbias."""
    q2 = np.asarray(q2, dtype=np.float64)
    c = np.asarray(codes, dtype=np.float64) - 128.0
    acc = np.zeros((q2.shape[0], c.shape[0]), dtype=np.float32)
    for k0 in range(0, q2.shape[1], 32):
        acc = (acc.astype(np.float64) + q2[:, k0:k0 + 32] @ c[:, k0:k0 + 32].T).astype(np.float32)
    qb = np.asarray(qbias, dtype=np.float32).astype(np.float64)
    return (acc.astype(np.float64) * np.asarray(qscale, dtype=np.float64)[:, None] + qb[:, None]).astype(np.float32)


def abs_products(q2, codes) -> np.ndarray:
    """sum_j |q''_j c_j| per (query, document)."""
    return np.abs(np.asarray(q2, dtype=np.float64)) @ np.abs(np.asarray(codes, dtype=np.float64) - 128.0).T


def arithmetic_bound(q2, qscale, codes, score, d=None) -> np.ndarray:
    """d: the number of columns that carry products (default: the padded width, which is never smaller)."""
    d = np.asarray(q2).shape[1] if d is None else d
    return d * 2.0 ** -23 * np.asarray(qscale, dtype=np.float64)[:, None] * abs_products(q2, codes) + 2.0 ** -23 * np.abs(score)


def row_kernel_case(seed=11, n=3000, d=200):
    """The rows of the quantiser tests (tests/test_gpu_scoreu8.py test 7; checked on the CPU by tests/test_scoreu8_ref.py): columns of very
    different magnitudes and offsets, column 17 constant (step == 0).  fp32 [n, d]."""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((n, d)) * np.geomspace(1e-3, 10, d)[None, :] + np.linspace(-1, 1, d)[None, :]).astype(np.float32)
    x[:, 17] = 0.375
    return x


def near_half(t64, tol=1e-4) -> np.ndarray:
    """Elements whose float64 quotient is finite, inside (-0.5, 255.5) and within tol of a half-integer: where fp32 may pick either
    neighbour.  A uniform fraction puts 2 tol = 0.02 % of the elements there."""
    live = np.isfinite(t64)
    t = np.where(live, t64, 0.0)
    return live & (np.abs(t - np.floor(t) - 0.5) < tol) & (t > -0.5) & (t < 255.5)


def quantisation_bound(q, x, start, step) -> np.ndarray:
    """q [nq, d], x [N, d]: the UNquantised operands; [nq, N]."""
    q, x = np.abs(np.asarray(q, dtype=np.float64)), np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    lo, st = np.asarray(start, dtype=np.float64)[:d], np.asarray(step, dtype=np.float64)[:d]
    hi = lo + 255.0 * st
    clamp = np.maximum(0.0, np.maximum(lo[None, :] - x, x - hi[None, :]))
    return (q @ (st / 2.0))[:, None] + q @ clamp.T
