"""CPU reference of the fp8 (e4m3fn) corpus scorer, sgpt_score_topk_q8: numpy / torch, float64.

A quantised corpus is `codes` uint8 [N, d] (OCP e4m3fn) + `scale` fp32 [N] (powers of two); document n is decode(codes[n]) * scale[n],
exactly.  The scorer multiplies f16 queries with those rows in fp32; the reference does it in float64.  Two bounds:

arithmetic_bound   |kernel score - float64 score of the same operands| <= d * 2^-23 * sum_i |q_i c_i|: at most d fp32 roundings of
                   relative 2^-24 on partial sums bounded by sum_i |q_i c_i| (the products q_i c_i themselves are exact in fp32: 11 x 4
                   significant bits), with a factor 2 for the MFMA's internal summation order.
quantisation_bound |score on the quantised rows - score on the fp32 rows| <= 2^-4 * sum_i |q_i c_i| + 2^-10 * scale * sum_i |q_i|:
                   e4m3 round-to-nearest has relative error <= 2^-4 per normal element (3 mantissa bits), and an element in the
                   subnormal range is off by at most half the subnormal spacing, 2^-10 * scale.
"""
import numpy as np
import torch


def decode_e4m3(codes) -> np.ndarray:
    """uint8 e4m3fn codes -> float64 values (NaN for the codes 0x7f / 0xff), by torch's own float8_e4m3fn."""
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(codes, dtype=np.uint8)))
    return t.view(torch.float8_e4m3fn).to(torch.float64).numpy()


def dequantize(codes, scale) -> np.ndarray:
    """float64 [N, d]: the exact rows of the quantised corpus."""
    return decode_e4m3(codes) * np.asarray(scale, dtype=np.float64)[:, None]


def quantize_rows(x):
    """fp32 rows -> (codes, scale) by the rule of sgpt_fp8_quantize_rows, written with torch's cast: scale = the smallest power of
    two with max|row| / scale <= 448 (1 for a zero row), codes = RNE(row / scale)."""
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=1).astype(np.float64)
    m, e = np.frexp(amax)                                   # amax = m 2^e, 0.5 <= m < 1; 448 = 0.875 * 2^9
    k = np.clip(np.where(m <= 0.875, e - 9, e - 8), -126, 127)
    scale = np.where(amax > 0, np.ldexp(1.0, k), 1.0).astype(np.float32)
    codes = torch.from_numpy(x / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return codes, scale


def scores64(q16, rows64) -> np.ndarray:
    """float64 scores [nq, N] of f16 queries against exact rows; a NaN score (a NaN code in the row) is -1, as the scorer's."""
    q = np.asarray(q16, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = q @ np.nan_to_num(rows64, nan=0.0).T
    s[:, np.isnan(rows64).any(axis=1)] = -1.0
    return s


def abs_products(q16, rows64) -> np.ndarray:
    """sum_i |q_i c_i| per (query, document): the magnitude both bounds scale with."""
    return np.abs(np.asarray(q16, dtype=np.float64)) @ np.abs(np.nan_to_num(rows64, nan=0.0)).T


def topk_lowest_index(scores, k, idx_base=0):
    """(values, indices) of the k best per row, sorted descending, ties to the lowest index."""
    s = np.asarray(scores)
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -s), axis=1)[:, :k]
    return np.take_along_axis(s, order, axis=1), order + idx_base


def arithmetic_bound(q16, rows64) -> np.ndarray:
    d = np.asarray(q16).shape[1]
    return d * 2.0 ** -23 * abs_products(q16, rows64)


def quantisation_bound(q, rows, scale) -> np.ndarray:
    """q [nq, d], rows [N, d]: the UNquantised operands (float); scale [N]: the rows' quantisation scales."""
    q = np.asarray(q, dtype=np.float64)
    return 2.0 ** -4 * (np.abs(q) @ np.abs(np.asarray(rows, dtype=np.float64)).T) + \
        2.0 ** -10 * np.abs(q).sum(axis=1)[:, None] * np.asarray(scale, dtype=np.float64)[None, :]


def unit_corpus(seed, N, d, nq):
    """The corpus of the GPU tests: unit rows around a common offset (as tests/test_gpu_kernels.py's short-query-batch tests), unit
    queries.  fp32 torch tensors on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1)
    base = torch.randn(1, d, generator=g) * 2
    c = torch.nn.functional.normalize(base + torch.randn(N, d, generator=g), dim=1)
    return q, c
