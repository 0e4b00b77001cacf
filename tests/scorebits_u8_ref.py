"""CPU reference of the binary corpus with a uint8 second stage, sgpt_score_topk_bits_u8 / sgpt_u8_rescore: numpy, integers / float64.

Built from the two references it joins.  Stage 1 is scorebits_ref's on the matrix q - center (one fp32 subtraction per element): integers,
compared bit for bit.  Stage 2 is the value <q, x^_n> of the RAW q against the de-quantised row x^_n = start + codes[n] * step of
scoreu8_ref, in float64 here and fp32 on the device.

bound   |device value - float64 value| <= (d + 2) 2^-23 (sum_j |q_j step_j c_nj| + sum_j |q_j mid_j|) + 2^-23 |value|,
        c = code - 128, mid = start + 128 step: the bound of include/sgpt_hip.h.  The device evaluates qbias + sum_j q'_j c_nj with
        q'_j = fp32(q_j step_j) and qbias = sum_j q_j mid_j in fp32.  Every partial sum passes at most d inexact additions (pad columns
        add exact zeros), q'_j and q_j mid_j round once and mid_j once more, each relative 2^-24, with a factor 2 for the second-order
        terms; the last addition rounds the value itself.
"""
import numpy as np

import scorebits_ref as B
import scoreu8_ref as U
from score8_ref import topk_lowest_index


def values64(q, codes, start, step) -> np.ndarray:
    """float64 [nq, N]: <q, x^_n> over the d true columns (the pad columns de-quantise to 0 + 128 * 0); a NaN value is -1, as the
    kernel's."""
    q = np.asarray(q, dtype=np.float64)
    rows = U.dequantize(codes, start, step)[:, :q.shape[1]]
    with np.errstate(invalid="ignore"):
        v = q @ rows.T
    return np.where(np.isnan(v), -1.0, v)


def bound(q, codes, start, step, values=None) -> np.ndarray:
    """[nq, N]: the bound of the header for every (query, document); values: values64's result (computed here when None)."""
    q = np.asarray(q, dtype=np.float64)
    d = q.shape[1]
    st, lo = np.asarray(step, dtype=np.float64)[:d], np.asarray(start, dtype=np.float64)[:d]
    c = np.asarray(codes, dtype=np.float64)[:, :d] - 128.0
    prod = (np.abs(q) * np.abs(st)[None, :]) @ np.abs(c).T
    bias = (np.abs(q) * np.abs(lo + 128.0 * st)[None, :]).sum(axis=1)[:, None]
    values = values64(q, codes, start, step) if values is None else values
    return (d + 2) * 2.0 ** -23 * (prod + bias) + 2.0 ** -23 * np.abs(values)


def centred(q, center) -> np.ndarray:
    """The matrix stage 1 sees: q - center, one IEEE fp32 subtraction per element (q itself without a centre)."""
    q = np.asarray(q, dtype=np.float32)
    return q if center is None else q - np.asarray(center, dtype=np.float32)[None, :]


def rescore(q, codes, start, step, idx, idx_base=0):
    """sgpt_u8_rescore: (values float64 [nq, m], indices int64 [nq, m]) slot for slot; a slot with idx < 0 or idx - idx_base outside
    [0, N) gives (-inf, -1)."""
    idx = np.asarray(idx, dtype=np.int64)
    N = np.asarray(codes).shape[0]
    row = idx - idx_base
    ok = (idx >= 0) & (row >= 0) & (row < N)
    vals = values64(q, codes, start, step)
    out = np.take_along_axis(vals, np.where(ok, row, 0), axis=1)
    return np.where(ok, out, -np.inf), np.where(ok, idx, -1)


def pipeline(q, center, bits, codes, start, step, k, kp, idx_base=0):
    """The two stages: (values float64 [nq, min(k, N)], indices, the stage-1 candidates [nq, min(kp, N)]).  Candidates by
    scorebits_ref.stage1 on q - center; order by float64 value descending, ties to the lowest index."""
    q = np.asarray(q, dtype=np.float32)
    d = q.shape[1]
    _, cand = B.stage1(centred(q, center), bits, d, kp, idx_base)
    vals = values64(q, codes, start, step)
    cv = np.take_along_axis(vals, cand - idx_base, axis=1)
    order = np.lexsort((cand, -cv), axis=1)[:, :k]
    return np.take_along_axis(cv, order, axis=1), np.take_along_axis(cand, order, axis=1), cand


def clustered_anisotropic(seed=5, n_centres=1000, per=20, d=768, nq=32):
    """The fixture of scripts/score_bits_u8_quality.py: clustered rows, three channels scaled by 30, a common offset, unit rows; queries
    are perturbed corpus rows.  (corpus fp32 [n_centres * per, d], queries fp32 [nq, d])"""
    g = np.random.default_rng(seed)
    mu = g.standard_normal(d)
    centres = g.standard_normal((n_centres, d))
    x = np.repeat(centres, per, axis=0) + 0.5 * g.standard_normal((n_centres * per, d))
    x[:, :3] *= 30.0
    x += 4.0 * mu[None, :]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pick = g.choice(x.shape[0], nq, replace=False)
    q = x[pick] + 0.3 * g.standard_normal((nq, d)) / np.sqrt(d)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return x.astype(np.float32), q.astype(np.float32)


def overlap(got_idx, want_idx) -> float:
    """Mean share of want's indices found in got, per query."""
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(got_idx, want_idx)]))


__all__ = ["values64", "bound", "centred", "rescore", "pipeline", "clustered_anisotropic", "overlap", "topk_lowest_index"]
