"""Test infrastructure: packed variable-length causal (+ sliding-window, + ALiBi) attention in float64 numpy -- the reference
of tests/test_gpu_attention.py, pinned against torch's scaled_dot_product_attention in tests/test_attn_ref.py.

Sequence b owns the token rows [off[b], off[b] + lens[b]) of the packed axis and attends only to its own span.  Key j (counted
from the sequence start) is visible to query i iff j <= i and, when window > 0, j > i - window -- GPT-Neo's causal / local
"bias" buffers (HF:gpt_neo:56-66, oracle.gptneo_forward).  score = scale * q.k + slope_h * j (BLOOM's ALiBi term,
HF:bloom build_alibi_tensor: the key position from the sequence start), exact softmax, P.V."""
import numpy as np


def visible(n: int, window: int = 0) -> np.ndarray:
    """bool [n, n]: key j visible to query i."""
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    m = j <= i
    if window > 0:
        m &= j > i - window
    return m


def packed_attention(q, k, v, off, lens, H: int, window: int = 0, scale: float = 1.0, slopes=None) -> np.ndarray:
    """q, k, v: [rows, H * dh] token-major (any float type; computed in float64).  off, lens: per-sequence first row and
    real token count.  Returns float64 [rows, H * dh]: the context of every real token row, NaN on every other row."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    rows, d = q.shape
    dh = d // H
    out = np.full((rows, d), np.nan)
    sl = None if slopes is None else np.asarray(slopes, dtype=np.float64)
    for s0, n in zip(np.asarray(off).tolist(), np.asarray(lens).tolist()):
        qs = q[s0:s0 + n].reshape(n, H, dh).transpose(1, 0, 2)
        ks = k[s0:s0 + n].reshape(n, H, dh).transpose(1, 0, 2)
        vs = v[s0:s0 + n].reshape(n, H, dh).transpose(1, 0, 2)
        vis = visible(n, window)
        o = np.empty((H, n, dh))
        for h in range(H):                                         # one head at a time: [n, n] scores (n = 2048: 32 MB)
            s = scale * (qs[h] @ ks[h].T)
            if sl is not None:
                s = s + sl[h] * np.arange(n, dtype=np.float64)[None, :]
            s = np.where(vis, s, -np.inf)
            s = s - s.max(axis=-1, keepdims=True)                  # the diagonal is always visible: finite max
            p = np.exp(s)
            p /= p.sum(axis=-1, keepdims=True)
            o[h] = p @ vs[h]
        out[s0:s0 + n] = o.transpose(1, 0, 2).reshape(n, d)
    return out


def layout(lens, align: int = 2, row_tile: int = 32):
    """Packed layout of sgpt_encode (sgpt_amd.model.pack_layout): allocations rounded up to `align` rows, the token axis to
    `row_tile`.  Returns (off int64[B], alloc int64[B], T_pad, max_alloc)."""
    lens = np.asarray(lens, dtype=np.int64)
    alloc = (lens + align - 1) // align * align
    off = np.concatenate([[0], np.cumsum(alloc)[:-1]]).astype(np.int64)
    total = int(alloc.sum())
    return off, alloc, (total + row_tile - 1) // row_tile * row_tile, int(alloc.max())
