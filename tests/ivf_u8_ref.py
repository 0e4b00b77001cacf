"""numpy restatement of the IVF corpus over uint8 lists (include/sgpt_hip.h: sgpt_u8_gather_quantize_rows, sgpt_ivf_search_u8;
sgpt_amd/corpus.py::IVFUint8Corpus, CorpusBuilders.ivf_index(precision="uint8")), in float64, built from the references it joins: the
lists, probe sets and restricted top-k of ivf_ref, the quantiser of scoreu8_ref, the value of a code row of scorebits_u8_ref.

bound   |device value - float64 value| <= gamma_n (sum_j |q_j step_j c_nj| + sum_j |q_j mid_j|), c = code - 128, mid = start + 128 step,
        gamma_n = n u / (1 - n u), u = 2^-24, n = score_roundings(d): the count of the header.  The device evaluates
        qbias + sum_j q'_j c_nj with q'_j = fp32(q_j step_j).  G lanes cover a row of ld = ceil(d / 128) * 128 bytes (G = 8, 16, 32, 32, 64
        for ld = 128, 256, 384, 512, beyond), each lane four accumulators.  A product passes the rounding of q', at most
        4 ceil(ld / (16 G)) fmas, 2 joining and log2(G) butterfly additions and the addition of qbias; a term of qbias passes the two
        roundings of mid, its product, at most ceil(d / 256) + 8 additions of the prologue and that last addition."""
import numpy as np

import ivf_ref as R
import scorebits_u8_ref as B
import scoreu8_ref as U


def lanes_per_row(ld):
    """G: the lanes of a wavefront that cover one row of ld bytes."""
    return 8 if ld <= 128 else 16 if ld <= 256 else 32 if ld <= 512 else 64


def score_roundings(d):
    """Roundings on the longest path of the uint8 scan's value (the header's n)."""
    ld = U.ld_of(d)
    g = lanes_per_row(ld)
    rounds = (ld + 16 * g - 1) // (16 * g)
    return max(4 * rounds + int(np.log2(g)) + 4, (d + 255) // 256 + 12)


def values64(q, codes, start, step):
    """float64 [nq, N]: <q, x^_n> of every code row (NaN -> -1)."""
    return B.values64(q, codes, start, step)


def score_terms(q, codes, start, step):
    """sum_j |q_j step_j c_nj| + sum_j |q_j mid_j|, [nq, N]."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    d = q.shape[1]
    st, lo = np.asarray(step, dtype=np.float64)[:d], np.asarray(start, dtype=np.float64)[:d]
    c = np.asarray(codes, dtype=np.float64)[:, :d] - 128.0
    return (np.abs(q) * np.abs(st)[None, :]) @ np.abs(c).T + (np.abs(q) * np.abs(lo + 128.0 * st)[None, :]).sum(axis=1)[:, None]


def score_bound(q, codes, start, step):
    return R.gamma(score_roundings(np.asarray(q).shape[1])) * score_terms(q, codes, start, step)


class _Rows:
    """What ivf_ref.search indexes as `rows` and hands to scores64: here the float64 rows the codes stand for."""

    def __init__(self, codes, start, step, d):
        self.x = U.dequantize(codes, start, step)[:, :d]

    def __getitem__(self, pos):
        return self.x[pos]


def search_u8(q, codes, start, step, ids, offsets, probes, k, idx_base=0, run=None):
    """ivf_ref.search over the values of the code rows: (val float64 [nq, k], idx int64 [nq, k], the candidate positions per query)."""
    q = np.asarray(q, dtype=np.float32)
    return R.search(q, _Rows(codes, start, step, q.shape[1]), ids, offsets, probes, k, idx_base, run)


def build_u8(x, nlist, n_iter, seed):
    """Unit rows -> (centroids fp32, codes uint8 list-major, start, step, ids, offsets, rows f16 list-major): ivf_ref.build, the lists
    quantised with the ranges of the f16-rounded rows."""
    c, rows16, ids, offsets = R.build(x, nlist, n_iter, seed)
    rows32 = rows16.astype(np.float32)
    start, step = U.ranges(rows32)
    return c, U.quantize_rows(rows32, start, step), start, step, ids, offsets, rows16
