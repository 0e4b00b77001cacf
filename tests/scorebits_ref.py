"""CPU reference of the binary-corpus scorer, sgpt_score_topk_bits: numpy, integers / float64.

A binary corpus is `bits` uint8 [N, ldb], ldb = 4 * ceil(d / 32): dimension i of a document is bit 7 - i % 8 of byte i / 8 (the order of
np.packbits), set exactly when the element is > 0; pad bits are zero.  Stage 1 ranks by the agreement a = d - 2 * hamming(sign q, bits[n])
= <sign q, sign d_n> (signs +-1), an integer, so everything about it is compared bit for bit.  The re-scored values are float64 here and
fp32 on the device; their bounds:

sign_bound   |kernel value - float64 value| <= d * 2^-23 * sum_i |q_i| / sqrt(d): at most d fp32 roundings of relative 2^-24 on partial
             sums bounded by sum_i |q_i|, a factor 2 for the summation order (which also covers the final division).
fp8_bound    the same with sum_i |q_i c_i| (score8_ref.arithmetic_bound): the fp32 x e4m3 product rounds once, which the factor covers.
"""
import numpy as np

from score8_ref import topk_lowest_index

POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def ldb_of(d) -> int:
    return 4 * ((d + 31) // 32)


def pack(x, center=None) -> np.ndarray:
    """fp32 rows [n, d] -> uint8 [n, ldb]: np.packbits(x - center > 0), zero bytes up to ldb."""
    x = np.asarray(x, dtype=np.float32)
    if center is not None:
        x = x - np.asarray(center, dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore"):
        p = np.packbits(x > 0, axis=-1)
    out = np.zeros((x.shape[0], ldb_of(x.shape[1])), dtype=np.uint8)
    out[:, :p.shape[1]] = p
    return out


def hamming(qbits, bits) -> np.ndarray:
    """int64 [nq, N]: XOR + a 256-entry popcount table, one query at a time."""
    out = np.empty((qbits.shape[0], bits.shape[0]), dtype=np.int64)
    for m in range(qbits.shape[0]):
        out[m] = POP8[np.bitwise_xor(bits, qbits[m][None, :])].sum(axis=1, dtype=np.int64)
    return out


def hamming_words(qbits, bits) -> np.ndarray:
    """The same on 32-bit words with numpy's own population count where this numpy has one (ten times faster on 300 k rows: what the
    large cases of the GPU tests use); tests/test_scorebits_ref.py holds it against the table."""
    if not hasattr(np, "bitwise_count"):
        return hamming(qbits, bits)
    b, q = np.ascontiguousarray(bits).view(np.uint32), np.ascontiguousarray(qbits).view(np.uint32)
    out = np.empty((q.shape[0], b.shape[0]), dtype=np.int64)
    for m in range(q.shape[0]):
        out[m] = np.bitwise_count(np.bitwise_xor(b, q[m][None, :])).sum(axis=1, dtype=np.int64)
    return out


def agreement(qbits, bits, d) -> np.ndarray:
    return d - 2 * hamming_words(qbits, bits)


def signs(bits, d) -> np.ndarray:
    """float64 [N, d]: the +-1 sign vectors over the d true dimensions."""
    return np.unpackbits(bits, axis=-1)[:, :d].astype(np.float64) * 2.0 - 1.0


def stage1(q, bits, d, kp, idx_base=0):
    """(a [nq, min(kp, N)] int64, idx) of the best by (a descending, index ascending); q fp32 rows, packed here."""
    a = agreement(pack(q), bits, d)
    return topk_lowest_index(a, min(kp, bits.shape[0]), idx_base)


def mode0_values(a, d) -> np.ndarray:
    return np.asarray(a, dtype=np.float32) / np.float32(d)


def sign_values(q, bits, d) -> np.ndarray:
    """float64 [nq, N]: <q, s_n> / sqrt(d)."""
    return np.asarray(q, dtype=np.float64) @ signs(bits, d).T / np.sqrt(np.float64(d))


def sign_bound(q, d) -> np.ndarray:
    """[nq, 1]"""
    return (d * 2.0 ** -23 * np.abs(np.asarray(q, dtype=np.float64)).sum(axis=1) / np.sqrt(np.float64(d)))[:, None]


def check_rescored(got_val, got_idx, cand_idx, vals64, bound, k, idx_base=0):
    """The rule of the mode 1 / mode 2 tests.  got_*: the device's [nq, k]; cand_idx: the reference's stage-1 candidates [nq, kp];
    vals64 [nq, N] float64 values of every document; bound [nq, N] or [nq, 1].  Every returned index is a candidate; every value is
    within the bound of the float64 value of its index; the returned set is the float64 top-k of the candidates except where the
    float64 values in question differ by less than twice the bound; the order is descending."""
    bound = np.broadcast_to(bound, vals64.shape)
    for m in range(got_idx.shape[0]):
        cand = cand_idx[m] - idx_base
        mine = got_idx[m] - idx_base
        assert set(mine.tolist()) <= set(cand.tolist()), f"query {m}: an index outside the stage-1 candidates"
        assert len(set(mine.tolist())) == len(mine)
        assert np.all(np.abs(got_val[m].astype(np.float64) - vals64[m, mine]) <= bound[m, mine]), f"query {m}: value outside the bound"
        assert np.all(np.diff(got_val[m]) <= 0)
        order = cand[np.lexsort((cand, -vals64[m, cand]))]
        want = order[:k]
        missing, extra = set(want.tolist()) - set(mine.tolist()), set(mine.tolist()) - set(want.tolist())
        # a document the device preferred to a float64 winner: both device values are within the bound of their float64 values
        assert all(vals64[m, j] - vals64[m, e] <= bound[m, j] + bound[m, e] for j in missing for e in extra), \
            f"query {m}: not the float64 top-k of the candidates"
