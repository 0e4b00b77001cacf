"""Reference of the top-k select (csrc/topk.hip::topk_select_kernel), numpy only: a full sort of the virtual row under the one order the
file promises, and a classifier that says which exit of the kernel an input reaches.

The order (comment above `sorts_before`): higher score first on the order-preserving uint32 image of the fp32 score, ties -> lower index.
-0.0 is folded into +0.0; a positive NaN ranks above +inf, a negative NaN below -inf.

What the header (include/sgpt_hip.h) promises and this file pins down:
  * -inf.  "unused tail = (-inf, -1)", and a list is read up to its first index < 0 (sgpt_eval_ranked, the next merge).  An entry whose
    score is -inf -- an empty slot (id < 0), the excluded id, or a real document that scored -inf -- is therefore one thing on every
    path: it comes back as (-inf, -1), behind every entry with a score above -inf.  (Keeping the document's index instead would put
    real entries behind empty ones: index -1 sorts before every document.)  select_ref returns (-inf, -1); that is what is tested.
  * repeated (score, id) pairs (a caller's lists handed to sgpt_topk_merge may repeat an id) are each emitted, on every path.
  * k > 2048: the k best as a SET, in no particular order (the kernel has no room to sort them); tested as a multiset.
Not pinned down by the header, and not tested: a NEGATIVE NaN that reaches the output of a row with fewer than k scores above -inf
(it sorts below the -inf entries here)."""
import os
import re

import numpy as np

TOPK_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgpt_amd", "csrc", "topk.hip")

EXITS = ("all_survive", "short", "one_pass_keys", "one_pass_comparator", "one_pass_bitonic", "one_pass_overflow_radix", "radix",
         "radix_index_select", "radix_unsorted")


def key32(v):
    """Ascending uint32 order == ascending score order; -0.0 folded into +0.0."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def virtual_row(fresh, idx_base, prev_val, prev_idx, nan_to_m1, exclude):
    """[fresh scores (ids idx_base + position) | previous list] as the Row struct reads it: a previous entry with id < 0 or
    id == exclude is empty (-inf, -1); NaN -> -1 on both legs when nan_to_m1 is set."""
    fresh = np.zeros(0, np.float32) if fresh is None else np.asarray(fresh, np.float32)
    pv = np.zeros(0, np.float32) if prev_val is None else np.asarray(prev_val, np.float32).copy()
    pi = np.zeros(0, np.int64) if prev_idx is None else np.asarray(prev_idx, np.int64).copy()
    empty = pi < 0
    if exclude is not None:
        empty |= pi == exclude
    pv[empty] = -np.inf
    pi[empty] = -1
    vals = np.concatenate([fresh, pv])
    ids = np.concatenate([np.int64(idx_base) + np.arange(len(fresh), dtype=np.int64), pi])
    if nan_to_m1:
        vals = np.where(np.isnan(vals), np.float32(-1.0), vals)
    return vals.astype(np.float32), ids


def select_ref(fresh, idx_base, prev_val, prev_idx, k, nan_to_m1, exclude=None):
    """One row -> (values[k], indices[k]): the whole virtual row sorted, no selection algorithm."""
    vals, ids = virtual_row(fresh, idx_base, prev_val, prev_idx, nan_to_m1, exclude)
    ids = np.where(vals == -np.inf, np.int64(-1), ids)                  # (-inf, -1): see the module docstring
    order = np.lexsort((ids, -key32(vals).astype(np.int64)))[:k]
    ov = np.full(k, -np.inf, np.float32)
    oi = np.full(k, -1, np.int64)
    ov[:len(order)] = vals[order]
    oi[:len(order)] = ids[order]
    return ov, oi


def gathered_to_rows(gv, gi):
    """[world][nq][k] -> [nq][world * k]: entry j of a row is list j // k, column j % k."""
    world, nq, k = gv.shape
    return gv.transpose(1, 0, 2).reshape(nq, world * k), gi.transpose(1, 0, 2).reshape(nq, world * k)


_constants = {}


def constants():
    """The thresholds between the kernel's exits, read out of topk.hip."""
    if not _constants:
        src = open(TOPK_HIP).read()
        for name in ("TK_THREADS", "TK_SORT_MAX", "TK_FAST_KMAX", "TK_FAST_MIN_ROW"):
            _constants[name] = int(re.search(r"constexpr\s+(?:int|long)\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
        _constants["SAMPLES_PER_THREAD"] = int(re.search(r"stride\s*=\s*total\s*/\s*\(TK_THREADS\s*\*\s*(\d+)\)", src).group(1))
        _constants["CAND_KEYS_MAX"] = int(re.search(r"cnt\s*<=\s*(\d+)\s*&&\s*in_lds", src).group(1))
    return _constants


def path_of(n, n_prev, k, row_values, indices):
    """Which exit of topk_select_kernel the virtual row (row_values, indices) = virtual_row(...) of n fresh + n_prev previous entries
    takes.  Proves which branch an input reaches; never supplies an expected value."""
    c = constants()
    T, sort_max = c["TK_THREADS"], c["TK_SORT_MAX"]
    v = np.asarray(row_values, np.float32)
    ids = np.asarray(indices, np.int64)
    total = n + n_prev
    assert len(v) == total == len(ids)
    in_lds = k <= sort_max
    if total <= k:
        return "all_survive"
    if k <= c["TK_FAST_KMAX"] and total <= sort_max and in_lds:
        return "short"
    if k <= c["TK_FAST_KMAX"] and total >= c["TK_FAST_MIN_ROW"]:
        spt = c["SAMPLES_PER_THREAD"]
        stride = total // (T * spt)
        pos = (np.arange(spt)[:, None] * T + np.arange(T)[None, :]) * stride
        s = v[pos]
        smax = np.where(np.isnan(s), -np.inf, s).max(axis=0)            # fmaxf drops a NaN
        tau = max(np.sort(w)[::-1][k - 1] for w in smax.reshape(T // 64, 64))
        if tau > -np.inf:
            cand = ~(v < tau)                                            # everything not below tau (a NaN included)
            cnt = int(cand.sum())
            if cnt <= c["CAND_KEYS_MAX"] and in_lds:
                return "one_pass_keys" if (ids[cand] < 0xffffffff).all() else "one_pass_comparator"
            return "one_pass_bitonic" if cnt <= sort_max else "one_pass_overflow_radix"
    if not in_lds:
        return "radix_unsorted"
    key = key32(v)
    kth = np.sort(key)[::-1][k - 1]
    krem = k - int((key > kth).sum())
    return "radix_index_select" if int((key == kth).sum()) > krem else "radix"
