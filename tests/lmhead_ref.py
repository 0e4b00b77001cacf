"""Test infrastructure: the LM-head log-likelihood path (include/sgpt_hip.h::sgpt_lm_logprobs, csrc/encode.hip) in float64 numpy
-- log_softmax(float64(hidden[row_idx]) @ float64(W).T + float64(b))[targets] and the greedy token -- with the case table of
tests/test_gpu_lmhead.py, a mirror of the chunk loop's workspace layout, the derived error bound, and a numpy emulation of the
chunk loop that can carry one defect at a time.  Checked without a GPU by tests/test_lmhead_ref.py.

Widths.  sgpt_model_load accepts d_model % 128 == 0 only (include/sgpt_hip.h), so the two widths of the table are the two
smallest loadable ones that differ in the depth of the k-loop: 128 (two 64-element fp32 k-steps of the 'deep' kernel, four
32-element ones of the others) and 384 (six / twelve).  No model of width 64 or 320 can be loaded."""
import functools
from collections import namedtuple

import numpy as np

import gemm_ref as G
import rowops_ref as R

# ---------------------------------------------------------------- the workspace layout of sgpt_lm_logprobs -----------------------
CHUNK = 1024                                           # rows per chunk: `R = n < 1024 ? n : 1024`


def align_up(v, a):
    return (v + a - 1) // a * a


Layout = namedtuple("Layout", "R rows_bytes ldv lg_bytes")


def layout(n, d, V):
    """A mirror of the three lines of sgpt_lm_logprobs that place its two buffers in the context's workspace: the gathered rows
    [R, d] fp32 at byte 0, the logits chunk [R, ldv] fp32 behind them.  Two calls with the same (min(n, 1024), d, ldv) put
    every logits element -- the pad columns [V, ldv) among them -- at the same address: test_stale_pad_columns relies on it."""
    ldv = (V + 3) // 4 * 4
    Rr = n if n < CHUNK else CHUNK
    return Layout(Rr, align_up(Rr * d * 4, 256), ldv, align_up(Rr * ldv * 4, 256))


def chunks(n):
    """(r0, nr) of every iteration of the host loop."""
    Rr = layout(n, 4, 4).R
    return [(r0, min(n - r0, Rr)) for r0 in range(0, n, Rr)]


def chunk_variants(n, V, d):
    """(kernel, block order) of the fp32 GEMM of every chunk (gemm_ref.linear_variant: M = nr, N = V, K = d, epi 0)."""
    return [G.linear_variant("fp32", G.EPI_STORE, False, nr, V, d) for _, nr in chunks(n)]


# ---------------------------------------------------------------- the cases ------------------------------------------------------
# head: 'tied' (GPT-Neo, wte.weight) | 'bias' (GPT-J, lm_head.weight + lm_head.bias).  operands: 'exact' and / or 'gauss'.
# patterns: the row-index patterns run at this case (PATTERNS); the first is run with every operand kind, the others with both
# kinds too where listed.  variants: what chunk_variants must give -- tests/test_lmhead_ref.py asserts it, so a change of the
# launch rule breaks this table before it silently un-covers a leg.
Case = namedtuple("Case", "name V d head n operands patterns variants")
PATTERNS = ("spans", "reversed", "random-small", "random-large", "repeat")
NS = (1, 5, 1023, 1024, 1025, 2048, 2049, 3109)        # one chunk, exactly one, one + a one-row tail, two, two + tail, three + ragged
V_SUPER = 9473                                         # the smallest V % 4 != 0 with 8 * ceil(V / 128) >= 600 128x128 tiles at M = 1024
V_REAL = 50257
_DEEP, _RS128, _RS64 = ("rs64-deep", "run"), ("rs128", "supertile"), ("rs64", "supertile")


def _cases():
    out = []
    for n in NS:
        pats = PATTERNS if n in (1025, 2049) else PATTERNS[:1]
        out.append(Case(f"chunks-n{n}", 211, 128, "tied", n, ("exact", "gauss"), pats, (_DEEP,) * len(chunks(n))))
    for n in (1025, 2049):
        out.append(Case(f"bias-n{n}", 257, 384, "bias", n, ("exact", "gauss"), PATTERNS[:1], (_DEEP,) * len(chunks(n))))
    # the full chunk on 128x128 tiles in supertile order (8 x 75 tiles); its one-row tail is 149 64x64 tiles in run order
    out.append(Case("super-n1025", V_SUPER, 128, "tied", 1025, ("exact", "gauss"), PATTERNS[:1], (_RS128, _DEEP)))
    # the real vocabulary: 8 x 393 128x128 tiles, and the one-row tail on 786 64x64 tiles in supertile order with MT == 1
    out.append(Case("real-n1025", V_REAL, 128, "tied", 1025, ("gauss",), PATTERNS[:1], (_RS128, _RS64)))
    return out


CASES = _cases()


def case(name):
    return next(c for c in CASES if c.name == name)


def runs(c):
    """(operands, pattern) of every run of case c."""
    return [(o, p) for o in c.operands for p in c.patterns]


# ---------------------------------------------------------------- operands -------------------------------------------------------
DUP = {211: (3, 200), 257: (3, 7), V_SUPER: (3, 9000)}   # j1 < j2: LM-head rows with identical weights (and bias): other / same column tile
DUP_EVERY = 37                                         # every 37th selected hidden row has the duplicated rows as its maximum


@functools.lru_cache(maxsize=4)
def head_operands(V, d, head, kind):
    """(W [V, d] fp32, bias [V] fp32 or None).
    exact: multiples of 2^-3 in [-1, 1]; rows DUP[V] are equal, all of magnitude 1, with the largest bias.
    gauss: W ~ N(0, 9 / d) so that logits of N(0, 1) hidden rows have a standard deviation near 3; bias ~ N(0, 0.25)."""
    rng = np.random.default_rng([V, d, head == "bias", kind == "exact"])
    if kind == "exact":
        W = rng.integers(-8, 9, size=(V, d)).astype(np.float32) / np.float32(8)
        b = rng.integers(-8, 9, size=V).astype(np.float32) / np.float32(8) if head == "bias" else None
        j1, j2 = DUP[V]
        W[:, 0] = 0                                               # every other row: sum |w| <= d - 1, so its logit stays below ...
        W[j1] = W[j2] = np.where(rng.integers(0, 2, size=d) == 0, np.float32(-1), np.float32(1))
        if b is not None:
            b[j1] = b[j2] = 1.0                                   # ... sign(W[j1]) . W[j1] + b[j1] = d (+ 1), the duplicated rows'
    else:
        W = (rng.standard_normal((V, d)) * (3.0 / np.sqrt(d))).astype(np.float32)
        b = (rng.standard_normal(V) * 0.5).astype(np.float32) if head == "bias" else None
    return W, b


def row_pattern(pattern, n, rng):
    """(row_idx int32 [n], T_pad): which rows of `hidden` a call selects.
    spans: ascending runs of 7 .. 13 rows with gaps of 3 .. 40 between them (what crossencoder._score_batches produces);
    reversed: the same, last row first; random-small / random-large: a uniform draw with repeats from T_pad < n / T_pad > n rows;
    repeat: one row n times."""
    if pattern in ("spans", "reversed"):
        idx, at = [], int(rng.integers(0, 20))
        while len(idx) < n:
            at += int(rng.integers(3, 41))
            ln = int(rng.integers(7, 14))
            idx.extend(range(at, at + ln))
            at += ln
        idx = np.asarray(idx[:n], dtype=np.int32)
        T_pad = align_up(int(idx[-1]) + 1 + int(rng.integers(0, 40)), 32)
        return (idx[::-1].copy() if pattern == "reversed" else idx), T_pad
    if pattern in ("random-small", "random-large"):
        T_pad = max(32, n // 2 // 32 * 32) if pattern == "random-small" else align_up(2 * n, 32)
        return rng.integers(0, T_pad, size=n).astype(np.int32), T_pad
    if pattern == "repeat":
        return np.full(n, 37, dtype=np.int32), 64
    raise ValueError(pattern)


def make_hidden(T_pad, d, row_idx, kind, W, rng):
    """hidden fp32 [T_pad, d]: NaN in every row no row_idx entry selects; the selected rows are N(0, 1) (gauss) or multiples of
    2^-3 in [-1, 1] (exact), where every DUP_EVERY-th selected row is sign(W[j1]): its largest logits are the duplicated rows'."""
    hidden = np.full((T_pad, d), np.nan, dtype=np.float32)
    sel = np.unique(row_idx)
    if kind == "exact":
        hidden[sel] = rng.integers(-8, 9, size=(len(sel), d)).astype(np.float32) / np.float32(8)
        j1 = DUP[W.shape[0]][0]
        hidden[sel[::DUP_EVERY]] = np.sign(W[j1])
    else:
        hidden[sel] = rng.standard_normal((len(sel), d)).astype(np.float32)
    return hidden


# ---------------------------------------------------------------- the float64 reference and the bound ----------------------------
BLOCK_BYTES = 100e6                                    # a row block of float64 logits stays near this size


def logits64(hidden, row_idx, W, bias, lo=0, hi=None):
    """float64(hidden[row_idx[lo:hi]]) @ float64(W).T + float64(bias): [hi - lo, V]."""
    x = G.product(hidden[np.asarray(row_idx[lo:hi])], W)
    return x if bias is None else x + np.asarray(bias, np.float64)[None, :]


def logit_at(hidden, row_idx, W, bias, tokens):
    """The float64 logit of row i at token tokens[i]: [n]."""
    tokens = np.asarray(tokens)
    x = np.einsum("nd,nd->n", np.asarray(hidden[np.asarray(row_idx)], np.float64), np.asarray(W[tokens], np.float64))
    return x if bias is None else x + np.asarray(bias, np.float64)[tokens]


def row_stats(hidden, row_idx, W, bias):
    """Per row, in row blocks: mx (the largest float64 logit), am (its first index), gap (to the second largest), lse
    (log sum exp(x - mx)) and E = max_j gemm_ref.bound(a, w, bias, None, K)[i, j]."""
    n, (V, K) = len(row_idx), W.shape
    step = max(1, int(BLOCK_BYTES // (8 * V)))
    mx, am, gap, lse, E = np.empty(n), np.empty(n, np.int64), np.empty(n), np.empty(n), np.empty(n)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        x = logits64(hidden, row_idx, W, bias, lo, hi)
        r = np.arange(hi - lo)
        am[lo:hi] = np.argmax(x, axis=1)
        mx[lo:hi] = x[r, am[lo:hi]]
        with np.errstate(all="ignore"):
            lse[lo:hi] = np.log(np.exp(x - mx[lo:hi, None]).sum(axis=1))
        if V > 1:
            x[r, am[lo:hi]] = -np.inf
            gap[lo:hi] = mx[lo:hi] - x.max(axis=1)
        else:
            gap[lo:hi] = np.inf
        del x
        E[lo:hi] = G.bound(hidden[np.asarray(row_idx[lo:hi])], W, bias, None, K).max(axis=1)
    return mx, am, gap, lse, E


def choose_targets(n, V, am, rng):
    """Random targets with 0, V - 1 and the float64 argmax among them (every 7th row each)."""
    tg = rng.integers(0, V, size=n)
    tg[0::7] = am[0::7]
    tg[1::7] = 0
    tg[2::7] = V - 1
    return tg.astype(np.int32)


def logprob_bound(V, xt_minus_max):
    """The bound of tests/test_gpu_rowops.py for the log-softmax kernel on given fp32 logits."""
    return 2.0 ** -22 * (V / 256 + 16) + 2.0 ** -23 * np.abs(xt_minus_max)


Ref = namedtuple("Ref", "case kind pattern hidden row_idx T_pad W bias targets lp am gap E B bound")
GREEDY_LEFT_OUT_MAX = 0.01


@functools.lru_cache(maxsize=None)
def reference(name, kind, pattern, seed=0):
    """Inputs and float64 results of one run of a case, computed once per process.  bound = 2 E + B:
    |lp - ref| <= 2 max_j E[i, j] + B[i] -- the log-sum-exp and the gathered logit each move by at most max_j |delta logit|,
    E the project's bound of an fp32 chain of any order (gemm_ref.bound), B the bound of the log-softmax kernel itself."""
    c = case(name)
    rng = np.random.default_rng([seed, c.V, c.d, c.n, PATTERNS.index(pattern), kind == "exact"])
    W, bias = head_operands(c.V, c.d, c.head, kind)
    row_idx, T_pad = row_pattern(pattern, c.n, rng)
    hidden = make_hidden(T_pad, c.d, row_idx, kind, W, rng)
    mx, am, gap, lse, E = row_stats(hidden, row_idx, W, bias)
    targets = choose_targets(c.n, c.V, am, rng)
    xt = logit_at(hidden, row_idx, W, bias, targets)
    B = logprob_bound(c.V, xt - mx)
    return Ref(c, kind, pattern, hidden, row_idx, T_pad, W, bias, targets, (xt - mx) - lse, am, gap, E, B, 2.0 * E + B)


def greedy_left_out(ref):
    """Rows whose float64 top-two gap does not exceed 2 max_j E: their greedy token is not compared with the float64 argmax."""
    return ref.gap <= 2.0 * ref.E


def exact_logits(ref):
    """The logits of an exact-operand run as fp32 [n, ldv], NaN behind column V: what the GEMM must produce bit for bit."""
    x = logits64(ref.hidden, ref.row_idx, ref.W, ref.bias)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x), "the operands are not exact in fp32"
    out = np.full((x.shape[0], layout(ref.case.n, ref.case.d, ref.case.V).ldv), np.nan, dtype=np.float32)
    out[:, :ref.case.V] = x32
    return out


# ---------------------------------------------------------------- the chunk loop in numpy, with one defect at a time -------------
DEFECTS = ("row_idx not advanced", "targets not advanced", "out not advanced", "log-softmax ld = V", "bias dropped",
           "tail with the previous row count", "gather reads row + 1")
SENTINEL = np.float32(77.0)                            # a log-probability is never positive
STALE = np.float32(1e30)                               # what the workspace holds before the call


def emulate(hidden, row_idx, W, bias, targets, defect=None):
    """sgpt_lm_logprobs as numpy: per chunk gather -> fp32 logits (gemm_ref.fp32_chain, groups of 4, + bias in fp32) into a
    [R, ldv] buffer that starts out holding STALE -> log-softmax gathered at the target (float64 arithmetic on the fp32
    logits, rounded to fp32 once) and the first maximum.  The output and the index arrays carry CHUNK guard entries behind n: the
    guard indices select a NaN row, the guard outputs hold SENTINEL.  Returns (lp fp32 [n + CHUNK], greedy int64 [n + CHUNK])."""
    assert defect is None or defect in DEFECTS
    n, (V, d) = len(row_idx), W.shape
    L = layout(n, d, V)
    hid = np.vstack([hidden, np.full((1, d), np.nan, np.float32)])              # row T_pad: what the guards (and row + 1) reach
    ri = np.concatenate([np.asarray(row_idx, np.int64), np.full(CHUNK, hidden.shape[0], np.int64)])
    tg = np.concatenate([np.asarray(targets, np.int64), np.zeros(CHUNK, np.int64)])
    out, greedy = np.full(n + CHUNK, SENTINEL, np.float32), np.full(n + CHUNK, -7, np.int64)
    ws = np.full(L.R * L.ldv, STALE, np.float32)
    logits = ws.reshape(L.R, L.ldv)
    prev = None
    with np.errstate(all="ignore"):
        for r0, nr in chunks(n):
            if defect == "tail with the previous row count" and prev is not None:
                nr = prev
            i0 = 0 if defect == "row_idx not advanced" else r0
            t0 = 0 if defect == "targets not advanced" else r0
            o0 = 0 if defect == "out not advanced" else r0
            idx = ri[i0:i0 + nr] + (1 if defect == "gather reads row + 1" else 0)
            x = G.fp32_chain(hid[idx], W, 4)
            if bias is not None and defect != "bias dropped":
                x = (x + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
            logits[:nr, :V] = x
            seen = ws[:nr * V].reshape(nr, V) if defect == "log-softmax ld = V" else logits[:nr, :V]
            lp, am = R.logprob_rows(seen, V, tg[t0:t0 + nr])
            out[o0:o0 + nr], greedy[o0:o0 + nr] = lp.astype(np.float32), am
            prev = nr
    return out, greedy


def worst_ratio(lp, ref):
    """max_i |lp[i] - ref.lp[i]| / ref.bound[i] over the n rows of the run; inf where a value is not finite."""
    got = np.asarray(lp, np.float64)[:ref.case.n]
    ratio = np.abs(got - ref.lp) / ref.bound
    return float(np.where(np.isfinite(got), ratio, np.inf).max())


def defect_seen(lp, ref, margin=4.0):
    """A NaN, a row outside `margin` times its bound, or a guard entry that was written."""
    lp = np.asarray(lp)
    return worst_ratio(lp, ref) > margin or bool((lp[ref.case.n:] != SENTINEL).any())
