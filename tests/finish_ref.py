"""Test infrastructure: the kernels that finish an embedding (csrc/elementwise.hip: pool_kernel, l2norm_kernel, pairwise_kernel,
cvt16_kernel, crest16_kernel) in float64 numpy -- the references of tests/test_gpu_finish.py, pinned against the oracle, torch
and the golden fixtures in tests/test_finish_ref.py.

Every reference takes arrays of any float type and computes in float64 from their exact values.  Every bound is an a-priori
count of fp32 roundings (unit roundoff 2^-24) along the kernel's own chain of operations with about a factor two of head-room;
the emulate_* functions restate that chain in fp32 numpy (per-lane strided partial sums, then the xor butterfly 32..1; for
pooling one sequential chain over t with separate multiply and add) so that the CPU tests can prove each bound on every input
the GPU tests use.  The case lists and input builders of both files live here."""
import numpy as np

from rowops_ref import EPS32, f64, pool_padded, ulp16

F32 = np.float32
U32 = 2.0 ** -24                                          # unit roundoff of fp32
FMTS16 = ("bf16", "f16")
NAN16 = {"bf16": 0x7FC0, "f16": 0x7E00}


def ratio(err, bound) -> float:
    """max err / bound of a bounded case.  An exact result under a zero bound counts 0 and any error under a zero bound inf; a
    NaN or an infinity anywhere in err or bound is inf too (max() and comparisons would let a NaN through as a pass)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if not (np.isfinite(err).all() and np.isfinite(bound).all()):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------- 16-bit formats, RNE
def round16(x, fmt: str) -> np.ndarray:
    """The round-to-nearest-even 16-bit pattern (uint16) of every element of an fp32 array.  bf16 in integer arithmetic:
    (bits + 0x7fff + ((bits >> 16) & 1)) >> 16, a NaN staying a (quiet) NaN of its sign; f16 through numpy.float16, whose
    conversion from fp32 is the IEEE one (ties to even, gradual underflow, overflow to inf from 65520 on)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if fmt == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    bits = x.view(np.uint32).astype(np.uint64)
    out = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (bits >> 16) | 0x40, out).astype(np.uint16)


def widen16(bits, fmt: str) -> np.ndarray:
    """uint16 patterns -> the fp32 array of their exact values."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if fmt == "f16":
        return bits.view(np.float16).astype(F32)
    return (bits.astype(np.uint32) << 16).view(F32)


def to_fmt(x, fmt: str):
    """fp32 array -> (the fp32 array of its values rounded to fmt, their uint16 patterns); 'f32': (x, None)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if fmt == "f32":
        return x, None
    bits = round16(x, fmt)
    return widen16(bits, fmt), bits


def _bits32(words) -> np.ndarray:
    return np.array(words, dtype=np.uint32).view(F32)


def cvt_table(fmt: str) -> np.ndarray:
    """The edge inputs (fp32) of the fp32 -> 16-bit conversion: +-0, +-inf; the exact half-way points between neighbouring 16-bit
    values of both parities at several exponents (subnormal ones included) with one fp32 ulp either side, both signs; f16: the
    subnormal range 2^-25 .. 2^-14, 65504, 65519.996, 65520 (-> inf); bf16: the largest finite value and the first fp32 that
    rounds to inf; fp32 subnormals; NaNs (a signalling one whose payload sits in the dropped bits among them)."""
    if fmt == "f16":
        low = [0x0000, 0x0001, 0x0002, 0x0155, 0x03FE, 0x03FF,               # subnormals of both parities, up to the first normal
               0x0400, 0x0401, 0x07FF, 0x1400, 0x1555, 0x3BFF, 0x3C00, 0x3C01, 0x3C02, 0x57FE, 0x57FF, 0x7800, 0x7BFD, 0x7BFE]
    else:
        low = [0x0000, 0x0001, 0x0002, 0x007E, 0x007F,                       # bf16 subnormals = fp32 subnormals
               0x0080, 0x0081, 0x00FF, 0x2A00, 0x2A55, 0x3F7F, 0x3F80, 0x3F81, 0x3F82, 0x477E, 0x477F, 0x7F00, 0x7F7D, 0x7F7E]
    low = np.array(low, dtype=np.uint16)
    a, b = widen16(low, fmt).astype(np.float64), widen16(low + 1, fmt).astype(np.float64)
    assert np.array_equal((b - a)[1:], ulp16(a[1:], fmt))                    # neighbours: one spacing of the format apart
    mid = ((a + b) / 2).astype(F32)
    assert np.array_equal(mid.astype(np.float64), (a + b) / 2)               # the half-way points are fp32 values
    ties = np.concatenate([mid, np.nextafter(mid, F32(np.inf)), np.nextafter(mid, F32(-np.inf)), a.astype(F32), b.astype(F32)])
    parts = [np.array([0.0, -0.0, np.inf, -np.inf], dtype=F32), ties, -ties]
    if fmt == "f16":
        parts.append(np.ldexp(F32(1.0), np.arange(-27, -13)).astype(F32))                    # 2^-27 .. 2^-14
        parts.append(np.array([1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -14 - 2.0 ** -25,
                               65504.0, 65519.996, 65520.0, 65536.0, 1e9, 3e38, -65504.0, -65519.996, -65520.0], dtype=F32))
        assert parts[-1][5] < 65520.0
    else:
        parts.append(_bits32([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF,    # largest finite; the first -> inf; FLT_MAX
                             0xFF7F7FFF, 0xFF7F8000]))
    parts.append(_bits32([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF, 0x00800000,
                          0x80000001, 0x80008000, 0x80018000, 0x807FFFFF]))                  # fp32 subnormals
    parts.append(_bits32([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF80FFFF]))      # NaNs
    return np.concatenate(parts).astype(F32)


CVT_NUMEL = [1, 255, 256, 257, 2097152 + 3]               # 8192 workgroups x 256 threads = 2 097 152: the last size loops


def cvt_inputs(numel: int, fmt: str) -> np.ndarray:
    """randn scaled over many binades, the edge table laid over its head (a single element: the tie just above 1)."""
    rng = np.random.default_rng(numel)
    x = (rng.standard_normal(numel, dtype=F32) * np.exp2(rng.integers(-20, 12, numel)).astype(F32)).astype(F32)
    t = cvt_table(fmt)
    k = min(numel, t.shape[0])
    x[:k] = t[:k] if k == t.shape[0] else t[16:16 + k]
    if numel > 2097152:                                     # the second pass of the grid-stride loop gets edges too
        x[-3:] = t[[4, 5, -1]]
    return x


def same16(got_bits, want_bits, fmt: str) -> bool:
    """Bit equality of two uint16 pattern arrays, NaN compared as 'is NaN'."""
    g, w = np.asarray(got_bits, dtype=np.uint16), np.asarray(want_bits, dtype=np.uint16)
    lim = 0x7F80 if fmt == "bf16" else 0x7C00
    gn, wn = (g & 0x7FFF) > lim, (w & 0x7FFF) > lim
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))


# ------------------------------------------------------------------------------------------------------------- pooling
POOL_MODES = ["weightedmean", "mean", "lasttoken", "learntmean", "cls"]
POOL_WEIGHTED = ["weightedmean", "mean", "learntmean"]
POOL_FMTS = ["f32", "bf16", "f16"]
POOL_D = [4, 64, 772, 1028, 4096]                           # 1028: one live thread in the second blockIdx.y column block
POOL_S = [1, 3, 33, 130]
POOL_MASKED = {"f32": 1e30, "bf16": 1e30, "f16": 6e4}      # what the masked positions hold


def pool_masks(S: int) -> np.ndarray:
    """B = 6, one mask of each kind: full; first token only; last token only; a middle run (left and right padding); holes
    (1 0 1 1 0 ...); all zero."""
    m = np.zeros((6, S), dtype=np.int32)
    m[0] = 1
    m[1, 0] = 1
    m[2, S - 1] = 1
    lo = S // 3
    m[3, lo:max(lo + 1, S - max(1, S // 4))] = 1
    m[4] = np.array([1, 0, 1, 1, 0], dtype=np.int32)[np.arange(S) % 5]
    return m


def pool_inputs(d: int, S: int, fmt: str):
    """-> (hidden fp32 [6, S, d] holding exactly the values of format fmt, their uint16 patterns or None, mask int32 [6, S],
    learntmean weights fp32 [S + 7] in [0.5, 1.5])."""
    rng = np.random.default_rng(100003 * d + S)
    h = rng.standard_normal((6, S, d), dtype=F32) * F32(3.0) + F32(1.0)
    mask = pool_masks(S)
    h[mask == 0] = F32(POOL_MASKED[fmt]) * np.where(rng.random((int((mask == 0).sum()), 1)) < 0.5, F32(-1.0), F32(1.0))
    h, bits = to_fmt(h, fmt)
    pw = rng.uniform(0.5, 1.5, S + 7).astype(F32)
    return h, bits, mask, pw


def pool(hidden, mask, mode: str, pos_weights=None) -> np.ndarray:
    """rowops_ref.pool_padded plus mode 'cls' (row 0 of every sequence, whatever the mask).  'lasttoken' of an all-zero mask is
    row 0, as the kernel and oracle.pool have it (pool_padded gives zeros there); the mean modes of an all-zero mask are zeros
    (a zero numerator over the clamped denominator)."""
    h, m = f64(hidden), np.asarray(mask) != 0
    if mode == "cls":
        return h[:, 0].copy()
    e = pool_padded(hidden, m, mode, pos_weights=pos_weights)
    if mode == "lasttoken":
        empty = ~m.any(axis=1)
        e[empty] = h[empty, 0]
    return e


def _pool_weights(mask, mode: str, pos_weights) -> np.ndarray:
    m = f64(np.asarray(mask) != 0)
    S = m.shape[1]
    if mode == "weightedmean":
        return m * np.arange(1, S + 1, dtype=np.float64)
    if mode == "learntmean":
        return m * f64(pos_weights)[:S]
    if mode == "mean":
        return m
    raise ValueError(f"no weights in pooling mode {mode}")


def pool_bound(hidden, mask, mode: str, pos_weights=None) -> np.ndarray:
    """Per element, 2^-23 (S + 4) sum_t |w_t| |h_t| / den over the unmasked positions: a chain of S multiply-adds (each product
    and each sum rounded) and one division; learntmean adds 2^-23 S |out| for the rounded sum of its weights (the integer
    weights of the other two modes add exactly).  lasttoken and cls are copies: no bound."""
    h, keep = f64(hidden), np.asarray(mask) != 0
    S = h.shape[1]
    w = _pool_weights(mask, mode, pos_weights)
    den = np.maximum(w.sum(axis=1), 1e-9)[:, None]
    terms = np.where(keep[:, :, None], np.abs(w)[:, :, None] * np.abs(h), 0.0)
    b = EPS32 * (S + 4) * terms.sum(axis=1) / den
    if mode == "learntmean":
        b = b + EPS32 * S * np.abs(pool(hidden, mask, mode, pos_weights))
    return b


def emulate_pool(hidden, mask, mode: str, pos_weights=None) -> np.ndarray:
    """pool_kernel in fp32 numpy: one sequential chain over t per element, product and sum rounded separately, a masked
    position entering with weight 0 (its value is still multiplied), the weight sum clamped at 1e-9f, one division."""
    h, m = np.asarray(hidden, dtype=F32), np.asarray(mask) != 0
    B, S, d = h.shape
    if mode in ("cls", "lasttoken"):
        return pool(h, m, mode).astype(F32)
    acc, den = np.zeros((B, d), dtype=F32), np.zeros(B, dtype=F32)
    for t in range(S):
        wt = F32(t + 1) if mode == "weightedmean" else (F32(pos_weights[t]) if mode == "learntmean" else F32(1.0))
        w = np.where(m[:, t], wt, F32(0.0)).astype(F32)
        den = den + w
        acc = acc + w[:, None] * h[:, t]
    return acc / np.maximum(den, F32(1e-9))[:, None]


# --------------------------------------------------------------------------------------- wave reductions of the row kernels
def _lane_sums(terms) -> np.ndarray:
    """terms fp32 [n, m]: lane l of a row's wave adds elements l, l + 64, ... in that order, from 0 -> [n, 64]."""
    n, m = terms.shape
    acc = np.zeros((n, 64), dtype=F32)
    for c0 in range(0, m, 64):
        seg = terms[:, c0:c0 + 64]
        acc[:, :seg.shape[1]] = acc[:, :seg.shape[1]] + seg
    return acc


def _wave_sum(p) -> np.ndarray:
    """The xor butterfly 32, 16, 8, 4, 2, 1 over [n, 64] fp32 -> [n] (every lane ends with the same bits)."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ o]
    return p[:, 0]


# --------------------------------------------------------------------------------------------------------- L2 normalise
ROW_N = [1, 4, 5, 1027]                                     # one wave; a full workgroup; a short last group; many groups + tail
ROW_D = [1, 3, 63, 64, 65, 100, 768, 772, 4096]
L2_FAMILIES = ["plain", "offset", "outlier", "tiny", "huge", "zero_row", "clamp_row"]


def l2_families(d: int):
    return [f for f in L2_FAMILIES if f != "huge" or d <= 128]   # 1e15: the squares stay finite only for narrow rows


def l2_inputs(n: int, d: int, family: str) -> np.ndarray:
    """5 randn; randn + 100; one channel x 300; scale 1e-15; scale 1e15; 5 randn whose LAST row (the short last workgroup) is
    zero; the same with a last row of norm 2e-14, under the 1e-12 clamp."""
    rng = np.random.default_rng(7919 * n + 31 * d + L2_FAMILIES.index(family))
    x = rng.standard_normal((n, d), dtype=F32)
    if family == "offset":
        x = x + F32(100.0)
    elif family == "outlier":
        x[:, d // 3] *= F32(300.0)
    elif family == "tiny":
        x = x * F32(1e-15)
    elif family == "huge":
        x = x * F32(1e15)
    else:
        x = x * F32(5.0)
    if family == "zero_row":
        x[-1] = 0
    elif family == "clamp_row":
        x[-1] = clamp_row(rng, d)
    return np.ascontiguousarray(x, dtype=F32)


def clamp_row(rng, d: int) -> np.ndarray:
    r = rng.standard_normal(d) + 0.25
    return (r * (2e-14 / np.sqrt((r * r).sum()))).astype(F32)


def l2_normalize(x) -> np.ndarray:
    x = f64(x)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)


def l2_bound(x) -> np.ndarray:
    """2^-24 (ceil(d / 64) / 2 + 8) |ref|: the sum of squares carries ceil(d / 64) roundings of a lane's chain (its first sum is
    exact, the squares add one) and six of the butterfly, all on positive terms, and the square root halves their relative
    effect; a correctly rounded sqrtf, a correctly rounded division and the fp32 value of the clamp constant remain."""
    d = np.shape(x)[1]
    return U32 * (-(-d // 64) / 2.0 + 8.0) * np.abs(l2_normalize(x))


def _emulate_norms(x) -> np.ndarray:
    with np.errstate(over="ignore", under="ignore"):
        return np.maximum(np.sqrt(_wave_sum(_lane_sums(x * x))), F32(1e-12))


def emulate_l2(x) -> np.ndarray:
    x = np.asarray(x, dtype=F32)
    return x / _emulate_norms(x)[:, None]


# ------------------------------------------------------------------------------------------------------- pairwise scores
def pairwise_inputs(n: int, d: int):
    """a = 3 randn, b = 3 randn + 1 on every other row.  From n = 4 on the last four rows are: a zero row in a; in b; in both;
    the clamp row (norm 2e-14) in a."""
    rng = np.random.default_rng(104729 * n + d)
    a = rng.standard_normal((n, d), dtype=F32) * F32(3.0)
    b = rng.standard_normal((n, d), dtype=F32) * F32(3.0) + (np.arange(n) % 2).astype(F32)[:, None]
    zero_a, zero_b = [], []
    if n >= 4:
        zero_a, zero_b = [n - 4, n - 2], [n - 3, n - 2]
        a[zero_a] = 0
        b[zero_b] = 0
        a[n - 1] = clamp_row(rng, d)
    return a, b, sorted(set(zero_a + zero_b))


def pairwise(a, b, cosine: bool):
    """-> (scores float64 [n], bound [n]).  Dot: sum_j a_j b_j within 2^-24 (ceil(d / 64) + 8) sum_j |a_j b_j| (a lane chain of
    ceil(d / 64) rounded products and sums, six butterfly sums).  Cosine in the header's order -- normalise both rows, then the
    product sum -- within 2^-24 (2 ceil(d / 64) + 24) sum_j |â_j b̂_j|: each normalised factor carries the L2 bound."""
    a, b = f64(a), f64(b)
    k = -(-a.shape[1] // 64)
    if cosine:
        a, b = l2_normalize(a), l2_normalize(b)
    return (a * b).sum(axis=1), U32 * ((2 * k + 24) if cosine else (k + 8)) * np.abs(a * b).sum(axis=1)


def emulate_pairwise(a, b, cosine: bool) -> np.ndarray:
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    if cosine:
        a, b = a / _emulate_norms(a)[:, None], b / _emulate_norms(b)[:, None]
    return _wave_sum(_lane_sums(a * b))


# ---------------------------------------------------------------------------------------------------------- crest factor
CREST_N = [1, 5, 1027]
CREST_D = [2, 64, 130, 768, 4096]


def crest_inputs(n: int, d: int, fmt: str, pad: int = 0, kind: str = "spike") -> np.ndarray:
    """uint16 patterns [n, d + pad].  kind 'spike': randn rows; the LAST row (the n % 4 tail wave) is 0.01 randn with one entry
    8 -- the largest crest; from n = 5 on row 0 is zero and row 1 holds an inf next to entries of 1000 (skipped: its crest would
    be the largest).  kind 'zeros': an all-zero matrix.  The pad columns hold NaN."""
    rng = np.random.default_rng(65537 * n + 17 * d + pad)
    x = rng.standard_normal((n, d), dtype=F32)
    x[-1] *= F32(0.01)
    x[-1, d // 2] = 8.0
    if n >= 5:
        x[0] = 0
        x[1] = 0.001
        x[1, 0] = 1000.0
        x[1, d - 1] = np.inf
    if kind == "zeros":
        x[:] = 0
        x[::2] = -0.0
    out = np.full((n, d + pad), NAN16[fmt], dtype=np.uint16)
    out[:, :d] = round16(x, fmt)
    return out


def crest_fp32_inputs() -> np.ndarray:
    """fp32 rows [5, 130] that are NOT f16 values (Context.row_crest rounds them to f16 first): four randn rows (crest ~3) and a
    last row of +-(1 + 3 * 2^-12) with one entry 8 (crest ~6.6).  f16 rounds every 1 + 3 * 2^-12 UP to 1 + 2^-10, which moves the
    rms and with it the crest by 1.6e-4 (relative), some 250 bounds: the crest of the unrounded rows is far outside."""
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 130), dtype=F32)
    x[-1] = F32(1.0 + 3 * 2.0 ** -12) * np.where(np.arange(130) % 2, F32(-1.0), F32(1.0))
    x[-1, 77] = 8.0
    return x


def row_crest(rows16, fmt: str) -> float:
    """max over the rows of max|v| / sqrt(sum v^2 / d) of uint16 patterns [n, d], over rows that are finite and not all zero;
    0.0 when there is none."""
    v = widen16(rows16, fmt).astype(np.float64)
    d = v.shape[1]
    best = 0.0
    for r in v:
        if np.isfinite(r).all() and (r != 0).any():
            best = max(best, float(np.abs(r).max() / np.sqrt((r * r).sum() / d)))
    return best


def crest_rel_bound(d: int) -> float:
    """Relative: 2^-24 (ceil(d / 128) + 8).  A lane adds ceil(d / 128) pair sums a^2 + b^2 (three roundings inside each, two of
    them in parallel) and the butterfly six, all positive; the root halves them; / d, sqrtf and the final division remain."""
    return U32 * (-(-d // 128) + 8)


def emulate_row_crest(rows16, fmt: str) -> float:
    """crest16_kernel in fp32 numpy: lane l takes the value pairs l, l + 64, ... of a row; ss += a * a + b * b; butterfly;
    mx / sqrtf(ss / d) of the rows with ss > 0 and mx < inf; the maximum over the rows, 0 without one."""
    v = widen16(rows16, fmt)
    d = v.shape[1]
    a, b = v[:, 0::2], v[:, 1::2]
    with np.errstate(over="ignore", invalid="ignore"):
        ss = _wave_sum(_lane_sums(a * a + b * b))
        mx = np.fmax.reduce(np.abs(v), axis=1)              # fmaxf: a NaN operand is ignored
        ok = (ss > 0) & (mx < np.inf)
        crest = mx[ok] / np.sqrt(ss[ok] / F32(d))
    return float(crest.max()) if crest.size else 0.0
