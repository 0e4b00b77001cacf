"""Test infrastructure: the encoder's row operations in float64 numpy -- the references of tests/test_gpu_rowops.py, pinned
against the oracle, torch and the golden fixtures in tests/test_rowops_ref.py.

Every function takes arrays of any float type and computes in float64 from their exact values: LayerNorm
(HF:gpt_neo:317-319), the final LayerNorm fused with the pooling of a packed batch (Pooling.py:99-125,
beir_dense_retriever.py:238-282, WeightedMeanPooling.py:21-39), GPT-J's rotate-every-two rotary embedding
(HF:gptj:57-67,190-210), the embedding gather-add (HF:gpt_neo:444,462-463) and the log-softmax gather with the greedy token
(sgptce.py:233-255).  The error-bound helpers state what an fp32 / 16-bit implementation of the same operation may differ by."""
import numpy as np

POOL_MODES = {"weightedmean": 0, "mean": 1, "lasttoken": 2, "learntmean": 3}
EPS32 = 2.0 ** -23


def f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = [64, 128, 772, 768, 1024, 1280, 1536, 2304, 2560, 2816, 3072, 4096]     # every NV of launch_layernorm, masked tails
LN_FAMILIES = ["plain", "offset", "outlier"]


def ln_inputs(T, d, family, seed):
    """The input families of the GPU test: plain 3 randn + 0.5, offset randn + 100, one outlier channel x 300."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, d), dtype=np.float32)
    if family == "plain":
        x = x * np.float32(3.0) + np.float32(0.5)
    elif family == "offset":
        x = x + np.float32(100.0)
    else:
        x[:, d // 3] *= np.float32(300.0)
    g = (1.0 + 0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    return x, g, b


def layernorm(x, gamma, beta, eps: float, stats: bool = False):
    """(x - mean) / sqrt(var + eps) * gamma + beta over the last axis, biased variance.  stats=True also returns (mean, rstd)."""
    x, g, b = f64(x), f64(gamma), f64(beta)
    mean = x.mean(axis=-1, keepdims=True)
    xc = x - mean
    rstd = 1.0 / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + float(eps))
    y = xc * rstd * g + b
    return (y, mean[..., 0], rstd[..., 0]) if stats else y


def layernorm_unit(x, gamma, ref, mean, rstd) -> np.ndarray:
    """Per row: B = 2^-23 [(|mean| + max|x|) rstd max|gamma| + max|ref|] -- one fp32 rounding of the centred value (its operands
    are as large as |mean| + max|x|) carried through the scaling, plus one of the result.  An fp32 LayerNorm is a few B from
    the float64 one whatever its reduction order."""
    x, g, ref = f64(x), f64(gamma), f64(ref)
    return EPS32 * ((np.abs(mean) + np.abs(x).max(axis=-1)) * rstd * np.abs(g).max() + np.abs(ref).max(axis=-1))


def ulp16(v, fmt: str) -> np.ndarray:
    """Spacing of the 16-bit format at |v|: 2^(e - 10) for IEEE half with its subnormal spacing 2^-24 as the floor, 2^(e - 7) for
    bfloat16, e = floor(log2 |v|)."""
    v = np.abs(f64(v))
    _, e = np.frexp(v)                                     # v = m 2^e, 0.5 <= m < 1: floor(log2 v) = e - 1
    if fmt == "f16":
        return np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 7)


# ---------------------------------------------------------------------------------- final LayerNorm + pooling, packed batch
def pool_weights(n: int, P: int, mode: str, pos_weights=None) -> np.ndarray:
    """Weights of the n real tokens of a sequence that sits behind P padding slots: the PADDED index P + t counts."""
    t = np.arange(n, dtype=np.int64)
    if mode == "weightedmean":
        return (P + t + 1).astype(np.float64)
    if mode == "mean":
        return np.ones(n)
    if mode == "learntmean":
        pw = f64(pos_weights)
        return pw[np.minimum(P + t, pw.shape[0] - 1)]       # the kernel's index clamp: the last weight repeats
    if mode == "lasttoken":
        w = np.zeros(n)
        w[n - 1:] = 1.0
        return w
    raise ValueError(f"unknown pooling mode {mode}")


def lnf_pool(x, seq_off, seq_len, pad_left=None, mode: str = "weightedmean", ln=None, normalize: bool = False, pos_weights=None,
             bound: bool = False):
    """x [rows, d]; sequence i owns rows [seq_off[i], seq_off[i] + seq_len[i]) -- no other row is read.  ln = (gamma, beta, eps)
    applies the final LayerNorm to every row first.  sum_t w_t h_t / max(sum_t w_t, 1e-9) (lasttoken: row len - 1), then
    optionally x / max(||x||, 1e-12).  A sequence of length 0 gives zeros.  Returns float64 [B, d]; with bound=True also the
    per-element error bound of an fp32 implementation that splits the rows over four chains and adds the four partial sums:
        2^-23 (ceil(len / 4) + 4) sum_t w_t |h_t| / den   [+ sum_t w_t 4 B_t / den with ln]   [/ ||e||, + 2^-22 |out| normalised]."""
    B = len(seq_len)
    d = np.shape(x)[1]
    out, bnd = np.zeros((B, d)), np.zeros((B, d))
    for i in range(B):
        s0, n = int(seq_off[i]), int(seq_len[i])
        if n == 0:
            continue
        P = 0 if pad_left is None else int(pad_left[i])
        h = f64(x[s0:s0 + n])
        unit = np.zeros(n)
        if ln is not None:
            raw = h
            h, mean, rstd = layernorm(raw, ln[0], ln[1], ln[2], stats=True)
            unit = layernorm_unit(raw, ln[0], h, mean, rstd)
        w = pool_weights(n, P, mode, pos_weights)
        den = 1.0 if mode == "lasttoken" else max(w.sum(), 1e-9)
        e = (w[:, None] * h).sum(axis=0) / den
        eb = EPS32 * (-(-n // 4) + 4) * (np.abs(w)[:, None] * np.abs(h)).sum(axis=0) / den + 4.0 * (np.abs(w) * unit).sum() / den
        if normalize:
            nrm = max(np.sqrt((e * e).sum()), 1e-12)
            e, eb = e / nrm, eb / nrm
            eb = eb + 2.0 * EPS32 * np.abs(e)
        out[i], bnd[i] = e, eb
    return (out, bnd) if bound else out


def pool_padded(hidden, mask, mode: str = "weightedmean", pos_weights=None, normalize: bool = False) -> np.ndarray:
    """The same pooling in the padded form the reference code has: hidden [B, S, d], mask {0,1} [B, S] (any padding side);
    weights follow the padded index."""
    h, m = f64(hidden), f64(mask)
    B, S, d = h.shape
    if mode == "lasttoken":
        idx = [int(np.nonzero(r)[0][-1]) if r.any() else 0 for r in m]
        e = h[np.arange(B), idx] * m.any(axis=1)[:, None]
    else:
        w = m.copy()
        if mode == "weightedmean":
            w = w * np.arange(1, S + 1, dtype=np.float64)
        elif mode == "learntmean":
            pw = f64(pos_weights)
            w = w * pw[np.minimum(np.arange(S), pw.shape[0] - 1)]
        elif mode != "mean":
            raise ValueError(f"unknown pooling mode {mode}")
        e = (h * w[:, :, None]).sum(axis=1) / np.maximum(w.sum(axis=1), 1e-9)[:, None]
    if normalize:
        e = e / np.maximum(np.sqrt((e * e).sum(axis=1, keepdims=True)), 1e-12)
    return e


def pack_padded(hidden, mask):
    """Padded [B, S, d] + contiguous {0,1} mask -> (rows [sum len, d], seq_off, seq_len, pad_left) of the packed form."""
    m = np.asarray(mask) != 0
    lens = m.sum(axis=1).astype(np.int64)
    pad_left = np.array([int(np.argmax(r)) if r.any() else 0 for r in m], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows = np.concatenate([np.asarray(hidden)[i, p:p + n] for i, (p, n) in enumerate(zip(pad_left, lens))], axis=0)
    return rows, off, lens, pad_left


# ------------------------------------------------------------------------------------------------------------- rotary
def rope(buf, pos, sin, cos, H: int, head_dim: int, rotary_dim: int, k_off: int, T=None) -> np.ndarray:
    """GPT-J rotate-every-two on the leading rotary_dim columns of each head of q (column 0) and k (column k_off) of rows
    [0, T) of buf [rows, ld]:  (x[2i], x[2i+1]) <- (x[2i] c - x[2i+1] s, x[2i+1] c + x[2i] s), s / c = sin / cos[pos[t], i].
    Every other element is returned as it came."""
    out = f64(buf).copy()
    T = out.shape[0] if T is None else T
    s, c = f64(sin)[np.asarray(pos)[:T]], f64(cos)[np.asarray(pos)[:T]]          # [T, rotary_dim / 2]
    for base in (0, k_off):
        for h in range(H):
            c0 = base + h * head_dim
            x0, x1 = out[:T, c0:c0 + rotary_dim:2].copy(), out[:T, c0 + 1:c0 + rotary_dim:2].copy()
            out[:T, c0:c0 + rotary_dim:2] = x0 * c - x1 * s
            out[:T, c0 + 1:c0 + rotary_dim:2] = x1 * c + x0 * s
    return out


# -------------------------------------------------------------------------------------------------------------- embed
def embed(ids, pos, wte, wpe=None) -> np.ndarray:
    e = f64(wte)[np.asarray(ids)]
    return e if wpe is None else e + f64(wpe)[np.asarray(pos)]


# ------------------------------------------------------------------------------------------------- log-softmax gather
def logprob_rows(logits, V: int, targets):
    """-> (log_softmax(logits[r, :V])[targets[r]] float64 [n], argmax with the first maximum winning int64 [n])."""
    x = f64(logits)[:, :V]
    mx = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(axis=1))
    r = np.arange(x.shape[0])
    return (x[r, np.asarray(targets)] - mx[:, 0]) - lse, np.argmax(x, axis=1)
