"""-m gpu: the kernels behind the bidirectional Llama / Mistral / Qwen embedders (ABI v24), stand-alone against float64.

1. sgpt_attention_gqa_ex(causal = 0): grouped K / V in the bidirectional mode of csrc/attn.hip, in the harness of
   tests/test_gpu_attention_bidir.py -- values exact in both 16-bit formats, sharp logits (std 3: a softmax row is carried by a handful of
   keys anywhere in the sequence, the future ones included), finite sentinels of magnitude 64..95 on every row that belongs to no token
   (the alignment row behind an odd length INSIDE the allocation, the filler up to T, the slack the key tiles over-read).  Sequences of
   1, 7, 64, 70 and 130 rows on one axis (1 and 7 leave seq_len one short of their allocation), 4 query heads over 4 / 2 / 1 key heads,
   head_dim 64 / 128, f16 / bf16 / fp32.  Bounds: that file's, per dtype -- 3 u16 max|v| and 1e-5 max|v|.  Bit for bit: n_kv_heads == H
   is sgpt_attention_ex(causal = 0); grouped heads are sgpt_attention_ex(causal = 0) on explicitly replicated K / V^T; causal = 1 is
   sgpt_attention_gqa.  A second layout of the same buffers takes seq_len 0 (a sequence of no keys: zero rows) and 33 of 70.
2. The same entry above 2048 rows: one sequence of 2049, 2200 and 4100 rows, 2 query heads on 1 key head, head_dim 64, f16 and fp32
   (attn_f32_long_kernel<false>), against float64 on sampled query rows -- the first, the last, and one on each side of every multiple of
   2048.  Bounds: 16-bit 3 u16 max|v| (tests/test_gpu_long_sequences.py: the probabilities and the context round once whatever the
   number of keys); fp32 the operation-count bound derived in that file's docstring, u max|v| [n + n / 64 + 6 + 4 C + 2 +
   2 ((dh + 3) Lmax + 2)] with n the keys of the row (here every row sees all n), C = ceil(n / 2048), Lmax from the inputs.
3. sgpt_lnf_pool_range: widths 128 / 768 / 4096, LayerNorm and RMSNorm (and none), the three pool modes, lengths 1, 7, 64, 70, 130 each
   with pool_lo in {0, 1, len - 1, len, len + 5, -2}, pad_left on some, NaN in every row the kernel must not read.  Bound: that of
   tests/test_gpu_rowops.py (rowops_ref.lnf_pool) on the rows of the range -- 2^-23 (ceil(m / 4) + 4) sum_t w_t |h_t| / den for the m
   pooled rows (a wave's chain holds every fourth row of the range) plus the den-weighted 4 B of the norm, over the L2 norm and plus
   2^-22 |out| when normalised.  pool_lo NULL and all zeros are sgpt_lnf_pool_ex bit for bit; an empty range is an exactly zero row."""
import math

import numpy as np
import pytest
import torch

import llama_ref as LR
import rowops_ref as RO
from attn_ref import layout
from bert_ref import packed_attention_bidir
from test_gpu_attention import BOUND16, HALF, SLACK_ROWS, U16, VT_SLACK, _bf16_exact

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 70, 130]
H = 4
OUT_FILL = 77.0
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


# ---- 1. grouped bidirectional attention ---------------------------------------------------------------------------------------

def make_inputs(lens, n_heads, n_kv, dh, seed):
    rng = np.random.default_rng(seed)
    off, alloc, T, max_alloc = layout(lens)
    scale = 1.0 / math.sqrt(dh)
    R, dq, dkv = T + SLACK_ROWS, n_heads * dh, n_kv * dh
    sig = math.sqrt(3.0 / (scale * math.sqrt(dh)))               # logits ~ N(0, 3^2)
    real = np.zeros(R, bool)
    for s0, n in zip(off.tolist(), lens):
        real[s0:s0 + n] = True
    q = _bf16_exact(rng.standard_normal((R, dq)) * sig)
    k = _bf16_exact(rng.standard_normal((R, dkv)) * sig)
    v = _bf16_exact(rng.integers(-16, 17, size=(R, dkv)) / 8.0)
    rows = np.nonzero(~real)[0]
    sent = (64.0 + (rows % 32))[:, None]
    sgn = lambda n: np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[None, :]  # noqa: E731
    q[rows], k[rows], v[rows] = sent * sgn(dq), sent * np.ones((1, dkv)), -sent * sgn(dkv)
    return dict(q=q, k=k, v=v, off=off, alloc=alloc, lens=np.asarray(lens), T=T, max_alloc=max_alloc, real=real, dh=dh, scale=scale,
                H=n_heads, Hkv=n_kv, vmax=float(np.abs(v[real]).max()))


def replicated(inp):
    g = inp["H"] // inp["Hkv"]
    return LR.repeat_kv(inp["k"], inp["Hkv"], g, inp["dh"]), LR.repeat_kv(inp["v"], inp["Hkv"], g, inp["dh"])


_CASES = {}


def case(n_kv, dh):
    """Inputs and float64 reference of one (key heads, head_dim), computed once and shared (read-only)."""
    if (n_kv, dh) not in _CASES:
        inp = make_inputs(LENS, H, n_kv, dh, seed=900 + 10 * n_kv + dh)
        kr, vr = replicated(inp)
        ref = packed_attention_bidir(inp["q"], kr, vr, inp["off"], inp["lens"], H, inp["scale"])
        ref.setflags(write=False)
        _CASES[(n_kv, dh)] = (inp, ref)
    return _CASES[(n_kv, dh)]


def run(ctx, inp, fmt, entry, causal=False, seq_len=None, k=None, v=None):
    """One launch.  entry 'gqa_ex': sgpt_attention_gqa_ex on the case's K / V heads; 'gqa': sgpt_attention_gqa; 'ex': sgpt_attention_ex on
    H heads of k / v (the replicated ones, or the case's own when it has H of them).  Returns the [T, H dh + 8] output on the host."""
    T, dh, n_heads = inp["T"], inp["dh"], inp["H"]
    k = inp["k"] if k is None else k
    v = inp["v"] if v is None else v
    dq, dkv = n_heads * dh, k.shape[1]
    q, k, v = torch.from_numpy(inp["q"]), torch.from_numpy(k), torch.from_numpy(v)
    if fmt == "fp32":
        buf = torch.cat([q, k, v], dim=1).float().cuda()
        kk, vv = buf[:T, dq:dq + dkv], buf[:T, dq + dkv:]
    else:
        buf = torch.cat([q, k], dim=1).to(HALF[fmt]).cuda()
        kk, vv = buf[:T, dq:], v[:T + VT_SLACK].T.contiguous().to(HALF[fmt]).cuda()
    so = torch.tensor(np.concatenate([inp["off"], [inp["off"][-1] + inp["alloc"][-1]]]), dtype=torch.int32, device="cuda")
    sl = None if seq_len is None else torch.tensor(np.asarray(seq_len), dtype=torch.int32, device="cuda")
    out = torch.full((T, dq + 8), OUT_FILL, dtype=torch.float32 if fmt == "fp32" else HALF[fmt], device="cuda")
    if entry == "gqa_ex":
        ctx.attention_gqa_ex(buf[:T, :dq], kk, vv, out, so, n_heads, dkv // dh, dh, inp["max_alloc"], causal, seq_len=sl, scale=inp["scale"])
    elif entry == "gqa":
        ctx.attention(buf[:T, :dq], kk, vv, out, so, n_heads, dh, inp["max_alloc"], scale=inp["scale"], n_kv_heads=dkv // dh)
    else:
        assert dkv == dq
        ctx.attention(buf[:T, :dq], kk, vv, out, so, n_heads, dh, inp["max_alloc"], scale=inp["scale"], causal=causal, seq_len=sl)
    torch.cuda.synchronize()
    out = out.cpu()
    in_alloc = np.zeros(T, bool)
    for s0, a in zip(inp["off"].tolist(), inp["alloc"].tolist()):
        in_alloc[s0:s0 + a] = True
    assert (out[torch.from_numpy(~in_alloc)].double() == OUT_FILL).all(), "a row outside every allocation was written"
    assert (out[:, dq:].double() == OUT_FILL).all(), "a column past H * head_dim was written"
    return out


def _bound(inp, fmt):
    return (1e-5 if fmt == "fp32" else BOUND16 * U16[fmt]) * inp["vmax"]


@pytest.mark.parametrize("n_kv", [4, 2, 1])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("fmt", ["f16", "bf16", "fp32"])
def test_grouped_bidirectional_attention_vs_float64(ctx, fmt, dh, n_kv):
    inp, ref = case(n_kv, dh)
    dq = H * dh
    rows = np.nonzero(inp["real"][:inp["T"]])[0]
    out = run(ctx, inp, fmt, "gqa_ex", seq_len=inp["lens"])
    got = out[:, :dq].double().numpy()[rows]
    assert np.isfinite(got).all()
    err, bound = float(np.abs(got - ref[rows]).max()), _bound(inp, fmt)
    print(f"gqa bidir {fmt} dh{dh} H/Hkv={H // n_kv}: max|ctx - ref| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # only the addresses differ from the bidirectional attention on explicitly replicated K / V^T
    kr, vr = replicated(inp)
    assert torch.equal(out, run(ctx, inp, fmt, "ex", seq_len=inp["lens"], k=kr, v=vr)), "grouped K / V differs from replicated K / V"
    if n_kv == H:
        assert torch.equal(out, run(ctx, inp, fmt, "ex", seq_len=inp["lens"])), "n_kv_heads == H is sgpt_attention_ex itself"
    # causal = 1, seq_len = NULL: sgpt_attention_gqa exactly
    assert torch.equal(run(ctx, inp, fmt, "gqa_ex", causal=True), run(ctx, inp, fmt, "gqa")), "causal = 1 is not sgpt_attention_gqa"
    # seq_len shorter than the allocation: a sequence of no keys, and 33 keys of a 70-row allocation
    lens2 = [0, 7, 64, 33, 130]
    out2 = run(ctx, inp, fmt, "gqa_ex", seq_len=lens2)
    assert not out2[0:2, :dq].double().numpy().any(), "a sequence of no keys gives zero rows"
    keep = [i for i, n in enumerate(lens2) if n > 0]
    ref2 = packed_attention_bidir(inp["q"], kr, vr, inp["off"][keep], np.asarray(lens2)[keep], H, inp["scale"])
    rows2 = np.concatenate([np.arange(inp["off"][i], inp["off"][i] + lens2[i]) for i in keep])
    err2 = float(np.abs(out2[:, :dq].double().numpy()[rows2] - ref2[rows2]).max())
    assert err2 <= bound, (err2, bound)
    assert np.abs(ref2[inp["off"][3]:inp["off"][3] + 33] - ref[inp["off"][3]:inp["off"][3] + 33]).max() > 0.1     # the cut keys mattered


def test_grouped_bidirectional_refusals(ctx):
    inp, _ = case(2, 64)
    T, dq = inp["T"], H * 64
    buf = torch.cat([torch.from_numpy(inp["q"]), torch.from_numpy(inp["k"])], dim=1).to(torch.bfloat16).cuda()
    vt = torch.from_numpy(inp["v"])[:T + VT_SLACK].T.contiguous().to(torch.bfloat16).cuda()
    so = torch.tensor(np.concatenate([inp["off"], [inp["off"][-1] + inp["alloc"][-1]]]), dtype=torch.int32, device="cuda")
    sl = torch.tensor(inp["lens"], dtype=torch.int32, device="cuda")
    out = torch.zeros((T, dq), dtype=torch.bfloat16, device="cuda")
    args = (buf[:T, :dq], buf[:T, dq:], vt, out, so, H, 2, 64, inp["max_alloc"])
    ctx.attention_gqa_ex(*args, False, seq_len=sl, scale=0.125)
    bad = {"window": dict(window=8), "alibi": dict(alibi=torch.ones(H)), "x3": dict(x3=True, qk_lo_delta=8, v_lo_delta=8),
           "split context": dict(ctx_lo_delta=8)}
    for what, kw in bad.items():
        with pytest.raises(ValueError, match="sgpt_attention_gqa_ex"):
            ctx.attention_gqa_ex(*args, False, seq_len=sl, **kw)
            pytest.fail(f"accepted: {what}")
    with pytest.raises(ValueError, match="sgpt_attention_gqa_ex"):                 # out_fp8
        ctx.attention_gqa_ex(buf[:T, :dq], buf[:T, dq:], vt, torch.zeros((T, dq + 16), dtype=torch.uint8, device="cuda"), so, H, 2, 64,
                             inp["max_alloc"], False, seq_len=sl, out_scale=1.0)
    with pytest.raises(ValueError, match="seq_len belongs to the bidirectional mode"):
        ctx.attention_gqa_ex(*args, True, seq_len=sl)
    with pytest.raises(ValueError, match="n_heads % n_kv_heads"):
        ctx.attention_gqa_ex(buf[:T, :dq], buf[:T, dq:], vt, out, so, H, 3, 64, inp["max_alloc"], False)
    for bad_alloc in (inp["max_alloc"] + 1, 32770, 0):                              # odd, above SGPT_MAX_SEQ_LEN, below 2
        with pytest.raises(ValueError, match="max_alloc_len even, in \\[2, 32768\\]"):
            ctx.attention_gqa_ex(buf[:T, :dq], buf[:T, dq:], vt, out, so, H, 2, 64, bad_alloc, False)
    lib = ctx.lib                                                                   # 16-bit head_dim 256
    assert lib.sgpt_attention_gqa_ex(ctx.handle, 1, buf.data_ptr(), buf[:, dq:].data_ptr(), vt.data_ptr(), buf.stride(0), vt.stride(0),
                                     out.data_ptr(), out.stride(0), so.data_ptr(), len(LENS), T, 1, 1, 256, 0, 0.0625, None, inp["max_alloc"],
                                     0, 1.0, None, 0, 0, 0, 0, 0, 0, None, None) == -1
    torch.cuda.synchronize()


# ---- 2. above 2048 rows ------------------------------------------------------------------------------------------------------------

def sampled_rows(L):
    rows = {0, L - 1}
    for b in range(2048, L, 2048):
        rows |= {b - 1, b}
    return sorted(rows)


def ref_rows(inp, rows, n):
    """float64 context of the query rows `rows` of the one sequence [0, n): every key of it visible."""
    dh, g = inp["dh"], inp["H"] // inp["Hkv"]
    out = np.empty((len(rows), inp["H"] * dh))
    for h in range(inp["H"]):
        kv = h // g
        s = inp["scale"] * (inp["q"][rows, h * dh:(h + 1) * dh] @ inp["k"][:n, kv * dh:(kv + 1) * dh].T)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h * dh:(h + 1) * dh] = (p / p.sum(axis=1, keepdims=True)) @ inp["v"][:n, kv * dh:(kv + 1) * dh]
    return out


@pytest.mark.parametrize("L", [2049, 2200, 4100])
@pytest.mark.parametrize("fmt", ["f16", "fp32"])
def test_long_grouped_bidirectional_attention_on_sampled_rows(ctx, fmt, L):
    inp = make_inputs([L], 2, 1, 64, seed=L)
    assert inp["max_alloc"] > 2048
    rows = sampled_rows(L)
    assert rows[0] == 0 and rows[-1] == L - 1 and {2047, 2048} <= set(rows) and (L < 4096 or {4095, 4096} <= set(rows))
    ref = ref_rows(inp, rows, L)
    out = run(ctx, inp, fmt, "gqa_ex", seq_len=[L])
    assert torch.equal(out, run(ctx, inp, fmt, "gqa_ex", seq_len=[L])), "two runs of one call differ"
    got = out[:, :128].double().numpy()
    assert np.isfinite(got[:L]).all()
    err = float(np.abs(got[rows] - ref).max())
    if fmt == "fp32":
        q, k = np.abs(inp["q"][:L]).astype(np.float32), np.abs(inp["k"][:L]).astype(np.float32)
        lmax = inp["scale"] * max(float((q[:, h * 64:(h + 1) * 64] @ k.T).max()) for h in range(2))
        mult = U32 * (L + L / 64 + 6 + 4 * -(-L // 2048) + 2 + 2 * ((64 + 3) * lmax + 2))
        assert mult < 1e-3, "the derived bound must stay below 1e-3 max|v| (a dropped chunk costs ~0.5 max|v|)"
        bound = mult * inp["vmax"]
    else:
        bound = BOUND16 * U16[fmt] * inp["vmax"]
    print(f"long gqa bidir {fmt} L={L}: max|ctx - ref| on rows {rows} = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the causal context of the same rows is far away (but for the last row, which sees every key either way)
    causal = run(ctx, inp, fmt, "gqa_ex", causal=True)[:, :128].double().numpy()
    assert np.abs(causal[rows[:-1]] - ref[:-1]).max() > 0.25 and np.abs(causal[L - 1] - ref[-1]).max() <= 2 * bound
    kr, vr = replicated(inp)
    assert torch.equal(out, run(ctx, inp, fmt, "ex", seq_len=[L], k=kr, v=vr)), "grouped K / V differs from replicated K / V"


# ---- 3. pooling from a row on ------------------------------------------------------------------------------------------------------

EPS = 1e-5
POOL_LENS = [1, 7, 64, 70, 130]
MODE_CODE = {"weightedmean": 0, "mean": 1, "lasttoken": 2}


def pool_case(d):
    """30 sequences: every length with every pool_lo of {0, 1, len - 1, len, len + 5, -2}; pad_left on every third; NaN outside."""
    lens, los = [], []
    for n in POOL_LENS:
        for lo in (0, 1, n - 1, n, n + 5, -2):
            lens.append(n)
            los.append(lo)
    off, alloc, T, _ = layout(lens)
    pl = np.asarray([(3 * i) % 7 if i % 3 == 0 else 0 for i in range(len(lens))], np.int32)
    rng = np.random.default_rng(d)
    x = np.full((T, d), np.nan, dtype=np.float32)
    for s0, n in zip(off.tolist(), lens):
        x[s0:s0 + n] = rng.standard_normal((n, d), dtype=np.float32) * np.float32(2.0) + np.float32(0.3)
    g = (1.0 + 0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    so = np.concatenate([off, [off[-1] + alloc[-1]]]).astype(np.int32)
    return dict(x=x, g=g, b=b, off=off, so=so, lens=np.asarray(lens, np.int32), lo=np.asarray(los, np.int32), pl=pl)


def pool_ref(c, mode, norm, normalize):
    """float64 [B, d] and the per-element bound of the module docstring."""
    B, d = len(c["lens"]), c["x"].shape[1]
    out, bnd = np.zeros((B, d)), np.zeros((B, d))
    for i in range(B):
        s0, n, P = int(c["off"][i]), int(c["lens"][i]), int(c["pl"][i])
        raw = c["x"][s0:s0 + n].astype(np.float64)
        h, unit = raw, np.zeros(n)
        if norm == "ln":
            h, mean, rstd = RO.layernorm(raw, c["g"], c["b"], EPS, stats=True)
            unit = RO.layernorm_unit(raw, c["g"], h, mean, rstd)
        elif norm == "rms":
            h = LR.rms_norm(raw, c["g"], EPS)
            unit = RO.layernorm_unit(raw, c["g"], h, np.zeros(n), 1.0 / np.sqrt((raw * raw).mean(-1) + EPS))
        lo = min(max(int(c["lo"][i]), 0), n)
        t = np.arange(n - 1, n) if mode == "lasttoken" else np.arange(lo, n)
        w = (t + P + 1.0) if mode == "weightedmean" else np.ones(len(t))
        den = 1.0 if mode == "lasttoken" else max(float(w.sum()), 1e-9)
        e = (w[:, None] * h[t]).sum(0) / den
        eb = 2.0 ** -23 * (-(-len(t) // 4) + 4) * (w[:, None] * np.abs(h[t])).sum(0) / den + 4.0 * float((w * unit[t]).sum()) / den
        if normalize:
            nrm = max(math.sqrt(float((e * e).sum())), 1e-12)
            e, eb = e / nrm, eb / nrm + 2.0 ** -22 * np.abs(e / nrm)
        out[i], bnd[i] = e, eb
    return out, bnd


@pytest.mark.parametrize("norm", ["ln", "rms", None])
@pytest.mark.parametrize("d", [128, 768, 4096])
def test_lnf_pool_range_vs_float64(ctx, d, norm):
    c = pool_case(d)
    xd, so, sl, pd, lo = dev(c["x"]), dev(c["so"]), dev(c["lens"]), dev(c["pl"]), dev(c["lo"])
    g, b = dev(c["g"]), dev(c["b"])
    kw = dict(ln=(g, b, EPS)) if norm == "ln" else (dict(rms=(g, EPS)) if norm == "rms" else {})
    empty = np.nonzero(np.clip(c["lo"], 0, None) >= c["lens"])[0]
    assert len(empty) == 2 * len(POOL_LENS) + 1                  # pool_lo = len and len + 5 of every length, and row 1 of the 1-token one
    zeros = dev(np.zeros_like(c["lo"]))
    B = len(c["lens"])
    worst = 0.0
    for mode in MODE_CODE:
        for normalize in (False, True):
            got = ctx.lnf_pool_range(xd, so, sl, lo, pd, mode=mode, normalize=normalize, **kw)
            ref, bound = pool_ref(c, mode, norm, normalize)
            got64 = got.double().cpu().numpy()
            assert np.isfinite(got64).all(), "a row outside the range (or outside the sequence) leaked into the pooled vectors"
            if mode != "lasttoken":
                assert not got64[empty].any(), "an empty range must give an exactly zero row"
                assert not ref[empty].any()
            ok = bound > 0
            ratio = float((np.abs(got64 - ref)[ok] / bound[ok]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0 and (got64[~ok] == ref[~ok]).all(), (mode, normalize, ratio)
            # NULL and all zeros: sgpt_lnf_pool_ex bit for bit
            ex = torch.empty((B, d), dtype=torch.float32, device="cuda:0")
            st = ctx.lib.sgpt_lnf_pool_ex(ctx.handle, xd.data_ptr(), g.data_ptr() if norm else None, b.data_ptr() if norm == "ln" else None,
                                          so.data_ptr(), sl.data_ptr(), pd.data_ptr(), B, d, EPS, 1 if norm else 0, MODE_CODE[mode],
                                          1 if normalize else 0, None, 0, ex.data_ptr(), None, 1 if norm == "rms" else 0, None)
            assert st == 0
            assert torch.equal(ctx.lnf_pool_range(xd, so, sl, None, pd, mode=mode, normalize=normalize, **kw), ex)
            assert torch.equal(ctx.lnf_pool_range(xd, so, sl, zeros, pd, mode=mode, normalize=normalize, **kw), ex)
            if mode == "lasttoken":
                assert torch.equal(got, ex), "lasttoken is row len - 1 whatever pool_lo is"
    print(f"lnf_pool_range d={d} {norm}: worst error / bound = {worst:.3f}")


def test_lnf_pool_range_refusals(ctx):
    c = pool_case(128)
    xd, so, sl, lo = dev(c["x"]), dev(c["so"]), dev(c["lens"]), dev(c["lo"])
    B = len(c["lens"])
    out = torch.empty((B, 128), device="cuda:0")
    pw = torch.ones(256, device="cuda:0")

    def call(mode, pool_lo, norm_kind=0):
        return ctx.lib.sgpt_lnf_pool_range(ctx.handle, xd.data_ptr(), None, None, so.data_ptr(), sl.data_ptr(), None, B, 128, EPS, 0, mode, 0,
                                           pw.data_ptr(), 256, out.data_ptr(), None, norm_kind, pool_lo, None)
    assert call(1, lo.data_ptr()) == 0 and call(3, None) == 0
    assert call(3, lo.data_ptr()) == -1                          # learntmean with a range
    assert call(4, lo.data_ptr()) == -1 and call(4, None) == -1  # cls
    assert call(1, lo.data_ptr(), norm_kind=2) == -1
    torch.cuda.synchronize()
