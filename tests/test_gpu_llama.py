"""-m gpu: the Llama / Mistral family (SGPT_ARCH_LLAMA) on the device -- its four pieces of device arithmetic one by one against
float64, and the forward against HF LlamaModel / MistralModel's recorded values (tests/golden/tiny_llama*.npz, tiny_mistral_window.npz).

Bars.
RMSNorm: the tolerance tests/test_gpu_rowops.py holds the RowLN arithmetic to -- fp32 4 B per row with B = 2^-23 [max|x| rstd
  max|gamma| + max|ref|] (rowops_ref.layernorm_unit with mean = 0: an RMSNorm centres nothing), 16-bit ulp16(ref) / 2 + 4 B; and the
  16-bit output is the fp32-mode output rounded ONCE: bit-equal to torch's RNE cast of it.
sgpt_rope_half: the table values are the kernel's own, so per element two fp32 products and one sum: 2 u32 (|x[i]| + |x[i + dh/2]|)
  with u32 = 2^-23 (|s|, |c| <= 1), plus ulp16(ref) / 2 -- the one rounding -- for a 16-bit buffer.
Grouped attention: fp32 against tests/attn_ref.py on np.repeat-ed K / V heads at that file's fp32 tolerance (1e-5 max|v|); 16-bit at
  the tolerance of tests/test_gpu_attention.py (3 u16 max|v|); and bit for bit sgpt_attention on explicitly replicated K and V^T.
sgpt_swiglu: the inputs are exact in the operand format, so the error is the kernel's fp32 arithmetic and one output rounding.
  out = g / (1 + e^-g) * u: expf is good to 1 ulp (2^-23 relative on e^-g, hence at most that on the denominator), the sum
  1 + e^-g, the IEEE divide and the product round once each (2^-24 relative each): |out - ref| <= (2 + 3) * 2^-24 |ref| to first
  order.  Asserted as 8 * 2^-24 |ref| (+ 2^-126: a product below the normal range) and, for a 16-bit output, + ulp16(ref) / 2.
Forward, fp32: TOL_FP32 = 1e-3 on every hidden state and on the three pooled embeddings, the bar of tests/test_gpu_encode.py and
  tests/test_gpu_bert.py.  f16: the project's 1e-3 bar on L2-normalised pooled embeddings (max abs) and on their cosine matrix;
  bf16: 8 x that (8 x the f16 rounding unit), as tests/test_gpu_bert.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import attn_ref
import llama_ref as R
import rowops_ref as RO
from helpers import maxabs
from test_llama_ref import MODES, TAGS, load_llama_case, ref_forward

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3
TOL_F16 = 1e-3
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
TDT = {"fp32": torch.float32, **HALF}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
LENS = [1, 7, 64, 70, 130]
SENTINEL = 77.0


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def host64(t) -> np.ndarray:
    return t.detach().to("cpu", torch.float64).numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def range_flag(ctx) -> int:
    v = C.c_int32(0)
    assert ctx.lib.sgpt_range_check(ctx.handle, C.byref(v), 1, None) == 0
    return v.value


_models = {}


def llama_model(tag, dtype):
    from sgpt_amd import SGPTModel
    if (tag, dtype) not in _models:
        fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
        _models[(tag, dtype)] = SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    return _models[(tag, dtype)]


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------------

def rms_setup(T, d):
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((T, d)) * rng.uniform(0.5, 30, size=(T, 1)) + rng.uniform(-1, 1, size=(T, 1))).astype(np.float32)
    g = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32)
    ref = R.rms_norm(x, g, 1e-5)
    rstd = 1.0 / np.sqrt((x.astype(np.float64) ** 2).mean(-1) + 1e-5)
    unit = RO.layernorm_unit(x, g, ref, np.zeros(T), rstd)[:, None]
    return x, g, ref, unit


@pytest.mark.parametrize("d", [128, 768, 4096])
def test_rmsnorm_vs_float64(ctx, d):
    T = 32
    x, g, ref, unit = rms_setup(T, d)
    out = torch.full((T + 3, d), SENTINEL, dtype=torch.float32, device="cuda:0")
    ctx.rmsnorm(dev(x), dev(g), 1e-5, out=out)
    assert (out[T:] == SENTINEL).all(), "rows past T were written"
    r = float((np.abs(host64(out[:T]) - ref) / unit).max())
    print(f"rmsnorm fp32 d={d}: worst error / bound = {r / 4:.3f}")
    assert r <= 4.0
    xin = dev(x)
    ctx.rmsnorm(xin, dev(g), 1e-5, out=xin)
    assert torch.equal(xin, out[:T]), "in place differs from out of place"
    for fmt in ("f16", "bf16"):
        o16 = torch.full((T + 3, d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx.rmsnorm(dev(x), dev(g), 1e-5, out_dtype=HALF[fmt], out=o16)
        assert (o16[T:] == SENTINEL).all(), "rows past T were written"
        assert torch.equal(bits(o16[:T]), bits(out[:T].to(HALF[fmt]))), "the 16-bit output is not the fp32 output rounded once (RNE)"
        bound = 0.5 * RO.ulp16(ref, fmt) + 4.0 * unit
        r = float((np.abs(host64(o16[:T]) - ref) / bound).max())
        print(f"rmsnorm {fmt} d={d}: worst error / bound = {r:.3f}")
        assert r <= 1.0
    assert range_flag(ctx) == 0


def test_rmsnorm_records_f16_overflow_and_refuses_bad_arguments(ctx):
    d = 128
    x = torch.randn((8, d), device="cuda:0")
    x[3] *= 1e-3                                                   # a small row normalises to unit scale too: the gain decides
    range_flag(ctx)
    ctx.rmsnorm(x, torch.full((d,), 40000.0, device="cuda:0"), out_dtype=torch.bfloat16)
    assert range_flag(ctx) == 0
    ctx.rmsnorm(x, torch.full((d,), 40000.0, device="cuda:0"), out_dtype=torch.float16)
    assert range_flag(ctx) & 1
    ctx.rmsnorm(x, torch.ones(d, device="cuda:0"), out_dtype=torch.float16)
    assert range_flag(ctx) == 0
    g = torch.ones(d, device="cuda:0")
    o = torch.empty((8, d), device="cuda:0")
    lib, h = ctx.lib, ctx.handle
    assert lib.sgpt_rmsnorm(h, x.data_ptr(), g.data_ptr(), 8, 130, 1e-5, o.data_ptr(), 0, None) == -1          # d % 4
    assert lib.sgpt_rmsnorm(h, x.data_ptr(), g.data_ptr(), 8, 8192, 1e-5, o.data_ptr(), 0, None) == -1         # d > 4096
    assert lib.sgpt_rmsnorm(h, x.data_ptr(), None, 8, d, 1e-5, o.data_ptr(), 0, None) == -1
    assert lib.sgpt_rmsnorm(h, x.data_ptr(), g.data_ptr(), 8, d, 1e-5, o.data_ptr(), 2, None) == -1            # fp8: no such output
    assert lib.sgpt_rmsnorm(h, x.data_ptr(), g.data_ptr(), 8, d, 1e-5, x.data_ptr(), 3, None) == -1            # 16-bit in place


@pytest.mark.parametrize("tag", ["tiny_llama", "tiny_llama_dh128"])
def test_rms_mode_of_the_pool_kernel(ctx, tag):
    """sgpt_lnf_pool_ex(norm_kind = 1) on a residual stream of the float64 reference (the input of the last block, in the packed
    layout of sgpt_encode) against llama_ref's RMSNorm + pooling, the three pool modes, with and without the L2 normalisation."""
    from sgpt_amd.model import pack_host
    fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
    hs = ref_forward(tag)
    g = w["norm.weight"]
    pk = pack_host(seqs)
    ln = np.asarray(pk["seq_len"], np.int64)
    off = np.asarray(pk["seq_off"], np.int64)[:len(ln)]
    d = cfg.hidden_size
    x = np.full((pk["T_pad"], d), np.nan, np.float32)              # rows outside every sequence are never read
    for i, o in enumerate(off.tolist()):
        x[o:o + ln[i]] = hs[i][cfg.num_layers - 1].astype(np.float32)
    xd = dev(x)
    so, sl = dev(np.asarray(pk["seq_off"], np.int32)), dev(np.asarray(pk["seq_len"], np.int32))
    for mode in MODES:
        for normalize in (False, True):
            got = ctx.lnf_pool(xd, so, sl, rms=(dev(g), cfg.layer_norm_epsilon), mode=mode, normalize=normalize).cpu().numpy()
            ref = np.stack([R.pool(R.rms_norm(x[o:o + n], g, cfg.layer_norm_epsilon), mode) for o, n in zip(off.tolist(), ln.tolist())])
            if normalize:
                ref = _norm(ref)
            assert np.isfinite(got).all()
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            assert err < 2e-6, (mode, normalize, err)              # the bar of tests/test_rowops_ref.py for LayerNorm + pooling, 32 u |ref|
    o = torch.empty((len(seqs), d), device="cuda:0")
    assert ctx.lib.sgpt_lnf_pool_ex(ctx.handle, xd.data_ptr(), dev(g).data_ptr(), None, so.data_ptr(), sl.data_ptr(), None, len(seqs), d,
                                    1e-5, 1, 1, 0, None, 0, o.data_ptr(), None, 2, None) == -1          # norm_kind 0 | 1
    assert ctx.lib.sgpt_lnf_pool_ex(ctx.handle, xd.data_ptr(), dev(g).data_ptr(), None, so.data_ptr(), sl.data_ptr(), None, len(seqs), d,
                                    1e-5, 1, 1, 0, None, 0, o.data_ptr(), None, 0, None) == -1          # LayerNorm needs beta


# ---- half-split rotary -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("Hkv", [1, 2, 4])
def test_rope_half_vs_float64(ctx, Hkv, dh, dt):
    """q block (4 heads) at column 0, 8 sentinel columns, the k block (Hkv heads) at k_off, 8 more sentinel columns; positions
    repeated, out of order and out of range (clamped into the 40-row tables)."""
    from sgpt_amd.model import rotary_tables_half
    H, T, max_pos = 4, 32, 40
    k_off = H * dh + 8
    ld = k_off + Hkv * dh + 8
    sin, cos = rotary_tables_half(max_pos, dh, 10000.0)
    rng = np.random.default_rng(Hkv * dh)
    pos = rng.integers(0, max_pos, size=T).astype(np.int32)
    pos[:6] = [0, 39, 39, -5, 40, 1000]
    gen = torch.Generator(device="cuda:0").manual_seed(dh + Hkv)
    buf = (torch.randn((T + 1, ld), generator=gen, device="cuda:0") * 2.0).to(TDT[dt])
    before = buf.clone()
    ctx.rope_half(buf, dev(pos), dev(sin), dev(cos), H, Hkv, dh, k_off=k_off, T=T)
    x = host64(before)
    ref = x.copy()
    ref[:T, :H * dh] = R.rope_half(x[:T, :H * dh], pos, H, dh, sin=sin, cos=cos)
    ref[:T, k_off:k_off + Hkv * dh] = R.rope_half(x[:T, k_off:k_off + Hkv * dh], pos, Hkv, dh, sin=sin, cos=cos)
    touched = np.zeros((T + 1, ld), dtype=bool)
    touched[:T, :H * dh] = True
    touched[:T, k_off:k_off + Hkv * dh] = True
    same = (bits(buf) == bits(before)).cpu().numpy()
    assert same[~touched].all(), "a sentinel column, a key head past H_kv or the row after T was written"
    assert same[:T][pos[:T] <= 0].all(), "position 0 (and what clamps to it) is the identity"
    half = dh // 2
    pair = np.zeros((T + 1, ld))
    for c0 in [h * dh for h in range(H)] + [k_off + h * dh for h in range(Hkv)]:
        s = np.abs(x[:T, c0:c0 + half]) + np.abs(x[:T, c0 + half:c0 + dh])
        pair[:T, c0:c0 + half] = s
        pair[:T, c0 + half:c0 + dh] = s
    bound = 2 * 2.0 ** -23 * pair + (0.0 if dt == "fp32" else 0.5 * RO.ulp16(ref, dt))
    err = np.abs(host64(buf) - ref)
    assert (err[touched] <= bound[touched]).all(), float((err[touched] / bound[touched]).max())
    moved = np.abs(host64(buf) - x)[touched].max()
    assert moved > 1.0                                             # the rotation happened


def test_rope_half_refusals(ctx):
    from sgpt_amd.model import rotary_tables_half
    sin, cos = (dev(t) for t in rotary_tables_half(8, 64))
    buf = torch.zeros((4, 256), device="cuda:0")
    pos = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    lib, h = ctx.lib, ctx.handle
    ok = lambda *a: lib.sgpt_rope_half(h, buf.data_ptr(), 0, *a, pos.data_ptr(), sin.data_ptr(), cos.data_ptr(), 4, 2, 1, 64, 8, None)  # noqa: E731
    assert ok(256, 128) == 0
    assert ok(256, 120) == -1                                      # k block inside the q block
    assert ok(256, 200) == -1                                      # k block past the row
    assert ok(254, 128) == -1                                      # ld % 4
    assert lib.sgpt_rope_half(h, buf.data_ptr(), 0, 256, 128, pos.data_ptr(), sin.data_ptr(), cos.data_ptr(), 4, 2, 1, 60, 8, None) == -1   # head_dim % 8
    assert lib.sgpt_rope_half(h, buf.data_ptr(), 2, 256, 128, pos.data_ptr(), sin.data_ptr(), cos.data_ptr(), 4, 2, 1, 64, 8, None) == -1   # fp8
    torch.cuda.synchronize()


# ---- grouped attention -----------------------------------------------------------------------------------------------------

SLACK_ROWS = 320                       # q over-read reaches T + 255, the key tiles T + 63 (tests/test_gpu_attention.py)


def _exact16(x):
    """Values exact in bf16 AND f16 (bf16-rounded, magnitudes inside the f16 normal range)."""
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


_attn_cache = {}


def gqa_case(Hkv, dh):
    """Inputs + float64 references (window 0 and 16) of one (H_kv, head_dim), computed once and shared."""
    if (Hkv, dh) not in _attn_cache:
        H = 4
        off, alloc, T, max_alloc = attn_ref.layout(LENS)
        rng = np.random.default_rng(100 * Hkv + dh)
        q = _exact16(rng.standard_normal((T, H * dh)))
        k = _exact16(rng.standard_normal((T, Hkv * dh)))
        v = _exact16(rng.standard_normal((T, Hkv * dh)) * 2)
        scale = 1.0 / math.sqrt(dh)
        g = H // Hkv
        kr, vr = R.repeat_kv(k, Hkv, g, dh), R.repeat_kv(v, Hkv, g, dh)
        refs = {wdw: attn_ref.packed_attention(q, kr, vr, off, LENS, H, wdw, scale) for wdw in (0, 16)}
        real = np.zeros(T, dtype=bool)
        for o, n in zip(off.tolist(), LENS):
            real[o:o + n] = True
        _attn_cache[(Hkv, dh)] = dict(H=H, off=off, alloc=alloc, T=T, max_alloc=max_alloc, q=q, k=k, v=v, kr=kr, vr=vr, scale=scale,
                                      refs=refs, real=real, vmax=float(np.abs(v[real]).max()))
    return _attn_cache[(Hkv, dh)]


def _seq_off(c):
    return dev(np.concatenate([c["off"], [c["off"][-1] + c["alloc"][-1]]]).astype(np.int32))


def _qk16(c, k, fmt):
    """[T + slack, H dh + k columns] q | k rows (slack rows: finite sentinels) and V^T [k columns, T + slack]."""
    T, dq = c["T"], c["q"].shape[1]
    qk = torch.full((T + SLACK_ROWS, dq + k.shape[1]), 64.0, dtype=HALF[fmt], device="cuda:0")
    qk[:T, :dq] = dev(c["q"], HALF[fmt])
    qk[:T, dq:] = dev(k, HALF[fmt])
    return qk


def _vt16(c, v, fmt):
    T = c["T"]
    vt = torch.full((v.shape[1], T + SLACK_ROWS), 64.0, dtype=HALF[fmt], device="cuda:0")
    vt[:, :T] = dev(np.ascontiguousarray(v.T), HALF[fmt])
    return vt


@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("Hkv", [1, 2, 4])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_grouped_attention_16bit(ctx, fmt, Hkv, dh, window):
    c = gqa_case(Hkv, dh)
    H, T, dq = c["H"], c["T"], c["H"] * dh
    so = _seq_off(c)
    qk, vt = _qk16(c, c["k"], fmt), _vt16(c, c["v"], fmt)
    out = torch.full((T + 1, dq), SENTINEL, dtype=HALF[fmt], device="cuda:0")
    ctx.attention(qk[:, :dq], qk[:, dq:], vt, out, so, H, dh, c["max_alloc"], window=window, scale=c["scale"], n_kv_heads=Hkv)
    # the same arithmetic on explicitly replicated K and V^T through sgpt_attention: only the addresses differ
    qk2, vt2 = _qk16(c, c["kr"], fmt), _vt16(c, c["vr"], fmt)
    out2 = torch.full((T + 1, dq), SENTINEL, dtype=HALF[fmt], device="cuda:0")
    ctx.attention(qk2[:, :dq], qk2[:, dq:], vt2, out2, so, H, dh, c["max_alloc"], window=window, scale=c["scale"])
    torch.cuda.synchronize()
    real = torch.from_numpy(c["real"]).cuda()
    assert torch.equal(bits(out[:T][real]), bits(out2[:T][real])), "grouped K / V differs from replicated K / V"
    assert (out[T] == SENTINEL).all()
    if Hkv == H:                                                   # n_kv_heads == H on the same buffers: sgpt_attention itself
        out3 = torch.full((T + 1, dq), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx.attention(qk[:, :dq], qk[:, dq:], vt, out3, so, H, dh, c["max_alloc"], window=window, scale=c["scale"])
        assert torch.equal(bits(out), bits(out3))
    err = np.abs(host64(out[:T])[c["real"]] - c["refs"][window][c["real"]]).max()
    bound = 3.0 * U16[fmt] * c["vmax"]
    print(f"gqa {fmt} Hkv={Hkv} dh={dh} window={window}: max error / bound = {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("Hkv", [1, 2, 4])
def test_grouped_attention_fp32(ctx, Hkv, dh, window):
    c = gqa_case(Hkv, dh)
    H, T, dq, dkv = c["H"], c["T"], c["H"] * dh, Hkv * dh
    so = _seq_off(c)
    buf = torch.full((T + 32, dq + 2 * dkv), 64.0, device="cuda:0")     # (the wrapper takes the row count as the token axis: % 32)
    buf[:T] = dev(np.concatenate([c["q"], c["k"], c["v"]], axis=1))
    out = torch.full((T + 32, dq), SENTINEL, device="cuda:0")
    ctx.attention(buf[:, :dq], buf[:, dq:dq + dkv], buf[:, dq + dkv:], out, so, H, dh, c["max_alloc"], window=window, scale=c["scale"],
                  n_kv_heads=Hkv)
    buf2 = torch.full((T + 32, 3 * dq), 64.0, device="cuda:0")
    buf2[:T] = dev(np.concatenate([c["q"], c["kr"], c["vr"]], axis=1))
    out2 = torch.full((T + 32, dq), SENTINEL, device="cuda:0")
    ctx.attention(buf2[:, :dq], buf2[:, dq:2 * dq], buf2[:, 2 * dq:], out2, so, H, dh, c["max_alloc"], window=window, scale=c["scale"])
    torch.cuda.synchronize()
    real = torch.from_numpy(c["real"]).cuda()
    assert torch.equal(bits(out[:T][real]), bits(out2[:T][real])), "grouped K / V differs from replicated K / V"
    err = np.abs(host64(out[:T])[c["real"]] - c["refs"][window][c["real"]]).max()
    assert (out[T:] == SENTINEL).all(), "rows past the token axis were written"
    assert err <= 1e-5 * c["vmax"], err / c["vmax"]


def test_grouped_attention_refusals(ctx):
    c = gqa_case(2, 64)
    H, T, dq = 4, c["T"], 256
    so = _seq_off(c)
    qk, vt = _qk16(c, c["k"], "bf16"), _vt16(c, c["v"], "bf16")
    out = torch.zeros((T, dq), dtype=torch.bfloat16, device="cuda:0")
    slopes = torch.ones(H, device="cuda:0")
    lib, h = ctx.lib, ctx.handle

    def call(n_kv=2, alibi=None, out_fp8=0, x3=0, ctx_lo=0, dh=64, Hh=H):
        return lib.sgpt_attention_gqa(h, 1, qk.data_ptr(), qk[:, dq:].data_ptr(), vt.data_ptr(), qk.stride(0), vt.stride(0), out.data_ptr(),
                                      out.stride(0), so.data_ptr(), len(LENS), T, Hh, n_kv, dh, 0, 0.125, alibi, c["max_alloc"], out_fp8, 1.0,
                                      None, x3, 8 if x3 else 0, 8 if x3 else 0, ctx_lo, 0, None)
    assert call() == 0
    assert call(n_kv=3) == -1 and call(n_kv=0) == -1 and call(n_kv=8) == -1
    assert call(alibi=slopes.data_ptr()) == -1
    assert call(out_fp8=1) == -1 and call(x3=1) == -1 and call(ctx_lo=256) == -1
    assert call(dh=256, Hh=1, n_kv=1) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ctx.attention(qk[:, :dq], qk[:, dq:], vt, out, so, H, 64, c["max_alloc"], n_kv_heads=2, causal=False)


# ---- SwiGLU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ffn", [256, 384])
@pytest.mark.parametrize("fmt", ["fp32", "f16", "bf16"])
def test_swiglu_vs_float64(ctx, fmt, ffn):
    T = 32
    rng = np.random.default_rng(ffn)
    gu = rng.standard_normal((T, 2 * ffn)) * 3
    gu = np.where(np.abs(gu) < 2.0 ** -10, 2.0 ** -10, gu)        # (a bf16-rounded value below 2^-17 is not exact in f16)
    gu[0, :8] = [-30, -12, -1e-3, 0.0, 1e-3, 5, 12, 30]            # both tails of the sigmoid, and its centre
    gu = _exact16(gu)                                              # exact in every operand format
    ref = R.swiglu(gu)
    got = ctx.swiglu(dev(gu, TDT[fmt]))
    assert got.shape == (T, ffn) and got.dtype == TDT[fmt]
    bound = 8 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -126 + (0.0 if fmt == "fp32" else 0.5 * RO.ulp16(ref, fmt))
    err = np.abs(host64(got) - ref)
    print(f"swiglu {fmt} ffn={ffn}: worst error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert range_flag(ctx) == 0


def test_swiglu_records_f16_overflow_and_refuses_bad_arguments(ctx):
    gu = torch.zeros((4, 16), dtype=torch.float16, device="cuda:0")
    gu[1, 2], gu[1, 10] = 300.0, 300.0                             # silu(300) * 300 = 90000 > 32768
    range_flag(ctx)
    out = ctx.swiglu(gu)
    assert range_flag(ctx) & 1 and torch.isinf(out[1, 2])
    ctx.swiglu(gu.to(torch.bfloat16))
    assert range_flag(ctx) == 0
    gu[1, 10] = 1.0
    assert float(ctx.swiglu(gu)[1, 2]) == 300.0 and range_flag(ctx) == 0
    lib, h = ctx.lib, ctx.handle
    o = torch.empty((4, 8), dtype=torch.float16, device="cuda:0")
    assert lib.sgpt_swiglu(h, gu.data_ptr(), 3, 4, 8, o.data_ptr(), None) == 0
    assert lib.sgpt_swiglu(h, gu.data_ptr(), 3, 4, 4, o.data_ptr(), None) == -1        # ffn % 8 (16-bit)
    assert lib.sgpt_swiglu(h, gu.data_ptr(), 2, 4, 8, o.data_ptr(), None) == -1        # fp8
    assert lib.sgpt_swiglu(h, gu.data_ptr(), 3, 4, 8, gu.data_ptr(), None) == -1       # in place
    assert lib.sgpt_swiglu(h, None, 3, 4, 8, o.data_ptr(), None) == -1
    torch.cuda.synchronize()


# ---- forward ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_llama_forward_fp32_vs_hf_golden(tag):
    fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
    m = llama_model(tag, "fp32")
    L = cfg.num_layers
    for mode in MODES:
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        err = maxabs(got, fx[f"emb_{mode}"])
        print(f"{tag} fp32 {mode}: max|emb - ref| = {err:.3e}")
        assert err < TOL_FP32, (tag, mode)
    want = fx["hidden"]
    worst = 0.0
    for li in range(L + 1):                                      # hidden_states[li] per token, as HF numbers them
        hid = m.token_embeddings(seqs, layer_idx=li)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            e = maxabs(hid[i].cpu().numpy(), want[li, a:b])
            worst = max(worst, e)
            assert e < TOL_FP32, (tag, li, i)
    print(f"{tag} fp32 hidden states: max|h - ref| = {worst:.3e}")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_llama_forward_16bit_vs_hf_golden(tag, dtype):
    fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
    m = llama_model(tag, dtype)
    for mode in MODES:
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        ref = fx[f"emb_{mode}"]
        assert np.isfinite(got).all()
        err = maxabs(_norm(got), _norm(ref))
        dev_ = maxabs(_norm(got) @ _norm(got).T, _norm(ref) @ _norm(ref).T)
        print(f"{tag} {dtype} {mode}: max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dev_:.3e}")
        bar = TOL_F16 if dtype == "f16" else 8 * TOL_F16
        assert err < bar and dev_ < bar, (tag, mode)
        gn = m.encode_ids(seqs, mode=mode, normalize=True).cpu().numpy()
        assert maxabs(gn, _norm(got)) < 1e-6
    assert m.range_flags(reset=False) == 0


# ---- invariants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_llama_every_hidden_state_through_encode_layers(dtype):
    fx, hf, cfg, w, seqs, cuts = load_llama_case("tiny_llama")
    m = llama_model("tiny_llama", dtype)
    want = fx["hidden"].astype(np.float64)
    for mode in MODES:
        ref = np.stack([[R.pool(want[li, a:b], mode) for a, b in zip(cuts[:-1], cuts[1:])] for li in range(cfg.num_layers + 1)])
        layers, mean = m.encode_packed_layers(m.pack(seqs), mode=mode, per_layer=True)
        layers, mean = layers.cpu().numpy(), mean.cpu().numpy()
        assert layers.shape == (cfg.num_layers + 1, len(seqs), cfg.hidden_size)
        if dtype == "fp32":
            assert maxabs(layers, ref) < TOL_FP32 and maxabs(mean, ref.mean(0)) < TOL_FP32
        else:
            for li in range(cfg.num_layers + 1):
                assert maxabs(_norm(layers[li]), _norm(ref[li])) < TOL_F16, (mode, li)


@pytest.mark.parametrize("tag", ["tiny_llama_g4", "tiny_mistral_window"])
@pytest.mark.parametrize("dtype", ["f16", "fp32"])
def test_llama_batch_invariance_and_layout_invariance(tag, dtype):
    """A batch and its sentences encoded alone agree bit for bit; so do a 32-row layout and the same sequence inside a 256-row one."""
    fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
    m = llama_model(tag, dtype)
    batch = m.encode_ids(seqs, mode="weightedmean")
    for i, s in enumerate(seqs):
        alone = m.encode_ids([s], mode="weightedmean")
        assert torch.equal(alone[0], batch[i]), (tag, dtype, i)
    one = (seqs[1] * 3)[:18]
    assert len(one) == 18
    pb = m.pack([one])
    assert pb.T_pad == 32
    alone = m.encode_packed(pb, mode="mean")
    pb2 = m.pack([one] + seqs[2:])
    assert pb2.T_pad > 32, pb2.T_pad
    bulk = m.encode_packed(pb2, mode="mean")
    assert torch.equal(alone[0], bulk[0]), (tag, dtype)


def test_llama_256_row_layout(ctx):
    """The layout test above with a layout of exactly 256 rows (the 256x256-tile kernels' row count)."""
    fx, hf, cfg, w, seqs, cuts = load_llama_case("tiny_llama")
    m = llama_model("tiny_llama", "f16")
    one = (seqs[1] * 3)[:18]
    fill = [seqs[2], seqs[3], seqs[2], seqs[1] + seqs[1] + seqs[1][:4]]     # 18 + 64 + 70 + 64 + 18 allocated rows = 234 -> 256
    pb2 = m.pack([one] + fill)
    assert pb2.T_pad == 256, pb2.T_pad
    assert torch.equal(m.encode_packed(m.pack([one]), mode="mean")[0], m.encode_packed(pb2, mode="mean")[0])


# ---- end to end ------------------------------------------------------------------------------------------------------------

def test_llama_embedder_and_search_end_to_end():
    from test_llama_ref import _Tok
    from sgpt_amd.beir import CustomEmbedder, DenseRetrievalExactSearch
    m = llama_model("tiny_llama", "f16")
    tok = _Tok()
    rng = np.random.default_rng(4)
    texts = [" ".join(f"w{j}" for j in rng.integers(0, 190, size=n)) for n in (3, 9, 17, 40, 5, 28)]
    framed = [[tok.bos_token_id] + tok.convert_tokens_to_ids(t.split()) for t in texts]
    emb = CustomEmbedder(model=m, tokenizer=tok, method="weightedmean", maxseqlen=64)
    want = m.encode_ids(framed, mode="weightedmean").cpu().numpy()
    assert maxabs(emb.embed_device(texts, True).cpu().numpy(), want) < 1e-6
    corpus = {f"d{i}": {"title": "", "text": t} for i, t in enumerate(texts)}
    queries = {"q0": texts[1], "q1": texts[3], "q2": texts[4]}
    res = DenseRetrievalExactSearch(emb, corpus_chunk_size=4).search(corpus, queries, 3, "cos_sim")
    # documents are embedded from title + " " + text (the reference's corpus formatting): rank the same embeddings in numpy
    docs = emb.embed_device([(c["title"] + " " + c["text"]).strip() for c in corpus.values()], False).cpu().numpy().astype(np.float64)
    qs = emb.embed_device(list(queries.values()), True).cpu().numpy().astype(np.float64)
    cos = _norm(qs) @ _norm(docs).T
    for qi, qid in enumerate(queries):
        order = [f"d{j}" for j in np.argsort(-cos[qi], kind="stable")[:3]]
        got = sorted(res[qid], key=res[qid].get, reverse=True)[:3]
        assert got == order, (qid, got, order)
    with pytest.raises(ValueError, match="Llama"):
        CustomEmbedder(model=m, tokenizer=tok, method="mean", specb=True)


def test_llama_loads_from_a_checkpoint_folder(tmp_path):
    """A sentence-transformers folder as HF saves a *ForCausalLM checkpoint -- `model.`-prefixed names and an `lm_head` -- through
    SGPTModel.from_pretrained and SentenceTransformerSGPT.from_pretrained: the embeddings of the model built from the plain dict."""
    from test_llama_ref import _Tok
    from sgpt_amd import SGPTModel
    from sgpt_amd.formats import write_st_folder
    from sgpt_amd.st import SentenceTransformerSGPT
    fx, hf, cfg, w, seqs, cuts = load_llama_case("tiny_mistral_window")
    sd = {"model." + k: v for k, v in w.items()}
    sd["lm_head.weight"] = np.ones_like(w["embed_tokens.weight"])
    p = str(tmp_path / "st")
    write_st_folder(p, hf, sd, pooling_mode="weightedmean", max_seq_length=64, normalize=True)
    want = llama_model("tiny_mistral_window", "f16").encode_ids(seqs, mode="weightedmean")
    m = SGPTModel.from_pretrained(p, device="cuda:0", dtype="f16")
    assert m.cfg.model_type == "llama" and m.cfg.window_size == 16 and m.cfg.num_kv_heads == 1
    assert torch.equal(m.encode_ids(seqs, mode="weightedmean"), want)
    m.close()
    st = SentenceTransformerSGPT.from_pretrained(p, tokenizer=_Tok(), device="cuda:0", dtype="f16")
    assert st.pooling_mode == "weightedmean" and st.normalize
    texts = ["w5 w9 w120 w33", "w7", " ".join(f"w{i}" for i in range(80))]            # the last one is cut to 63 tokens + BOS
    ids = [[1] + [int(t[1:]) + 3 for t in x.split()][:63] for x in texts]
    ref = llama_model("tiny_mistral_window", "f16").encode_ids(ids, mode="weightedmean", normalize=True).cpu().numpy()
    assert maxabs(st.encode(texts), ref) < 1e-6
    st.model.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_llama_refuses_what_it_does_not_build():
    from sgpt_amd import SGPTModel
    fx, hf, cfg, w, seqs, cuts = load_llama_case("tiny_llama")
    for dtype in ("fp8", "fp8mfma"):
        with pytest.raises(ValueError, match="Llama"):
            SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    for kw in (dict(precision="x3"), dict(precision="auto-class"), dict(precise_qk="full")):
        with pytest.raises(ValueError, match="Llama"):
            SGPTModel(cfg, w, device="cuda:0", dtype="f16", **kw)
    m = llama_model("tiny_llama", "f16")
    assert m.precision == "plain"
    with pytest.raises(ValueError, match="learntmean"):
        m.encode_ids(seqs[:3], mode="learntmean")
    with pytest.raises(ValueError, match="lm_logprobs"):
        m.lm_logprobs(torch.zeros((32, cfg.hidden_size), device="cuda"), [0], [1])
    # the C ABI refuses on its own, whatever the Python host checked first
    lib, h = m.ctx.lib, m.handle
    plan = np.ones(cfg.num_layers * 5, dtype=np.int32)
    assert lib.sgpt_model_set_precision(h, plan.ctypes.data_as(C.c_void_p), plan.size) == -1
    n = C.c_int32(0)
    assert lib.sgpt_model_range_adapt(h, C.byref(n), None) == -1
    sh = np.zeros(cfg.num_layers * 4, dtype=np.int32)
    assert lib.sgpt_model_set_range_shifts(h, sh.ctypes.data_as(C.c_void_p), sh.size) == -1
    assert lib.sgpt_model_precision_probe_begin(h) == -1
    out = torch.zeros(1, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.sgpt_lm_logprobs(h, torch.zeros((32, cfg.hidden_size), device="cuda").data_ptr(), idx.data_ptr(), idx.data_ptr(), 1,
                                out.data_ptr(), None, None) == -1
    pb = m.pack(seqs[:2])
    o = torch.zeros((2, cfg.hidden_size), device="cuda")
    for mode in (3, 4):                                          # learntmean, cls
        assert lib.sgpt_encode(h, pb.ids.data_ptr(), pb.pos.data_ptr(), pb.seq_off.data_ptr(), pb.seq_len.data_ptr(), pb.pad_left.data_ptr(),
                               pb.B, pb.T_pad, pb.max_alloc, mode, cfg.num_layers, 1, 0, o.data_ptr(), None, None) == -1
    # load-time refusals of the descriptor: fp8 dtypes, split operands, n_kv_heads that does not divide the heads
    from sgpt_amd import _lib
    for kw in (dict(compute_dtype=_lib.SGPT_FP8W), dict(compute_dtype=_lib.SGPT_FP8M), dict(qk_split=1), dict(split_weights=1),
               dict(n_kv_heads=3)):
        d = dict(arch=_lib.SGPT_ARCH_LLAMA, n_layers=1, d_model=128, n_heads=2, d_ffn=256, vocab=10, max_pos=16, window=0, ln_eps=1e-5,
                 attn_scale=0.125, compute_dtype=_lib.SGPT_F16, rotary_dim=64, qk_split=0, split_weights=0, n_kv_heads=1)
        d.update(kw)
        desc = _lib.ModelDesc(**d)
        views = (_lib.TensorView * 1)(_lib.TensorView(b"x", 0, 0))
        hh = C.c_void_p()
        assert lib.sgpt_model_load(m.ctx.handle, C.byref(desc), views, 0, C.byref(hh)) == -1, kw
    desc = _lib.ModelDesc(arch=_lib.SGPT_ARCH_GPTNEO, n_layers=1, d_model=128, n_heads=2, d_ffn=256, vocab=10, max_pos=16, window=0,
                          ln_eps=1e-5, attn_scale=1.0, compute_dtype=_lib.SGPT_F16, n_kv_heads=1)
    assert lib.sgpt_model_load(m.ctx.handle, C.byref(desc), views, 0, C.byref(hh)) == -1        # grouped K / V is this family's
