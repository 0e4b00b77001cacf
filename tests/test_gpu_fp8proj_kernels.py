"""-m gpu: the two quantising row kernels of the fp8 projections of the Llama family, sgpt_rmsnorm_fp8 and sgpt_swiglu_fp8, against
float64 (include/sgpt_hip.h ABI v25).

Both write, per row, one power-of-two scale -- the smallest 2^k with max|row| / 2^k <= 448 -- and the RNE e4m3fn codes of row / scale.
What is asserted, per kernel:
  scale   equals the rule applied to the FLOAT64 row maximum.  That is only decidable where the reference maximum is further from a
          switch point of the rule (1.75 x 2^e) than the fp32 arithmetic's bound; the inputs are drawn from seeds for which that holds,
          which the CPU test of this file checks (and the GPU tests again, on the arrays they use).
  codes   every code is the RNE encoding of SOME value inside reference +- bound (tests/test_gpu_attention.py::
          test_attention_out_fp8_codes does the same for the e4m3 context): dec(code) lies between the encodings of the band's ends.
  share   at most 1e-3 of the codes differ from the plain encoding of the reference (a value within the bound of a rounding
          boundary may go either way; the reference rounded to fp32 alone flips about 1e-4 of them).
Bounds.  RMSNorm: 4 B per row, B = rowops_ref.layernorm_unit with mean 0, the fp32 bar of tests/test_gpu_llama.py::test_rmsnorm_vs_float64.
SwiGLU: h (1 +- 2^-20) -- eight fp32 units in the last place, twice the four of expf, the add, the divide and the multiply; the 16-bit
inputs are exact.  Shapes: the issue's, plus for SwiGLU one width for every register-step variant of the launcher (<= 4096, 8192, 16384,
28672 columns, and the re-reading variant beyond)."""
import numpy as np
import pytest
import torch

import fp8proj_ref as F
import llama_ref as R
import rowops_ref as RO
from fp8proj_ref import O

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = 0x5A
RMS_SHAPES = [(7, 128), (7, 768), (7, 4096), (257, 256)]
SWIGLU_SHAPES = [(5, 256), (5, 2304), (5, 14336), (64, 512), (3, 8192), (3, 28672), (3, 28688)]
SHARE = 1e-3


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


_cache = {}


def rms_case(T, d):
    """x, gamma, float64 reference, per-row bound -- from the first seed whose row maxima are all clear of a scale switch point."""
    if ("rms", T, d) not in _cache:
        for seed in range(100 * d + T, 100 * d + T + 8):
            rng = np.random.default_rng(seed)
            x = (rng.standard_normal((T, d)) * rng.uniform(0.5, 30, size=(T, 1)) + rng.uniform(-1, 1, size=(T, 1))).astype(np.float32)
            g = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32)
            ref = R.rms_norm(x, g, 1e-5)
            rstd = 1.0 / np.sqrt((x.astype(np.float64) ** 2).mean(-1) + 1e-5)
            b = 4.0 * RO.layernorm_unit(x, g, ref, np.zeros(T), rstd)
            amax = np.abs(ref).max(axis=1)
            if (F.switch_margin(amax) > 2.0 * b / amax).all():
                _cache[("rms", T, d)] = (x, g, ref, b, seed)
                break
    return _cache[("rms", T, d)]


def swiglu_case(T, ffn, fmt):
    """gu (exact in fmt; gate in [-12, 12], row 2 all zeros), float64 h, from the first seed whose row maxima are clear of a switch."""
    if ("swiglu", T, ffn, fmt) not in _cache:
        for seed in range(7 * ffn + T, 7 * ffn + T + 8):
            rng = np.random.default_rng(seed)
            gate = rng.uniform(-12.0, 12.0, size=(T, ffn))
            gate[:, 0], gate[:, 1] = -12.0, 12.0                       # both tails of the sigmoid in every row
            up = rng.standard_normal((T, ffn)) * rng.uniform(0.05, 20.0, size=(T, 1))
            gu = np.concatenate([gate, up], axis=1).astype(np.float32)
            gu[2] = 0.0
            gu = torch.from_numpy(gu).to(HALF[fmt])
            h = R.swiglu(gu.to(torch.float64).numpy())
            amax = np.abs(h).max(axis=1)
            if (F.switch_margin(amax)[amax > 0] > 2.0 ** -19).all():
                _cache[("swiglu", T, ffn, fmt)] = (gu, h, seed)
                break
    return _cache[("swiglu", T, ffn, fmt)]


def test_seeds_keep_every_row_maximum_clear_of_a_scale_switch():
    """CPU: every case finds its seed (the first one tried, but for chance), so the scale assertions below are decidable."""
    for T, d in RMS_SHAPES:
        assert rms_case(T, d)[4] - (100 * d + T) < 8
    for T, ffn in SWIGLU_SHAPES:
        for fmt in HALF:
            gu, h, seed = swiglu_case(T, ffn, fmt)
            assert seed - (7 * ffn + T) < 8
            assert (h[2] == 0).all() and np.abs(gu[:, :ffn].to(torch.float64).numpy()).max() == 12.0


def check_codes(name, codes, scale, ref, band):
    """codes uint8 [T, n], scale fp32 [T] from the device; ref float64 [T, n]; band float64, broadcastable: |value - ref| <= band."""
    want_scale = F.pow2_scale(np.abs(ref).max(axis=1))
    assert np.array_equal(scale.astype(np.float64), want_scale), f"{name}: row scales differ from the rule on the float64 row maximum"
    r = ref / want_scale[:, None]
    b = band / want_scale[:, None]
    want = O.fp8_e4m3fn_encode(r.astype(np.float32))
    lo = O.fp8_e4m3fn_decode(O.fp8_e4m3fn_encode((r - b).astype(np.float32)))
    hi = O.fp8_e4m3fn_decode(O.fp8_e4m3fn_encode((r + b).astype(np.float32)))
    dec = O.fp8_e4m3fn_decode(codes)
    assert ((dec >= lo) & (dec <= hi)).all(), f"{name}: an e4m3 code outside the rounding of reference +- bound"
    differ = (dec != O.fp8_e4m3fn_decode(want))                  # (+0 and -0 are one value)
    share = float(differ.mean())
    print(f"{name}: codes that differ from the plain encoding of the reference: {share:.2e} (at most {SHARE:g})")
    assert share <= SHARE, name
    assert np.abs(dec).max() <= 448.0 and (np.abs(dec).max(axis=1)[want_scale != 1.0] >= 224.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,d", RMS_SHAPES)
def test_rmsnorm_fp8_vs_float64(ctx, T, d):
    x, g, ref, b, _ = rms_case(T, d)
    codes, scale = ctx.rmsnorm_fp8(dev(x), dev(g), 1e-5)
    torch.cuda.synchronize()
    assert codes.shape == (T, d) and scale.shape == (T,)
    check_codes(f"rmsnorm_fp8 T={T} d={d}", codes.cpu().numpy(), scale.cpu().numpy(), ref, b[:, None])
    # rows past T are not written
    lib, h = ctx.lib, ctx.handle
    big = torch.full((T + 2, d), SENTINEL, dtype=torch.uint8, device="cuda:0")
    sc = torch.full((T + 2,), -1.0, device="cuda:0")
    xd, gd = dev(x), dev(g)
    assert lib.sgpt_rmsnorm_fp8(h, xd.data_ptr(), gd.data_ptr(), T, d, 1e-5, big.data_ptr(), sc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:T], codes) and (big[T:] == SENTINEL).all() and (sc[T:] == -1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("T,ffn", SWIGLU_SHAPES)
def test_swiglu_fp8_vs_float64(ctx, T, ffn, fmt):
    from sgpt_amd import _lib
    gu, h, _ = swiglu_case(T, ffn, fmt)
    lib, hd = ctx.lib, ctx.handle
    gd = gu.to("cuda:0")
    big = torch.full((T + 2, ffn), SENTINEL, dtype=torch.uint8, device="cuda:0")
    sc = torch.full((T + 2,), -1.0, device="cuda:0")
    assert lib.sgpt_swiglu_fp8(hd, gd.data_ptr(), _lib.SGPT_BF16 if fmt == "bf16" else _lib.SGPT_F16, T, ffn, big.data_ptr(), sc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (big[T:] == SENTINEL).all() and (sc[T:] == -1.0).all(), "rows past T were written"
    codes, scale = big[:T].cpu().numpy(), sc[:T].cpu().numpy()
    assert scale[2] == 1.0 and (codes[2] & 0x7F == 0).all(), "a row of zeros: scale 1, zero codes"
    check_codes(f"swiglu_fp8 {fmt} T={T} ffn={ffn}", codes, scale, h, np.abs(h) * 2.0 ** -20)
    c2, s2 = ctx.swiglu_fp8(gd)
    assert torch.equal(c2, big[:T]) and torch.equal(s2, sc[:T])


@pytest.mark.gpu
def test_argument_refusals(ctx):
    from sgpt_amd import _lib
    lib, h = ctx.lib, ctx.handle
    BF16, F32 = _lib.SGPT_BF16, _lib.SGPT_F32
    x = torch.zeros((8, 8192), device="cuda:0")
    g = torch.ones(8192, device="cuda:0")
    q = torch.full((8, 8192), SENTINEL, dtype=torch.uint8, device="cuda:0")
    s = torch.full((8,), -1.0, device="cuda:0")

    def err():
        return (lib.sgpt_last_error(h) or b"").decode()
    for d in (130, 8192, 0):
        assert lib.sgpt_rmsnorm_fp8(h, x.data_ptr(), g.data_ptr(), 8, d, 1e-5, q.data_ptr(), s.data_ptr(), None) == -1
        assert err() == "sgpt_rmsnorm_fp8: bad arguments (d % 4 == 0, d <= 4096)"
    assert lib.sgpt_rmsnorm_fp8(h, x.data_ptr(), g.data_ptr(), 8, 128, 1e-5, None, s.data_ptr(), None) == -1
    assert lib.sgpt_rmsnorm_fp8(h, x.data_ptr() + 4, g.data_ptr(), 8, 128, 1e-5, q.data_ptr(), s.data_ptr(), None) == -1
    assert err() == "sgpt_rmsnorm_fp8: 16-byte aligned x / gamma, 4-byte aligned codes / row_scale"
    gu = torch.zeros((8, 1024), dtype=torch.bfloat16, device="cuda:0")
    assert lib.sgpt_swiglu_fp8(h, gu.data_ptr(), BF16, 8, 504, q.data_ptr(), s.data_ptr(), None) == -1               # ffn % 16
    assert err() == "sgpt_swiglu_fp8: ffn % 16; 16-byte aligned gu / codes; codes is a buffer of its own"
    assert lib.sgpt_swiglu_fp8(h, gu.data_ptr() + 8, BF16, 4, 512, q.data_ptr(), s.data_ptr(), None) == -1
    assert lib.sgpt_swiglu_fp8(h, gu.data_ptr(), BF16, 8, 512, gu.data_ptr(), s.data_ptr(), None) == -1
    assert lib.sgpt_swiglu_fp8(h, gu.data_ptr(), F32, 8, 256, q.data_ptr(), s.data_ptr(), None) == -1                # fp32 input
    assert err() == "sgpt_swiglu_fp8: dtype SGPT_BF16 | SGPT_F16"
    assert lib.sgpt_swiglu_fp8(h, gu.data_ptr(), BF16, 0, 512, q.data_ptr(), s.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (q == SENTINEL).all() and (s == -1.0).all(), "a refused call wrote"
