"""-m gpu: the encoder's row kernels (csrc/elementwise.hip: embed, layernorm, layernorm_split, lnf_pool, rope, logprob_rows),
each launched alone through its C-ABI entry and compared with the float64 restatement of the same operation on the same
inputs (tests/rowops_ref.py, pinned on the CPU by tests/test_rowops_ref.py).  Inputs are fp32 (or 16-bit) tensors whose exact
values go to float64; every bound is the rounding of the number formats along the kernel's own chain of operations, stated
where it is used, and every case prints its worst `error / bound` ("rowops:" lines, visible with -s / -rA).

What the whole-model parities cannot see and these can: the NV dispatch of launch_layernorm at widths that are not a multiple
of 256 or sit below their NV (masked lanes), the f16 range shift and the [hi | lo | hi] layout, single rows of the ln_f + pool
loop (stride, tail guard, t_lo, pad_left, the learntmean clamp, rows that must not be read, the non-finite flag), the
pass-through columns of the rotary embedding, real vocabulary sizes and the first-maximum rule of the log-prob kernel, and the
index clamps of ids / pos / targets -- those without ever indexing outside an allocation."""
import numpy as np
import pytest
import torch

import rowops_ref as R

pytestmark = pytest.mark.gpu

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
PBITS = {"bf16": 8, "f16": 11}                     # significand bits of the 16-bit formats
EPS = 1e-5


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def host64(t) -> np.ndarray:
    """Exact float64 values of a device tensor of any float format."""
    return t.detach().to("cpu", torch.float64).numpy()


def report(what, ratio):
    print(f"rowops: {what}: worst error / bound = {ratio:.3f}")
    return ratio


# ============================================================================================================== LayerNorm
SENTINEL = 77.0


def ln_setup(T, d, family):
    x, g, b = R.ln_inputs(T, d, family, seed=1000 * d + T)
    ref, mean, rstd = R.layernorm(x, g, b, EPS, stats=True)
    unit = R.layernorm_unit(x, g, ref, mean, rstd)[:, None]
    return dev(x), dev(g), dev(b), ref, unit


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("T", [1, 5, 1027])
@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_every_width_fp32_and_16bit(ctx, d, T, family):
    """fp32: |got - ref| <= 4 B per row, B = 2^-23 [(|mean| + max|x|) rstd max|gamma| + max|ref|] (rowops_ref.layernorm_unit; two
    independent fp32 implementations reach 0.98 B on the CPU over these widths and families, the factor 4 covers the device's
    butterfly order).  16-bit: |got - mul ref| <= ulp16(mul ref) / 2 + 4 B mul -- one correct rounding of an fp32 value that is
    itself inside the fp32 bound; truncation or a missed shift is outside it.  Rows past T of a larger output keep their
    sentinel; in place (fp32) gives the bits of out of place."""
    x, g, b, ref, unit = ln_setup(T, d, family)
    out = torch.full((T + 3, d), SENTINEL, dtype=torch.float32, device="cuda:0")
    ctx.layernorm(x, g, b, EPS, out=out)
    assert (out[T:] == SENTINEL).all(), "rows past T were written"
    r = report(f"layernorm fp32 d={d} T={T} {family}", float((np.abs(host64(out[:T]) - ref) / unit).max()))
    assert r <= 4.0
    xin = x.clone()
    ctx.layernorm(xin, g, b, EPS, out=xin)
    assert torch.equal(xin, out[:T]), "in place differs from out of place"
    for fmt, mul in (("bf16", 1.0), ("f16", 1.0), ("f16", 2.0 ** -3)):
        o16 = torch.full((T + 3, d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx.layernorm(x, g, b, EPS, out_dtype=HALF[fmt], out_mul=mul, out=o16)
        assert (o16[T:] == SENTINEL).all(), "rows past T were written"
        bound = 0.5 * R.ulp16(mul * ref, fmt) + 4.0 * unit * mul
        r = report(f"layernorm {fmt} mul={mul} d={d} T={T} {family}", float((np.abs(host64(o16[:T]) - mul * ref) / bound).max()))
        assert r <= 1.0


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("T", [1, 5, 1027])
@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_split_layout(ctx, d, T, family):
    """[hi | lo | hi]: block 0 = the bits of the non-split kernel, block 2 = block 0, and hi + lo (float64) within
    4 B mul + 2^-2p |mul ref| of the reference (p = 11 f16, 8 bf16: lo = round16(v - hi) with |v - hi| <= 2^-p |v|); f16 adds
    2^-25, half its subnormal spacing, which the rounding of a lo below 2^-14 costs whatever |v| is."""
    x, g, b, ref, unit = ln_setup(T, d, family)
    for fmt, mul in (("bf16", 1.0), ("f16", 1.0), ("f16", 2.0 ** -3)):
        plain = ctx.layernorm(x, g, b, EPS, out_dtype=HALF[fmt], out_mul=mul)
        o3 = torch.full((T + 3, 3 * d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx.layernorm(x, g, b, EPS, out_dtype=HALF[fmt], out_mul=mul, split=True, out=o3)
        assert (o3[T:] == SENTINEL).all(), "rows past T were written"
        hi, lo, hi2 = o3[:T, :d], o3[:T, d:2 * d], o3[:T, 2 * d:]
        assert torch.equal(hi.contiguous().view(torch.int16), plain.view(torch.int16)), "block 0 is not the non-split output"
        assert torch.equal(hi2.contiguous().view(torch.int16), hi.contiguous().view(torch.int16)), "block 2 is not block 0"
        bound = 4.0 * unit * mul + 2.0 ** (-2 * PBITS[fmt]) * np.abs(mul * ref) + (2.0 ** -25 if fmt == "f16" else 0.0)
        r = report(f"layernorm_split {fmt} mul={mul} d={d} T={T} {family}",
                   float((np.abs(host64(hi) + host64(lo) - mul * ref) / bound).max()))
        assert r <= 1.0


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [512, 768, 1024])
def test_layernorm_prologue_of_the_query_projection_gives_the_standalone_bits(ctx, d, fmt):
    """csrc/rowln.h: "a LayerNorm that runs inside a projection's prologue produces the bits of the stand-alone kernel" --
    linear_query(x, ln) against linear_query(a = layernorm(x -> 16 bit)), the qkv and the gelu epilogue, bit for bit."""
    M = 96
    x, g, b, _, _ = ln_setup(M, d, "plain")
    gen = torch.Generator(device="cuda:0").manual_seed(d)
    a = ctx.layernorm(x, g, b, EPS, out_dtype=HALF[fmt])
    w = (torch.randn((3 * d, d), generator=gen, device="cuda:0") * d ** -0.5).to(HALF[fmt])
    qk, vt = ctx.linear_query(w, x=x, ln=(g, b, EPS), epi="qkv", n_split=2 * d)
    qk2, vt2 = ctx.linear_query(w, a=a, epi="qkv", n_split=2 * d)
    assert torch.isfinite(qk.float()).all() and float(qk.float().abs().max()) > 0.1
    assert torch.equal(qk.view(torch.int16), qk2.view(torch.int16)) and torch.equal(vt.view(torch.int16), vt2.view(torch.int16))
    w = (torch.randn((4 * d, d), generator=gen, device="cuda:0") * d ** -0.5).to(HALF[fmt])
    bias = torch.randn((4 * d,), generator=gen, device="cuda:0") * 0.3
    h = ctx.linear_query(w, x=x, ln=(g, b, EPS), bias=bias, epi="gelu")
    h2 = ctx.linear_query(w, a=a, bias=bias, epi="gelu")
    assert float(h.float().abs().max()) > 0.1 and torch.equal(h.view(torch.int16), h2.view(torch.int16))


DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 3}          # element-type codes of include/sgpt_hip.h


def bits16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_writeback_rmsnorm_and_fp8_stores_every_width(ctx, d):
    """The three store loops the tests above do not reach, at every NV rung with its masked tail, T = 5: one full workgroup of
    four rows and one row of the next, whose other three waves leave at the row guard.  Every output has T + 3 rows of sentinel.
    Write-back: x becomes the bits of the fp32 LayerNorm and the 16-bit copy is x rounded once.  RMSNorm: the bars of
    tests/test_gpu_llama.py::test_rmsnorm_vs_float64 -- fp32 within 4 B of float64 (rms_setup's unit), in place = out of place,
    16 bit = the fp32 output rounded once, range word 0.  Quantising LayerNorm against y = the fp32 LayerNorm of the same inputs
    (csrc/rowln.h: the same loads, reductions and arithmetic, so the bits the fp8 kernel holds): the scale is the power of two with
    224 < max|y| / scale <= 448 (csrc/rowln.h::fp8_pow2_scale: m 2^e -> 256 m for m <= 1.75, else 128 m), and every code is one
    round-to-nearest of the exactly scaled y / scale to e4m3 -- |decode(code) scale - y| <= scale / 2 * max(2^(floor(log2 |y / scale|) - 3),
    2^-9), half a spacing of the format at that value (2^-9 below its normal range); nothing saturates since |y / scale| <= 448."""
    from test_gpu_llama import rms_setup
    T = 5
    x, g, b, _, _ = ln_setup(T, d, "plain")
    y = ctx.layernorm(x, g, b, EPS)
    p = lambda t: t.data_ptr()                                                                  # noqa: E731
    for fmt in ("f16", "bf16"):
        xin = torch.full((T + 3, d), SENTINEL, dtype=torch.float32, device="cuda:0")
        xin[:T] = x
        o16 = torch.full((T + 3, d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx._chk(ctx.lib.sgpt_layernorm_writeback(ctx.handle, p(xin), p(g), p(b), T, d, EPS, p(o16), DT[HALF[fmt]], None), "writeback")
        assert (xin[T:] == SENTINEL).all() and (o16[T:] == SENTINEL).all(), "rows past T were written"
        assert torch.equal(xin[:T].view(torch.int32), y.view(torch.int32)), f"write-back {fmt}: x is not the fp32 LayerNorm"
        assert torch.equal(bits16(o16[:T]), bits16(xin[:T].to(HALF[fmt]))), f"write-back {fmt}: the 16-bit copy is not x rounded once"

    xr, gr, ref, unit = rms_setup(T, d)
    xr, gr = dev(xr), dev(gr)
    ctx.range_check()
    out = torch.full((T + 3, d), SENTINEL, dtype=torch.float32, device="cuda:0")
    ctx.rmsnorm(xr, gr, 1e-5, out=out)
    assert (out[T:] == SENTINEL).all(), "rows past T were written"
    assert report(f"rmsnorm fp32 d={d} T={T}", float((np.abs(host64(out[:T]) - ref) / unit).max())) <= 4.0
    xin = xr.clone()
    ctx.rmsnorm(xin, gr, 1e-5, out=xin)
    assert torch.equal(xin, out[:T]), "in place differs from out of place"
    for fmt in ("f16", "bf16"):
        o16 = torch.full((T + 3, d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
        ctx.rmsnorm(xr, gr, 1e-5, out_dtype=HALF[fmt], out=o16)
        assert (o16[T:] == SENTINEL).all(), "rows past T were written"
        assert torch.equal(bits16(o16[:T]), bits16(out[:T].to(HALF[fmt]))), f"rmsnorm {fmt} is not the fp32 output rounded once"
    assert ctx.range_check() == 0

    codes = torch.full((T + 3, d), 0x55, dtype=torch.uint8, device="cuda:0")
    scale = torch.full((T + 3,), SENTINEL, dtype=torch.float32, device="cuda:0")
    ctx._chk(ctx.lib.sgpt_layernorm_fp8(ctx.handle, p(x), p(g), p(b), T, d, EPS, p(codes), p(scale), None), "layernorm_fp8")
    assert (codes[T:] == 0x55).all() and (scale[T:] == SENTINEL).all(), "rows past T were written"
    y64, sc = host64(y), host64(scale[:T])[:, None]
    assert (np.frexp(sc)[0] == 0.5).all(), "a row scale is not a power of two"
    top = np.abs(y64).max(axis=1, keepdims=True) / sc
    print(f"rowops: layernorm_fp8 d={d}: max|y| / scale in [{top.min():.2f}, {top.max():.2f}]")
    assert ((top > 224) & (top <= 448)).all(), "not the smallest power-of-two scale that keeps the row inside e4m3"
    v = np.abs(y64) / sc
    spacing = np.maximum(np.ldexp(1.0, np.frexp(v)[1] - 1 - 3), 2.0 ** -9)      # frexp: v = m 2^e, 1/2 <= m < 1 -> floor(log2 v) = e - 1
    err = np.abs(host64(codes[:T].view(torch.float8_e4m3fn).float()) * sc - y64) / (0.5 * sc * spacing)
    over = int((err > 1.0).sum())
    assert report(f"layernorm_fp8 d={d} T={T} ({over} elements over)", float(err.max())) <= 1.0


# ============================================================================================================ ln_f + pool
POOL_LENS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 127, 128, 300, 2048]
POOL_PAD = [0, 3, 0, 1, 0, 7, 0, 0, 12, 0, 5, 0, 40, 0]


def pool_layout():
    from sgpt_amd.model import pack_host
    pk = pack_host([[1] * n for n in POOL_LENS], pad_left=POOL_PAD)
    off, ln, pl = (np.array(pk[k], dtype=np.int64) for k in ("seq_off", "seq_len", "pad_left"))
    assert ln.tolist() == POOL_LENS and pl.tolist() == POOL_PAD and pk["max_pos"] == max(n + p for n, p in zip(POOL_LENS, POOL_PAD)) - 1
    real = np.zeros(pk["T_pad"], dtype=bool)
    for s0, n in zip(off.tolist(), ln.tolist()):
        real[s0:s0 + n] = True
    assert (~real).sum() > 0, "the layout has no filler rows"
    return pk, off[:-1], ln, pl, real


def pool_rows(d, real, seed):
    """fp32 [T_pad, d]: 2 randn + 0.3 on the real rows, NaN on every filler row (beyond len, between sequences, the tail)."""
    rng = np.random.default_rng(seed)
    x = np.full((real.shape[0], d), np.nan, dtype=np.float32)
    x[real] = rng.standard_normal((int(real.sum()), d), dtype=np.float32) * np.float32(2.0) + np.float32(0.3)
    return x


@pytest.mark.parametrize("mode", ["weightedmean", "mean", "lasttoken", "learntmean", "learntmean-short"])
@pytest.mark.parametrize("d", [64, 768, 1280, 2560, 4096])
def test_lnf_pool_packed_layout(ctx, d, mode):
    """Lengths 1 .. 2048 around the kernel's 4-wave x LPB batches (LPB = 4 up to d = 1024, 2 above), pad_left on some, NaN in
    every row the kernel must not read.  Per element: 2^-23 (ceil(len / 4) + 4) sum_t w_t |h_t| / den -- the recursive-summation
    bound of one wave's chain plus the four-way combine -- plus the den-weighted mean of the rows' 4 B with the LayerNorm, all
    over the norm and plus 2^-22 |out| when normalised (rowops_ref.lnf_pool).  learntmean: a table exactly max_pos + 1 long, and
    one 37 shorter whose last weight the clamp repeats."""
    pk, off, ln, pl, real = pool_layout()
    x = pool_rows(d, real, seed=d)
    rng = np.random.default_rng(d + 1)
    g = (1.0 + 0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d, dtype=np.float32)).astype(np.float32)
    pw, kmode = None, mode
    if mode.startswith("learntmean"):
        pw = rng.uniform(0.5, 1.5, pk["max_pos"] + 1 - (37 if mode.endswith("short") else 0)).astype(np.float32)
        kmode = "learntmean"
    xd, so, sl, pd = dev(x), dev(pk["seq_off"]), dev(pk["seq_len"]), dev(pk["pad_left"])
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    worst = 0.0
    for apply_ln in (False, True):
        for nrm in (False, True):
            lnp = (g, b, EPS) if apply_ln else None
            got = ctx.lnf_pool(xd, so, sl, pd, ln=None if lnp is None else (dev(g), dev(b), EPS), mode=kmode, normalize=nrm,
                               position_weights=None if pw is None else dev(pw), nonfinite_flag=flag)
            ref, bound = R.lnf_pool(x, off, ln, pl, kmode, ln=lnp, normalize=nrm, pos_weights=pw, bound=True)
            got64 = host64(got)
            assert np.isfinite(got64).all(), "a filler row leaked into the pooled embeddings"
            ratio = np.abs(got64 - ref) / bound
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"apply_ln={apply_ln} normalize={nrm}: sequence of length {POOL_LENS[int(ratio.max(axis=1).argmax())]}"
            if kmode == "lasttoken" and not apply_ln and not nrm:
                assert torch.equal(got, xd[dev(off + ln - 1)]), "lasttoken without ln_f is a copy of row len - 1"
    assert int(flag.item()) == 0, "nonfinite_flag raised on finite rows"
    report(f"lnf_pool d={d} {mode}", worst)


@pytest.mark.parametrize("d", [64, 1280])
def test_lnf_pool_empty_sequence_and_nonfinite_flag(ctx, d):
    """seq_len = 0 gives a zero row in every mode; the flag word is raised by +inf and by NaN in a real row, and by nothing else."""
    rng = np.random.default_rng(d)
    x = np.full((16, d), np.nan, dtype=np.float32)
    off, ln, pl = np.array([0, 6, 6], np.int32), np.array([5, 0, 7], np.int32), np.array([2, 9, 0], np.int32)
    x[0:5] = rng.standard_normal((5, d), dtype=np.float32)
    x[6:13] = rng.standard_normal((7, d), dtype=np.float32)
    g, b = dev(np.ones(d, np.float32)), dev(np.zeros(d, np.float32))
    pw = dev(rng.uniform(0.5, 1.5, 16).astype(np.float32))
    flag = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    for mode in R.POOL_MODES:
        for lnp in (None, (g, b, EPS)):
            for nrm in (False, True):
                got = ctx.lnf_pool(dev(x), dev(off), dev(ln), dev(pl), ln=lnp, mode=mode, normalize=nrm, position_weights=pw, nonfinite_flag=flag)
                assert (got[1] == 0).all() and torch.isfinite(got).all() and float(got[0].abs().max()) > 0, (mode, nrm)
    assert int(flag.item()) == 0
    for bad in (np.inf, np.nan):
        for lnp in (None, (g, b, EPS)):
            y = x.copy()
            y[8, d // 2] = bad
            flag.zero_()
            got = ctx.lnf_pool(dev(y), dev(off), dev(ln), dev(pl), ln=lnp, mode="mean", nonfinite_flag=flag)
            assert int(flag.item()) == 1, f"{bad} in a real row did not raise the flag"
            assert torch.isfinite(got[0]).all() and not torch.isfinite(got[2]).all()
    # without a flag word the same call is accepted
    ctx.lnf_pool(dev(x), dev(off), dev(ln), dev(pl), mode="mean")


# =================================================================================================================== RoPE
ROPE_SHAPES = [(2, 256, 64), (16, 256, 64), (12, 64, 64), (4, 128, 32)]
ROPE_T, ROPE_MAXPOS = 37, 2048


def rope_tables(rot):
    from sgpt_amd.model import rotary_tables
    return rotary_tables(ROPE_MAXPOS, rot)


def rope_positions(T, seed):
    pos = np.random.default_rng(seed).integers(0, ROPE_MAXPOS, T).astype(np.int32)
    pos[[0, 3, T - 1]] = [ROPE_MAXPOS - 1, 0, 0]                      # non-monotone; the last table row, and 0 twice
    return pos


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H,dh,rot", ROPE_SHAPES)
def test_rope_both_layouts(ctx, H, dh, rot, dt):
    """The two layouts of the encoder: fp32 [q | k | v] rows (ld = 3 dm, k_off = dm), 16-bit [q | k] rows (ld = 2 dm).  Reference:
    the same fp32 table values and the buffer's exact values in float64.  Per pair 2^-22 (|x0| + |x1|) -- two products and a sum
    in fp32 -- plus ulp16(ref) / 2 for a 16-bit buffer.  Untouched, bit for bit: columns >= rot of every head, the V block, the
    row after T, and every row at position 0.  T H rot / 2 is no multiple of the 256-thread block except at H rot / 2 = 512
    (16 heads), where no T can make it one."""
    dm, T = H * dh, ROPE_T
    assert (T * H * rot // 2) % 256 != 0 or (H * rot // 2) % 256 == 0
    ld = 3 * dm if dt == "f32" else 2 * dm
    tdt = torch.float32 if dt == "f32" else HALF[dt]
    sin, cos = rope_tables(rot)
    pos = rope_positions(T, seed=H + dh)
    gen = torch.Generator(device="cuda:0").manual_seed(H * dh + rot)
    buf = (torch.randn((T + 1, ld), generator=gen, device="cuda:0") * 2.0).to(tdt)
    before = buf.clone()
    ctx.rope(buf, dev(pos), dev(sin), dev(cos), H, dh, rot, k_off=dm, T=T)
    x = host64(before)
    ref = R.rope(x, pos, sin, cos, H, dh, rot, k_off=dm, T=T)
    touched = np.zeros((T + 1, ld), dtype=bool)
    pair = np.zeros((T + 1, ld))
    for base in (0, dm):
        for h in range(H):
            c0 = base + h * dh
            touched[:T, c0:c0 + rot] = True
            s = np.abs(x[:T, c0:c0 + rot:2]) + np.abs(x[:T, c0 + 1:c0 + rot:2])
            pair[:T, c0:c0 + rot:2] = s
            pair[:T, c0 + 1:c0 + rot:2] = s
    ibits = torch.int32 if dt == "f32" else torch.int16
    same = (buf.view(ibits) == before.view(ibits)).cpu().numpy()
    assert same[~touched].all(), "a pass-through column, the V block or the row after T changed"
    assert same[np.flatnonzero(pos == 0)].all(), "position 0 is the identity"
    assert not same[0, :rot].all(), "the rotation did not run"
    bound = 2.0 ** -22 * pair + (0.0 if dt == "f32" else 0.5 * R.ulp16(ref, dt))
    err = np.abs(host64(buf) - ref)
    assert report(f"rope {dt} H={H} dh={dh} rot={rot}", float((err[touched] / bound[touched]).max())) <= 1.0


# ================================================================================================================== embed
@pytest.mark.parametrize("T", [1, 6, 1027])
@pytest.mark.parametrize("d", [64, 772, 4096])
def test_embed_is_the_fp32_sum(ctx, d, T):
    rng = np.random.default_rng(d + T)
    vocab, max_pos = 300, 1100
    wte = rng.standard_normal((vocab, d), dtype=np.float32)
    wpe = rng.standard_normal((max_pos, d), dtype=np.float32) * np.float32(0.37)
    ids, pos = rng.integers(0, vocab, T).astype(np.int32), rng.integers(0, max_pos, T).astype(np.int32)
    ids[0], pos[0] = vocab - 1, max_pos - 1
    ids[-1], pos[-1] = (0, 0) if T > 1 else (ids[-1], pos[-1])
    out = torch.full((T + 2, d), SENTINEL, dtype=torch.float32, device="cuda:0")
    ctx.embed(dev(ids), dev(pos), dev(wte), dev(wpe), out=out)
    assert (out[T:] == SENTINEL).all()
    assert np.array_equal(out[:T].cpu().numpy(), wte[ids] + wpe[pos]), "not the fp32 sum wte[id] + wpe[pos]"
    assert np.array_equal(out[:T].cpu().numpy(), R.embed(ids, pos, wte, wpe).astype(np.float32))
    got = ctx.embed(dev(ids), None, dev(wte))
    assert np.array_equal(got.cpu().numpy(), wte[ids]), "without a position table the token rows come through as they are"


# ========================================================================================================== log-prob rows
def logprob_rows_case(V, rng):
    """Rows [kinds, V] fp32 and their targets: the row kinds of the issue, each where V leaves room for it."""
    rows, tg, kinds = [], [], []

    def add(kind, r, t):
        rows.append(r.astype(np.float32)), tg.append(int(t)), kinds.append(kind)
    rnd = lambda: rng.standard_normal(V, dtype=np.float32) * np.float32(3.0)   # noqa: E731
    add("random", rnd(), rng.integers(0, V))
    add("random-2", rnd(), V - 1)
    add("all-equal", np.full(V, 1.25, np.float32), rng.integers(0, V))
    dup = [i for i in (3, 3 + 64, 3 + 256, 3 + 256 * 7, 3 + 256 * 100 + 64) if i < V] or [0]
    r = rnd()
    r[dup] = 30.0                                                              # the same maximum in other lanes, waves, strides
    add("dup-max", r, dup[-1])
    r = rnd()
    r[0] = 25.0
    add("max-at-0", r, V // 2)
    r = rnd()
    r[V - 1] = 25.0
    add("max-at-end", r, 0)
    r = rnd()
    r[V // 3] = 60.0
    add("dominant", r, V // 3)
    add("dominant-other", r.copy(), (V // 3 + 1) % V)
    r = rnd()
    t = int(rng.integers(0, V))
    ninf = [i for i in rng.integers(0, V, 40).tolist() + [0, V - 1] if i != t]
    if V > 1:
        r[ninf] = -np.inf
    add("neg-inf", r, t)
    add("shifted", rnd() + np.float32(1e4), rng.integers(0, V))
    return np.stack(rows), np.array(tg, dtype=np.int32), kinds


@pytest.mark.parametrize("V", [1, 211, 255, 256, 257, 50257, 250880])
def test_logprob_rows_vocabularies_and_first_maximum(ctx, V):
    """log_softmax gathered at the target, and the greedy token, against float64 on the same fp32 logits: 2^-22 (V / 256 + 16) +
    2^-23 |x_t - max| -- a thread's chain of V / 256 exp terms and the tree above it, expf and logf to a few ulp, and the
    rounding of x_t - max.  The two real vocabularies sit in rows padded to a multiple of 256 with NaN behind column V.  Greedy
    is the FIRST maximum wherever it is duplicated; +1e4 on every logit changes nothing (its reference: the shifted fp32 inputs)."""
    rng = np.random.default_rng(V)
    x, tg, kinds = logprob_rows_case(V, rng)
    ld = (V + 255) // 256 * 256 if V > 1000 else V
    xp = np.full((x.shape[0], ld), np.nan, dtype=np.float32)
    xp[:, :V] = x
    lp, am = ctx.logprob_rows(dev(xp), dev(tg), V=V)
    ref, ref_am = R.logprob_rows(x, V, tg)
    got = host64(lp)
    assert np.isfinite(got).all(), "a padding column leaked, or a row overflowed"
    mx = x.astype(np.float64).max(axis=1)
    bound = 2.0 ** -22 * (V / 256 + 16) + 2.0 ** -23 * np.abs(x[np.arange(len(tg)), tg].astype(np.float64) - mx)
    ratio = np.abs(got - ref) / bound
    assert np.array_equal(am.cpu().numpy(), ref_am), [k for k, a, r in zip(kinds, am.cpu().tolist(), ref_am.tolist()) if a != r]
    assert abs(got[kinds.index("all-equal")] + np.log(V)) <= bound[kinds.index("all-equal")] and am[kinds.index("all-equal")] == 0
    if V > 3 + 64:
        assert int(am[kinds.index("dup-max")]) == 3, "greedy is the lowest index of a duplicated maximum"
    assert report(f"logprob_rows V={V}", float(ratio.max())) <= 1.0, kinds[int(ratio.argmax())]
    lp2, none = ctx.logprob_rows(dev(xp), dev(tg), V=V, greedy=False)          # out_greedy = NULL
    assert none is None and torch.equal(lp2, lp)


# =========================================================================================================== index clamps
def test_index_clamps_stay_inside_the_declared_tables(ctx):
    """ids / pos / targets outside [0, declared) give the result of the nearest valid index.  Every table is a view that starts
    8 rows into a larger tensor and has rows behind it, all holding different data: an unclamped read is a visible mismatch,
    and never leaves the allocation."""
    rng = np.random.default_rng(11)
    d, vocab, max_pos, T = 64, 10, 12, 8
    big_e, big_p = dev(rng.standard_normal((8 + 24 + 8, d), dtype=np.float32)), dev(rng.standard_normal((8 + 24 + 8, d), dtype=np.float32))
    wte, wpe = big_e[8:32], big_p[8:32]                                        # 24 rows allocated, 10 / 12 declared
    ids = np.array([0, 9, 10, 23, -1, 5, 17, -7], np.int32)
    pos = np.array([11, 12, -1, 3, 23, 0, 15, -3], np.int32)
    want = (wte[dev(np.clip(ids, 0, vocab - 1)).long()] + wpe[dev(np.clip(pos, 0, max_pos - 1)).long()])
    assert torch.equal(ctx.embed(dev(ids), dev(pos), wte, wpe, vocab=vocab, max_pos=max_pos), want)
    assert torch.equal(ctx.embed(dev(ids), None, wte, vocab=vocab), wte[dev(np.clip(ids, 0, vocab - 1)).long()])

    H, dh, rot, mp = 2, 64, 32, 20
    dm = H * dh
    from sgpt_amd.model import rotary_tables
    sin, cos = rotary_tables(8 + 40 + 8, rot)
    sin_v, cos_v = dev(sin)[8:48], dev(cos)[8:48]                              # the view's row r is angle row 8 + r
    pos = np.array([0, 19, 20, 39, -1, -8, 7, 25], np.int32)
    buf = dev(rng.standard_normal((T, 2 * dm), dtype=np.float32))
    before = host64(buf)
    ctx.rope(buf, dev(pos), sin_v, cos_v, H, dh, rot, k_off=dm, max_pos=mp)
    ref = R.rope(before, np.clip(pos, 0, mp - 1), sin[8:48], cos[8:48], H, dh, rot, k_off=dm)
    tol = 2.0 ** -22 * 2 * np.abs(before).max()
    assert np.abs(host64(buf) - ref).max() <= tol
    wrong = R.rope(before, pos + 8, sin, cos, H, dh, rot, k_off=dm)           # what an unclamped read gives: rows of the larger tensor
    assert np.abs(wrong - ref).max() > 1000 * tol

    V, ld, n = 200, 256, 6
    big_l = dev(rng.standard_normal((8 + n + 8, ld), dtype=np.float32) * np.float32(3.0))
    logits = big_l[8:8 + n]
    tg = np.array([0, 199, 200, 255, -1, -300], np.int32)
    lp, _ = ctx.logprob_rows(logits, dev(tg), V=V)
    ref, _ = R.logprob_rows(logits.cpu().numpy(), V, np.clip(tg, 0, V - 1))
    assert np.abs(host64(lp) - ref).max() <= 2.0 ** -22 * 17 + 2.0 ** -23 * 30


# ============================================================================================================== refusals
def test_entries_refuse_bad_arguments_before_launching(ctx):
    """One bad argument per call -> SGPT_ERR_INVALID (ValueError), and the output still holds its sentinel."""
    L, h, s = ctx.lib, ctx.handle, None
    f32 = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")     # noqa: E731
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda:0")                        # noqa: E731
    x, g, b, out = f32(4, 64), f32(64), f32(64), f32(4, 64)
    x6, g6, out6 = f32(4, 66), f32(66), f32(4, 66)
    o16 = torch.full((4, 3 * 64), SENTINEL, dtype=torch.float16, device="cuda:0")
    wide = f32(2, 4100)
    ids, pos, off, ln = i32(0, 1, 2, 3), i32(0, 1, 2, 3), i32(0, 2), i32(2, 2)
    sin, cos = f32(8, 16), f32(8, 16)
    p = lambda t: None if t is None else t.data_ptr()                                           # noqa: E731
    bad = {
        "embed d % 4": lambda: L.sgpt_embed(h, p(ids), p(pos), p(x6), p(x6), 4, 66, 4, 4, p(out6), s),
        "embed null ids": lambda: L.sgpt_embed(h, None, p(pos), p(x), p(x), 4, 64, 4, 4, p(out), s),
        "embed null out": lambda: L.sgpt_embed(h, p(ids), p(pos), p(x), p(x), 4, 64, 4, 4, None, s),
        "embed wpe without pos": lambda: L.sgpt_embed(h, p(ids), None, p(x), p(x), 4, 64, 4, 4, p(out), s),
        "layernorm d % 4": lambda: L.sgpt_layernorm(h, p(x6), p(g6), p(g6), 4, 66, EPS, p(out6), 0, 1.0, 0, s),
        "layernorm d > 4096": lambda: L.sgpt_layernorm(h, p(wide), p(wide), p(wide), 2, 4100, EPS, p(wide), 0, 1.0, 0, s),
        "layernorm null gamma": lambda: L.sgpt_layernorm(h, p(x), None, p(b), 4, 64, EPS, p(out), 0, 1.0, 0, s),
        "layernorm null out": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, None, 0, 1.0, 0, s),
        "layernorm out_dtype": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(out), 2, 1.0, 0, s),
        "layernorm split fp32": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(out), 0, 1.0, 1, s),
        "layernorm out_mul 3": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(o16), 3, 3.0, 0, s),
        "layernorm out_mul 0": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(o16), 3, 0.0, 0, s),
        "layernorm out_mul < 0": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(o16), 3, -0.5, 0, s),
        "layernorm out_mul on bf16": lambda: L.sgpt_layernorm(h, p(x), p(g), p(b), 4, 64, EPS, p(o16), 1, 0.5, 0, s),
        "lnf_pool d % 4": lambda: L.sgpt_lnf_pool(h, p(x6), p(g6), p(g6), p(off), p(ln), None, 2, 66, EPS, 1, 0, 0, None, 0, p(out6), None, s),
        "lnf_pool d > 4096": lambda: L.sgpt_lnf_pool(h, p(wide), p(wide), p(wide), p(off), p(ln), None, 1, 4100, EPS, 1, 0, 0, None, 0, p(wide), None, s),
        "lnf_pool mode 4": lambda: L.sgpt_lnf_pool(h, p(x), p(g), p(b), p(off), p(ln), None, 2, 64, EPS, 1, 4, 0, None, 0, p(out), None, s),
        "lnf_pool mode -1": lambda: L.sgpt_lnf_pool(h, p(x), p(g), p(b), p(off), p(ln), None, 2, 64, EPS, 1, -1, 0, None, 0, p(out), None, s),
        "lnf_pool null seq_len": lambda: L.sgpt_lnf_pool(h, p(x), p(g), p(b), p(off), None, None, 2, 64, EPS, 1, 0, 0, None, 0, p(out), None, s),
        "lnf_pool ln without gamma": lambda: L.sgpt_lnf_pool(h, p(x), None, p(b), p(off), p(ln), None, 2, 64, EPS, 1, 0, 0, None, 0, p(out), None, s),
        "lnf_pool learntmean without weights": lambda: L.sgpt_lnf_pool(h, p(x), p(g), p(b), p(off), p(ln), None, 2, 64, EPS, 1, 3, 0, None, 0, p(out), None, s),
        "rope odd rotary_dim": lambda: L.sgpt_rope(h, p(out), 0, 64, 32, p(pos), p(sin), p(cos), 4, 1, 32, 31, 8, s),
        "rope rotary_dim > head_dim": lambda: L.sgpt_rope(h, p(out), 0, 64, 32, p(pos), p(sin), p(cos), 4, 1, 32, 34, 8, s),
        "rope k inside q": lambda: L.sgpt_rope(h, p(out), 0, 64, 16, p(pos), p(sin), p(cos), 4, 1, 32, 32, 8, s),
        "rope ld too short": lambda: L.sgpt_rope(h, p(out), 0, 48, 32, p(pos), p(sin), p(cos), 4, 1, 32, 32, 8, s),
        "rope dtype": lambda: L.sgpt_rope(h, p(out), 2, 64, 32, p(pos), p(sin), p(cos), 4, 1, 32, 32, 8, s),
        "rope null pos": lambda: L.sgpt_rope(h, p(out), 0, 64, 32, None, p(sin), p(cos), 4, 1, 32, 32, 8, s),
        "rope null table": lambda: L.sgpt_rope(h, p(out), 0, 64, 32, p(pos), None, p(cos), 4, 1, 32, 32, 8, s),
        "logprob null targets": lambda: L.sgpt_logprob_rows(h, p(x), 64, 64, None, 4, p(out), None, s),
        "logprob null out": lambda: L.sgpt_logprob_rows(h, p(x), 64, 64, p(ids), 4, None, None, s),
        "logprob ld < V": lambda: L.sgpt_logprob_rows(h, p(x), 32, 64, p(ids), 4, p(out), None, s),
        "logprob V = 0": lambda: L.sgpt_logprob_rows(h, p(x), 64, 0, p(ids), 4, p(out), None, s),
    }
    for what, call in bad.items():
        with pytest.raises(ValueError):
            ctx._chk(call(), what)
    torch.cuda.synchronize()
    for t in (out, out6, o16, wide):
        assert (t == SENTINEL).all(), "a refused call wrote its output"
    with pytest.raises(ValueError):
        ctx.lnf_pool(x, off, ln, mode="maxpool")
