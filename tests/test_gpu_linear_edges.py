"""-m gpu: the register-staged GEMM (gemm_kernel of csrc/gemm.hip: 64x64 and 128x128 tiles, 64- and 128-element k-steps, k-groups)
where such a kernel goes wrong -- ragged M, N and K, fp32 operands, the 128x128 tile, the supertile block order with unfriendly
tile counts, a K tail under k-groups, odd N -- against the float64 reference and the DERIVED bound of tests/gemm_ref.py
((K + 4) 2^-23 (|a| |w|^T + |bias| + |resid|); tests/test_gemm_ref.py shows without a GPU that the shape table reaches every branch of
the launch rule, that an fp32 chain of the same inputs stays under a quarter of the bound and that a dropped 16-byte k-chunk
leaves it by more than 4 x).  tests/test_gpu_linear.py covers the aligned shapes and the 256x256 LDS-DMA kernel.

The C entries are called directly: the output lives inside a larger buffer whose guard elements (and, before the call, the
output itself) hold a NaN bit pattern, so a stray store, an unwritten element and a clamped row that got stored all show.
Every call is made twice into fresh buffers and must return the same bits.

Tolerances: `bound` for fp32 outputs; + u16 |ref| (2^-8 bf16 / 2^-11 f16) for one rounding to a 16-bit output; through a GELU
the accumulation bound times 1.13 (max |gelu'|) plus the function's own allowance -- 2e-3 (bf16) / 5e-4 (f16) absolute for the
fast sigmoid form of the 16-bit tanh GELU (tests/test_gpu_linear.py), 2e-5 + 1e-6 |ref| for the fp32 tanh GELU and for the
erf GELU in every format (tests/test_gpu_bert.py; the erf epilogue is the same fp32 code whatever the operand format).

Record of how much room the derived bounds leave (worst error / tolerance per case, printed under `-s` by check_case): NOT YET
RECORDED -- this file has so far run only against a CPU imitation of the two entries (which exercises the buffers, references,
tolerances and assertions, not the kernel).  The first run on the device prints the lines to copy here with the date; a case
beyond its tolerance is a finding about gemm.hip, not about the bound."""
import functools

import numpy as np
import pytest
import torch

import gemm_ref as G
from gemm_gpu_util import CODE, DEV, GUARD, SENT16, TORCH, guarded, run, tolerance

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16", "fp32"]
ERR_INVALID = -1
IDS = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


# ---------------------------------------------------------------- inputs, references, guarded buffers ----------------------------

@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """Operands of a case on the device, their float64 values, and the two float64 products every check of the case shares."""
    x = G.make_inputs(G.case(name), dtype)
    for k in ("a", "w", "bias", "resid"):
        x[k + "_d"] = x[k].to(DEV).contiguous()
    x["u"] = G.product(x["a64"], x["w64"])
    x["s"] = G.abs_product(x["a64"], x["w64"])
    return x


def combos(c, dtype):
    """(epi, out16, with bias, in place) the shape and format allow."""
    h = dtype != "fp32"
    if c.tag == "oddn":                                 # the LM head: fp32 logits
        return [(0, False, False, False), (0, False, True, False)]
    if c.tag == "last":
        return [(0, h, True, False)]
    out = [(0, False, False, False), (0, False, True, False)]
    if h:
        out += [(0, True, False, False), (0, True, True, False)]
    out += [(1, h, True, False), (9, h, True, False), (2, False, True, False), (2, False, True, True)]
    if h and c.M % 128 == 0:
        out += [(4, True, False, False), (4, True, True, False)]
    return out


def check_case(ctx, c, dtype, which=None):
    """Every epilogue of the case against gemm_ref within the tolerance; prints worst error / tolerance.  Returns the outputs."""
    x = inputs(c.name, dtype)
    outs, line = {}, []
    for epi, out16, with_bias, inplace in (which or combos(c, dtype)):
        what = f"{c.name} {dtype} epi {epi}{' 16-bit' if out16 else ' fp32'}{' +bias' if with_bias else ''}{' in place' if inplace else ''}"
        got_d = run(ctx, dtype, epi, out16, x["a_d"], x["w_d"], x["bias_d"] if with_bias else None, x["resid_d"], inplace, what)
        got = got_d.double().cpu().numpy()
        b64, r64 = (x["bias64"] if with_bias else None), (x["resid64"] if epi == 2 else None)
        ref = G.epilogue(x["u"], b64, r64, epi)
        bnd = G.bound_from(x["s"], b64, r64, x["K"])
        tol = tolerance(dtype, epi, out16, ref, bnd.T if epi == 4 else bnd)
        ratio = np.abs(got - ref) / tol
        worst = float(ratio.max())
        line.append(f"{epi}{'h' if out16 else 's'}{'b' if with_bias else ''}{'i' if inplace else ''}={worst:.3f}")
        assert worst <= 1.0, f"{what}: {worst:.2f} x the tolerance at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"
        outs[(epi, out16, with_bias, inplace)] = got_d
    print(f"{c.name} {dtype} worst error / tolerance: {' '.join(line)}")
    return outs


# ---------------------------------------------------------------- every epilogue at every ragged shape ---------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [c for c in G.CASES if c.tag in ("epi", "oddn")], **IDS)
def test_epilogues_at_ragged_shapes_vs_float64(ctx, c, dtype):
    outs = check_case(ctx, c, dtype)
    if (2, False, True, True) in outs:                  # in place on the residual stream: the same bits as out of place
        assert torch.equal(outs[(2, False, True, True)], outs[(2, False, True, False)])


# ---------------------------------------------------------------- exact layout probes -------------------------------------------

PROBES = ["kt-65x68", "st64-1540x1412", "st128-3100x3076", "run128-2500x1924", "kg2-130x68", "lmhead-37x50257", "odd-65x1001"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PROBES)
def test_integer_probe_is_exact_at_ragged_shapes(ctx, name, dtype):
    """Small-integer operands with patterns of periods 13 (rows of A), 61 (rows of W) and 11 / 7 along k -- no tile size, k-step
    or chunk is a period -- and every sum below 2^24: epi 0 (fp32 out) and epi 2 equal the integer product bit for bit, so a
    dropped or doubled k-chunk, a stored clamped row or a swapped tile fails without any tolerance."""
    c = G.case(name)
    M, N, K = c.M, c.N, G.case_k(c, dtype)
    m, n, k = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    a = ((5 * m + 11 * k) % 13 - 6).astype(np.float64)
    w = ((3 * n + 7 * k) % 61 - 30).astype(np.float64)
    bias = ((np.arange(N) * 5) % 17 - 8).astype(np.float64)
    resid = ((7 * np.arange(M)[:, None] + 3 * np.arange(N)[None, :]) % 201 - 100).astype(np.float64)
    want = a @ w.T                                      # integers below 2^53: exact
    assert np.abs(want).max() + 108 < 2 ** 24
    a_d = torch.from_numpy(a).to(TORCH[dtype]).to(DEV)
    w_d = torch.from_numpy(w).to(TORCH[dtype]).to(DEV)
    assert np.array_equal(a_d.double().cpu().numpy(), a) and np.array_equal(w_d.double().cpu().numpy(), w)
    bias_d, resid_d = torch.from_numpy(bias).float().to(DEV), torch.from_numpy(resid).float().to(DEV).contiguous()
    old = ctx.set_low_latency(c.ll)
    try:
        got = run(ctx, dtype, 0, False, a_d, w_d, None, None, what=f"{name} probe epi 0")
        assert np.array_equal(got.double().cpu().numpy(), want)
        got = run(ctx, dtype, 0, False, a_d, w_d, bias_d, None, what=f"{name} probe epi 0 + bias")
        assert np.array_equal(got.double().cpu().numpy(), want + bias[None, :])
        if N % 4 == 0:
            for inplace in (False, True):
                got = run(ctx, dtype, 2, False, a_d, w_d, bias_d, resid_d, inplace, what=f"{name} probe epi 2")
                assert np.array_equal(got.double().cpu().numpy(), want + bias[None, :] + resid)
    finally:
        ctx.set_low_latency(old)


# ---------------------------------------------------------------- bit invariance across tile sizes and k-steps -------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", G.BLOCK_CASES)
def test_block_bits_do_not_depend_on_tile_or_k_step(ctx, name, dtype):
    """The top-left 130 x 68 block of a large call (128x128 or 64x64 tiles, 64-element k-steps) equals the same block computed as
    a problem of its own (64x64 tiles, 128-element k-steps) bit for bit: store, both GELUs, bias + residual."""
    x = inputs(name, dtype)
    h = dtype != "fp32"
    bm, bn = G.BLOCK_M, G.BLOCK_N
    a_s, w_s, b_s = x["a_d"][:bm].contiguous(), x["w_d"][:bn].contiguous(), x["bias_d"][:bn].contiguous()
    r_s = x["resid_d"][:bm, :bn].contiguous()
    for epi, out16 in [(0, False), (1, h), (2, False), (9, h)] + ([(0, True)] if h else []):
        big = run(ctx, dtype, epi, out16, x["a_d"], x["w_d"], x["bias_d"], x["resid_d"], what=f"{name} {dtype} epi {epi}")
        small = run(ctx, dtype, epi, out16, a_s, w_s, b_s, r_s, what=f"{name} {dtype} block epi {epi}")
        assert torch.equal(big[:bm, :bn].contiguous().view(torch.int32 if not out16 else torch.int16),
                           small.view(torch.int32 if not out16 else torch.int16)), f"{name} {dtype} epi {epi} (16-bit out: {out16})"


# ---------------------------------------------------------------- k-groups with a K tail ------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_k_groups_with_a_tail_and_the_one_group_control(ctx, dtype):
    """Low-latency mode on: K = 1528 [fp32: 764] is 12 k-steps, two groups of 6, the last step of group 1 the partial one --
    deterministic over three runs, within the bound, and not the bits of the k-ascending sum (or the test would be vacuous).
    K = 1400 [700] is 11 steps: one group, the bits of mode off."""
    h = dtype != "fp32"
    which = [(0, False, True, False), (1, h, True, False), (2, False, True, False), (2, False, True, True), (9, h, True, False)]
    old = ctx.set_low_latency(False)
    try:
        for name, split in (("kg2-130x68", True), ("kg1-130x68", False)):
            c = G.case(name)
            ctx.set_low_latency(False)
            off = check_case(ctx, c, dtype, which)
            ctx.set_low_latency(True)
            runs = [check_case(ctx, c, dtype, which) for _ in range(3 if split else 1)]
            for r in runs[1:]:
                assert all(torch.equal(r[k], runs[0][k]) for k in which), "k-group result changed between identical launches"
            if split:
                assert not torch.equal(runs[0][which[0]], off[which[0]]) and not torch.equal(runs[0][which[2]], off[which[2]]), \
                    "the k-group kernel did not run"
            else:
                assert all(torch.equal(runs[0][k], off[k]) for k in which), "one group: the k-ascending sum, bit for bit"
    finally:
        ctx.set_low_latency(old)


# ---------------------------------------------------------------- split (hi + lo) epilogues ---------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("epi,triple", [(0, False), (0, True), (1, False), (1, True), (4, False)])
def test_split_epilogues_at_a_ragged_shape(ctx, dtype, epi, triple):
    """sgpt_linear_split at M = 130 (128 for the transposed store), N = 68, K = 136: hi is the plain output bit for bit, hi + lo is
    within bound + u16^2 |ref| of the float64 value (lo = round16(v - hi): a relative u16 of a relative u16; f16: + 2^-25 for the
    subnormal grid of lo), and the sentinel columns behind each of the two or three column blocks are untouched."""
    gap = 4
    c = G.case("vt-128x68" if epi == 4 else "kt-130x68")
    x = dict(inputs(c.name, dtype))
    M, N, K = c.M, c.N, 136
    a_d, w_d = x["a_d"][:, :K].contiguous(), x["w_d"][:, :K].contiguous()
    a64, w64 = x["a64"][:, :K], x["w64"][:, :K]
    bias_d = x["bias_d"] if epi == 1 else None
    plain = run(ctx, dtype, epi, True, a_d, w_d, bias_d, None, what="plain")
    nblk = 3 if triple else 2
    if epi == 4:
        ldo, lo_delta, hi2_delta, total = M, N * M + GUARD, 0, 2 * N * M + GUARD
    else:
        ldo, lo_delta, hi2_delta = nblk * (N + gap), N + gap, (2 * (N + gap) if triple else 0)
        total = M * ldo
    bufs = []
    for _ in range(2):
        buf, body = guarded(total, TORCH[dtype])
        st = ctx.lib.sgpt_linear_split(ctx.handle, CODE[dtype], epi, a_d.data_ptr(), w_d.data_ptr(),
                                       None if bias_d is None else bias_d.data_ptr(), body.data_ptr(), ldo, lo_delta, hi2_delta, M, N, K, None)
        ctx._chk(st, "sgpt_linear_split")
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1])
    assert bool((buf[:GUARD] == SENT16).all()) and bool((buf[GUARD + total:] == SENT16).all())
    ibody = buf[GUARD:GUARD + total]
    if epi == 4:
        hi, lo = body[:N * M].view(N, M), body[N * M + GUARD:].view(N, M)
        assert bool((ibody[N * M:N * M + GUARD] == SENT16).all()), "a store between the hi and the lo array"
        blocks = [ibody[:N * M], ibody[N * M + GUARD:]]
    else:
        grid, igrid = body.view(M, nblk, N + gap), ibody.view(M, nblk, N + gap)
        assert bool((igrid[:, :, N:] == SENT16).all()), "a store behind a column block"
        hi, lo = grid[:, 0, :N], grid[:, 1, :N]
        blocks = [igrid[:, j, :N] for j in range(nblk)]
        if triple:
            assert torch.equal(igrid[:, 2, :N], igrid[:, 0, :N]), "the second hi copy"
    assert all(not bool((b == SENT16).any()) for b in blocks), "an element was left unwritten"
    assert torch.equal(hi.contiguous().view(torch.int16), plain.contiguous().view(torch.int16)), "hi is the plain output"
    ref = G.split_ref(a64, w64, x["bias64"] if epi == 1 else None, epi)
    bnd = G.bound(a64, w64, x["bias64"] if epi == 1 else None, None, K)
    u = G.U16[dtype]
    tol = (G.GELU_SLOPE * bnd + (2e-3 if dtype == "bf16" else 5e-4)) if epi == 1 else (bnd.T if epi == 4 else bnd)
    tol = tol + u * u * np.abs(ref) + (2.0 ** -25 if dtype == "f16" else 0.0)
    got = hi.double().cpu().numpy() + lo.double().cpu().numpy()
    worst = float((np.abs(got - ref) / tol).max())
    print(f"split {dtype} epi {epi} triple {triple}: worst error / tolerance = {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- f16 range flag at a ragged shape --------------------------------

def test_f16_range_flag_at_a_ragged_shape(ctx):
    """M = 65, N = 68, K = 136, f16: the last real row and column (64, 67) -- the row that the 63 clamped rows of the second row
    tile re-read, the column its clamped columns re-read -- holds the one element of magnitude 32768: the flag is raised.  With
    that row halved (16384 at (64, 67), computed 64 x 4 times over by the clamped lanes) it is not.  A clamped lane computes
    exactly the value of row M - 1, so no input exists that overflows ONLY in a clamped lane: that sub-case of the range check
    cannot be constructed, and what is shown is that the duplicates of an in-range row do not raise the flag."""
    c = G.case("kt-65x68")
    x = inputs(c.name, "f16")
    K = 136
    a, w = x["a"][:, :K].clone(), x["w"][:, :K].clone()
    a[c.M - 1] = 0.0
    a[c.M - 1, 0] = 256.0
    w[c.N - 1, 0] = 128.0
    w_d = w.to(DEV)
    ctx.range_check()                                   # clear
    for scale, flagged in ((1.0, True), (0.5, False)):
        a_d = (a.float() * scale).half().to(DEV)
        out = run(ctx, "f16", 0, True, a_d, w_d, None, None, what=f"range x{scale}")
        assert float(out[c.M - 1, c.N - 1]) == 32768.0 * scale
        assert float(out.float().abs().max()) == 32768.0 * scale
        assert bool(ctx.range_check()) == flagged
        assert not ctx.range_check()                    # and it resets


# ---------------------------------------------------------------- refusals --------------------------------------------------------

@pytest.mark.parametrize("dtype,epi,out,M,N,K", [
    ("f16", 0, "f16", 130, 68, 12), ("bf16", 2, "fp32", 130, 68, 20),          # K % 8 (16-bit)
    ("fp32", 0, "fp32", 130, 68, 6), ("fp32", 1, "fp32", 130, 68, 10),          # K % 4 (fp32)
    ("f16", 1, "f16", 128, 66, 16), ("f16", 2, "fp32", 128, 66, 16), ("bf16", 4, "bf16", 128, 66, 16), ("fp32", 9, "fp32", 128, 66, 16),
    ("f16", 4, "f16", 130, 68, 16),                                               # epi 4 with M % 128
    ("fp32", 0, "f16", 128, 68, 16), ("fp32", 0, "bf16", 128, 68, 16),           # fp32 operands, 16-bit output
])
def test_refused_shapes_leave_the_output_untouched(ctx, dtype, epi, out, M, N, K):
    a_d = torch.ones((M, K), dtype=TORCH[dtype], device=DEV)
    w_d = torch.ones((N, K), dtype=TORCH[dtype], device=DEV)
    bias_d = torch.ones((N,), device=DEV)
    resid_d = torch.ones((M, N), device=DEV)
    buf, body = guarded(M * N, TORCH[out])
    before = buf.clone()
    st = ctx.lib.sgpt_linear(ctx.handle, CODE[dtype], epi, CODE[out], a_d.data_ptr(), w_d.data_ptr(), bias_d.data_ptr(),
                             resid_d.data_ptr() if epi == 2 else None, body.data_ptr(), M, N, K, None)
    assert st == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ---------------------------------------------------------------- odd N, 16-bit output (keep this test last) ----------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_n_with_a_16_bit_output(ctx, dtype):
    """N = 1001, epi 0 + bias, output in the operand format: the rows of a dense [65, 1001] 16-bit array start on 2-byte
    boundaries, so the 8-byte vector stores of the epilogue are not 8-byte aligned (fp32: 16-byte stores on 4-byte boundaries) --
    the header allows it; and the last column group reads its bias element by element."""
    c = G.case("odd-65x1001")
    assert G.CASES[-1] is c
    check_case(ctx, c, dtype)
