"""-m gpu: the fp8 (e4m3) MFMA GEMM (gemm256q_kernel of csrc/gemm256q.hip, entry sgpt_linear_fp8) where it differs from a plain tiled
GEMM -- the carry-over between the tiles of one workgroup's run (the next tile's first k-steps fetched under the current tile's
last ones, ring positions carried mod 3 and mod 2, so that a tile starts from sd = 0, 1 or 2), both deep operands, runs with
skipped slots inside, workgroups without a tile, the per-tile indexing of the row and channel scales, the placement of all four
epilogues, the per-ctx workgroup cap, the saturation flag over a run, and the refusals of the entry.

Exact tests.  The operands of gemm_ref.exact_case are small-integer e4m3 codes under power-of-two scales with an integer bias and
residual: every product, every sum in any order and every epilogue intermediate is exact in fp32 (tests/test_gemm_ref.py shows
it without a GPU, and that a k-step taken from the neighbouring tile of a run or from a stale ring slot changes more than nine
tenths of a tile's sums).  So the kernel has ONE right answer per element and the tests assert torch.equal against the integer
product computed in float64 on the CPU: fp32 (epi 2) as it is, 16-bit stores (epi 0, 4) as torch's round-to-nearest-even cast
of the exact value, e4m3 codes (epi 1) as torch's float8_e4m3fn conversion.  For epi 1 the bias of gemm_ref.gelu_exact_setup keeps
every u = acc + bias >= 16 (the tanh is saturated: gelu_new(u) = u but for the last bit of the reciprocal) and every u / out_scale at
2^-19 relative (16 fp32 ulps) or more from every rounding boundary of e4m3, so that a last-bit difference in rcp or exp2 cannot
move a code; a bias per column cannot make every u / out_scale exactly representable (see gelu_exact_setup).

Random operands (Gaussian data with log-normal row magnitudes through sgpt_fp8_quantize_rows, a_scalar 0.3, Gaussian bias and
residual) are compared with the float64 product of the de-quantised operands under the DERIVED bound of tests/gemm_ref.py: (K + 4)
2^-23 (|a| |w|^T + |bias| + |resid|) for fp32 (the epilogue's five roundings at 2^-24 each fit the 4 x 2^-23); + u16 |ref| for a
16-bit store; for epi 1 1.13 x the bound + 5e-4 (the allowance gemm_gpu_util.tolerance gives the fast tanh form behind f16 operands,
the smaller of its two) + half an e4m3 step of the reference, max(2^-4 |ref|, 2^-10 out_scale).

Buffers and sentinels: tests/gemm_gpu_util.py.  Every call is made twice and must return the same bits.

Worst error / tolerance of the random cases (printed under `-s`), first device run, 2026-10-20, MI355X (55 passed; every exact
test bit for bit at the first attempt -- no defect found in gemm256q.hip).  Key: epilogue, output type, b = with bias, i = in place.
A 16-bit store and the e4m3 store sit near 1 by construction: the tolerance is the accumulation bound plus ONE half-step rounding
to the output format, which the worst element uses up; the fp32 output uses under half of the derived bound.
  q8-ringA-k256: 2fp32bi=0.393 1e4m3b=0.936 0bf16b=0.976 0f16=0.825 4bf16=0.963 4f16b=0.919
  q8-ringW-k512: 2fp32bi=0.140 1e4m3b=0.934 0bf16b=0.962 0f16=0.668 4bf16=0.925 4f16b=0.827
  q8-ringA-k768: 2fp32bi=0.055 1e4m3b=0.929 0bf16b=0.941 0f16=0.508 4bf16=0.874 4f16b=0.766
  q8-groups:     2fp32bi=0.450 1e4m3b=0.937 0bf16b=0.979 0f16=0.831 4bf16=0.967 4f16b=0.918"""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import gemm_ref as G
from gemm_gpu_util import CODE, DEV, GUARD, TORCH, check_guards, guarded, tolerance

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
IDS = dict(ids=lambda c: c.name)
EXACT_ROWS = [c for c in G.CASES256Q if c.tag in ("ring", "uneven", "single", "groups")]
GRID_ROWS = [c for c in G.CASES256Q if c.tag == "grid"]
VARIANTS = list(G.SCALE_VARIANTS)
# (epi, output type, with bias, in place)
EVERY_EPILOGUE = ([(2, "fp32", True, False), (2, "fp32", True, True), (1, "e4m3", True, False)]
                  + [(epi, dt, wb, False) for epi in (0, 4) for dt in ("bf16", "f16") for wb in (False, True)])
RANDOM_EPILOGUES = [(2, "fp32", True, True), (1, "e4m3", True, False), (0, "bf16", True, False), (0, "f16", False, False),
                    (4, "bf16", False, False), (4, "f16", True, False)]
GRID_EPILOGUES = [(2, "fp32", True, True), (4, "bf16", True, False), (4, "f16", False, False)]
OUT_T = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.uint8}


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


@contextlib.contextmanager
def workgroup_cap(ctx, cap):
    """The per-ctx workgroup cap for the block, restored afterwards; the setter returns the previous value."""
    old = ctx.set_gemm_cu_cap(cap)
    try:
        assert ctx.set_gemm_cu_cap(cap) == cap
        yield
    finally:
        back = ctx.set_gemm_cu_cap(old)
    assert back == cap


def codes_of(x):
    """Small integers (numpy) as e4m3 codes on the device."""
    t = torch.from_numpy(x.astype(np.float32)).to(torch.float8_e4m3fn)
    assert np.array_equal(t.float().numpy(), x)
    return t.view(torch.uint8).to(DEV).contiguous()


def f32_dev(x):
    """A float64 array that is exactly representable in fp32, on the device."""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(x32.astype(np.float64), x), "the reference is not an fp32 number"
    return torch.from_numpy(x32).to(DEV)


@functools.lru_cache(maxsize=1)
def dev_case(name):
    """gemm_ref.exact_case with the operands on the device (one case kept at a time)."""
    x = dict(G.exact_case(name))
    x.update(a8=codes_of(x["a"]), w8=codes_of(x["w"]), sa_d=f32_dev(x["sa"]), sw_d=f32_dev(x["sw"]), bias_d=f32_dev(x["bias"]),
             resid_d=f32_dev(x["resid"]))
    return x


def run_fp8(ctx, epi, out, a8, sa_d, a_scalar, w8, sw_d, bias_d, resid_d, out_scale=1.0, inplace=False, what=""):
    """sgpt_linear_fp8 into guarded buffers, twice; guards, no sentinel left, same bits.  out: 'fp32' | 'bf16' | 'f16' | 'e4m3'.
    Returns the output (device), [M, N] or [N, M] for epi 4."""
    (M, K), N = a8.shape, w8.shape[0]
    out_t = OUT_T[out]
    bufs = []
    for _ in range(2):
        buf, body = guarded(M * N, out_t, init=resid_d if (epi == 2 and inplace) else None)
        resid_p = None if epi != 2 else (body.data_ptr() if inplace else resid_d.data_ptr())
        st = ctx.lib.sgpt_linear_fp8(ctx.handle, epi, CODE.get(out, 0), a8.data_ptr(), None if sa_d is None else sa_d.data_ptr(), a_scalar,
                                     w8.data_ptr(), sw_d.data_ptr(), None if bias_d is None else bias_d.data_ptr(), resid_p, body.data_ptr(),
                                     out_scale, M, N, K, None)
        ctx._chk(st, f"sgpt_linear_fp8 {what}")
        check_guards(buf, M * N, what)
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), f"{what}: two identical calls, different bits"
    return body.view((N, M) if epi == 4 else (M, N))


def label(name, variant, epi, out, with_bias, inplace, cap=None):
    return (f"{name} {variant} epi {epi} {out}{' +bias' if with_bias else ''}{' in place' if inplace else ''}"
            f"{'' if cap is None else f' cap {cap}'}")


def first_difference(got, want):
    """Where two device tensors of one shape first differ, for the assertion message: (index, got, want, count)."""
    ne = (got != want)
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return idx, got[idx].item(), want[idx].item(), int(ne.sum())


def check_exact(ctx, name, variant, epilogues, cap=None):
    """The listed epilogues of a case on the exact operands: every element equal to the one right answer.  Returns the outputs."""
    x = dev_case(name)
    rows, a_scalar = G.SCALE_VARIANTS[variant]
    sa_d = x["sa_d"] if rows else None
    v = G.exact_scaled(x, variant)                       # acc sa a_scalar sw, float64, exact
    outs = {}
    ctx.range_check()                                    # clear
    for epi, out, with_bias, inplace in epilogues:
        what = label(name, variant, epi, out, with_bias, inplace, cap)
        if epi == 1:
            bias64, out_scale, u = G.gelu_exact_setup(x["acc"], x["sa"] if rows else None, x["sw"], a_scalar)
            assert float(u.min()) >= 16.0 and float(G.e4m3_tie_distance(u / out_scale).min()) >= G.GELU_EXACT_MARGIN
            want = f32_dev(u / out_scale).cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
            bias_d = f32_dev(bias64)
        else:
            out_scale, bias_d = 1.0, (x["bias_d"] if with_bias else None)
            val = v + x["bias"][None, :] if with_bias else v
            if epi == 2:
                val = val + x["resid"]
            want = f32_dev(val.T if epi == 4 else val)
            if out != "fp32":
                want = want.to(TORCH[out])               # one rounding to nearest even of the exact value
        got = run_fp8(ctx, epi, out, x["a8"], sa_d, a_scalar, x["w8"], x["sw_d"], bias_d, x["resid_d"], out_scale, inplace, what)
        assert torch.equal(got, want), f"{what}: (index, got, exact, differing elements) = {first_difference(got, want)}"
        assert ctx.range_check() == 0, f"{what}: range flag"
        outs[(epi, out, with_bias, inplace)] = got
    return outs


# ---------------------------------------------------------------- exact sums over a run of tiles ---------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", EXACT_ROWS, **IDS)
def test_every_epilogue_is_exact_over_a_tile_run(ctx, c, variant):
    """24 tiles on 8 workgroups (runs of 3 whose tiles start from every ring position, deep A and deep W), 20 tiles on 5 of 8
    workgroups, one tile, and 81 tiles with skipped slots inside the runs: every epilogue, every scale variant, bit for bit."""
    with workgroup_cap(ctx, c.cu_cap):
        outs = check_exact(ctx, c.name, variant, EVERY_EPILOGUE)
    assert torch.equal(outs[(2, "fp32", True, True)], outs[(2, "fp32", True, False)])


@pytest.mark.parametrize("c", GRID_ROWS, **IDS)
def test_default_grid_is_exact(ctx, c):
    """288 tiles on a device of 256 CUs without a cap: runs of two tiles and of one, both orientations; the read-modify-write
    epilogue in place and the transposed store."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    L = G.tiles256q(c.M, c.N, ncu)
    if max(len(r) for r in L.runs) < 2:
        pytest.skip(f"{c.name}: on this device of {ncu} CUs the launch has {L.grid} workgroups for {L.tiles_total} slots: no run of two tiles")
    with workgroup_cap(ctx, 0):
        check_exact(ctx, c.name, "both", GRID_EPILOGUES)


# ---------------------------------------------------------------- bits do not depend on the cap ----------------------------------

def test_bits_do_not_depend_on_the_workgroup_cap(ctx):
    """include/sgpt_hip.h: results do not depend on sgpt_ctx_set_gemm_cu_cap -- 24 tiles on 24+ workgroups (cap 0), on 8 (runs of
    3), on 24 and under a cap that is no multiple of 8: all epilogues give the bits of the exact reference, hence the same bits."""
    outs = {}
    for cap in G.CAPQ:
        with workgroup_cap(ctx, cap):
            outs[cap] = check_exact(ctx, "q8-cap", "both", EVERY_EPILOGUE, cap)
    for cap in G.CAPQ[1:]:
        for key, o in outs[cap].items():
            ity = {1: torch.uint8, 2: torch.int32, 4: torch.int16}[o.element_size()]
            assert torch.equal(o.view(ity), outs[0][key].view(ity)), f"q8-cap {key}: cap {cap} differs from cap 0"


# ---------------------------------------------------------------- random operands against float64 ---------------------------------

@pytest.mark.parametrize("name", ["q8-ringA-k256", "q8-ringW-k512", "q8-ringA-k768", "q8-groups"])
def test_random_operands_vs_float64(ctx, name):
    c = G.case(name)
    M, N, K = c.M, c.N, c.K
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N + 7 * K)
    a = torch.randn((M, K), generator=g, device=DEV) * torch.exp(torch.randn((M, 1), generator=g, device=DEV))
    w = torch.randn((N, K), generator=g, device=DEV) / math.sqrt(K)
    bias_d = torch.randn((N,), generator=g, device=DEV) * 0.3
    resid_d = torch.randn((M, N), generator=g, device=DEV) * 2
    a8, sa_d = ctx.fp8_quantize_rows(a)
    w8, sw_d = ctx.fp8_quantize_rows(w)
    a_scalar = float(np.float32(0.3))
    dq = lambda codes, s: codes.view(torch.float8_e4m3fn).float().double().cpu().numpy() * s.double().cpu().numpy()[:, None]
    a64, w64 = dq(a8, sa_d) * a_scalar, dq(w8, sw_d)
    bias64, resid64 = bias_d.double().cpu().numpy(), resid_d.double().cpu().numpy()
    u, s = G.product(a64, w64), G.abs_product(a64, w64)
    line = []
    ctx.range_check()
    with workgroup_cap(ctx, c.cu_cap):
        for epi, out, with_bias, inplace in RANDOM_EPILOGUES:
            what = label(name, "random", epi, out, with_bias, inplace)
            b64, r64 = (bias64 if with_bias else None), (resid64 if epi == 2 else None)
            ref = G.epilogue(u, b64, r64, epi)
            bnd = G.bound_from(s, b64, r64, K)
            bnd = bnd.T if epi == 4 else bnd
            out_scale = 1.0
            if epi == 1:
                out_scale = 2.0 ** math.ceil(math.log2(float(np.abs(ref).max()) * 1.5 / 448))
                tol = tolerance("f16", 1, False, ref, bnd) + np.maximum(2.0 ** -4 * np.abs(ref), 2.0 ** -10 * out_scale)
            else:
                tol = tolerance(out if out != "fp32" else "f16", epi, out != "fp32", ref, bnd)
            got_d = run_fp8(ctx, epi, out, a8, sa_d, a_scalar, w8, sw_d, bias_d if with_bias else None, resid_d, out_scale, inplace, what)
            got = (got_d.view(torch.float8_e4m3fn).float().double() * out_scale if epi == 1 else got_d.double()).cpu().numpy()
            assert np.isfinite(got).all(), f"{what}: not finite"
            ratio = np.abs(got - ref) / tol
            worst = float(ratio.max())
            line.append(f"{epi}{out}{'b' if with_bias else ''}{'i' if inplace else ''}={worst:.3f}")
            assert worst <= 1.0, f"{what}: {worst:.2f} x the tolerance at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"
            assert ctx.range_check() == 0, f"{what}: range flag"
    print(f"{name} random worst error / tolerance: {' '.join(line)}")


# ---------------------------------------------------------------- the saturation flag over a run ---------------------------------

def test_saturation_flag_from_one_element_of_the_last_tile_of_a_run(ctx):
    """2048 x 768 x 512 on 8 workgroups, epi 1: a workgroup walks three tiles and ORs its saturation bit once per tile.  With a
    zero bias and out_scale twice what the largest |u| needs, nothing saturates.  The bias of ONE column of the last tile of a
    workgroup's run is then raised so that the column's largest u -- a row of that tile, at least 4 out_scale above the second
    largest -- lands at 448 out_scale (1 + 2^-8) and every other element of the column below 448 out_scale (1 - 2^-8): bit 1 of
    sgpt_range_check, the next read 0, and the element's code is 448.  With that element at 448 out_scale (1 - 2^-8): 0."""
    c = G.case("q8-ringA-k512")
    x = dev_case(c.name)
    L = G.launch_of_q8(c)
    v = G.exact_scaled(x, "row")
    out_scale = 2.0 ** (math.ceil(math.log2(float(np.abs(v).max()) / 448.0)) + 1)
    T = 448.0 * out_scale
    found = None
    for b, run in enumerate(L.runs):
        assert len(run) == 3
        m0, n0 = run[-1]
        cols = v[:, n0:n0 + 256]
        top = np.sort(cols, axis=0)[-2:]                 # second largest, largest of every column
        arg = cols.argmax(axis=0)
        ok = (arg >= m0) & (arg < m0 + 256) & (top[1] - top[0] >= 4.0 * out_scale)
        if ok.any():
            j = int(np.flatnonzero(ok)[0])
            found = (b, int(arg[j]), n0 + j, float(top[1, j]), float(top[0, j]))
            break
    assert found is not None, "no column of a last tile whose largest element stands out"
    b, m, n, u1, u2 = found
    ctx.range_check()
    with workgroup_cap(ctx, c.cu_cap):
        for factor, flagged in ((1.0 + 2.0 ** -8, True), (1.0 - 2.0 ** -8, False)):
            bias = np.zeros(c.N)
            bias[n] = T * factor - u1
            assert u2 + bias[n] < T * (1.0 - 2.0 ** -8) or not flagged
            assert float((v[:, n] + bias[n]).min()) > -T / 2
            got = run_fp8(ctx, 1, "e4m3", x["a8"], x["sa_d"], 1.0, x["w8"], x["sw_d"], f32_dev(bias), None, out_scale,
                          what=f"saturation: element ({m}, {n}) of the last tile of workgroup {b} at {factor:.5f} x 448 out_scale")
            flag = ctx.range_check()
            assert flag == (2 if flagged else 0), f"element ({m}, {n}) at {factor:.5f} x 448 out_scale: range_check() = {flag}"
            assert ctx.range_check() == 0
            if flagged:
                assert int(got[m, n]) == 0x7E


# ---------------------------------------------------------------- refusals --------------------------------------------------------

BASE = dict(M=256, N=256, K=256, epi=2, out="fp32", a_scalar=1.0, out_scale=1.0, null=())
REFUSALS = [
    ("M % 256", dict(M=384)), ("N % 256", dict(N=128)), ("K % 256", dict(K=384)), ("K = 128", dict(K=128)),
    ("epi 9", dict(epi=9)), ("epi 3", dict(epi=3)),
    ("epi 0 to fp32", dict(epi=0)), ("epi 4 to fp32", dict(epi=4)),
    ("epi 1 without bias", dict(epi=1, out="e4m3", null=("bias",))), ("epi 2 without bias", dict(null=("bias",))),
    ("epi 2 without resid", dict(null=("resid",))),
    ("a_scalar 0", dict(a_scalar=0.0)), ("a_scalar < 0", dict(a_scalar=-1.0)),
    ("epi 1 out_scale 0", dict(epi=1, out="e4m3", out_scale=0.0)), ("epi 1 out_scale < 0", dict(epi=1, out="e4m3", out_scale=-2.0)),
    ("null A", dict(null=("a",))), ("null W", dict(null=("w",))), ("null w_scale", dict(null=("w_scale",))), ("null out", dict(null=("out",))),
]


@pytest.mark.parametrize("why,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_the_output_untouched(ctx, why, change):
    """SGPT_ERR_INVALID and nothing launched: the sentinel-filled output (room for 512 x 512 elements) is as it was."""
    p = dict(BASE, **change)
    a8 = torch.zeros((512, 512), dtype=torch.uint8, device=DEV)
    w8 = torch.zeros((512, 512), dtype=torch.uint8, device=DEV)
    ones = torch.ones((512,), dtype=torch.float32, device=DEV)
    resid = torch.zeros((512, 512), dtype=torch.float32, device=DEV)
    buf, body = guarded(512 * 512, OUT_T[p["out"]])
    before = buf.clone()
    ptr = lambda key, t: None if key in p["null"] else t.data_ptr()
    st = ctx.lib.sgpt_linear_fp8(ctx.handle, p["epi"], CODE.get(p["out"], 0), ptr("a", a8), ptr("a_scale", ones), p["a_scalar"], ptr("w", w8),
                                 ptr("w_scale", ones), ptr("bias", ones), ptr("resid", resid), ptr("out", body), p["out_scale"],
                                 p["M"], p["N"], p["K"], None)
    assert st == ERR_INVALID, f"{why}: status {st}"
    torch.cuda.synchronize()
    assert torch.equal(buf, before), f"{why}: the output was written"


def test_the_accepted_form_of_the_refusal_arguments_runs(ctx):
    """The unchanged BASE call of the refusal test is served (so each refusal above is caused by its one change)."""
    a8 = torch.zeros((256, 256), dtype=torch.uint8, device=DEV)
    ones = torch.ones((256,), dtype=torch.float32, device=DEV)
    resid = torch.full((256, 256), 3.0, dtype=torch.float32, device=DEV)
    got = run_fp8(ctx, 2, "fp32", a8, ones, 1.0, a8, ones, ones, resid, what="base call")
    assert torch.equal(got, torch.full_like(got, 4.0))
