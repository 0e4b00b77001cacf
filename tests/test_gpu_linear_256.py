"""-m gpu: the persistent 256x256 LDS-DMA GEMM (gemm256d_kernel of csrc/gemm.hip) where it differs from a plain tiled GEMM -- the
carry-over between the tiles of one workgroup's run (look-ahead of two tiles, the next tile's first k-steps fetched under the
current tile's last ones, ring positions carried mod 3 and mod 2: six ring states, one per nk % 6), the supertile tile order with
its skipped slots, the per-ctx workgroup cap, the split store and the f16 range tracker over a run, and the bulk fused QKV launch
with per-tile operand roles (sgpt_linear_qkv) -- against the float64 reference and the DERIVED bound of tests/gemm_ref.py.

The shapes are gemm_ref.CASES256, written for a device of 256 CUs (the tests skip on another); gemm_ref.tiles256 mirrors the
launch, and tests/test_gemm_ref.py shows without a GPU that the table reaches every branch of the tile walk, that the walk visits
every tile once, and that a stale ring slot or a prefetch from the wrong tile leaves the tolerance by more than 4 x on a quarter
of a tile.  Buffers, sentinels and tolerances: tests/gemm_gpu_util.py.  Every call is made twice and must return the same bits.

Record of how much room the derived bounds leave (worst error / tolerance per case, printed under `-s`): RECORD below, from the
run of 2026-10-20 on an MI355X (109 passed).  A 16-bit store sits near 1 by construction (the tolerance is the accumulation bound
plus ONE half-ulp rounding of the output, which the worst element uses up); the fp32 outputs use under 1 % of the bound.  A case
beyond its tolerance, a guard hit or a bit mismatch is a finding about gemm.hip, not about the bound.

RECORD -- 2026-10-20, MI355X, worst error / tolerance (key: epilogue, h = 16-bit / s = fp32 output, b = with bias, i = in place)
ringA-k128 bf16: 0h=0.983 0hb=0.984 1hb=0.924 9hb=0.982 2sb=0.006 2sbi=0.006 4h=0.983 4hb=0.984
ringA-k128 f16: 0h=0.902 0hb=0.905 1hb=0.798 9hb=0.883 2sb=0.007 2sbi=0.007 4h=0.902 4hb=0.905
ringA-k192 bf16: 0h=0.970 0hb=0.967 1hb=0.907 9hb=0.962 2sb=0.004 2sbi=0.004 4h=0.970 4hb=0.967
ringA-k192 f16: 0h=0.819 0hb=0.819 1hb=0.722 9hb=0.791 2sb=0.004 2sbi=0.004 4h=0.819 4hb=0.819
ringA-k256 bf16: 0h=0.954 0hb=0.954 1hb=0.897 9hb=0.940 2sb=0.003 2sbi=0.003 4h=0.954 4hb=0.954
ringA-k256 f16: 0h=0.817 0hb=0.815 1hb=0.758 9hb=0.794 2sb=0.004 2sbi=0.004 4h=0.817 4hb=0.815
ringA-k320 bf16: 0h=0.946 0hb=0.943 1hb=0.911 9hb=0.938 2sb=0.002 2sbi=0.002 4h=0.946 4hb=0.943
ringA-k320 f16: 0h=0.762 0hb=0.752 1hb=0.697 9hb=0.727 2sb=0.003 2sbi=0.003 4h=0.762 4hb=0.752
ringA-k384 bf16: 0h=0.943 0hb=0.934 1hb=0.901 9hb=0.928 2sb=0.002 2sbi=0.002 4h=0.943 4hb=0.934
ringA-k384 f16: 0h=0.683 0hb=0.686 1hb=0.633 9hb=0.658 2sb=0.002 2sbi=0.002 4h=0.683 4hb=0.686
ringA-k448 bf16: 0h=0.926 0hb=0.929 1hb=0.884 9hb=0.909 2sb=0.002 2sbi=0.002 4h=0.926 4hb=0.929
ringA-k448 f16: 0h=0.638 0hb=0.625 1hb=0.563 9hb=0.583 2sb=0.002 2sbi=0.002 4h=0.638 4hb=0.625
ringW-k128 bf16: 0h=0.984 0hb=0.984 1hb=0.924 9hb=0.981 2sb=0.006 2sbi=0.006 4h=0.984 4hb=0.984
ringW-k128 f16: 0h=0.907 0hb=0.907 1hb=0.804 9hb=0.892 2sb=0.006 2sbi=0.006 4h=0.907 4hb=0.907
ringW-k192 bf16: 0h=0.968 0hb=0.971 1hb=0.909 9hb=0.964 2sb=0.004 2sbi=0.004 4h=0.968 4hb=0.971
ringW-k192 f16: 0h=0.876 0hb=0.870 1hb=0.804 9hb=0.846 2sb=0.004 2sbi=0.004 4h=0.876 4hb=0.870
ringW-k256 bf16: 0h=0.961 0hb=0.947 1hb=0.897 9hb=0.941 2sb=0.003 2sbi=0.003 4h=0.961 4hb=0.947
ringW-k256 f16: 0h=0.812 0hb=0.825 1hb=0.767 9hb=0.804 2sb=0.003 2sbi=0.003 4h=0.812 4hb=0.825
ringW-k320 bf16: 0h=0.954 0hb=0.941 1hb=0.908 9hb=0.935 2sb=0.004 2sbi=0.004 4h=0.954 4hb=0.941
ringW-k320 f16: 0h=0.753 0hb=0.750 1hb=0.694 9hb=0.725 2sb=0.003 2sbi=0.003 4h=0.753 4hb=0.750
ringW-k384 bf16: 0h=0.940 0hb=0.939 1hb=0.905 9hb=0.932 2sb=0.002 2sbi=0.002 4h=0.940 4hb=0.939
ringW-k384 f16: 0h=0.685 0hb=0.702 1hb=0.629 9hb=0.654 2sb=0.003 2sbi=0.003 4h=0.685 4hb=0.702
ringW-k448 bf16: 0h=0.920 0hb=0.923 1hb=0.886 9hb=0.911 2sb=0.002 2sbi=0.002 4h=0.920 4hb=0.923
ringW-k448 f16: 0h=0.617 0hb=0.635 1hb=0.581 9hb=0.601 2sb=0.002 2sbi=0.002 4h=0.617 4hb=0.635
single bf16: 0h=0.971 0hb=0.968 1hb=0.909 9hb=0.966 2sb=0.004 2sbi=0.004 4h=0.971 4hb=0.968
single f16: 0h=0.891 0hb=0.892 1hb=0.791 9hb=0.875 2sb=0.005 2sbi=0.005 4h=0.891 4hb=0.892
uneven bf16: 0h=0.969 0hb=0.967 1hb=0.906 9hb=0.962 2sb=0.004 2sbi=0.004 4h=0.969 4hb=0.967
uneven f16: 0h=0.823 0hb=0.830 1hb=0.723 9hb=0.792 2sb=0.004 2sbi=0.004 4h=0.823 4hb=0.830
two-tile bf16: 0h=0.983 0hb=0.982 1hb=0.915 9hb=0.972 2sb=0.006 2sbi=0.006 4h=0.983 4hb=0.982
two-tile f16: 0h=0.902 0hb=0.907 1hb=0.804 9hb=0.891 2sb=0.006 2sbi=0.006 4h=0.902 4hb=0.907
cap24 bf16: 0h=0.946 0hb=0.943 1hb=0.911 9hb=0.938 2sb=0.002 2sbi=0.002 4h=0.946 4hb=0.943
cap24 f16: 0h=0.762 0hb=0.752 1hb=0.697 9hb=0.727 2sb=0.003 2sbi=0.003 4h=0.762 4hb=0.752
cap100 bf16: 0h=0.946 0hb=0.943 1hb=0.911 9hb=0.938 2sb=0.002 2sbi=0.002 4h=0.946 4hb=0.943
cap100 f16: 0h=0.762 0hb=0.752 1hb=0.697 9hb=0.727 2sb=0.003 2sbi=0.003 4h=0.762 4hb=0.752
grid-8448x2304: bf16 epi 2 in place 0.005, epi 4 0.971; f16 epi 2 in place 0.005, epi 4 0.885
super-m: bf16 epi 2 in place 0.007, epi 4 0.984; f16 epi 2 in place 0.008, epi 4 0.918
super-n: bf16 epi 2 in place 0.007, epi 4 0.984; f16 epi 2 in place 0.008, epi 4 0.919
super-3: bf16 epi 2 in place 0.008, epi 4 0.984; f16 epi 2 in place 0.010, epi 4 0.913
split ringA-k192 (triple False / True alike): epi 0 bf16 0.053 f16 0.004; epi 1 bf16 0.027 f16 0.003; epi 4 bf16 0.053 f16 0.004
split ringW-k320 (triple False / True alike): epi 0 bf16 0.036 f16 0.002; epi 1 bf16 0.021 f16 0.003; epi 4 bf16 0.036 f16 0.002
qkv 16640x768x192 split 512 cap 0: bf16 q|k=0.976 V^T=0.969; f16 q|k=0.855 V^T=0.865
qkv 8448x1536x320 split 1024 cap 0 and cap 8 alike: bf16 q|k=0.953 V^T=0.957; f16 q|k=0.764 V^T=0.766"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import gemm_ref as G
from gemm_gpu_util import CODE, DEV, GUARD, SENT16, TORCH, check_guards, guarded, run, tolerance

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
ERR_INVALID = -1
IDS = dict(ids=lambda c: c.name)
SMALL_ROWS = [c for c in G.CASES256 if c.tag in ("ring", "small", "cap")]
BIG_ROWS = [c for c in G.CASES256 if c.tag in ("grid", "super")]
INVARIANT_ROWS = [c for c in G.CASES256 if c.tag == "ring" or c.name in ("uneven", "two-tile")]
# (epi, 16-bit output, with bias, in place)
EVERY_EPILOGUE = [(0, True, False, False), (0, True, True, False), (1, True, True, False), (9, True, True, False),
                  (2, False, True, False), (2, False, True, True), (4, True, False, False), (4, True, True, False)]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != G.NCU256:
        pytest.skip(f"gemm_ref.CASES256 is written for {G.NCU256} CUs (runs of 3 / 2 / 1 tiles, 1024-tile threshold); this device has {ncu}")
    return get_context("cuda:0")


@contextlib.contextmanager
def launch_settings(ctx, policy, cu_cap):
    """Tile policy and workgroup cap of the context for the block, restored afterwards; each setter returns the previous value."""
    old_policy, old_cap = ctx.set_tile_policy(policy), ctx.set_gemm_cu_cap(cu_cap)
    try:
        assert ctx.set_tile_policy(policy) == policy and ctx.set_gemm_cu_cap(cu_cap) == cu_cap
        yield
    finally:
        back = ctx.set_tile_policy(old_policy), ctx.set_gemm_cu_cap(old_cap)
    assert back == (policy, cu_cap)


def _inputs(name, dtype, products):
    x = G.make_inputs(G.case(name), dtype)
    for k in ("a", "w", "bias", "resid"):
        x[k + "_d"] = x[k].to(DEV).contiguous()
    if products:
        x["u"] = G.product(x["a64"], x["w64"])
        x["s"] = G.abs_product(x["a64"], x["w64"])
    return x


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """Operands of a small case on the device, their float64 values, and the two float64 products every check of the case shares."""
    return _inputs(name, dtype, True)


@functools.lru_cache(maxsize=1)
def big_inputs(name, dtype):
    """The same for a large case, without the products (computed in row blocks by check_blocks); one case kept at a time."""
    return _inputs(name, dtype, False)


def label(c, dtype, epi, out16, with_bias, inplace):
    return f"{c.name} {dtype} epi {epi}{' 16-bit' if out16 else ' fp32'}{' +bias' if with_bias else ''}{' in place' if inplace else ''}"


def check_case(ctx, c, dtype, which):
    """The listed epilogues of a small case against gemm_ref within the tolerance, under the case's policy and cap; prints worst
    error / tolerance.  Returns the outputs."""
    x = inputs(c.name, dtype)
    outs, line = {}, []
    with launch_settings(ctx, c.policy, c.cu_cap):
        for epi, out16, with_bias, inplace in which:
            what = label(c, dtype, epi, out16, with_bias, inplace)
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


# ---------------------------------------------------------------- every epilogue over a run of tiles ------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", SMALL_ROWS, **IDS)
def test_epilogues_over_a_tile_run_vs_float64(ctx, c, dtype):
    """24 / 20 / 16 tiles on 8 workgroups (runs of 3, of 3 and 2, of 2), one tile on eight, 24 on 24: every nk % 6, both deep
    operands, every epilogue of the kernel."""
    outs = check_case(ctx, c, dtype, EVERY_EPILOGUE)
    assert torch.equal(outs[(2, False, True, True)], outs[(2, False, True, False)])       # in place: the same bits


# ---------------------------------------------------------------- the default grid and the supertile order, every element --------

def check_blocks(ctx, c, dtype, epi, out16, inplace):
    """One epilogue of a large case: every output element against the float64 reference, the reference computed in row blocks of
    A (column blocks of the transposed output) of about 8 M elements."""
    x = big_inputs(c.name, dtype)
    what = label(c, dtype, epi, out16, True, inplace)
    with launch_settings(ctx, c.policy, c.cu_cap):
        got_d = run(ctx, dtype, epi, out16, x["a_d"], x["w_d"], x["bias_d"], x["resid_d"], inplace, what)
    rows = max(256, (8 << 20) // c.N // 256 * 256)
    worst, where = 0.0, None
    for r0 in range(0, c.M, rows):
        r1 = min(c.M, r0 + rows)
        a64 = x["a64"][r0:r1]
        r64 = x["resid64"][r0:r1] if epi == 2 else None
        ref = G.epilogue(G.product(a64, x["w64"]), x["bias64"], r64, epi)
        bnd = G.bound_from(G.abs_product(a64, x["w64"]), x["bias64"], r64, x["K"])
        tol = tolerance(dtype, epi, out16, ref, bnd.T if epi == 4 else bnd)
        got = (got_d[:, r0:r1] if epi == 4 else got_d[r0:r1]).double().cpu().numpy()
        ratio = np.abs(got - ref) / tol
        if float(ratio.max()) > worst:
            i, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
            worst, where = float(ratio.max()), ((int(i), r0 + int(j)) if epi == 4 else (r0 + int(i), int(j)))
    print(f"{what} worst error / tolerance: {worst:.3f}")
    assert worst <= 1.0, f"{what}: {worst:.2f} x the tolerance at {where}"
    return got_d


@pytest.mark.parametrize("epi", [2, 4], ids=["resid-in-place", "transposed"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", BIG_ROWS, **IDS)
def test_default_grid_and_supertile_order_vs_float64(ctx, c, dtype, epi):
    """297 tiles on 256 workgroups (runs of 2 and 1, default policy and grid), and the supertile branch of tile_coords -- more than
    1024 tiles: ragged bands, skipped slots inside a run, column groups of 8 and 6, BT < GN, both orientations -- with the
    read-modify-write epilogue in place and the transposed store."""
    L = G.launch_of(c)
    assert L.balanced == (c.tag == "grid") and len({len(r) for r in L.runs}) > 1
    check_blocks(ctx, c, dtype, epi, epi == 4, epi == 2)


# ---------------------------------------------------------------- bits do not depend on the cap or on the kernel -----------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", INVARIANT_ROWS, **IDS)
def test_bits_do_not_depend_on_the_workgroup_cap_or_the_kernel(ctx, c, dtype):
    """include/sgpt_hip.h: the result of sgpt_linear does not depend on sgpt_ctx_set_gemm_cu_cap (one workgroup per tile, runs of
    3 on 8 workgroups, 24 workgroups, a cap that is no multiple of 8) nor on which kernel ran (policy 0: the register-staged
    kernel takes these shapes)."""
    x = inputs(c.name, dtype)
    assert G.linear_variant(dtype, 0, True, c.M, c.N, c.K, tile_policy=0)[0] != "256d"
    for epi, out16, with_bias in [(0, True, True), (1, True, True), (9, True, True), (2, False, True), (4, True, True)]:
        outs = {}
        for policy, cap in [(0, 0), (1, 0), (1, 8), (1, 24), (1, 100)]:
            with launch_settings(ctx, policy, cap):
                outs[(policy, cap)] = run(ctx, dtype, epi, out16, x["a_d"], x["w_d"], x["bias_d"], x["resid_d"],
                                          what=f"{c.name} {dtype} epi {epi} policy {policy} cap {cap}")
        ity = torch.int16 if out16 else torch.int32
        for key, o in outs.items():
            assert torch.equal(o.view(ity), outs[(1, 0)].view(ity)), f"{c.name} {dtype} epi {epi}: (policy, cap) {key} differs from (1, 0)"


# ---------------------------------------------------------------- split (hi + lo) store over a run --------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi,triple", [(0, False), (0, True), (1, False), (1, True), (4, False)])
@pytest.mark.parametrize("name", ["ringA-k192", "ringW-k320"])
def test_split_store_over_a_tile_run(ctx, name, epi, triple, dtype):
    """sgpt_linear_split on the 256x256 kernel, runs of 3 tiles: hi is the plain output bit for bit, the second hi copy equals hi,
    the sentinel columns behind each column block and the guards around the array are untouched, and hi + lo is the float64 value
    within the accumulation tolerance of an fp32 output (derived bound; GELU allowances) plus the two-rounding term of
    tests/test_gpu_precision.py::test_split_store_epilogues, 4 u16^2 |ref| + 2e-7 (lo = round16(v - hi), f16 subnormal floor)."""
    gap = 8                                             # keeps the 16-byte row pieces of the store aligned
    c = G.case(name)
    x = inputs(c.name, dtype)
    M, N, K = c.M, c.N, c.K
    bias_d, b64 = (x["bias_d"], x["bias64"]) if epi == 1 else (None, None)
    nblk = 3 if triple else 2
    if epi == 4:
        ldo, lo_delta, hi2_delta, total = M, N * M + GUARD, 0, 2 * N * M + GUARD
    else:
        ldo, lo_delta, hi2_delta = nblk * (N + gap), N + gap, (2 * (N + gap) if triple else 0)
        total = M * ldo
    with launch_settings(ctx, c.policy, c.cu_cap):
        plain = run(ctx, dtype, epi, True, x["a_d"], x["w_d"], bias_d, None, what="plain")
        bufs = []
        for _ in range(2):
            buf, body = guarded(total, TORCH[dtype])
            st = ctx.lib.sgpt_linear_split(ctx.handle, CODE[dtype], epi, x["a_d"].data_ptr(), x["w_d"].data_ptr(),
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
    ref = G.epilogue(x["u"], b64, None, epi)
    bnd = G.bound_from(x["s"], b64, None, K)
    u = G.U16[dtype]
    tol = tolerance(dtype, epi, False, ref, bnd.T if epi == 4 else bnd) + 4 * u * u * np.abs(ref) + 2e-7
    got = hi.double().cpu().numpy() + lo.double().cpu().numpy()
    worst = float((np.abs(got - ref) / tol).max())
    print(f"split {name} {dtype} epi {epi} triple {triple}: worst error / tolerance = {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- the f16 range tracker over a run -------------------------------

def test_range_flag_from_any_tile_of_a_run(ctx):
    """2048 x 768 x 128 on 8 workgroups: workgroup 0 walks three tiles and reports its range word once, after the last.  One
    output element of magnitude 32768 -- every other element is zero -- in the first, the middle or the last tile of that run
    raises bit 0 of sgpt_range_check (and the next read is 0); 16384 does not; neither does bf16."""
    c = G.case("ringA-k128")
    run0 = G.launch_of(c).runs[0]
    assert len(run0) == 3
    ctx.range_check()                                   # clear
    with launch_settings(ctx, c.policy, c.cu_cap):
        for dtype, value, flagged in (("f16", 32768.0, True), ("f16", 16384.0, False), ("bf16", 32768.0, False)):
            for m0, n0 in run0:
                m, n = m0 + 37, n0 + 201
                a = torch.zeros((c.M, c.K), dtype=TORCH[dtype])
                w = torch.zeros((c.N, c.K), dtype=TORCH[dtype])
                a[m, 0], w[n, 0] = value / 128.0, 128.0
                out = run(ctx, dtype, 0, True, a.to(DEV), w.to(DEV), None, None, what=f"range {dtype} {value} in tile ({m0}, {n0})")
                assert float(out[m, n]) == value and int((out != 0).sum()) == 1
                assert bool(ctx.range_check()) == flagged, f"{dtype} {value} in tile ({m0}, {n0}) of workgroup 0's run"
                assert not ctx.range_check()            # and it resets


# ---------------------------------------------------------------- the bulk fused QKV launch ---------------------------------------

QKV_SHAPES = [(16640, 768, 512, 192, 0), (8448, 1536, 1024, 320, 0), (8448, 1536, 1024, 320, 8)]      # M, N, n_split, K, cu_cap


def run_qkv(ctx, dtype, a_d, w_d, n_split, what):
    """sgpt_linear_qkv into two guarded buffers, twice: guards, no sentinel left, finite, same bits.  Returns (q|k, V^T)."""
    (M, K), N = a_d.shape, w_d.shape[0]
    kept = []
    for _ in range(2):
        (qb, q), (vb, vt) = guarded(M * n_split, TORCH[dtype]), guarded((N - n_split) * M, TORCH[dtype])
        ctx._chk(ctx.lib.sgpt_linear_qkv(ctx.handle, CODE[dtype], a_d.data_ptr(), w_d.data_ptr(), q.data_ptr(), vt.data_ptr(),
                                         n_split, M, N, K, None), f"sgpt_linear_qkv {what}")
        check_guards(qb, M * n_split, what + " q|k")
        check_guards(vb, (N - n_split) * M, what + " V^T")
        kept.append((qb, vb))
    assert torch.equal(kept[0][0], kept[1][0]) and torch.equal(kept[0][1], kept[1][1]), f"{what}: two identical calls, different bits"
    q, vt = q.view(M, n_split), vt.view(N - n_split, M)
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(vt).all()), f"{what}: not finite"
    return q, vt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,n_split,K,cu_cap", QKV_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[3]}-cap{s[4]}" for s in QKV_SHAPES])
def test_bulk_qkv_vs_float64_and_the_two_launch_form(ctx, M, N, n_split, K, cu_cap, dtype):
    """EPI_QKV on the 256x256 kernel (the launch csrc/encode.hip makes for a bulk batch): 195 tiles one per workgroup; 198 tiles one
    per workgroup and on 8 workgroups, where a run goes from q | k tiles to V tiles -- operand roles swapped -- and back while it
    prefetches.  Both outputs against float64, and bit for bit the outputs of sgpt_linear epi 0 on W[:n_split] and epi 4 on the rest."""
    L = G.tiles256(M, N, G.NCU256, cu_cap)
    is_v = [[n0 >= n_split for _, n0 in r] for r in L.runs]
    if cu_cap:
        assert any((False, True) in zip(r, r[1:]) and (True, False) in zip(r, r[1:]) for r in is_v), "no q -> V and V -> q inside one run"
    else:
        assert all(len(r) <= 1 for r in L.runs) and L.balanced
    x = G.make_inputs(G.Case256("qkv", M, N, K, 0, cu_cap, "qkv"), dtype)
    a_d, w_d = x["a"].to(DEV), x["w"].to(DEV)
    with launch_settings(ctx, 0, cu_cap):
        q, vt = run_qkv(ctx, dtype, a_d, w_d, n_split, f"{M}x{N}x{K} {dtype} cap {cu_cap}")
        q2 = run(ctx, dtype, 0, True, a_d, w_d[:n_split].contiguous(), None, None, what="q|k launch")
        vt2 = run(ctx, dtype, 4, True, a_d, w_d[n_split:].contiguous(), None, None, what="V^T launch")
    assert torch.equal(q.view(torch.int16), q2.view(torch.int16)), "q | k differs from sgpt_linear epi 0"
    assert torch.equal(vt.view(torch.int16), vt2.view(torch.int16)), "V^T differs from sgpt_linear epi 4"
    line = []
    for got_d, w64, epi in ((q, x["w64"][:n_split], 0), (vt, x["w64"][n_split:], 4)):
        ref = G.epilogue(G.product(x["a64"], w64), None, None, epi)
        bnd = G.bound_from(G.abs_product(x["a64"], w64), None, None, K)
        ratio = np.abs(got_d.double().cpu().numpy() - ref) / tolerance(dtype, epi, True, ref, bnd.T if epi == 4 else bnd)
        line.append(f"{'V^T' if epi == 4 else 'q|k'}={float(ratio.max()):.3f}")
        assert float(ratio.max()) <= 1.0, f"{'V^T' if epi == 4 else 'q|k'}: {float(ratio.max()):.2f} x the tolerance"
    print(f"qkv {M}x{N}x{K} split {n_split} cap {cu_cap} {dtype} worst error / tolerance: {' '.join(line)}")


@pytest.mark.parametrize("M,N,n_split,K", [(16640, 768, 384, 192), (16640, 768, 768, 192), (8192, 768, 512, 192), (16640, 768, 512, 64)],
                         ids=["n_split % 256", "n_split >= N", "too few q|k tiles", "K = 64"])
def test_bulk_qkv_refusals_leave_both_outputs_untouched(ctx, M, N, n_split, K):
    a_d = torch.ones((M, K), dtype=torch.float16, device=DEV)
    w_d = torch.ones((N, K), dtype=torch.float16, device=DEV)
    (qb, q), (vb, vt) = guarded(M * n_split, torch.float16), guarded(max(N - n_split, 256) * M, torch.float16)
    before = qb.clone(), vb.clone()
    for policy in (0, 1):
        with launch_settings(ctx, policy, 0):
            st = ctx.lib.sgpt_linear_qkv(ctx.handle, CODE["f16"], a_d.data_ptr(), w_d.data_ptr(), q.data_ptr(), vt.data_ptr(), n_split, M, N, K, None)
        assert st == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(qb, before[0]) and torch.equal(vb, before[1])
