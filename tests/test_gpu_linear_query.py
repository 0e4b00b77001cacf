"""-m gpu: the query- and mid-sized projection kernels (qgemm_kernel of csrc/qgemm.hip, the entry sgpt_linear_query) per tile and
ring depth -- every plain tile from 32x16 to 128x128 in each depth class it has, with a ring of exactly one group (K / stage == D:
the re-arm loop never runs) and of two or three, whole, ragged and single ragged row tiles, workgroup lists shorter than the eight
XCDs and of 8 c0 + rem, every epilogue the entry reaches (store with and without bias, bias + GELU, bias + residual out of place
and in place, q | k | V^T with and without bias and n_split on a tile boundary); the LayerNorm-prologue tiles at d = 512 / 768 /
1024 with ragged row tiles, several column tiles per workgroup (short last group, n_split inside a group, more than 1024 bias
floats per workgroup); the f16 range word from a ragged row tile and from a V^T tile -- against the float64 reference and the
DERIVED bound of tests/gemm_ref.py, with the tolerances of tests/gemm_gpu_util.py unchanged.

The tile is forced per context (sgpt_ctx_set_query_tile), so a case knows which instantiation it ran; the shapes are
gemm_ref.CASESQ, and tests/test_gemm_ref.py shows without a GPU that the mirror of the launcher gives each case the tile, depth and
group it states and that each case shows the edges it is listed for.  Only the column groups of the prologue cases depend on the
CU count (256: the tests skip on another device, like tests/test_gpu_linear_256.py).

Every call is made twice into fresh buffers and must return the same bits.  An output lives in a buffer of the sentinel NaN
pattern with 64 elements in front and 128 spare ROWS behind it: every element of the problem must be written, nothing else.  The
entry's outputs are dense (ldo = N or n_split, ldo2 = M -- it takes no leading dimensions), so there are no spare columns: a
store to a token row >= M of a ragged row tile lands in the spare rows behind the row-major output, and in V^T[n][M ..] = the
start of row n + 1 -- for the last V row the spare rows again, which is where an unguarded store of the V^T epilogue shows.
Every result is also bit for bit that of sgpt_linear on the same operands (q | k and V^T: of its store on the two row blocks of
W): each kernel feeds an output element the k-ascending MFMA chain.

Worst error / tolerance per case is printed under `-s` (lines starting with `Q `).  First run on an MI355X (256 CUs), worst over
the shapes of a (tile, depth): every case passed.  fp32 output (bias + residual, out of place and in place): at most 0.003 of the
bound on every tile and depth, either format.  16-bit outputs, where the one rounding to the output format is most of the
tolerance -- store with / without bias, q | k | V^T with / without bias (the same figures: the same values), bias + GELU:
  bf16  32x16 D6 0.68 / 0.66 / 0.61, D4 0.71 / 0.74 / 0.67; 32x32 D6 0.80 / 0.81 / 0.77, D4 0.87 / 0.86 / 0.84; 32x64 D6 0.81 / 0.81 /
        0.76, D4 0.89 / 0.89 / 0.86; 64x32 D6 0.82 / 0.81 / 0.76, D4 0.89 / 0.86 / 0.84; 64x64 D6 0.81 / 0.81 / 0.76, D4 0.88 / 0.89 / 0.84;
        128x64 D3 0.92 / 0.94 / 0.89, D2 0.95 / 0.95 / 0.89; 128x128 D2 0.95 / 0.95 / 0.90
  f16   32x16 D6 0.21 / 0.21 / 0.19, D4 0.35 / 0.32 / 0.32; 32x32 D6 0.36 / 0.36 / 0.32, D4 0.56 / 0.54 / 0.51; 32x64 D6 0.40 / 0.36 /
        0.37, D4 0.56 / 0.56 / 0.51; 64x32 D6 0.46 / 0.36 / 0.32, D4 0.56 / 0.55 / 0.51; 64x64 D6 0.45 / 0.50 / 0.37, D4 0.56 / 0.56 / 0.51;
        128x64 D3 0.67 / 0.68 / 0.59, D2 0.79 / 0.78 / 0.72; 128x128 D2 0.82 / 0.78 / 0.75
  LayerNorm prologue (q | k | V^T with bias / without / bias + GELU): bf16 32x32 D6 0.84 / 0.84 / 0.79, D4 0.85 / 0.90 / 0.79; 32x64
        D6 0.83 / 0.82 / 0.79, D4 0.92 / 0.90 / 0.89; 64x64 D6 0.85 / 0.85 / 0.80, D4 0.88 / 0.89 / 0.84; f16 32x32 D6 0.41 / 0.42 /
        0.37, D4 0.60 / 0.58 / 0.55; 32x64 D6 0.41 / 0.40 / 0.36, D4 0.62 / 0.58 / 0.57; 64x64 D6 0.41 / 0.42 / 0.38, D4 0.60 / 0.59 / 0.55
No bit differed from sgpt_linear, between two calls, or between the prologue and the plain tile; no sentinel was touched or left.

Not reachable through sgpt_linear_query, so not covered here: the 128x128 class-4 instantiation (D = 2 in both classes and q_class
answers 6 whenever it answers: never launched); the prologue's NV / SIX pairs the dispatch does not form (NV = 3 only with d =
768 = SIX, NV = 4 only with d = 512 / 1024 = not SIX); the fp32-out store (the entry writes the operand format for epi 0); ln_mul
other than 1 (sgpt_encode passes 2^-k under a range shift) and leading dimensions other than the dense K / N / n_split / M the
entry sets: those two are reached through sgpt_encode alone, whose end-to-end tests (tests/test_gpu_encode.py) are their only
cover."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import gemm_ref as G
from gemm_gpu_util import CODE, DEV, GUARD, SENT16, SENT32, TORCH, run, tolerance

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
ERR_INVALID = -1
TAIL_ROWS = 128                                        # spare rows behind an output: more than any row tile can overshoot
EPS = 1e-5
QKV = G.EPI_QKV
# (epi, with bias, in place)
PLAIN_EPILOGUES = [(0, True, False), (0, False, False), (1, True, False), (2, True, False), (2, True, True), (QKV, True, False), (QKV, False, False)]
LN_EPILOGUES = [(QKV, True, False), (QKV, False, False), (1, True, False)]
PLAIN_ROWS = {(k, D): [c for c in G.CASESQ if c.tag == "plain" and (c.tile, c.D) == (k, D)] for k, _, _, _, _, D, _, _ in G.Q_PLAIN}
LN_ROWS = [c for c in G.CASESQ if c.ln]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != G.NCU256:
        pytest.skip(f"gemm_ref.CASESQ is written for {G.NCU256} CUs (column tiles per workgroup of the LayerNorm-prologue cases); this device has {ncu}")
    return get_context("cuda:0")


@contextlib.contextmanager
def forced_tile(ctx, k):
    """The context's query tile for the block, restored afterwards; the setter returns the previous value."""
    old = ctx.set_query_tile(k)
    assert old >= 0
    try:
        assert ctx.set_query_tile(k) == k
        yield
    finally:
        back = ctx.set_query_tile(old)
    assert back == k


# ---------------------------------------------------------------- buffers and the twice-called entry ------------------------------

def qbuffer(rows, cols, out_t, init=None):
    """[GUARD | rows x cols | TAIL_ROWS x cols] as integers, everything the sentinel; the middle also as a view of the output type."""
    ity, sent = (torch.int32, SENT32) if out_t == torch.float32 else (torch.int16, SENT16)
    buf = torch.full((GUARD + (rows + TAIL_ROWS) * cols,), sent, dtype=ity, device=DEV)
    body = buf[GUARD:GUARD + rows * cols].view(out_t).view(rows, cols)
    if init is not None:
        body.copy_(init)
    return buf, body


def check_qbuffer(buf, n, what):
    sent = SENT32 if buf.dtype == torch.int32 else SENT16
    assert bool((buf[:GUARD] == sent).all()), f"{what}: a store in front of the output"
    assert bool((buf[GUARD + n:] == sent).all()), f"{what}: a store behind the output (a token row >= M)"
    assert not bool((buf[GUARD:GUARD + n] == sent).any()), f"{what}: an element of the output was left unwritten"


def _ptr(t):
    return None if t is None else t.data_ptr()


def query(ctx, dtype, epi, w_d, a_d=None, x_d=None, ln=None, bias_d=None, resid_d=None, inplace=False, n_split=0, what="", expect=0):
    """sgpt_linear_query into sentinel buffers, twice: status, guards, no sentinel left, finite, same bits.  Returns the output, or
    (q | k, V^T) for epi 7.  expect = ERR_INVALID: the call must be refused and leave both buffers untouched."""
    src = a_d if a_d is not None else x_d
    (M, K), N = src.shape, w_d.shape[0]
    out_t = torch.float32 if epi == 2 else TORCH[dtype]
    kept = []
    for _ in range(2):
        ob, out = qbuffer(M, n_split if epi == QKV else N, out_t, init=resid_d if (epi == 2 and inplace) else None)
        vb, vt = qbuffer(N - n_split, M, out_t) if epi == QKV else (None, None)
        resid_p = None if epi != 2 else (out.data_ptr() if inplace else resid_d.data_ptr())
        gamma, beta = ln if ln is not None else (None, None)
        st = ctx.lib.sgpt_linear_query(ctx.handle, CODE[dtype], epi, _ptr(a_d), _ptr(x_d), _ptr(gamma), _ptr(beta), EPS, w_d.data_ptr(),
                                       _ptr(bias_d), resid_p, out.data_ptr(), _ptr(vt), n_split, M, N, K, None)
        if expect != 0:
            assert st == expect, f"{what}: status {st}"
            torch.cuda.synchronize()
            sent = SENT32 if ob.dtype == torch.int32 else SENT16
            assert bool((ob == sent).all()) and (vb is None or bool((vb == sent).all())), f"{what}: a refused call wrote"
            return None
        ctx._chk(st, f"sgpt_linear_query {what}")
        check_qbuffer(ob, out.numel(), what + (" q|k" if epi == QKV else ""))
        if epi == QKV:
            check_qbuffer(vb, vt.numel(), what + " V^T")
        kept.append((ob, vb))
    assert torch.equal(kept[0][0], kept[1][0]) and (epi != QKV or torch.equal(kept[0][1], kept[1][1])), f"{what}: two identical calls, different bits"
    assert bool(torch.isfinite(out).all()) and (vt is None or bool(torch.isfinite(vt).all())), f"{what}: not finite"
    return (out, vt) if epi == QKV else out


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------- operands and float64 references, shared ------------------------

@functools.lru_cache(maxsize=48)
def plain_inputs(M, N, K, dtype):
    """Operands of an M x N x K problem on the device (gemm_ref.make_inputs: exact in the operand format), the float64 bias and
    residual, and the two float64 products every epilogue, tile and depth at this shape shares."""
    x = G.make_inputs(G.CaseQ("shape", M, N, K, 0, False, 0, 0, 0, 0, 0, 1, frozenset(), "shape"), dtype)
    out = {k + "_d": x[k].to(DEV).contiguous() for k in ("a", "w", "bias", "resid")}
    out.update(bias64=x["bias64"], resid64=x["resid64"], K=K, u=G.product(x["a64"], x["w64"]), s=G.abs_product(x["a64"], x["w64"]))
    return out


def ratio_of(got_d, ref, tol):
    r = np.abs(got_d.double().cpu().numpy() - ref) / tol
    return float(r.max()), np.unravel_index(int(r.argmax()), r.shape)


def check_against_float64(x, dtype, epi, with_bias, n_split, got, what):
    """One epilogue's result against the float64 value within tests/gemm_gpu_util.tolerance; returns the worst error / tolerance
    (q | k | V^T: of both outputs)."""
    b64 = x["bias64"] if with_bias else None
    if epi == QKV:
        worst = 0.0
        for part, cols, vt in ((got[0], slice(0, n_split), False), (got[1], slice(n_split, None), True)):
            pb = None if b64 is None else b64[cols]
            ref = G.epilogue(x["u"][:, cols], pb, None, G.EPI_VT if vt else G.EPI_STORE)
            bnd = G.bound_from(x["s"][:, cols], pb, None, x["K"])
            w, at = ratio_of(part, ref, tolerance(dtype, G.EPI_VT if vt else 0, True, ref, bnd.T if vt else bnd))
            assert w <= 1.0, f"{what} {'V^T' if vt else 'q|k'}: {w:.2f} x the tolerance at {at}"
            worst = max(worst, w)
        return worst
    r64 = x["resid64"] if epi == 2 else None
    ref = G.epilogue(x["u"], b64, r64, epi)
    w, at = ratio_of(got, ref, tolerance(dtype, epi, epi != 2, ref, G.bound_from(x["s"], b64, r64, x["K"])))
    assert w <= 1.0, f"{what}: {w:.2f} x the tolerance at {at}"
    return w


def check_against_sgpt_linear(ctx, x, dtype, epi, with_bias, n_split, got, what, a_d=None):
    """Bit for bit the bulk entry's result on the same operands (q | k | V^T: its store on W[:n_split] and, transposed, on the rest --
    sgpt_linear's own transposed store needs M % 128 == 0)."""
    a_d = x["a_d"] if a_d is None else a_d
    bias_d = x["bias_d"] if with_bias else None
    if epi == QKV:
        for part, cols, vt in ((got[0], slice(0, n_split), False), (got[1], slice(n_split, None), True)):
            want = run(ctx, dtype, 0, True, a_d, x["w_d"][cols].contiguous(), None if bias_d is None else bias_d[cols].contiguous(), None,
                       what=what + " sgpt_linear")
            assert torch.equal(bits(part), bits(want.T if vt else want)), f"{what} {'V^T' if vt else 'q|k'}: not the bits of sgpt_linear"
        return
    want = run(ctx, dtype, epi, epi != 2, a_d, x["w_d"], bias_d, x["resid_d"], what=what + " sgpt_linear")
    assert torch.equal(bits(got), bits(want)), f"{what}: not the bits of sgpt_linear"


def tag(epi, with_bias, inplace):
    return f"{epi}{'b' if with_bias else ''}{'i' if inplace else ''}"


# ---------------------------------------------------------------- the plain kernels: every tile, depth class and ring length ------

def check_plain_case(ctx, c, dtype):
    x = plain_inputs(c.M, c.N, c.K, dtype)
    line = []
    with forced_tile(ctx, c.tile):
        for epi, with_bias, inplace in PLAIN_EPILOGUES:
            what = f"{c.name} {dtype} epi {tag(epi, with_bias, inplace)}"
            ns = c.n_split if epi == QKV else 0
            got = query(ctx, dtype, epi, x["w_d"], a_d=x["a_d"], bias_d=x["bias_d"] if with_bias else None, resid_d=x["resid_d"], inplace=inplace,
                        n_split=ns, what=what)
            line.append(f"{tag(epi, with_bias, inplace)}={check_against_float64(x, dtype, epi, with_bias, ns, got, what):.3f}")
            check_against_sgpt_linear(ctx, x, dtype, epi, with_bias, ns, got, what)
    print(f"Q {c.bm}x{c.bn} D{c.D} {dtype} {c.name} worst error / tolerance: {' '.join(line)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", sorted(PLAIN_ROWS), ids=lambda k: "{}x{}-D{}".format(*G.Q_TILES[k[0] - 1][:2], k[1]))
def test_plain_tile_at_each_depth_and_ring_length_vs_float64(ctx, key, dtype):
    """One forced tile in one depth class: K of one ring group and of two or three, both M of gemm_ref.Q_ROWS (32-row tiles: 32 and
    96; 64-row: 96 = a whole and a ragged tile, and 64; 128-row: 160 and 64 = one ragged tile), both N of gemm_ref.Q_COLS (fewer
    workgroups than XCDs; 8 c0 + rem), every epilogue."""
    rows = PLAIN_ROWS[key]
    assert len(rows) == 8
    for c in rows:
        check_plain_case(ctx, c, dtype)


# ---------------------------------------------------------------- the LayerNorm prologue ------------------------------------------

def ln_inputs(ctx, c, dtype):
    """x fp32 [M, d] with a row offset and spread, gamma and beta; a = the context's LayerNorm of x in the operand format (its own
    float64 test: tests/test_gpu_rowops.py) -- the operand whose float64 value the products are taken of; w, bias from make_inputs."""
    rng = np.random.default_rng([7, c.M, c.N, c.K])
    x_d = torch.from_numpy((rng.standard_normal((c.M, c.K)) * 3.0 + 0.5).astype(np.float32)).to(DEV)
    gamma = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(c.K)).astype(np.float32)).to(DEV)
    beta = torch.from_numpy((0.1 * rng.standard_normal(c.K)).astype(np.float32)).to(DEV)
    a_d = ctx.layernorm(x_d, gamma, beta, EPS, out_dtype=TORCH[dtype])
    m = G.make_inputs(c, dtype)
    a64 = a_d.double().cpu().numpy()
    return dict(x_d=x_d, ln=(gamma, beta), a_d=a_d, w_d=m["w"].to(DEV).contiguous(), bias_d=m["bias"].to(DEV), resid_d=None, bias64=m["bias64"],
                K=c.K, u=G.product(a64, m["w64"]), s=G.abs_product(a64, m["w64"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", LN_ROWS, ids=lambda c: c.name)
def test_layernorm_prologue_vs_the_plain_tile_and_float64(ctx, c, dtype):
    """linear_query(x, ln) on a forced prologue tile: bit for bit linear_query(a = layernorm(x)) on the plain tile of the same size
    (which is bit for bit sgpt_linear), and within the float64 bound of linear_ref(a, ...) -- q | k | V^T with and without bias and
    bias + GELU (the 4096-row case: GELU and q | k | V^T with bias)."""
    x = ln_inputs(ctx, c, dtype)
    L = G.launch_q(c)
    assert (L.bm, L.bn, L.D, L.group) == (c.bm, c.bn, c.D, c.group)
    line = []
    for epi, with_bias, _ in (LN_EPILOGUES if c.M < 4096 else [(1, True, False), (QKV, True, False)]):
        what = f"{c.name} {dtype} epi {tag(epi, with_bias, False)}"
        ns = c.n_split if epi == QKV else 0
        bias_d = x["bias_d"] if with_bias else None
        with forced_tile(ctx, c.tile):
            got = query(ctx, dtype, epi, x["w_d"], x_d=x["x_d"], ln=x["ln"], bias_d=bias_d, n_split=ns, what=what + " prologue")
        with forced_tile(ctx, G.Q_LN_AS_PLAIN[c.tile]):
            plain = query(ctx, dtype, epi, x["w_d"], a_d=x["a_d"], bias_d=bias_d, n_split=ns, what=what + " plain")
        for g, p in zip(got if epi == QKV else (got,), plain if epi == QKV else (plain,)):
            assert torch.equal(bits(g), bits(p)), f"{what}: the prologue's result is not the plain tile's on layernorm(x)"
        line.append(f"{tag(epi, with_bias, False)}={check_against_float64(x, dtype, epi, with_bias, ns, got, what):.3f}")
        check_against_sgpt_linear(ctx, x, dtype, epi, with_bias, ns, plain, what, a_d=x["a_d"])
    print(f"Q ln{c.bm}x{c.bn} D{c.D} G{c.group} {dtype} {c.name} worst error / tolerance: {' '.join(line)}")


def test_prologue_tile_beyond_the_lds_limit_is_refused(ctx):
    """64x64 at d = 1024: 128 KiB of A panel, 32 KiB of ring and the bias exceed 160 KiB -- refused, nothing written; the same shape on
    the launcher's own choice and the same tile at d = 768 are served."""
    tile, M, N, d, ns = G.Q_LN_REFUSED
    x_d = torch.ones((M, d), device=DEV)
    gamma, beta = torch.ones((d,), device=DEV), torch.zeros((d,), device=DEV)
    w_d = torch.ones((N, d), dtype=torch.float16, device=DEV)
    with forced_tile(ctx, tile):
        query(ctx, "f16", QKV, w_d, x_d=x_d, ln=(gamma, beta), n_split=ns, what="64x64 d=1024", expect=ERR_INVALID)
        assert "not served" in ctx.lib.sgpt_last_error(ctx.handle).decode()
    x_d[:, ::2] = -1.0
    query(ctx, "f16", QKV, w_d, x_d=x_d, ln=(gamma, beta), n_split=ns, what="d=1024, the launcher's choice")


# ---------------------------------------------------------------- the knob ---------------------------------------------------------

def test_query_tile_knob_and_refusals_of_a_forced_tile(ctx):
    """The setter returns the previous value, refuses k outside 0 .. 7 with -1 and no change; a forced tile that does not serve the
    shape is the entry's "not served" with nothing launched (the refusals gemm_ref.q_launch mirrors)."""
    assert ctx.set_query_tile(0) == 0
    assert ctx.set_query_tile(3) == 0 and ctx.set_query_tile(8) == -1 and ctx.set_query_tile(-1) == -1 and ctx.set_query_tile(0) == 3
    for M, N, K, epi, ns, ln, k in [(32, 128, 768, 0, 0, False, 5), (96, 96, 768, 0, 0, False, 5), (96, 128, 768, 0, 0, False, 1),
                                    (96, 128, 768, QKV, 32, False, 5), (96, 192, 768, QKV, 128, True, 4)]:
        assert G.q_launch(M, N, K, epi, ns, ln, k) is None and G.q_launch(M, N, K, epi, ns, ln, 0) is not None
        w_d = torch.ones((N, K), dtype=torch.bfloat16, device=DEV)
        a_d = torch.ones((M, K), dtype=torch.bfloat16, device=DEV)
        x_d, lnp = (torch.ones((M, K), device=DEV), (torch.ones((K,), device=DEV), torch.zeros((K,), device=DEV))) if ln else (None, None)
        with forced_tile(ctx, k):
            query(ctx, "bf16", epi, w_d, a_d=None if ln else a_d, x_d=x_d, ln=lnp, n_split=ns, what=f"{M}x{N}x{K} tile {k}", expect=ERR_INVALID)
        if ln:
            x_d[:, ::2] = -1.0
        query(ctx, "bf16", epi, w_d, a_d=None if ln else a_d, x_d=x_d, ln=lnp, n_split=ns, what=f"{M}x{N}x{K} tile 0")


# ---------------------------------------------------------------- the f16 range word ----------------------------------------------

RANGE_SHAPES = [(1, 96, 64, 1024, 32), (2, 96, 64, 512, 32), (3, 96, 128, 512, 64), (4, 96, 64, 512, 32), (5, 96, 128, 512, 64),
                (6, 160, 128, 256, 64), (6, 64, 128, 256, 64), (7, 160, 256, 256, 128)]       # forced tile, M, N, K, n_split


@pytest.mark.parametrize("k,M,N,K,ns", RANGE_SHAPES, ids=[f"tile{s[0]}-{s[1]}x{s[2]}" for s in RANGE_SHAPES])
def test_f16_range_word_from_a_ragged_row_tile_and_from_a_vt_tile(ctx, k, M, N, K, ns):
    """One output element of magnitude 32768, every other zero, at the last token row -- in the last, on the 64- and 128-row tiles
    ragged, row tile -- and the last column: through the row-major store, and (the column being a V column) through the V^T tile of
    the q | k | V^T launch.  Either raises bit 0 of sgpt_range_check, which then reads 0 again; 16384 does not; bf16 never does."""
    bm = G.Q_TILES[k - 1][0]
    assert G.q_launch(M, N, K, QKV, ns, False, k) is not None and (bm == 32 or M % bm != 0)
    ctx.range_check()                                   # clear
    with forced_tile(ctx, k):
        for dtype, value, flagged in (("f16", 32768.0, True), ("f16", 16384.0, False), ("bf16", 32768.0, False)):
            a = torch.zeros((M, K), dtype=TORCH[dtype])
            w = torch.zeros((N, K), dtype=TORCH[dtype])
            a[M - 1, 0], w[N - 1, 0] = value / 128.0, 128.0
            a_d, w_d = a.to(DEV), w.to(DEV)
            out = query(ctx, dtype, 0, w_d, a_d=a_d, what=f"range {dtype} {value} store")
            assert float(out[M - 1, N - 1]) == value and int((out != 0).sum()) == 1
            assert bool(ctx.range_check()) == flagged, f"{dtype} {value} in the last row tile"
            assert not ctx.range_check()                # and it resets
            qk, vt = query(ctx, dtype, QKV, w_d, a_d=a_d, n_split=ns, what=f"range {dtype} {value} qkv")
            assert float(vt[N - ns - 1, M - 1]) == value and int((vt != 0).sum()) == 1 and int((qk != 0).sum()) == 0
            assert bool(ctx.range_check()) == flagged, f"{dtype} {value} in a V^T tile"
            assert not ctx.range_check()


# ---------------------------------------------------------------- the knob stops at sgpt_linear_query ------------------------------

def test_encode_does_not_read_the_query_tile(ctx):
    """sgpt_encode treats a refused query launch as an error, so the test knob must not reach it: with tile 7 forced (128x128, which
    refuses a 32-row layout and N = 768 * 3 with n_split off its boundary) a one-query encode at SGPT-125M width succeeds and
    returns the bits it returns with the knob at 0."""
    from oracle import sgpt_oracle as O
    from sgpt_amd import SGPTConfig, SGPTModel
    kw = dict(vocab_size=211, max_position_embeddings=96, hidden_size=768, num_layers=2, num_heads=12, window_size=8)
    model = SGPTModel(SGPTConfig(**kw), O.synth_weights(O.NeoConfig(**kw), seed=12, std=0.03), device="cuda:0", dtype="f16", ctx=ctx)
    try:
        seqs = [np.random.default_rng(3).integers(0, 211, size=18).tolist()]
        pb = model.pack(seqs)
        assert pb.T_pad == 32 and G.q_launch(32, 2304, 768, QKV, 1536, True, 7) is None and G.q_launch(32, 768, 768, 0, 0, False, 7) is None
        want = model.encode_packed(pb, normalize=True)
        with forced_tile(ctx, 7):
            got = model.encode_packed(pb, normalize=True)
        assert torch.equal(got, want)
    finally:
        model.close()
