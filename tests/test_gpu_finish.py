"""-m gpu: the kernels that finish an embedding (csrc/elementwise.hip: pool_kernel, l2norm_kernel, pairwise_kernel, cvt16_kernel,
crest16_kernel), each launched alone through its C-ABI entry and compared with the float64 restatement of the same operation
on the same inputs (tests/finish_ref.py, pinned on the CPU by tests/test_finish_ref.py, which also proves every bound used here
on every input used here with an fp32 emulation of the kernel's own summation order).  Every output is allocated with one extra
row / 64 extra elements of a sentinel that must survive the call; every bounded case prints its worst `error / bound` on a line
beginning "finish:" (visible with -s / -rA).

What the golden-fixture tests of test_gpu_kernels.py cannot see and these can: f16 hidden states, lasttoken / cls off the
fixtures, masks with holes, the second blockIdx.y column block of the pooling kernel; column tails and short last workgroups of
the one-wave-per-row kernels; the rounding mode, the subnormals, the overflow edge and the grid-stride second pass of the
16-bit conversion; the value of the crest factor; and what every entry does with arguments it must refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

import finish_ref as F

pytestmark = pytest.mark.gpu

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"f32": 0, "bf16": 1, "f16": 3}                       # element-type codes of include/sgpt_hip.h
SGPT_ERR_INVALID = -1
SENTINEL = 77.0                                             # a value of all three formats


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def dev16(bits, fmt):
    return dev(np.ascontiguousarray(bits).view(np.int16)).view(HALF[fmt])


def bits16(t) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bits32(t) -> np.ndarray:
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def host64(t) -> np.ndarray:
    return t.detach().to("cpu", torch.float64).numpy()


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)


ratio = F.ratio                                             # max err / bound; inf as soon as anything in it is not finite


def report(what, r):
    print(f"finish: {what}: worst error / bound = {r:.3f}")
    return r


def untouched(t) -> bool:
    return bool((t == SENTINEL).all())


# ================================================================================================================ pooling
def raw_pool(ctx, hidden, fmt, mask, mode, pw, out):
    B, S, d = hidden.shape
    if mode == "learntmean":
        st = ctx.lib.sgpt_pool_learnt(ctx.handle, ptr(hidden), DT[fmt], ptr(mask), B, S, d, ptr(pw), ptr(out), stream())
    else:
        st = ctx.lib.sgpt_pool(ctx.handle, ptr(hidden), DT[fmt], ptr(mask), B, S, d, F.POOL_MODES.index(mode), ptr(out), stream())
    ctx._chk(st, f"pool {mode}")


@pytest.mark.parametrize("S", F.POOL_S)
@pytest.mark.parametrize("d", F.POOL_D)
def test_pool_every_mode_format_and_mask_kind(ctx, d, S):
    """B = 6, one mask of each kind (full, first only, last only, a middle run, holes, all zero), large finite values under the
    mask.  weightedmean / mean / learntmean (weights in [0.5, 1.5], the table longer than S): |got - ref| <= 2^-23 (S + 4)
    sum_t |w_t h_t| / den [+ 2^-23 S |ref| learntmean] (finish_ref.pool_bound), the all-zero row exact zeros.  lasttoken / cls:
    the bits of the selected input row, widened to fp32."""
    assert F.POOL_MODES.index("learntmean") == 3 and F.POOL_MODES.index("cls") == 4
    for fmt in F.POOL_FMTS:
        h, hb, mask, pw = F.pool_inputs(d, S, fmt)
        hd = dev(h) if hb is None else dev16(hb, fmt)
        md, pwd = dev(mask), dev(pw)
        worst = 0.0
        for mode in F.POOL_MODES:
            out = torch.full((7, d), SENTINEL, dtype=torch.float32, device="cuda:0")
            raw_pool(ctx, hd, fmt, md, mode, pwd, out)
            assert untouched(out[6]), f"{fmt} {mode}: the row past B was written"
            ref = F.pool(h, mask, mode, pw)
            if mode in ("lasttoken", "cls"):
                assert np.array_equal(bits32(out[:6]), ref.astype(np.float32).view(np.uint32)), f"{fmt} {mode}: not the bits of the input row"
                continue
            got = host64(out[:6])
            assert not got[5].any(), f"{fmt} {mode}: the all-zero mask does not pool to zeros"
            worst = max(worst, ratio(np.abs(got - ref), F.pool_bound(h, mask, mode, pw)))
        assert report(f"pool {fmt} d={d} S={S}", worst) <= 1.0
        # the Context method is the same launch
        assert np.array_equal(bits32(ctx.pool(hd, md, "cls")), bits32(out[:6]))
        raw_pool(ctx, hd, fmt, md, "learntmean", pwd, out)
        assert np.array_equal(bits32(ctx.pool(hd, md, "learntmean", position_weights=pwd)), bits32(out[:6]))


# =========================================================================================================== L2 normalise
def raw_l2(ctx, x, n, d, out, fmt):
    ctx._chk(ctx.lib.sgpt_l2_normalize(ctx.handle, ptr(x), n, d, ptr(out), DT[fmt], stream()), "sgpt_l2_normalize")


@pytest.mark.parametrize("n", F.ROW_N)
@pytest.mark.parametrize("d", F.ROW_D)
def test_l2_normalize_tails_formats_and_in_place(ctx, d, n):
    """fp32: |got - ref| <= 2^-24 (ceil(d / 64) / 2 + 8) |ref| (finish_ref.l2_bound), the zero row exact zeros.  bf16 / f16: the
    same call's fp32 output rounded once, bit for bit (both instantiations do the same fp32 arithmetic).  fp32 with out == in:
    the bits of the out-of-place call."""
    worst = 0.0
    for fam in F.l2_families(d):
        x = F.l2_inputs(n, d, fam)
        xd = dev(x)
        out = torch.full((n + 1, d), SENTINEL, dtype=torch.float32, device="cuda:0")
        raw_l2(ctx, xd, n, d, out, "f32")
        assert untouched(out[n]), f"{fam}: the row past n was written"
        got = host64(out[:n])
        if fam == "zero_row":
            assert not got[-1].any()
        worst = max(worst, ratio(np.abs(got - F.l2_normalize(x)), F.l2_bound(x)))
        got32 = out[:n].cpu().numpy()
        for fmt in F.FMTS16:
            o16 = torch.full((n + 1, d), SENTINEL, dtype=HALF[fmt], device="cuda:0")
            raw_l2(ctx, xd, n, d, o16, fmt)
            assert untouched(o16[n]), f"{fam} {fmt}: the row past n was written"
            assert np.array_equal(bits16(o16[:n]), F.round16(got32, fmt)), f"{fam}: the {fmt} output is not the fp32 output rounded once"
        buf = torch.full((n + 1, d), SENTINEL, dtype=torch.float32, device="cuda:0")
        buf[:n] = xd
        raw_l2(ctx, buf, n, d, buf, "f32")
        assert untouched(buf[n]) and np.array_equal(bits32(buf[:n]), bits32(out[:n])), f"{fam}: in place differs from out of place"
        assert torch.equal(ctx.l2_normalize(xd), out[:n])
    assert report(f"l2_normalize n={n} d={d}", worst) <= 1.0


# ========================================================================================================= pairwise scores
@pytest.mark.parametrize("n", F.ROW_N)
@pytest.mark.parametrize("d", F.ROW_D)
def test_pairwise_dot_and_cosine(ctx, d, n):
    """Dot within 2^-24 (ceil(d / 64) + 8) sum |a_j b_j|, cosine within 2^-24 (2 ceil(d / 64) + 24) sum |â_j b̂_j| of the float64
    value in the header's order (finish_ref.pairwise); a zero row in a, in b or in both gives a cosine of exactly 0."""
    a, b, zeros = F.pairwise_inputs(n, d)
    ad, bd = dev(a), dev(b)
    for cosine in (False, True):
        out = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device="cuda:0")
        ctx._chk(ctx.lib.sgpt_pairwise_scores(ctx.handle, ptr(ad), ptr(bd), n, d, int(cosine), ptr(out), stream()), "sgpt_pairwise_scores")
        assert untouched(out[n:]), "elements past n were written"
        got = host64(out[:n])
        assert not got[zeros].any(), "a zero row does not score exactly 0"
        ref, bound = F.pairwise(a, b, cosine)
        assert report(f"pairwise {'cos' if cosine else 'dot'} n={n} d={d}", ratio(np.abs(got - ref), bound)) <= 1.0
        assert torch.equal(ctx.pairwise_scores(ad, bd, cosine), out[:n])


# ============================================================================================================= conversion
def mismatches(x, got, want, k=8) -> str:
    bad = np.nonzero(got != want)[0][:k]
    return ", ".join(f"[{i}] 0x{x.view(np.uint32)[i]:08x} -> 0x{got[i]:04x} (want 0x{want[i]:04x})" for i in bad)


@pytest.mark.parametrize("fmt", F.FMTS16)
@pytest.mark.parametrize("numel", F.CVT_NUMEL)
def test_f32_to_16_is_round_to_nearest_even_bit_for_bit(ctx, numel, fmt):
    """The edge table (ties of both parities, 16-bit and fp32 subnormals, the overflow edge, infinities, NaNs) over randn data
    across 32 binades: the patterns of finish_ref.round16 (= torch's cast, test_finish_ref.py), NaN compared as NaN.  The last
    size is past the 8192 x 256 threads of the capped grid: its tail is converted by the second pass of the grid-stride loop."""
    x = F.cvt_inputs(numel, fmt)
    xd = dev(x)
    out = torch.full((numel + 64,), SENTINEL, dtype=HALF[fmt], device="cuda:0")
    ctx._chk(ctx.lib.sgpt_f32_to_16(ctx.handle, ptr(xd), numel, ptr(out), DT[fmt], stream()), "sgpt_f32_to_16")
    assert untouched(out[numel:]), "elements past numel were written"
    got, want = bits16(out[:numel]), F.round16(x, fmt)
    assert F.same16(got, want, fmt), mismatches(x, got, want)
    assert np.array_equal(bits16(ctx.to_16(xd, HALF[fmt])), got)
    if fmt == "bf16":
        out2 = torch.full((numel + 64,), SENTINEL, dtype=torch.bfloat16, device="cuda:0")
        ctx._chk(ctx.lib.sgpt_f32_to_bf16(ctx.handle, ptr(xd), numel, ptr(out2), stream()), "sgpt_f32_to_bf16")
        assert untouched(out2[numel:]) and np.array_equal(bits16(out2[:numel]), got)


# =========================================================================================================== crest factor
def raw_crest(ctx, x16, fmt, n, d, ld) -> float:
    out = C.c_float(SENTINEL)
    ctx._chk(ctx.lib.sgpt_row_crest(ctx.handle, ptr(x16), DT[fmt], n, d, ld, C.byref(out), stream()), "sgpt_row_crest")
    return float(out.value)


@pytest.mark.parametrize("fmt", F.FMTS16)
@pytest.mark.parametrize("n", F.CREST_N)
@pytest.mark.parametrize("d", F.CREST_D)
def test_row_crest_value(ctx, d, n, fmt):
    """max over the finite, non-zero rows of max|v| / rms(v), within the relative bound 2^-24 (ceil(d / 128) + 8) of float64
    (finish_ref.row_crest).  The spike row is the last one (the n % 4 tail wave carries the answer); from n = 5 on a zero row and
    a row with an inf are there to be skipped; ld = d and ld = d + 6 with NaN in the padding columns; an all-zero matrix is 0."""
    worst = 0.0
    for pad in (0, 6):
        bits = F.crest_inputs(n, d, fmt, pad=pad)
        ref = F.row_crest(bits[:, :d], fmt)
        got = raw_crest(ctx, dev16(bits, fmt), fmt, n, d, d + pad)
        worst = max(worst, ratio(abs(got - ref), F.crest_rel_bound(d) * ref))
        zeros = F.crest_inputs(n, d, fmt, pad=pad, kind="zeros")
        assert raw_crest(ctx, dev16(zeros, fmt), fmt, n, d, d + pad) == 0.0
    assert report(f"row_crest {fmt} n={n} d={d}", worst) <= 1.0


def test_row_crest_of_fp32_rows_rounds_to_f16_first(ctx):
    """Context.row_crest: fp32 rows whose f16 rounding moves the crest by some 250 bounds (finish_ref.crest_fp32_inputs), and
    16-bit rows as they are."""
    x = F.crest_fp32_inputs()
    ref = F.row_crest(F.round16(x, "f16"), "f16")
    got = ctx.row_crest(dev(x))
    assert report("row_crest fp32 -> f16 n=5 d=130", ratio(abs(got - ref), F.crest_rel_bound(130) * ref)) <= 1.0
    for fmt in F.FMTS16:
        bits = F.crest_inputs(5, 130, fmt)
        ref = F.row_crest(bits, fmt)
        assert ratio(abs(ctx.row_crest(dev16(bits, fmt)) - ref), F.crest_rel_bound(130) * ref) <= 1.0


# ================================================================================================================ refusals
BAD_DTYPES = [-1, 2, 4, 5, 99]                              # fp8 weight / matmul codes and codes that name nothing


def test_every_entry_refuses_bad_arguments_and_writes_nothing(ctx):
    """Null pointers (the context among them), non-positive sizes, d % 4 != 0 (pool), d % 2 != 0 or ld < d (crest), a bad pool mode, mode 3 through
    sgpt_pool, dtype codes outside the formats of the entry: SGPT_ERR_INVALID, and the sentinel-filled output as it was.  Every
    condition is checked on the host before anything is launched (csrc/ops.hip, csrc/score.hip); every buffer is sized for the
    widest format, so that no case could index outside an allocation even without its check."""
    B, S, d, n = 2, 3, 8, 5
    hidden = torch.ones((B, S, d), dtype=torch.float32, device="cuda:0")
    mask = torch.ones((B, S), dtype=torch.int32, device="cuda:0")
    pw = torch.ones((S + 1,), dtype=torch.float32, device="cuda:0")
    x = torch.ones((n, d), dtype=torch.float32, device="cuda:0")
    x16 = torch.ones((n, d), dtype=torch.float16, device="cuda:0")
    out = torch.empty((n + 1, d), dtype=torch.float32, device="cuda:0")          # every entry's output: fp32-sized, one extra row
    crest = C.c_float(SENTINEL)
    lib, h, P, NULL = ctx.lib, ctx.handle, ptr, C.c_void_p(0)

    def pool(hid=hidden, dt=0, m=mask, B=B, S=S, d=d, mode=0, o=out, h=h):
        return lib.sgpt_pool(h, P(hid), dt, P(m), B, S, d, mode, P(o), stream())

    def learnt(hid=hidden, dt=0, m=mask, B=B, S=S, d=d, w=pw, o=out, h=h):
        return lib.sgpt_pool_learnt(h, P(hid), dt, P(m), B, S, d, P(w), P(o), stream())

    def l2(i=x, n=n, d=d, o=out, dt=0, h=h):
        return lib.sgpt_l2_normalize(h, P(i), n, d, P(o), dt, stream())

    def pair(a=x, b=x, n=n, d=d, cos=1, o=out, h=h):
        return lib.sgpt_pairwise_scores(h, P(a), P(b), n, d, cos, P(o), stream())

    def cvt(i=x, numel=n * d, o=out, dt=3, h=h):
        return lib.sgpt_f32_to_16(h, P(i), numel, P(o), dt, stream())

    def cvtb(i=x, numel=n * d, o=out, h=h):
        return lib.sgpt_f32_to_bf16(h, P(i), numel, P(o), stream())

    def crst(i=x16, dt=3, n=n, d=d, ld=d, o=True, h=h):
        return lib.sgpt_row_crest(h, P(i), dt, n, d, ld, C.byref(crest) if o else None, stream())

    cases = []
    for name, f in (("sgpt_pool", pool), ("sgpt_pool_learnt", learnt)):
        cases += [(name, f, kw) for kw in (dict(hid=None), dict(m=None), dict(o=None), dict(B=0), dict(B=-1), dict(S=0), dict(S=-3),
                                           dict(d=0), dict(d=-4), dict(d=6), dict(d=7))]
        cases += [(name, f, dict(dt=c)) for c in BAD_DTYPES]
    cases += [("sgpt_pool", pool, dict(mode=m)) for m in (-1, 3, 5, 99)]
    cases += [("sgpt_pool_learnt", learnt, dict(w=None))]
    cases += [("sgpt_l2_normalize", l2, kw) for kw in (dict(i=None), dict(o=None), dict(n=0), dict(n=-1), dict(d=0), dict(d=-1))]
    cases += [("sgpt_l2_normalize", l2, dict(dt=c)) for c in BAD_DTYPES]
    cases += [("sgpt_pairwise_scores", pair, kw) for kw in (dict(a=None), dict(b=None), dict(o=None), dict(n=0), dict(n=-1), dict(d=0), dict(d=-1))]
    cases += [("sgpt_f32_to_16", cvt, kw) for kw in (dict(i=None), dict(o=None), dict(numel=0), dict(numel=-1))]
    cases += [("sgpt_f32_to_16", cvt, dict(dt=c)) for c in [0] + BAD_DTYPES]
    cases += [("sgpt_f32_to_bf16", cvtb, kw) for kw in (dict(i=None), dict(o=None), dict(numel=0), dict(numel=-1))]
    cases += [("sgpt_row_crest", crst, kw) for kw in (dict(i=None), dict(o=False), dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(d=0), dict(d=-2),
                                                        dict(d=3), dict(d=7), dict(ld=d - 2), dict(ld=0))]
    cases += [("sgpt_row_crest", crst, dict(dt=c)) for c in [0] + BAD_DTYPES]
    # a null context is the first condition of every check, and fail() (csrc/host.h) stores its message only in a context that is there
    cases += [(name, f, dict(h=None)) for name, f in (("sgpt_pool", pool), ("sgpt_pool_learnt", learnt), ("sgpt_l2_normalize", l2),
                                                       ("sgpt_pairwise_scores", pair), ("sgpt_f32_to_16", cvt), ("sgpt_f32_to_bf16", cvtb),
                                                       ("sgpt_row_crest", crst))]

    # the base arguments of every entry are good ones: a refusal below comes from the one argument that was changed
    for f in (pool, learnt, l2, pair, cvt, cvtb, crst):
        assert f() == 0
    torch.cuda.synchronize()
    assert crest.value == 1.0                                                     # a flat row
    wrong = []
    for name, f, kw in cases:
        out.fill_(SENTINEL)
        crest.value = SENTINEL
        st = f(**kw)
        torch.cuda.synchronize()
        if st != SGPT_ERR_INVALID:
            wrong.append(f"{name}({kw}) returned {st}")
        elif not untouched(out) or crest.value != SENTINEL:
            wrong.append(f"{name}({kw}) wrote to its output")
        elif not ctx.lib.sgpt_last_error(ctx.handle):
            wrong.append(f"{name}({kw}) left no message")
    assert not wrong, "\n".join(wrong)
