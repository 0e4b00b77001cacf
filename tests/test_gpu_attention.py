"""The attention kernels (csrc/attn.hip) directly against the float64 reference of tests/attn_ref.py, through sgpt_attention.

Inputs.  Every q / k / v value is exact in BOTH 16-bit formats (bf16-rounded, no f16 subnormals), and the reference gets the
same values as float64: no input rounding enters the comparison.  Logits are sharp: chosen queries get "needles" -- keys
whose logit is 9-12 above the background (std ~1) through a head-dim channel only that query and that key carry -- at
  the window's last visible key (i - window + 1) and, HIGHER, the first masked key (i - window);
  the diagonal (i) and, higher, the masked key i + 1;  key 0;  both sides of 16- and 64-key tile boundaries;
for queries at fragment / tile / window edges.  Every needle gets a channel of its own (16 background channels per head,
the rest for needles); make_inputs fails a case whose heads cannot hold all of its needles, so none is ever dropped and the
longest sequences carry them to their last query.  A masked key that leaks or a visible key that is dropped then moves the
context by O(max|v|) instead of 1e-3.  Every row that belongs to no sequence -- the alignment gap behind odd lengths, the
filler rows up to T, the slack rows behind T the key tiles (64 rows) and query fragments (256 rows) may read -- holds finite
sentinels of magnitude 64..95 (v: 32x max|v| of the real tokens): any read of them as a visible key shows.  Only the rows
of real tokens are compared; rows outside every allocation and the columns past H * dh must come back untouched.  Every
call runs twice and must give identical bits.

Tolerance, 16-bit operands (u16 = 2^-8 bf16, 2^-11 f16).  The products q.k are exact in fp32 and summed in fp32; the
logits (|s| <~ 20) carry ~2^-24 relative error, i.e. ~1e-6 of relative weight.  The kernel forms e_j = 2^(t_j - m) in fp32,
sums l = sum e_j unrounded, and feeds p_j = round16(e_j) to the P.V MFMA: |p_j - e_j| <= u16 e_j, so
|sum p_j v_j / l - sum e_j v_j / l| <= u16 max|v|.  (f16: e_j below 2^-14 round to the subnormal grid, absolute 2^-25 each,
at most 2048 of them: < 0.13 u16 max|v| more.)  The context is rounded once more on store: u16 max|v|.  The online
rescaling by alpha = 2^(m_old - m_new) is fp32.  So |ctx - ref| <= (2 + 0.13 + ~0) u16 max|v| < 3 u16 max|v|, with max|v|
over the real tokens of the call -- the bound asserted (BOUND16 = 3).  out_fp8: no 16-bit store (2 u16 before the e4m3
rounding); MODE 1: hi + lo carries the context to u16^2, so hi + lo obeys the same bound with room to spare.
fp32 kernel (attn_f32_kernel): exact-fp32 fma chains over <= 514 keys, worst case n * 2^-24 ~ 3e-5, random-walk
sqrt(n) * 2^-24 ~ 1.4e-6 relative to max|v|: bound 1e-5 max|v|.
MODE 2 ("x3"): q | k, V^T and the probabilities enter as hi + lo pairs, products to ~u16^2 (the lo.lo term dropped, each
operand x represented to u16^2 |x|): logits to 3 u16^2 L with L = scale * max_ij sum_c |q_ic k_jc|; a logit error d moves
the context by <= 2 d max|v|; P.V adds 3 u16^2, the split context store u16^2, fp32 arithmetic ~2^-19.  Bound:
max|v| (u16^2 (4 + 6 L) + 2^-19) -- ~1/10 of the plain bound for bf16.  f16 adds absolute terms: a lo half below 2^-14 sits
on the subnormal grid, so an operand is represented to u16^2 |x| + 2^-25, not relatively.  On the logits that adds
2^-25 A with A = scale * max_ij sum_c (|q_ic| + |k_jc|), i.e. 2 * 2^-25 A max|v| on the context; on P.V it adds 2^-25 (the
v halves) and 2^-25 max|v| per probability over <= n keys (l >= 1).  f16 bound: the above + 2^-25 (2 A max|v| + 1 +
n max|v|), ~1/30 of the plain f16 bound at n = 700.

Branches of launch_attn_bf16 (attn_variant mirrors the rule; test_lengths_reach_every_launch_branch asserts the cases
below reach each one -- a change of the rule fails it until the mirror and the cases follow):
  short2 / short4      head_dim 64, longest allocation <= 32 / <= 64 rows: 2- / 4-wave blocks      (lengths 1..32 / 33..64)
  zz8 / zz16           head_dim 64, > 128 rows: zig-zag fragment pairs in 8- / 16-wave blocks      (129, 255, 256, 512, 700, 2048 /
                                                                                                      257, 300, 400)
  w16                  head_dim 64, > 384 rows, last 256-query block at least half full            (650)
  8w-dh64/128/256      the 8-wave 128-query default                                              (65..128, 384, 513 / dh 128 / dh 256)
  fp8-dh64/128/256     e4m3 context output (bf16), 8-wave blocks
  split-dh64/128/256   MODE 1: split-precision context, 8-wave blocks
  x3-dh64/128          MODE 2: hi + lo operands (head_dim 256 has none: refused)
(The software-pipelined variant is a build option, off: not reachable.)"""
import math
import re

import numpy as np
import pytest
import torch

from attn_ref import layout, packed_attention
from oracle import sgpt_oracle as O

HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
BOUND16 = 3.0
SLACK_ROWS = 320                       # q over-read reaches T + 255, the key tiles T + 63
VT_SLACK = 64

LENS64 = [1, 2, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 384, 400, 512, 513, 650, 700, 2048]
LENS128 = [1, 2, 17, 33, 64, 65, 127, 128, 129, 255, 256, 257, 300, 384, 400, 513, 650, 700]
LENS256 = [1, 2, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 400, 513]


def attn_variant(dh, max_alloc, out_fp8=False, x3=False, split=False):
    """Python mirror of launch_attn_bf16's choice (csrc/attn.hip, default build options)."""
    if x3 or split:
        return f"{'x3' if x3 else 'split'}-dh{dh}"
    if dh == 64 and not out_fp8 and max_alloc > 128:
        nf = (max_alloc + 15) // 16
        pairs = (nf + 1) // 2
        fit8 = pairs <= 8 or pairs % 8 == 0 or pairs % 8 >= 6
        consecutive_fit = nf % 8 == 0 or nf % 8 >= 6
        zw = 8 if fit8 else (16 if (not consecutive_fit and pairs <= 16) else 0)
        if zw:
            return f"zz{zw}"
    if dh == 64 and not out_fp8 and max_alloc > 384 and (max_alloc - 1) % 256 >= 128:
        return "w16"
    if dh == 64 and not out_fp8 and max_alloc <= 64:
        return "short2" if max_alloc <= 32 else "short4"
    return f"{'fp8' if out_fp8 else '8w'}-dh{dh}"


ALL_BRANCHES = {"short2", "short4", "zz8", "zz16", "w16", "8w-dh64", "8w-dh128", "8w-dh256", "fp8-dh64", "fp8-dh128",
                "fp8-dh256", "split-dh64", "split-dh128", "split-dh256", "x3-dh64", "x3-dh128"}


def call_lens(L):
    """The sequences of one call whose longest is L: shorter ones (1, 2, odd), and a 1-token filler at the end."""
    extra = [x for x in (1, 2, 17, 33, L // 2 + 1, L - 1) if 0 < x < L]
    return [L] + sorted(set(extra), reverse=True) + [1]


FP8_CASES = [(64, 65, 0), (64, 300, 256), (64, 513, 0), (128, 129, 0), (128, 400, 256), (256, 65, 0), (256, 300, 0)]
SPLIT_CASES = [(64, 17, 0), (64, 300, 256), (128, 129, 0), (128, 513, 256), (256, 257, 0)]
X3_CASES = [(64, 17, 0), (64, 300, 256), (64, 700, 0), (128, 65, 0), (128, 400, 256)]


def max_alloc_of(L):
    return layout(call_lens(L))[3]


def test_lengths_reach_every_launch_branch():
    reached = {}
    for L in LENS64:
        reached.setdefault(attn_variant(64, max_alloc_of(L)), []).append(L)
    for L in LENS128:
        reached.setdefault(attn_variant(128, max_alloc_of(L)), []).append(L)
    for L in LENS256:
        reached.setdefault(attn_variant(256, max_alloc_of(L)), []).append(L)
    for dh, L, _ in FP8_CASES:
        reached.setdefault(attn_variant(dh, max_alloc_of(L), out_fp8=True), []).append(L)
    for dh, L, _ in SPLIT_CASES:
        reached.setdefault(attn_variant(dh, max_alloc_of(L), split=True), []).append(L)
    for dh, L, _ in X3_CASES:
        reached.setdefault(attn_variant(dh, max_alloc_of(L), x3=True, split=True), []).append(L)
    print({k: sorted(set(v)) for k, v in sorted(reached.items())})
    assert set(reached) == ALL_BRANCHES, sorted(ALL_BRANCHES ^ set(reached))


def test_attention_wrapper_refuses_mismatched_operands():
    """Context.attention's own checks run before any device work (no GPU needed): layouts the C entry cannot see through
    its flat arguments -- an fp32 v of another leading dimension (the fp32 kernel reads v with ldq), an out of another
    dtype, operands of mixed dtypes."""
    from sgpt_amd.runtime import Context
    T, d = 32, 64
    so = torch.tensor([0, 32], dtype=torch.int32)
    q32 = torch.zeros((T, 3 * d))
    bad = {
        "fp32 v leading dimension": (q32[:, :d], q32[:, d:2 * d], torch.zeros((T, d)), torch.zeros((T, d)), "leading dimension"),
        "out dtype": (q32[:, :d], q32[:, d:2 * d], q32[:, 2 * d:], torch.zeros((T, d), dtype=torch.float16), "out has q's dtype"),
        "fp8 out of f16": (torch.zeros((T, d), dtype=torch.float16),) * 3 + (torch.zeros((T, d), dtype=torch.uint8), "out has q's dtype"),
        "mixed operands": (q32[:, :d], torch.zeros((T, 3 * d), dtype=torch.float16)[:, d:2 * d], q32[:, 2 * d:], torch.zeros((T, d)),
                           "one dtype"),
        "float64 operands": (torch.zeros((T, d), dtype=torch.float64),) * 3 + (torch.zeros((T, d), dtype=torch.float64), "fp32, bf16 or f16"),
    }
    for what, (q, k, v, out, rule) in bad.items():
        with pytest.raises(ValueError, match=re.escape(rule)):
            Context.attention(None, q, k, v, out, so, 1, 64, 32)
            pytest.fail(f"accepted: {what}")


def test_needle_budget_of_the_longest_cases():
    """make_inputs gives every needle a channel of its own and fails when the heads run out; the longest dh 64 cases (the
    mirror fragments of zz8 at 2048, the three 256-query blocks of w16 at 650) carry needles all the way to their last query."""
    for L, window in ((2048, 0), (2048, 256), (2048, 47), (650, 0), (700, 256)):
        inp = make_inputs(call_lens(L), 12, 64, window, 1.0, seed=1000 * L + window)
        needles = inp["q"][:L].reshape(L, 12, 64)[:, :, 16:]
        hit = np.nonzero((needles == 4.0).any(axis=(1, 2)))[0]
        for i in (L - 1, L - 2, 511, 512, 639, 640, 1023, 1024):
            if i < L:
                assert i in hit, f"L={L} window={window}: no needle at query {i}"


# ------------------------------------------------------------------------------------------------------------------------
# inputs

def _bf16_exact(x):
    """float64 values exact in bf16 AND f16: bf16-rounded, magnitudes below f16's normal range flushed to 0."""
    r = torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).double().numpy()
    return np.where(np.abs(r) < 2.0 ** -14, 0.0, r)


def _positions(n, window, rng):
    base = {0, 1, 2, 14, 15, 16, 17, 31, 32, 33, 47, 48, 62, 63, 64, 65, 66, 95, 96, 127, 128, 129, 130, 191, 192, 255, 256,
            257, 258, 319, 320, 383, 384, 385, 447, 448, 511, 512, 513, 639, 640, 1023, 1024, 2046, 2047, n - 1, n - 2, n - 3}
    if window > 0:
        base |= {window + o for o in (-1, 0, 1, 14, 15, 16, 17, 47, 48, 62, 63, 64, 65, 126, 127, 128, 129)}
    base |= set(rng.integers(0, n, size=6).tolist())
    return sorted(p for p in base if 0 <= p < n)


def _plans(n, window, rng):
    """Needle plans [(query, [(key, logit above background), ...]), ...], edge cases first."""
    def vis(i, j):
        return 0 <= j <= i and (window == 0 or j > i - window)

    first, rest = [], []
    for i in _positions(n, window, rng):
        dec = [(i + 1, 12.0)] if i + 1 < n else []              # masked (the future): a higher logit than any visible needle
        if window > 0 and i - window >= 0:
            first.append((i, [(i - window + 1, 10.0), (i - window, 12.0)]))
        for t in (16, 64):
            b = t * (i // t)
            if b >= 1 and vis(i, b) and vis(i, b - 1):
                rest.append((i, [(b - 1, 10.0), (b, 9.0)]))
        rest.append((i, [(i, 10.0)] + dec))
        if i > 0 and vis(i, 0):
            rest.append((i, [(0, 10.0)] + dec))
    return first + rest


def make_inputs(lens, H, dh, window, scale, seed, x3=False):
    """q, k, v float64 [T + SLACK_ROWS, H dh] (real rows: needles + background; every other row: sentinels) and the layout.
    x3: fp32 values (NOT 16-bit exact: the hi + lo split carries them)."""
    rng = np.random.default_rng(seed)
    off, alloc, T, max_alloc = layout(lens)
    R, d = T + SLACK_ROWS, H * dh
    nb = 16                                                    # background channels per head: [0, 16)
    nr = dh - nb                                               # needle channels per head: [16, dh), one per needle
    sig = (1.0 / (scale * math.sqrt(nb))) ** 0.5               # background logits ~ N(0, 1)
    real = np.zeros(R, bool)
    for s0, n in zip(off.tolist(), lens):
        real[s0:s0 + n] = True
    q = rng.standard_normal((R, d)) * sig
    k = rng.standard_normal((R, d)) * sig
    v = rng.integers(-16, 17, size=(R, d)) / 8.0 if not x3 else rng.uniform(-2.0, 2.0, size=(R, d))
    for h in range(H):
        q[:, h * dh + nb:(h + 1) * dh] = 0.0
        k[:, h * dh + nb:(h + 1) * dh] = 0.0
    a = 4.0
    for s0, n in zip(off.tolist(), lens):
        used = [0] * H
        for p_i, (i, entries) in enumerate(_plans(n, window, rng)):
            for t in range(H):
                h = (p_i + t) % H
                if used[h] + len(entries) <= nr:
                    break
            else:                                              # every needle exists, or the case fails here
                raise AssertionError(f"needle budget: {H} heads x {nr} channels cannot place plan {p_i} (query {i}) of a "
                                     f"{n}-token sequence (window {window}); give the case more heads")
            for j, lg in entries:
                c = h * dh + nb + used[h]
                used[h] += 1
                q[s0 + i, c] = a
                k[s0 + j, c] = lg / (scale * a)
    cast = (lambda x: np.asarray(x, np.float32).astype(np.float64)) if x3 else _bf16_exact
    q, k, v = cast(q), cast(k), cast(v)
    rows = np.nonzero(~real)[0]
    sent = (64.0 + (rows % 32))[:, None]
    sgn = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)[None, :]
    q[rows] = sent * sgn
    k[rows] = sent
    v[rows] = -sent * sgn
    return dict(q=q, k=k, v=v, off=off, alloc=alloc, lens=np.asarray(lens), T=T, max_alloc=max_alloc, real=real, H=H, dh=dh)


_REF = {}


def reference(inp, window, scale, slopes, key):
    if key not in _REF:
        _REF.clear()
        _REF[key] = packed_attention(inp["q"], inp["k"], inp["v"], inp["off"], inp["lens"], inp["H"], window, scale, slopes)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------
# device side

@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _seq_off(inp):
    return torch.tensor(np.concatenate([inp["off"], [inp["off"][-1] + inp["alloc"][-1]]]), dtype=torch.int32, device="cuda")


def _buffers16(inp, fmt, x3=False):
    """qk [2 (x3) , R, 2d] (q | k rows, ldq = 2d, lo halves one plane behind), V^T [2 (x3), d, T + 64]."""
    T, d = inp["T"], inp["H"] * inp["dh"]
    dt = HALF[fmt]
    planes = []
    for name in ("q", "k", "v"):
        x = torch.from_numpy(inp[name])
        hi = x.to(dt)
        planes.append((hi, (x - hi.double()).to(dt)))
    qk = torch.empty((2 if x3 else 1, T + SLACK_ROWS, 2 * d), dtype=dt)
    vt = torch.empty((2 if x3 else 1, d, T + VT_SLACK), dtype=dt)
    for p in range(qk.shape[0]):
        qk[p, :, :d] = planes[0][p]
        qk[p, :, d:] = planes[1][p]
        vt[p] = planes[2][p][:T + VT_SLACK].T
    if not x3:
        for p in range(3):
            assert torch.equal(planes[p][1], torch.zeros_like(planes[p][1])), "16-bit cases feed exact values"
    return qk.cuda(), vt.cuda()


OUT_FILL = 77.0


def run16(ctx, inp, fmt, window, scale, alibi=None, out_fp8=False, out_scale=0.0, split=False, x3=False, flag=None):
    T, d = inp["T"], inp["H"] * inp["dh"]
    qk, vt = _buffers16(inp, fmt, x3)
    so = _seq_off(inp)
    outs = []
    for _ in range(2):
        if out_fp8:
            out = torch.full((T, d + 16), 0x5A, dtype=torch.uint8, device="cuda")
        else:
            out = torch.full((T, 3 * d if split else d + 8), OUT_FILL, dtype=HALF[fmt], device="cuda")
        ctx.attention(qk[0, :T, :d], qk[0, :T, d:], vt[0], out, so, inp["H"], inp["dh"], inp["max_alloc"], window=window,
                      scale=scale, alibi=alibi, out_scale=out_scale, range_flag=flag, x3=x3,
                      qk_lo_delta=qk[0].numel() if x3 else 0, v_lo_delta=vt[0].numel() if x3 else 0,
                      ctx_lo_delta=d if split else 0, ctx_hi2_delta=2 * d if split else 0)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "two runs of one call differ"
    out = outs[0].cpu()
    # rows outside every allocation (filler up to T) and the columns past the context are never written
    in_alloc = np.zeros(T, bool)
    for s0, a in zip(inp["off"].tolist(), inp["alloc"].tolist()):
        in_alloc[s0:s0 + a] = True
    fill = 0x5A if out_fp8 else OUT_FILL
    assert (out[torch.from_numpy(~in_alloc)].double() == fill).all(), "a row outside every allocation was written"
    if not split:
        assert (out[:, d:].double() == fill).all(), "a column past H * head_dim was written"
    return out


def _real_rows(inp):
    return np.nonzero(inp["real"][:inp["T"]])[0]


def _vmax(inp):
    return float(np.abs(inp["v"][inp["real"]]).max())


def check16(case, out, ref, inp, fmt):
    rows = _real_rows(inp)
    d = inp["H"] * inp["dh"]
    got = out[:, :d].double().numpy()[rows]
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref[rows]).max())
    bound = BOUND16 * U16[fmt] * _vmax(inp)
    print(f"{case} {fmt}: max|ctx - ref| = {err:.3e}  (bound {bound:.3e}, {err / bound:.2f})")
    assert err <= bound, f"{case} {fmt}: {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------------------------------
# the case matrix

@pytest.mark.gpu
@pytest.mark.parametrize("L,window", [(L, w) for L in LENS64 for w in (0, 256, 47, 8) if w != 8 or L <= 300])
def test_attention16_dh64_vs_float64(ctx, L, window):
    H = 12
    inp = make_inputs(call_lens(L), H, 64, window, 1.0, seed=1000 * L + window)
    ref = reference(inp, window, 1.0, None, ("64", L, window))
    for fmt in ("bf16", "f16"):
        check16(f"dh64 L={L} w={window} [{attn_variant(64, inp['max_alloc'])}]", run16(ctx, inp, fmt, window, 1.0), ref, inp, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("L,window,scale,heads", [(L, w, s, a) for L in LENS128 for (w, s, a) in
                                                  ((0, 1.0, 0), (256, 1.0, 0), (0, 128 ** -0.5, 0), (0, 128 ** -0.5, 12), (0, 1.0, 12))]
                         + [(L, 0, 128 ** -0.5, 32) for L in (2, 65, 129, 300)])
def test_attention16_dh128_vs_float64(ctx, L, window, scale, heads):
    """SGPT-1.3B / 2.7B (scale 1) and bloom-7b1 (1/sqrt(128), ALiBi) head shapes.  heads > 0: ALiBi with the slopes of that
    head count (32: bloom-7b1; 12: not a power of two -- the interleaved extra slopes)."""
    H = heads or 8
    slopes = O.alibi_slopes(heads) if heads else None
    inp = make_inputs(call_lens(L), H, 128, window, scale, seed=2000 * L + window + heads)
    ref = reference(inp, window, scale, slopes, ("128", L, window, scale, heads))
    al = None if slopes is None else torch.from_numpy(slopes)
    for fmt in ("bf16", "f16"):
        check16(f"dh128 L={L} w={window} scale={scale:.4f} alibi={heads}", run16(ctx, inp, fmt, window, scale, alibi=al), ref, inp, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENS256)
def test_attention16_dh256_vs_float64(ctx, L):
    """GPT-J-6B head shape: global causal attention, scale 1/sqrt(256)."""
    inp = make_inputs(call_lens(L), 4, 256, 0, 1.0 / 16, seed=3000 * L)
    ref = reference(inp, 0, 1.0 / 16, None, ("256", L))
    for fmt in ("bf16", "f16"):
        check16(f"dh256 L={L}", run16(ctx, inp, fmt, 0, 1.0 / 16), ref, inp, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("dh,L,window,heads", [(64, 1, 0, 0), (64, 65, 256, 0), (64, 300, 47, 0), (64, 513, 256, 0),
                                                (128, 129, 0, 12), (128, 400, 256, 0), (256, 65, 0, 0), (256, 300, 0, 0)])
def test_attention_fp32_vs_float64(ctx, dh, L, window, heads):
    """attn_f32_kernel (the parity gate's attention): same needles, fp32 operands [T][ldq] of one q | k | v buffer."""
    H = heads or (12 if dh == 64 else 4)
    scale = 1.0 if dh < 256 else 1.0 / 16
    slopes = O.alibi_slopes(heads) if heads else None
    inp = make_inputs(call_lens(L), H, dh, window, scale, seed=4000 * L + dh)
    ref = reference(inp, window, scale, slopes, ("f32", dh, L, window, heads))
    T, d = inp["T"], H * dh
    qkv = torch.empty((T + SLACK_ROWS, 3 * d), dtype=torch.float32)
    qkv[:, :d] = torch.from_numpy(inp["q"])
    qkv[:, d:2 * d] = torch.from_numpy(inp["k"])
    qkv[:, 2 * d:] = torch.from_numpy(inp["v"])
    qkv = qkv.cuda()
    so = _seq_off(inp)
    al = None if slopes is None else torch.from_numpy(slopes)
    outs = []
    for _ in range(2):
        out = torch.full((T, d), OUT_FILL, dtype=torch.float32, device="cuda")
        ctx.attention(qkv[:T, :d], qkv[:T, d:2 * d], qkv[:T, 2 * d:], out, so, H, dh, inp["max_alloc"], window=window,
                      scale=scale, alibi=al)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    rows = _real_rows(inp)
    got = outs[0].cpu().double().numpy()[rows]
    err = float(np.abs(got - ref[rows]).max())
    bound = 1e-5 * _vmax(inp)
    print(f"fp32 dh{dh} L={L} w={window} alibi={heads}: max|ctx - ref| = {err:.3e}  (bound {bound:.3e})")
    assert err <= bound


def _ordinal(codes):
    c = codes.astype(np.int64)
    return np.where(c & 0x80, -(c & 0x7F), c & 0x7F)


@pytest.mark.gpu
@pytest.mark.parametrize("dh,L,window", FP8_CASES)
def test_attention_out_fp8_codes(ctx, dh, L, window):
    """e4m3 context (SGPT_FP8M's out-projection operand): code == e4m3(ref / out_scale), except where the reference lies
    within the 16-bit bound b of a rounding boundary -- there the code may be the neighbour: every code must be the RNE
    encoding of some value in [ref - b, ref + b] / out_scale.  (Where the e4m3 step is finer than 2 b -- the subnormals and
    the low binades -- that admits more than one step; the printed maximum step difference shows how many.)  A clean call
    leaves the range flag at 0; an out_scale too small for the context raises bit 2 (value 4, as sgpt_model_range_check
    reports it)."""
    H = 12 if dh == 64 else 4
    scale = 1.0 if dh < 256 else 1.0 / 16
    inp = make_inputs(call_lens(L), H, dh, window, scale, seed=5000 * L + dh)
    ref = reference(inp, window, scale, None, ("fp8", dh, L, window))
    rows = _real_rows(inp)
    d = H * dh
    s = 0.25                                                   # real |ctx| / s <= 8, sentinel rows' <= 384: all inside e4m3
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = run16(ctx, inp, "bf16", window, scale, out_fp8=True, out_scale=s, flag=flag)
    assert int(flag.item()) == 0, "a clean call raised the range flag"
    got = out[:, :d].numpy()[rows]
    r = ref[rows] / s
    b = BOUND16 * U16["bf16"] * _vmax(inp) / s
    want = O.fp8_e4m3fn_encode(r.astype(np.float32))
    lo = O.fp8_e4m3fn_decode(O.fp8_e4m3fn_encode((r - b).astype(np.float32)))
    hi = O.fp8_e4m3fn_decode(O.fp8_e4m3fn_encode((r + b).astype(np.float32)))
    dec = O.fp8_e4m3fn_decode(got)
    exact = float((got == want).mean())
    step = int(np.abs(_ordinal(got) - _ordinal(want)).max())
    print(f"fp8 dh{dh} L={L} w={window}: codes equal {exact:.4f}, max code-step difference {step}")
    assert ((dec >= lo) & (dec <= hi)).all(), "an e4m3 code outside the rounding of ref +- the 16-bit bound"
    flag.zero_()
    run16(ctx, inp, "bf16", window, scale, out_fp8=True, out_scale=2.0 ** -8, flag=flag)   # |ctx| up to 2 -> 512 > 448
    assert int(flag.item()) == 4, f"saturated codes: range flag {int(flag.item())}, want bit 2 (4)"


def _ulp16(x, fmt):
    a = np.abs(x)
    mant = 7 if fmt == "bf16" else 10
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    if fmt == "f16":
        e = np.maximum(e, -14)
    return np.where(a > 0, 2.0 ** (e - mant), 2.0 ** (-133 if fmt == "bf16" else -24))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("dh,L,window", SPLIT_CASES)
def test_attention_split_context(ctx, fmt, dh, L, window):
    """MODE 1: [hi | lo | hi] rows -- hi = round16(v), lo = round16(v - hi) (|lo| <= half an ulp of hi), the second hi a
    copy of the first, hi + lo within the 16-bit bound of the reference."""
    H = 12 if dh == 64 else 4
    scale = 1.0 if dh < 256 else 1.0 / 16
    inp = make_inputs(call_lens(L), H, dh, window, scale, seed=6000 * L + dh)
    ref = reference(inp, window, scale, None, ("split", dh, L, window))
    d = H * dh
    out = run16(ctx, inp, fmt, window, scale, split=True)
    rows = _real_rows(inp)
    hi, lo, hi2 = (out[:, c * d:(c + 1) * d].double().numpy()[rows] for c in range(3))
    assert np.array_equal(hi, hi2), "the second hi differs from the first"
    assert (np.abs(lo) <= 0.5 * _ulp16(hi, fmt)).all(), "lo is not the rounding remainder of hi"
    err = float(np.abs(hi + lo - ref[rows]).max())
    err_hi = float(np.abs(hi - ref[rows]).max())
    bound = BOUND16 * U16[fmt] * _vmax(inp)
    print(f"split dh{dh} L={L} w={window} {fmt}: max|hi + lo - ref| = {err:.3e}, max|hi - ref| = {err_hi:.3e}  (bound {bound:.3e})")
    assert err <= bound and err_hi <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("dh,L,window", X3_CASES)
def test_attention_x3_vs_float64(ctx, fmt, dh, L, window):
    """MODE 2 on fp32 data: q | k, V^T as hi + lo halves, the context split; hi + lo against the float64 reference of the
    fp32 values within max|v| (u16^2 (4 + 6 L) + 2^-19), plus the absolute f16 subnormal terms -- the derivation in the
    module docstring."""
    H = 12 if dh == 64 else 4
    scale = 1.0
    inp = make_inputs(call_lens(L), H, dh, window, scale, seed=7000 * L + dh, x3=True)
    ref = reference(inp, window, scale, None, ("x3", dh, L, window))
    d = H * dh
    out = run16(ctx, inp, fmt, window, scale, split=True, x3=True)
    rows = _real_rows(inp)
    hi, lo = (out[:, c * d:(c + 1) * d].double().numpy()[rows] for c in range(2))
    err = float(np.abs(hi + lo - ref[rows]).max())
    Lmax = Amax = 0.0
    for s0, n in zip(inp["off"].tolist(), inp["lens"].tolist()):
        for h in range(H):
            qa = np.abs(inp["q"][s0:s0 + n, h * dh:(h + 1) * dh])
            ka = np.abs(inp["k"][s0:s0 + n, h * dh:(h + 1) * dh])
            Lmax = max(Lmax, float((qa @ ka.T).max()) * scale)
            Amax = max(Amax, (float(qa.sum(axis=1).max()) + float(ka.sum(axis=1).max())) * scale)
    u2 = U16[fmt] ** 2
    vmax = _vmax(inp)
    bound = vmax * (u2 * (4 + 6 * Lmax) + 2.0 ** -19)
    if fmt == "f16":                                           # lo halves on the subnormal grid: 2^-25 absolute per operand
        bound += 2.0 ** -25 * (2 * Amax * vmax + 1 + max(inp["lens"]) * vmax)
    plain = BOUND16 * U16[fmt] * vmax
    print(f"x3 dh{dh} L={L} w={window} {fmt}: max|ctx - ref| = {err:.3e}  (bound {bound:.3e}, L = {Lmax:.1f}; plain 16-bit bound {plain:.3e})")
    assert bound < plain / 4
    assert err <= bound


@pytest.mark.gpu
def test_attention_refuses_what_the_launcher_cannot_run(ctx):
    """Every combination launch_attn_bf16 would abort() on -- and the layout rules -- is a ValueError, nothing launched;
    the context keeps working."""
    inp = make_inputs([65, 17, 1], 4, 64, 0, 1.0, seed=9)
    T, d = inp["T"], 4 * 64
    qk, vt = _buffers16(inp, "bf16")
    so = _seq_off(inp)
    out16 = torch.zeros((T, 3 * d), dtype=torch.bfloat16, device="cuda")
    out8 = torch.zeros((T, d), dtype=torch.uint8, device="cuda")
    q, k = qk[0, :T, :d], qk[0, :T, d:]
    ma = inp["max_alloc"]

    def call(dtype=1, qq=q, kk=k, vv=vt[0], out=out16, ldq=2 * d, ldvt=None, ldo=3 * d, T_=T, H=4, dh=64, max_alloc=ma,
             out_fp8=0, out_scale=1.0, x3=0, qk_lo=0, v_lo=0, ctx_lo=0, ctx_hi2=0):
        st = ctx.lib.sgpt_attention(ctx.handle, dtype, qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), ldq,
                                    ldvt if ldvt is not None else vv.stride(0), out.data_ptr(), ldo, so.data_ptr(), so.numel() - 1,
                                    T_, H, dh, 0, 1.0, None, max_alloc, out_fp8, out_scale, None, x3, qk_lo, v_lo, ctx_lo,
                                    ctx_hi2, None)
        ctx._chk(st, "sgpt_attention")

    # (what, arguments, the rule that must refuse them: a fragment of sgpt_attention's message for exactly that check)
    head = "head_dim 64, 128 or 256"
    alloc = "max_alloc_len even, in [2, 2048]"
    refused = [
        ("head_dim 32", dict(dh=32, H=8), head),
        ("head_dim 96", dict(dh=96, H=2), head),
        ("head_dim 512", dict(dh=512, H=1), head),
        ("out_fp8 with split context", dict(out=out8, ldo=d, out_fp8=1, ctx_lo=d), "out_fp8 with a split-precision mode"),
        ("out_fp8 with x3", dict(out=out8, ldo=d, out_fp8=1, x3=1, qk_lo=8, v_lo=8), "out_fp8 with a split-precision mode"),
        ("out_fp8 with f16", dict(dtype=3, out=out8, ldo=d, out_fp8=1), "out_fp8 takes bf16 operands"),
        ("out_fp8 with fp32", dict(dtype=0, out=out8, ldo=d, out_fp8=1), "out_fp8 / x3 / split context are 16-bit modes"),
        ("out_fp8 without a scale", dict(out=out8, ldo=d, out_fp8=1, out_scale=0.0), "out_scale > 0"),
        ("x3 at head_dim 256", dict(dh=256, H=1, x3=1, qk_lo=8, v_lo=8), "x3 needs head_dim 64 | 128"),
        ("x3 without lo halves", dict(x3=1), "x3 needs non-zero lo deltas"),
        ("split context with fp32", dict(dtype=0, ctx_lo=d), "out_fp8 / x3 / split context are 16-bit modes"),
        ("hi2 without lo", dict(ctx_hi2=2 * d), "ctx_hi2_delta needs ctx_lo_delta"),
        ("max_alloc_len above 2048", dict(max_alloc=2050), alloc),
        ("max_alloc_len odd", dict(max_alloc=ma + 1), alloc),
        ("max_alloc_len 0", dict(max_alloc=0), alloc),
        ("T % 32", dict(T_=T - 16), "T % 32 == 0"),
        ("ldq % 8", dict(ldq=2 * d - 4), "ldq, ldo, qk / ctx deltas % 8"),
        ("ldq < H * head_dim", dict(ldq=d - 8), "ldq, ldo >= H * head_dim"),
        ("ldvt < T", dict(ldvt=T - 2), "ldvt >= T"),
        ("misaligned q", dict(qq=qk[0, :T, 1:]), "16-byte aligned q / k / out"),
        ("bad dtype", dict(dtype=2), "dtype SGPT_F32 | SGPT_BF16 | SGPT_F16"),
    ]
    for what, kw, rule in refused:
        with pytest.raises(ValueError, match=re.escape(rule)):
            call(**kw)
            pytest.fail(f"accepted: {what}")
    # still usable: the same buffers, a valid call, against the reference
    ref = reference(inp, 0, 1.0, None, ("refuse",))
    out = torch.zeros((T, d), dtype=torch.bfloat16, device="cuda")
    ctx.attention(q, k, vt[0], out, so, 4, 64, ma)
    torch.cuda.synchronize()
    rows = _real_rows(inp)
    assert np.abs(out.cpu().double().numpy()[rows] - ref[rows]).max() <= BOUND16 * U16["bf16"] * _vmax(inp)
