"""-m gpu: the bidirectional mode of the attention kernels (csrc/attn.hip, CAUSAL = false) through sgpt_attention_ex, against the
float64 reference of tests/bert_ref.py.

Inputs.  As tests/test_gpu_attention.py: every q / k / v value is exact in both 16-bit formats and the reference gets the same
values in float64; rows that belong to no token -- the alignment row behind an odd length (INSIDE the allocation: only seq_len
keeps it out of a bidirectional softmax), the filler up to T, the slack the key tiles over-read -- hold finite sentinels of
magnitude 64..95, so a key that leaks moves the context by O(32 max|v|).  The logits are sharp (std 3 over all head channels): a
softmax row is carried by a handful of keys anywhere in the sequence, the FUTURE ones included, so a visible key that is dropped
(a tile not visited, a diagonal mask left in) moves the context by O(max|v|) as well.

Cases.  The packed batch 1, 2, 3, 31, 33, 63, 64, 65, 127, 129 (both sides of the 32-row query tile, the 64-key tile and the
128-query block; the ragged last key tile is masked by the sequence end) plus one sequence of 300 rows (five key tiles, three
query blocks), H = 2, head_dim 64 and 128, f16 / bf16 / fp32.

Tolerance: that of tests/test_gpu_attention.py for the same dtype, unchanged -- 3 u16 max|v| for the 16-bit kernel (its derivation
bounds the probability rounding, the f16 subnormal flush over <= 2048 keys and the store rounding, none of which depends on how
many of the keys are visible) and 1e-5 max|v| for the fp32 kernel (derived there for <= 514 keys; the longest row here sums 300)."""
import math

import numpy as np
import pytest
import torch

from attn_ref import layout
from bert_ref import packed_attention_bidir
from test_gpu_attention import BOUND16, HALF, SLACK_ROWS, U16, VT_SLACK, _bf16_exact

pytestmark = pytest.mark.gpu

LENS = [1, 2, 3, 31, 33, 63, 64, 65, 127, 129, 300]
H = 2
OUT_FILL = 77.0


def make_inputs(dh, seed):
    rng = np.random.default_rng(seed)
    off, alloc, T, max_alloc = layout(LENS)
    scale = 1.0 / math.sqrt(dh)
    R, d = T + SLACK_ROWS, H * dh
    sig = math.sqrt(3.0 / (scale * math.sqrt(dh)))               # logits ~ N(0, 3^2)
    real = np.zeros(R, bool)
    for s0, n in zip(off.tolist(), LENS):
        real[s0:s0 + n] = True
    q = _bf16_exact(rng.standard_normal((R, d)) * sig)
    k = _bf16_exact(rng.standard_normal((R, d)) * sig)
    v = _bf16_exact(rng.integers(-16, 17, size=(R, d)) / 8.0)
    rows = np.nonzero(~real)[0]
    sent = (64.0 + (rows % 32))[:, None]
    sgn = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)[None, :]
    q[rows], k[rows], v[rows] = sent * sgn, sent * np.ones((1, d)), -sent * sgn
    return dict(q=q, k=k, v=v, off=off, alloc=alloc, lens=np.asarray(LENS), T=T, max_alloc=max_alloc, real=real, dh=dh, scale=scale)


_CASES = {}


def case(dh):
    """Inputs and float64 reference of one head_dim, computed once and shared."""
    if dh not in _CASES:
        inp = make_inputs(dh, seed=500 + dh)
        ref = packed_attention_bidir(inp["q"], inp["k"], inp["v"], inp["off"], inp["lens"], H, inp["scale"])
        ref.setflags(write=False)
        _CASES[dh] = (inp, ref)
    return _CASES[dh]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _layout_dev(inp):
    so = torch.tensor(np.concatenate([inp["off"], [inp["off"][-1] + inp["alloc"][-1]]]), dtype=torch.int32, device="cuda")
    sl = torch.tensor(inp["lens"], dtype=torch.int32, device="cuda")
    return so, sl


def _buffers(inp, fmt, q=None, k=None, v=None):
    """16-bit: q | k rows [R, 2d] and V^T [d, T + 64]; fp32: q | k | v rows [R, 3d]."""
    T, d = inp["T"], H * inp["dh"]
    q, k, v = (torch.from_numpy(inp[n] if a is None else a) for n, a in (("q", q), ("k", k), ("v", v)))
    if fmt == "fp32":
        return torch.cat([q, k, v], dim=1).float().cuda(), None
    dt = HALF[fmt]
    return torch.cat([q, k], dim=1).to(dt).cuda(), v[:T + VT_SLACK].T.contiguous().to(dt).cuda()


def run(ctx, inp, fmt, causal=False, use_seq_len=True, **over):
    T, d, dh = inp["T"], H * inp["dh"], inp["dh"]
    qkv, vt = _buffers(inp, fmt, **over)
    so, sl = _layout_dev(inp)
    out = torch.full((T, d + 8), OUT_FILL, dtype=torch.float32 if fmt == "fp32" else HALF[fmt], device="cuda")
    v = qkv[:T, 2 * d:] if fmt == "fp32" else vt
    ctx.attention(qkv[:T, :d], qkv[:T, d:2 * d], v, out, so, H, dh, inp["max_alloc"], scale=inp["scale"], causal=causal,
                  seq_len=sl if (use_seq_len and causal is False) else None)
    torch.cuda.synchronize()
    out = out.cpu()
    in_alloc = np.zeros(T, bool)
    for s0, a in zip(inp["off"].tolist(), inp["alloc"].tolist()):
        in_alloc[s0:s0 + a] = True
    assert (out[torch.from_numpy(~in_alloc)].double() == OUT_FILL).all(), "a row outside every allocation was written"
    assert (out[:, d:].double() == OUT_FILL).all(), "a column past H * head_dim was written"
    return out


def _bound(inp, fmt):
    vmax = float(np.abs(inp["v"][inp["real"]]).max())
    return (1e-5 if fmt == "fp32" else BOUND16 * U16[fmt]) * vmax


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("fmt", ["f16", "bf16", "fp32"])
def test_bidirectional_attention_vs_float64(ctx, dh, fmt):
    inp, ref = case(dh)
    rows = np.nonzero(inp["real"][:inp["T"]])[0]
    d = H * dh
    out = run(ctx, inp, fmt)
    assert torch.equal(out, run(ctx, inp, fmt)), "two runs of one call differ"
    got = out[:, :d].double().numpy()[rows]
    assert np.isfinite(got).all()
    err, bound = float(np.abs(got - ref[rows]).max()), _bound(inp, fmt)
    per_seq = {n: float(np.abs(out[s0:s0 + n, :d].double().numpy() - ref[s0:s0 + n]).max()) for s0, n in zip(inp["off"].tolist(), LENS)}
    print(f"bidir dh{dh} {fmt}: max|ctx - ref| = {err:.3e} (bound {bound:.3e}); per length {({n: f'{e:.1e}' for n, e in per_seq.items()})}")
    assert err <= bound
    # the reference itself differs from the causal one by O(max|v|) on these inputs: the check above has teeth
    from attn_ref import packed_attention
    causal = packed_attention(inp["q"], inp["k"], inp["v"], inp["off"], inp["lens"], H, 0, inp["scale"]) if fmt == "fp32" else None
    if causal is not None:
        assert np.abs(causal[rows] - ref[rows]).max() > 0.5


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("fmt", ["f16", "fp32"])
def test_bidirectional_attention_is_isolated_from_packed_neighbours(ctx, dh, fmt):
    """The rows of one sequence do not change by a bit when q / k / v of every OTHER sequence are replaced by large garbage."""
    inp, _ = case(dh)
    d = H * dh
    base = run(ctx, inp, fmt)
    rng = np.random.default_rng(9)
    for keep in (3, 6, 9, 10):                                   # lengths 31, 64, 129, 300
        s0, n = int(inp["off"][keep]), LENS[keep]
        garb = {}
        for name in ("q", "k", "v"):
            g = _bf16_exact(rng.choice([-1.0, 1.0], size=inp[name].shape) * rng.integers(200, 1000, size=inp[name].shape))
            g[s0:s0 + n] = inp[name][s0:s0 + n]
            garb[name] = g
        out = run(ctx, inp, fmt, **garb)
        assert torch.equal(out[s0:s0 + n, :d], base[s0:s0 + n, :d]), f"length {n}: a neighbour's rows reached the softmax"


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("fmt", ["f16", "bf16", "fp32"])
def test_causal_through_the_new_entry_is_bit_identical(ctx, dh, fmt):
    """sgpt_attention_ex(causal = 1) launches the kernels of sgpt_attention: the same bits on the same inputs (which reach the
    zig-zag, the 8-wave and -- alone -- the short launch shapes)."""
    inp, _ = case(dh)
    assert torch.equal(run(ctx, inp, fmt, causal=True), run(ctx, inp, fmt, causal=None))
    short = dict(inp)
    # (the whole batch has one launch shape, chosen by its longest sequence: run the short ones on their own as well)
    for lens in ([1, 2, 3, 31], [33, 63, 64]):
        off, alloc, T, max_alloc = layout(lens)
        sub = dict(short, off=off, alloc=alloc, lens=np.asarray(lens), T=T, max_alloc=max_alloc)
        T2, d = T, H * dh
        qkv, vt = _buffers(sub, fmt)
        so = torch.tensor(np.concatenate([off, [off[-1] + alloc[-1]]]), dtype=torch.int32, device="cuda")
        outs = []
        for causal in (True, None):
            out = torch.full((T2, d), OUT_FILL, dtype=torch.float32 if fmt == "fp32" else HALF[fmt], device="cuda")
            ctx.attention(qkv[:T2, :d], qkv[:T2, d:2 * d], qkv[:T2, 2 * d:] if fmt == "fp32" else vt, out, so, H, dh, max_alloc,
                          scale=inp["scale"], causal=causal)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1])


def test_whole_allocation_without_seq_len_and_refusals(ctx):
    """seq_len = NULL: every row of the allocation is a key (even lengths: the same result as with seq_len).  The modes the
    bidirectional kernels do not have are refused before any launch."""
    lens = [2, 64, 130]
    off, alloc, T, max_alloc = layout(lens)
    inp, _ = case(64)
    sub = dict(inp, off=off, alloc=alloc, lens=np.asarray(lens), T=T, max_alloc=max_alloc)
    assert torch.equal(run(ctx, sub, "f16", use_seq_len=False), run(ctx, sub, "f16", use_seq_len=True))
    d = H * 64
    qkv, vt = _buffers(sub, "bf16")
    so, sl = _layout_dev(sub)
    out = torch.zeros((T, d), dtype=torch.bfloat16, device="cuda")
    args = (qkv[:T, :d], qkv[:T, d:], vt, out, so, H, 64, max_alloc)
    bad = {"window": dict(window=8), "alibi": dict(alibi=torch.ones(H)), "x3": dict(x3=True, qk_lo_delta=8, v_lo_delta=8),
           "split context": dict(ctx_lo_delta=8)}
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            ctx.attention(*args, causal=False, seq_len=sl, **kw)
            pytest.fail(f"accepted: {what}")
    with pytest.raises(ValueError):
        ctx.attention(qkv[:T, :d], qkv[:T, d:], vt, torch.zeros((T, d + 16), dtype=torch.uint8, device="cuda"), so, H, 64, max_alloc,
                      causal=False, out_scale=1.0)
    with pytest.raises(ValueError):
        ctx.attention(*args, causal=True, seq_len=sl)              # seq_len belongs to the bidirectional mode
