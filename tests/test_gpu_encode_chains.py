"""-m gpu: a bulk encode call as two chains of whole sequences on two streams (include/sgpt_hip.h: sgpt_ctx_set_encode_chains;
csrc/encode.hip) must give the bits of the one-chain call -- every kernel computes a row / a sequence on its own, and both halves stay
on the 256x256 projection kernel.  SGPT-125M shape (d = 768): a half needs 43 row tiles (11 008 token rows) for that, so the layouts
here hold 22 528 rows and more; `min_rows` is forced low and `encode_chain_calls` tells whether a call was cut."""
import numpy as np
import pytest
import torch

from helpers import build_model, load_case

pytestmark = pytest.mark.gpu

MIN_ROWS = 8704          # two halves of 4352 rows, the smallest size that leaves the query path; the 256x256 rule asks for more (above)
HALF_ROWS = 11008        # 43 row tiles x 3 column tiles of the out-projection > 128: the 256x256 kernel


def _model(dtype):
    fx, cfg_kw, *_ = load_case("cfg1_125m_32x64")
    return build_model(cfg_kw, int(fx["seed"]), float(fx["std"]), dtype)


def _seqs(rng, lens):
    return [rng.integers(0, 50256, size=int(n)).tolist() for n in lens]


class chains:
    """`with chains(m, n):` -- the context's setting for the block (the model and its context are shared by the session)"""
    def __init__(self, m, n, min_rows=MIN_ROWS):
        self.ctx, self.n, self.min_rows = m.ctx, n, min_rows

    def __enter__(self):
        self.old = self.ctx.set_encode_chains(self.n, self.min_rows)

    def __exit__(self, *exc):
        self.ctx.set_encode_chains(self.old, 0)


def _on_off(m, pb, expect_cut):
    """The same packed batch with two chains and with one: (embeddings, embeddings); asserts that the first call was (not) cut."""
    n0 = m.ctx.encode_chain_calls()
    with chains(m, 2):
        on = m.encode_packed(pb, normalize=True)
    cut = m.ctx.encode_chain_calls() - n0
    with chains(m, 1):
        off = m.encode_packed(pb, normalize=True)
    assert m.ctx.encode_chain_calls() - n0 == cut, "n = 1 cut a call"
    assert cut == (1 if expect_cut else 0), (cut, pb.T_pad)
    assert bool(torch.isfinite(off).all())
    return on, off


def _cut_row(pb):
    """encode_split_point's rule on the batch's host layout (tests/test_encode_split.py holds the function itself to it)"""
    off, T = pb.off_host.tolist(), pb.T_pad
    cands = [(abs(2 * o - T), o) for o in off[1:-1] if o % 256 == 0 and T <= 3 * o <= 2 * T]
    return min(cands)[1] if cands else 0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_two_chains_give_the_bits_of_one(dtype):
    m = _model(dtype)
    rng = np.random.default_rng(31)
    # fixed length: 176 x 128 tokens, cut at row 11 264
    pb = m.pack(_seqs(rng, [128] * 176))
    assert pb.T_pad == 22528 and _cut_row(pb) == 11264
    on, off = _on_off(m, pb, True)
    assert torch.equal(on, off)
    # lengths U{16..128}, an odd number of sequences: a ragged cut, halves of different sizes, filler rows behind the last sequence
    pb = m.pack(_seqs(rng, rng.integers(16, 129, size=451)))
    r = _cut_row(pb)
    assert pb.B % 2 == 1 and r >= HALF_ROWS and pb.T_pad - r >= HALF_ROWS and 2 * r != pb.T_pad, (r, pb.T_pad)
    on, off = _on_off(m, pb, True)
    assert torch.equal(on, off)
    # the only 256-aligned sequence start (row 256) lies outside the middle third: one chain, same bits
    pb = m.pack(_seqs(rng, [128, 128, 120] + [128] * 175))
    assert [o for o in pb.off_host.tolist()[1:-1] if o % 256 == 0] == [256] and _cut_row(pb) == 0 and pb.T_pad >= 2 * HALF_ROWS
    on, off = _on_off(m, pb, False)
    assert torch.equal(on, off)


def test_switch_arguments_and_default():
    m = _model("bf16")
    old = m.ctx.set_encode_chains(2, 4096)
    try:
        assert m.ctx.set_encode_chains(1) == 2 and m.ctx.set_encode_chains(0) == 1
        for bad in ((3, 0), (-1, 0), (2, -5)):
            with pytest.raises(ValueError):
                m.ctx.set_encode_chains(*bad)
        assert m.ctx.set_encode_chains(0) == 0          # a refused call changed nothing
    finally:
        m.ctx.set_encode_chains(old)


def test_capture_records_one_chain_and_replay_equals_eager():
    """Under stream capture the call is recorded as one chain (no parallel branches in a captured graph), whatever the switch says."""
    from sgpt_amd import EncodeGraph
    m = _model("bf16")
    rng = np.random.default_rng(32)
    a, b = _seqs(rng, [128] * 176), _seqs(rng, [128] * 176)
    with chains(m, 1):
        want_a = m.encode_packed(m.pack(a), normalize=True).clone()
        want_b = m.encode_packed(m.pack(b), normalize=True).clone()
    for n in (0, 2):
        with chains(m, n):
            n0 = m.ctx.encode_chain_calls()
            g = EncodeGraph(m, a, normalize=True)          # one eager warm-up call, then the captured one
            warm = m.ctx.encode_chain_calls() - n0
            assert warm == 1 if n == 2 else warm <= 1, warm     # never two: the captured call is not cut
            assert torch.equal(g.replay(), want_a)
            assert torch.equal(g.replay(b), want_b)
            assert m.ctx.encode_chain_calls() - n0 == warm
            eager = m.encode_packed(m.pack(b), normalize=True)
            assert torch.equal(eager, want_b)
            del g


def test_consecutive_calls_of_different_sizes_and_a_dependent_op_on_the_callers_stream():
    m = _model("f16")
    rng = np.random.default_rng(33)
    pbs = [m.pack(_seqs(rng, lens)) for lens in ([128] * 176, [128] * 240, rng.integers(16, 129, size=451), [128] * 176)]
    n_cut = sum(1 for pb in pbs if _cut_row(pb))
    assert n_cut == 3 and _cut_row(pbs[2]) == 0       # (the third layout has no aligned start in its middle third: one chain between cut calls)
    with chains(m, 1):
        want = [m.encode_packed(pb, normalize=True).clone() for pb in pbs]
    d = m.cfg.hidden_size
    with chains(m, 2):
        # back to back, no synchronisation in between: the workspace is carved anew per call, the events are re-used
        n0 = m.ctx.encode_chain_calls()
        outs = [torch.empty((pb.B, d), dtype=torch.float32, device=m.device) for pb in pbs]
        for pb, o in zip(pbs, outs):
            m.encode_packed(pb, normalize=True, out=o)
        assert m.ctx.encode_chain_calls() - n0 == n_cut
        for o, w in zip(outs, want):
            assert torch.equal(o, w)
        # a side stream as the caller's: the op behind the call reads rows of both chains and must find them written
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for pb, w in zip(pbs, want):
                o = torch.full((pb.B, d), float("nan"), dtype=torch.float32, device=m.device)
                m.encode_packed(pb, normalize=True, out=o)
                copy = o.clone()
                sums = o.sum(dim=1)
                side.synchronize()
                assert torch.equal(copy, w) and torch.equal(sums, w.sum(dim=1))
        assert m.ctx.encode_chain_calls() - n0 == 2 * n_cut
