"""-m gpu: the filtered epilogue shared by the three 64-query-row scorer tiles (csrc/score64_epilogue.h), on its per-lane leg: thresholds
below -1, where a NaN score -- counted as -1 -- can still enter the top-k.  tests/test_gpu_kernels.py reaches that leg on the f16 tile
(test_score_topk_filtered_chunks_nan_and_negative_thresholds); the one-byte tiles' suites search unit rows and positive dot scores only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, NQ, K = 262_144 + 77, 128, 16, 11     # the smallest shard the planner filters at nq = 16, for every format (N >= 2 x 131 072)
NAN_DOC = 100_003                           # inside the one filtered launch, away from its ends


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


@pytest.fixture(scope="module")
def rows():
    """Documents -0.35 s + 0.1 noise (norm ~4, |element| < 1: well inside e4m3's range) against queries 0.25 |noise| s, s a sign pattern:
    <q, c> = -0.35 * 0.25 * sum |noise| + O(0.3) ~ -9, every score far below -1."""
    g = torch.Generator(device="cpu").manual_seed(64)
    s = torch.randn(D, generator=g).sign()
    q = torch.randn(NQ, D, generator=g).abs() * s * 0.25
    c = torch.randn(N, D, generator=g) * 0.1 - 0.35 * s[None, :]
    assert float((q @ c[:4096].T).max()) < -4
    return q.cuda(), c.cuda()


def _corpus(ctx, fmt, q, c):
    """-> (queries, corpus, slice(corpus, a, b), has a NaN document)"""
    from sgpt_amd import QuantizedCorpus, Uint8Corpus
    if fmt == "f16":
        c16 = c.to(torch.float16)
        c16[NAN_DOC] = float("nan")
        return q.to(torch.float16), c16, lambda a, b: c16[a:b], True
    if fmt == "fp8":
        qc = ctx.quantize_corpus(c, normalize=False)
        qc.codes[NAN_DOC, 5] = 0x7f                                   # e4m3fn NaN
        return q.to(torch.float16), qc, lambda a, b: QuantizedCorpus(qc.codes[a:b], qc.scale[a:b], False), True
    uc = ctx.scalar_quantize_corpus(c, normalize=False)              # (every uint8 code is a number: no NaN document in this format)
    return q, uc, lambda a, b: Uint8Corpus(uc.codes[a:b], uc.start, uc.step, False, D), False


@pytest.mark.parametrize("fmt", ["f16", "fp8", "uint8"])
def test_thresholds_below_minus_one_take_the_per_lane_leg(ctx, rows, fmt):
    """Dot scores around -9 (normalize=False), k = 11, nq = 16, N = 262 144 + 77, d = 128: the sampled thresholds lie below -1, so every
    tile of the filtered launch takes the per-lane leg (count, one atomicAdd per lane, predicated stores).  Values and indices equal the
    materialise-and-select route's over slices short enough that the planner filters none; at least one chunk was filtered and none
    overflowed; the NaN document (f16: a NaN row; fp8: a NaN code) scores -1.0 and ranks first for every query."""
    q, corpus, part, has_nan = _corpus(ctx, fmt, *rows)
    val, idx, n = ctx.score_topk(q, corpus, K, idx_base=7)
    chunks, over = ctx.score_overflow_count()
    print(f"{fmt}: filtered chunks {chunks}, overflowed {over}; best {val[:, 0].max().item():.4f}, k-th best {val[:, -1].min().item():.4f}")
    assert chunks >= 1 and over == 0
    assert val[:, -1].max() < -1                 # the k-th best, so every threshold the filtered launch held, lies below -1
    run = None
    for s in range(0, N, 100_000):
        run = ctx.score_topk(q, part(s, s + 100_000), K, idx_base=7 + s, run=run)
    wv, wi, wn = run
    assert n == wn == K
    assert torch.equal(val, wv) and torch.equal(idx, wi)
    assert (val[:, 1:] < -1).all()
    if has_nan:
        assert (val[:, 0] == -1.0).all() and (idx[:, 0] == 7 + NAN_DOC).all()
    else:
        assert (val[:, 0] < -1).all()
