"""-m gpu: the binary (1-bit) corpus -- sgpt_pack_sign_bits, sgpt_score_topk_bits, the Hamming tile (csrc/scorebits.hip), the re-scoring
kernels, Context.binarize_corpus / score_topk(BinaryCorpus), util.quantize_embeddings("ubinary") / semantic_search.

Stage 1 is integer arithmetic: packing, Hamming order, filtered chunks, ties and the running merge are compared bit for bit with
tests/scorebits_ref.py.  The re-scored values are held to the derived bounds of that file."""
import ctypes as C

import numpy as np
import pytest
import torch

import score8_ref as R
import scorebits_ref as B
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def _corpus(bits, d, **kw):
    from sgpt_amd import BinaryCorpus
    return BinaryCorpus(torch.from_numpy(np.ascontiguousarray(bits)).cuda(), d, **kw)


def _special_rows(n, d, seed):
    """Rows with +0, -0, NaN, +-inf, denormals and ordinary values of both signs in every byte position."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    spec = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 3e-39, -3e-39], dtype=np.float32)
    flat = x.reshape(-1)
    pos = np.arange(0, flat.size, 3)
    flat[pos] = spec[(pos // 3) % len(spec)]
    return x


@pytest.mark.parametrize("d", [1, 31, 32, 100, 768])
def test_packing_equals_packbits(ctx, d):
    """1. pack_sign_bits == np.packbits(x > 0), pad bits zero, with and without a centre (zeros in the centre keep denormals alive)."""
    x = _special_rows(67, d, d)
    got = ctx.pack_sign_bits(torch.from_numpy(x)).cpu().numpy()
    assert got.shape == (67, 4 * ((d + 31) // 32))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got[:, :(d + 7) // 8], np.packbits(x > 0, axis=-1))
    assert np.array_equal(got, B.pack(x))                      # (pad bytes and pad bits zero)
    center = np.random.default_rng(d + 1).standard_normal(d).astype(np.float32) * 0.5
    center[::4] = 0.0
    got_c = ctx.pack_sign_bits(torch.from_numpy(x), center=torch.from_numpy(center)).cpu().numpy()
    assert np.array_equal(got_c, B.pack(x, center))


def test_binarize_in_blocks_equals_one_call(ctx):
    """1. binarize_corpus in row blocks == one pack call over all rows; a million rows through the launcher."""
    N, d = 1_000_003, 32
    g = torch.Generator(device="cuda").manual_seed(11)
    emb = torch.randn(N, d, device="cuda", generator=g)
    center = torch.randn(d, device="cuda", generator=g) * 0.05
    for c in (None, center):
        bc = ctx.binarize_corpus(emb, center=c, block_rows=300_000)
        assert len(bc) == N and bc.bits.shape == (N, 4) and bc.dim == d and bc.fp8 is None
        assert bc.nbytes == 4 * N + (0 if c is None else 4 * d)
        assert torch.equal(bc.bits, ctx.pack_sign_bits(ctx.l2_normalize(emb), center=c))
    tail = emb[-5:].cpu().numpy()
    assert np.array_equal(ctx.binarize_corpus(emb[-5:]).bits.cpu().numpy(), np.packbits(tail > 0, axis=-1))
    with pytest.raises(ValueError, match="normalize=False"):
        ctx.binarize_corpus(emb[:4], normalize=False)


def _patterned(nq, N, d):
    """Asymmetric integer patterns (no two words, bytes, lanes or documents alike) with planted rows: document 5 equals query 0,
    document 9 is its complement over the d true bits, documents 100 .. 139 are identical."""
    n, i = np.arange(N)[:, None], np.arange(d)[None, :]
    docs = ((n * 7 + i * 11 + (n * i) % 5 + n // 64) % 13 - 6).astype(np.float32)
    m = np.arange(nq)[:, None]
    q = ((m * 5 + i * 3 + (m * i) % 7 + i // 32) % 9 - 4).astype(np.float32)
    q[0, q[0] == 0] = 1.0                                      # (so that the complement below flips every true bit)
    docs[5] = q[0]
    docs[9] = -q[0]
    docs[100:140] = docs[100]
    return q, docs


@pytest.mark.parametrize("nq", [1, 33, 64, 65, 130])
@pytest.mark.parametrize("d", [32, 100, 128, 768])
def test_hamming_order_is_exact(ctx, d, nq):
    """2. mode 0 with k = N: every value np.float32(a) / np.float32(d), every index the reference's (a descending, index ascending)."""
    N = 256 * 3 + 37
    q, docs = _patterned(nq, N, d)
    bits = B.pack(docs)
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), N, rescore="none")
    a = B.agreement(B.pack(q), bits, d)
    assert a[0, 5] == d and a[0, 9] == -d
    wa, wi = R.topk_lowest_index(a, N)
    assert n == N
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(val.cpu().numpy(), B.mode0_values(wa, d))
    got = torch.zeros_like(val).scatter_(1, idx, val).cpu().numpy()
    assert got[0, 5] == 1.0 and got[0, 9] == -1.0
    run = idx[:, :].cpu().numpy()
    for m in range(nq):                                        # the identical documents keep their index order
        pos = np.flatnonzero((run[m] >= 100) & (run[m] < 140))
        assert run[m][pos].tolist() == list(range(100, 140))


@pytest.mark.parametrize("d", [160, 1152, 2080])
def test_hamming_on_rows_wider_than_the_register_set(ctx, d):
    """Widths off the fast paths: 20-byte rows (dword loads), nine 16-byte pieces (one re-read per query), 65 dwords (dword loads,
    41 re-read)."""
    N, nq = 300, 3
    q, docs = _patterned(nq, N, d)
    bits = B.pack(docs)
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), N, rescore="none")
    wa, wi = R.topk_lowest_index(B.agreement(B.pack(q), bits, d), N)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), B.mode0_values(wa, d))


_random = {}


def _random_case(N, d):
    """(queries fp32 [64, d], bits [N, d / 8], agreement [64, N]) -- random bits, built and scored once per shape."""
    if (N, d) not in _random:
        rng = np.random.default_rng(N + d)
        bits = rng.integers(0, 256, (N, d // 8), dtype=np.uint8)
        q = rng.standard_normal((64, d)).astype(np.float32)
        _random[(N, d)] = (q, bits, B.agreement(B.pack(q), bits, d))
    return _random[(N, d)]


@pytest.mark.parametrize("nq", [1, 16, 64])
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("N", [256 * 5 + 37, 300_005])
def test_filtered_chunks_and_running_merge_are_exact(ctx, N, d, nq):
    """3. k = 11, idx_base = 3: the one-call result (300 005 documents take the sampled, filtered schedule with its ragged tail in the
    same launch) and the two-call running merge both equal the reference."""
    q, bits, a = _random_case(N, d)
    q, a = q[:nq], a[:nq]
    k, base, split = 11, 3, 700 if N < 10_000 else 70_000
    wa, wi = R.topk_lowest_index(a, k, base)
    dev = torch.from_numpy(bits).cuda()
    from sgpt_amd import BinaryCorpus
    val, idx, n = ctx.score_topk(torch.from_numpy(q), BinaryCorpus(dev, d), k, idx_base=base, rescore="none")
    assert n == k
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), B.mode0_values(wa, d))
    v1, i1, n1 = ctx.score_topk(torch.from_numpy(q), BinaryCorpus(dev[:split], d), k, idx_base=base, rescore="none")
    v2, i2, n2 = ctx.score_topk(torch.from_numpy(q), BinaryCorpus(dev[split:], d), k, idx_base=base + split, run=(v1, i1, n1), rescore="none")
    assert n1 == k and n2 == k
    assert np.array_equal(i2.cpu().numpy(), wi) and np.array_equal(v2.cpu().numpy(), B.mode0_values(wa, d))


def test_deep_lists_on_the_filtered_schedule(ctx):
    """k = 100 (the doubling schedule of k > 64) over 300 005 documents: the stage-1 order, exactly."""
    q, bits, a = _random_case(300_005, 128)
    wa, wi = R.topk_lowest_index(a[:16], 100)
    val, idx, n = ctx.score_topk(torch.from_numpy(q[:16]), _corpus(bits, 128), 100, rescore="none")
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), B.mode0_values(wa, 128))


@pytest.mark.parametrize("N", [100_000, 300_000])
def test_ties_and_overflow(ctx, N):
    """4. N identical documents: the first k indices for every query.  Identical documents in the second half only, better than the
    first half: the first k indices of the second half.  At 300 000 documents the pass is filtered, every document ties at the
    threshold, the candidate lists overflow and the predicated fallback gives the same answer."""
    d, nq, k, base = 128, 16, 11, 3
    rng = np.random.default_rng(N)
    q = np.abs(rng.standard_normal((nq, d)).astype(np.float32))
    q[:, rng.permutation(d)[:40]] *= -1                         # 88 positive dimensions per query
    bits = np.full((N, d // 8), 0xff, dtype=np.uint8)
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), k, idx_base=base, rescore="none")
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(base, base + k), (nq, 1)))
    assert np.array_equal(val.cpu().numpy(), np.full((nq, k), np.float32(88 - 40) / np.float32(d)))
    if N >= 262_144:
        chunks, overflowed = ctx.score_overflow_count()
        assert chunks >= 1 and overflowed >= 1
    bits[:N // 2] = 0x00
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), k, idx_base=base, rescore="none")
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(base + N // 2, base + N // 2 + k), (nq, 1)))
    assert np.array_equal(val.cpu().numpy(), np.full((nq, k), np.float32(88 - 40) / np.float32(d)))


_unit = {}


def _unit_case(d):
    if d not in _unit:
        q, c = R.unit_corpus(1317 + d, 256 * 5 + 37, d, 64)
        q, c = q.numpy(), c.numpy()
        bits = B.pack(c)
        codes, scale = R.quantize_rows(c)
        _unit[d] = (q, c, bits, codes, scale)
    return _unit[d]


@pytest.mark.parametrize("nq", [1, 16, 64])
@pytest.mark.parametrize("d", [128, 768])
def test_sign_rescoring(ctx, d, nq):
    """5. mode 1, k = 11 of kp = 44 candidates: indices inside the reference's (integer-exact) candidate set, values within
    d * 2^-23 * sum|q_i| / sqrt(d) of float64, the float64 top-k of the candidates up to twice that bound."""
    q, c, bits, _, _ = _unit_case(d)
    q = q[:nq]
    val, idx, n = ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), 11, idx_base=3, rescore="sign", rescore_multiplier=4)
    assert n == 11
    _, cand = B.stage1(q, bits, d, 44, idx_base=3)
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, B.sign_values(q, bits, d), B.sign_bound(q, d), 11, idx_base=3)


@pytest.mark.parametrize("nq", [1, 16, 64])
@pytest.mark.parametrize("d", [128, 768])
def test_fp8_rescoring(ctx, d, nq):
    """6. mode 2: the same against the de-quantised rows with the bound d * 2^-23 * sum|q_i c_i|; a NaN code among the candidates
    scores -1."""
    from sgpt_amd import QuantizedCorpus
    q, c, bits, codes, scale = _unit_case(d)
    q = q[:nq]
    _, cand = B.stage1(q, bits, d, 44, idx_base=3)
    codes = codes.copy()
    nan_doc = int(cand[0, 0] - 3)                               # the best stage-1 candidate of query 0 gets a NaN code
    codes[nan_doc, 7] = 0x7f
    fp8 = QuantizedCorpus(torch.from_numpy(codes).cuda(), torch.from_numpy(scale).cuda(), True, d)
    corpus = _corpus(bits, d, fp8=fp8)
    rows = R.dequantize(codes, scale)
    vals64, bound = R.scores64(q, rows), d * 2.0 ** -23 * R.abs_products(q, rows)
    val, idx, n = ctx.score_topk(torch.from_numpy(q), corpus, 11, idx_base=3, rescore="fp8", rescore_multiplier=4)
    assert n == 11
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, vals64, bound, 11, idx_base=3)
    val, idx, n = ctx.score_topk(torch.from_numpy(q), corpus, 44, idx_base=3, rescore="fp8", rescore_multiplier=1)   # every candidate
    B.check_rescored(val.cpu().numpy(), idx.cpu().numpy(), cand, vals64, bound, 44, idx_base=3)
    hit = idx[0] == nan_doc + 3
    assert hit.sum() == 1 and val[0][hit].item() == -1.0
    with pytest.raises(ValueError, match="keep_fp8"):
        ctx.score_topk(torch.from_numpy(q), _corpus(bits, d), 11, rescore="fp8")
    with pytest.raises(ValueError, match="rescore must be"):
        ctx.score_topk(torch.from_numpy(q), corpus, 11, rescore="int8")


def test_refusals_leave_the_outputs_untouched(ctx):
    """7. Every refusal of the C entry point returns SGPT_ERR_INVALID with nothing launched -- sentinel-filled outputs stay as they
    were -- then one well-formed call goes through."""
    nq, N, d, k, kp = 4, 300, 128, 5, 20
    q = torch.ones((nq, d), device="cuda")
    bits = torch.zeros((N, 16), dtype=torch.uint8, device="cuda")
    codes = torch.zeros((N, d), dtype=torch.uint8, device="cuda")
    scale = torch.ones(N, device="cuda")
    val = torch.full((nq, k), 7.0, device="cuda")
    idx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    n_out = C.c_int32(-3)

    def call(ctx_=ctx.handle, q_=q.data_ptr(), bits_=bits.data_ptr(), ldb=16, k_=k, kp_=kp, mode=1, codes_=None, scale_=None,
             val_=val.data_ptr(), idx_=idx.data_ptr(), n_run=0):
        return ctx.lib.sgpt_score_topk_bits(ctx_, q_, bits_, ldb, nq, N, d, k_, kp_, mode, codes_, scale_, 0, val_, idx_, n_run,
                                            C.byref(n_out), None)
    bad = [dict(ctx_=None), dict(q_=None), dict(bits_=None), dict(val_=None), dict(idx_=None), dict(ldb=12), dict(ldb=18), dict(ldb=0),
           dict(k_=0), dict(k_=-1), dict(kp_=k - 1), dict(kp_=1025), dict(k_=1025, kp_=1025), dict(mode=0), dict(mode=3), dict(mode=-1),
           dict(mode=2), dict(mode=2, codes_=codes.data_ptr()), dict(mode=2, scale_=scale.data_ptr()), dict(n_run=-1), dict(n_run=k + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # SGPT_ERR_INVALID
    pk = torch.full((N, 16), 9, dtype=torch.uint8, device="cuda")
    for kw in [dict(x=None), dict(out=None), dict(ldb=12), dict(ldb=18), dict(n=0), dict(d_=0)]:
        a = dict(x=q.data_ptr(), out=pk.data_ptr(), ldb=16, n=nq, d_=d)
        a.update(kw)
        assert ctx.lib.sgpt_pack_sign_bits(ctx.handle, a["x"], a["n"], a["d_"], None, a["out"], a["ldb"], None) == -1, kw
    torch.cuda.synchronize()
    assert (val == 7.0).all() and (idx == -7).all() and n_out.value == -3 and (pk == 9).all()
    assert call() == 0                                       # (and the well-formed calls go through: all-positive queries, zero bits)
    assert call(mode=0, kp_=k) == 0
    torch.cuda.synchronize()
    assert n_out.value == k
    assert call(mode=2, codes_=codes.data_ptr(), scale_=scale.data_ptr()) == 0
    torch.cuda.synchronize()
    assert n_out.value == k and (val == 0).all() and idx[:, 0].tolist() == [0] * nq


def _overlap(lists, golden):
    return float(np.mean([len(set(a) & set(b)) / 10 for a, b in zip(lists, golden)]))


def test_semantic_search_over_a_binary_corpus(ctx):
    """8. util.semantic_search over util.quantize_embeddings(docs, "ubinary") on the scoring fixture (width 100: 16-byte rows): the
    reference's result contract; Hamming only equals the reference's lists; sign and fp8 re-scoring follow the rules of tests 5 / 6.
    The top-10 overlaps with the fp32 golden lists are printed, not asserted (Gaussian fixtures without neighbourhood structure)."""
    from sgpt_amd import BinaryCorpus, util
    fx = np.load(f"{GOLDEN}/scoring.npz")
    q, docs = torch.from_numpy(fx["ss_q"]), torch.from_numpy(fx["ss_docs"])
    golden = fx["ss_idx"].tolist()
    corpus = util.quantize_embeddings(docs, precision="ubinary")
    assert isinstance(corpus, BinaryCorpus) and len(corpus) == 1000 and corpus.bits.shape == (1000, 16) and corpus.dim == 100
    assert corpus.center is None and corpus.fp8 is None and corpus.nbytes == 16000
    bits = corpus.bits.cpu().numpy()
    assert np.array_equal(bits, B.pack(docs.numpy()))
    qn = ctx.l2_normalize(q)
    qh = qn.cpu().numpy()
    # Hamming only
    wa, wi = B.stage1(qh, bits, 100, 10)
    val, idx, n = ctx.score_topk(qn, corpus, 10, rescore="none")
    assert n == 10 and np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), B.mode0_values(wa, 100))
    ov_none = _overlap(idx.cpu().tolist(), golden)
    assert ov_none == _overlap(wi.tolist(), golden)
    # sign re-scoring x4 (the default of semantic_search without an fp8 copy)
    hits = util.semantic_search(q, corpus, top_k=10, query_chunk_size=5, corpus_chunk_size=17)
    assert len(hits) == 20 and all(len(h) == 10 and set(h[0]) == {"corpus_id", "score"} for h in hits)
    assert all(h[i]["score"] >= h[i + 1]["score"] for h in hits for i in range(9))
    hv = np.array([[e["score"] for e in h] for h in hits], dtype=np.float32)
    hi = np.array([[e["corpus_id"] for e in h] for h in hits], dtype=np.int64)
    _, cand = B.stage1(qh, bits, 100, 40)
    B.check_rescored(hv, hi, cand, B.sign_values(qh, bits, 100), B.sign_bound(qh, 100), 10)
    ov_sign = _overlap(hi.tolist(), golden)
    # fp8 re-scoring of the same 40 candidates
    c8 = util.quantize_embeddings(docs, precision="ubinary", keep_fp8=True)
    assert c8.fp8 is not None and c8.fp8.codes.shape == (1000, 104) and c8.nbytes == 16000 + 1000 * 104 + 4000
    assert torch.equal(c8.bits, corpus.bits)
    # the copy comes from the rows of the bits' own block loop: bit for bit quantize_corpus's, over three blocks with a ragged last one
    e44 = docs[:300, :44].contiguous()
    blk8, want8 = ctx.binarize_corpus(e44, keep_fp8=True, block_rows=128).fp8, ctx.quantize_corpus(e44, normalize=True, block_rows=128)
    assert blk8.codes.shape == (300, 48) and torch.equal(blk8.codes, want8.codes) and torch.equal(blk8.scale, want8.scale)
    h8 = util.semantic_search(q, c8, top_k=10)
    v8 = np.array([[e["score"] for e in h] for h in h8], dtype=np.float32)
    i8 = np.array([[e["corpus_id"] for e in h] for h in h8], dtype=np.int64)
    rows = R.dequantize(c8.fp8.codes.cpu().numpy(), c8.fp8.scale.cpu().numpy())[:, :100]
    B.check_rescored(v8, i8, cand, R.scores64(qh, rows), 100 * 2.0 ** -23 * R.abs_products(qh, rows), 10)
    ov_fp8 = _overlap(i8.tolist(), golden)
    # centred on the corpus mean, sign re-scoring
    cc = util.quantize_embeddings(docs, precision="ubinary", center="mean")
    assert cc.center is not None and tuple(cc.center.shape) == (100,)
    hc = util.semantic_search(q, cc, top_k=10)
    ov_cent = _overlap([[e["corpus_id"] for e in h] for h in hc], golden)
    print(f"semantic_search, binary corpus: top-10 overlap with the fp32 golden lists: Hamming only {ov_none:.4f}, sign re-scoring x4 "
          f"{ov_sign:.4f}, centred + sign re-scoring x4 {ov_cent:.4f}, fp8 re-scoring x4 {ov_fp8:.4f}")
    with pytest.raises(ValueError, match="sign bits carry no norms"):
        util.semantic_search(q, corpus, score_function=util.dot_score)


def test_a_centred_corpus_is_not_rescored_with_fp8(ctx):
    """The search call takes one query matrix: the bits of a centred corpus need q - center, its fp8 copy the raw q.  score_topk refuses
    rescore="fp8" there, binarize_corpus refuses to build the pair, and semantic_search over a hand-built one re-scores with the sign
    bits -- the lists of the same corpus without the copy.  `out` of pack_sign_bits is checked before the kernel writes to it."""
    from sgpt_amd import BinaryCorpus, util
    q, c = R.unit_corpus(5, 600, 128, 7)
    with pytest.raises(ValueError, match="one query matrix"):
        ctx.binarize_corpus(c, center="mean", keep_fp8=True)
    cen = ctx.binarize_corpus(c, center="mean")
    assert np.array_equal(cen.bits.cpu().numpy(), B.pack(c.numpy(), cen.center.cpu().numpy()))
    both = BinaryCorpus(cen.bits, 128, center=cen.center, fp8=ctx.quantize_corpus(c))
    with pytest.raises(ValueError, match="one query matrix"):
        ctx.score_topk(q, both, 5, rescore="fp8")
    assert util.semantic_search(q, both, top_k=5) == util.semantic_search(q, cen, top_k=5)
    # the centred search is the uncentred one on shifted rows: stage 1 from the bits of q - center
    val, idx, n = ctx.score_topk(q, cen, 5, rescore="none")
    wa, wi = B.stage1(q.numpy() - cen.center.cpu().numpy()[None, :], cen.bits.cpu().numpy(), 128, 5)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(val.cpu().numpy(), B.mode0_values(wa, 128))
    with pytest.raises(ValueError, match="BinaryCorpus only"):
        ctx.score_topk(q, c.cuda(), 5, rescore="none")
    for bad in (torch.empty((7, 12), dtype=torch.uint8, device="cuda"), torch.empty((7, 16), dtype=torch.int8, device="cuda"),
                torch.empty((7, 16), dtype=torch.uint8), torch.empty((7, 32), dtype=torch.uint8, device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            ctx.pack_sign_bits(q, out=bad)

