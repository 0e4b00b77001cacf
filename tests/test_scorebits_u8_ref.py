"""CPU tests of the reference of the binary corpus with a uint8 second stage (tests/scorebits_u8_ref.py), of the Python surface's new
refusals, and of what the uint8 second stage buys on the clustered anisotropic fixture."""
import numpy as np
import pytest
import torch

import score8_ref as R8
import scorebits_ref as B
import scorebits_u8_ref as BU
import scoreu8_ref as U


def _case(d, N=300, nq=5, seed=3):
    q, c = R8.unit_corpus(seed + d, N, d, nq)
    q, c = q.numpy(), c.numpy()
    center = c.astype(np.float64).mean(axis=0).astype(np.float32)
    start, step = U.ranges(c)
    return q, c, center, B.pack(c, center), U.quantize_rows(c, start, step), start, step


@pytest.mark.parametrize("d", [100, 128])
def test_reference_pipeline(d):
    """Candidates equal stage1(q - center); values equal the de-quantised dot products; the order is value descending, ties to the lowest
    index; pad columns contribute nothing (d = 100: 28 of them)."""
    q, c, center, bits, codes, start, step = _case(d)
    k, kp, base = 11, 44, 3
    val, idx, cand = BU.pipeline(q, center, bits, codes, start, step, k, kp, idx_base=base)
    _, want_cand = B.stage1(q - center[None, :], bits, d, kp, idx_base=base)
    assert np.array_equal(cand, want_cand) and cand.shape == (5, kp)
    assert not np.array_equal(cand, B.stage1(q, bits, d, kp, idx_base=base)[1])        # (the centre changes the candidates)
    rows = U.dequantize(codes, start, step)
    assert rows.shape[1] == U.ld_of(d) and np.array_equal(rows[:, d:], np.zeros((300, U.ld_of(d) - d)))
    full = q.astype(np.float64) @ rows[:, :d].T
    assert np.array_equal(BU.values64(q, codes, start, step), full)
    assert np.all(codes[:, d:] == 128) and np.all(step[d:] == 0) and np.all(start[d:] == 0)   # the kernel's loop over ld: q' = 0, c = 0 there
    for m in range(5):
        assert set(idx[m].tolist()) <= set(cand[m].tolist())
        assert np.array_equal(val[m], full[m, idx[m] - base])
        order = cand[m][np.lexsort((cand[m], -full[m, cand[m] - base]))][:k]
        assert np.array_equal(idx[m], order)
    # the device form qbias + <q', code - 128> is the same number, and within the bound of it when rounded as the kernel rounds
    st, lo = step.astype(np.float64)[:d], start.astype(np.float64)[:d]
    form = (q.astype(np.float64) * (lo + 128.0 * st)).sum(axis=1)[:, None] + (q.astype(np.float64) * st) @ (codes[:, :d].astype(np.float64) - 128.0).T
    bound = BU.bound(q, codes, start, step)
    assert np.all(np.abs(form - full) <= 1e-6 * bound)
    qs32 = q * step[None, :d]
    qb32 = (q * (start + np.float32(128) * step)[None, :d]).sum(axis=1, dtype=np.float32)
    dev = (qs32 @ (codes[:, :d].astype(np.float32) - np.float32(128)).T + qb32[:, None]).astype(np.float32)
    assert np.all(np.abs(dev.astype(np.float64) - full) <= bound) and np.all(bound < 1e-4)


def test_reference_rescore_slots():
    q, c, center, bits, codes, start, step = _case(128)
    idx = np.array([[3, 302, 303, 2, -1, 150]] * 5, dtype=np.int64)
    val, out = BU.rescore(q, codes, start, step, idx, idx_base=3)
    full = BU.values64(q, codes, start, step)
    assert np.array_equal(out, np.array([[3, 302, -1, -1, -1, 150]] * 5))
    assert np.array_equal(val[:, [0, 1, 5]], full[:, [0, 299, 147]]) and np.all(np.isneginf(val[:, [2, 3, 4]]))
    qn = q.copy()
    qn[1, 7] = np.nan
    vn, _ = BU.rescore(qn, codes, start, step, idx, idx_base=3)
    assert np.all(vn[1, [0, 1, 5]] == -1.0) and np.all(np.isneginf(vn[1, [2, 3, 4]])) and np.array_equal(vn[0], val[0])


@pytest.fixture
def no_device(monkeypatch):
    """Whatever reaches for the device context stops there -- on any machine."""
    import sgpt_amd.runtime as RT
    import sgpt_amd.util as U_

    class Reached(Exception):
        pass

    def stop(device=None):
        raise Reached
    monkeypatch.setattr(U_, "get_context", stop)
    monkeypatch.setattr(RT, "get_context", stop)
    return Reached


def test_surface_without_a_device(no_device):
    from sgpt_amd import BinaryCorpus, QuantizedCorpus, Uint8Corpus, _lib, util
    assert _lib.SGPT_ABI_VERSION >= 21
    assert "sgpt_score_topk_bits_u8" in _lib.SIGNATURES and "sgpt_u8_rescore" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sgpt_score_topk_bits_u8"][1]) == 20 and len(_lib.SIGNATURES["sgpt_u8_rescore"][1]) == 16
    emb = torch.zeros(4, 16)
    for prec in ("fp8", "uint8"):                            # keep_uint8 belongs to "ubinary", like keep_fp8
        with pytest.raises(ValueError, match="keep_uint8"):
            util.quantize_embeddings(emb, precision=prec, keep_uint8=True)
    with pytest.raises(ValueError, match="keep_uint8"):      # ranges without the uint8 copy they would apply to
        util.quantize_embeddings(emb, precision="ubinary", ranges=np.zeros((2, 16)))
    with pytest.raises(ValueError, match="keep_uint8"):
        util.quantize_embeddings(emb, precision="ubinary", calibration_embeddings=emb)
    with pytest.raises(ValueError, match="not both"):
        util.quantize_embeddings(emb, precision="ubinary", keep_uint8=True, ranges=np.zeros((2, 16)), calibration_embeddings=emb)
    with pytest.raises(ValueError, match="'int8'"):
        util.quantize_embeddings(emb, precision="int8", keep_uint8=True)
    for kw in (dict(), dict(center="mean"), dict(keep_fp8=True), dict(ranges=np.stack([-np.ones(16), np.ones(16)])),
               dict(calibration_embeddings=emb[:2])):        # accepted, with or without a centre: goes on to the device
        with pytest.raises(no_device):
            util.quantize_embeddings(emb, precision="ubinary", keep_uint8=True, **kw)
    codes = torch.full((4, 128), 128, dtype=torch.uint8)
    u8 = Uint8Corpus(codes, torch.zeros(128), torch.zeros(128), normalized=True, dim=16)
    fp8 = QuantizedCorpus(torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), normalized=True, dim=16)
    bits = torch.zeros(4, 4, dtype=torch.uint8)
    plain, with8 = BinaryCorpus(bits, 16), BinaryCorpus(bits, 16, fp8=fp8)
    both = BinaryCorpus(bits, 16, center=torch.zeros(16), fp8=fp8, u8=u8)
    assert plain.u8 is None and both.u8 is u8
    assert both.nbytes == 16 + 16 * 4 + (4 * 16 + 4 * 4) + (4 * 128 + 2 * 128 * 4)
    with pytest.raises(ValueError, match="same rows"):
        BinaryCorpus(torch.zeros(5, 4, dtype=torch.uint8), 16, u8=u8)
    with pytest.raises(ValueError, match="same rows"):
        BinaryCorpus(bits, 17, u8=u8)
    with pytest.raises(ValueError, match="same rows"):
        BinaryCorpus(bits, 16, u8=fp8)
    # what semantic_search re-scores with: the uint8 copy where there is one, today's answer otherwise
    assert [util._binary_rescore(c) for c in (plain, with8, BinaryCorpus(bits, 16, u8=u8), both, BinaryCorpus(bits, 16, fp8=fp8, u8=u8))] == \
        ["sign", "fp8", "uint8", "uint8", "uint8"]


def test_uint8_rescoring_ranks_better_than_sign_and_no_worse_than_fp8():
    """The clustered anisotropic fixture (scripts/score_bits_u8_quality.py), bits centred on the corpus mean, k = 10 of kp = 40: the
    top-10 overlap with the float64 ranking of uint8 re-scoring is strictly above that of sign re-scoring and not below that of fp8
    re-scoring of the same candidates.  (Printed, not asserted: 0.89 / 0.59 / 0.83.)"""
    x, q = BU.clustered_anisotropic()
    d = x.shape[1]
    _, gold = R8.topk_lowest_index(q.astype(np.float64) @ x.astype(np.float64).T, 10)
    center = x.astype(np.float64).mean(axis=0).astype(np.float32)
    bits = B.pack(x, center)
    qc = BU.centred(q, center)
    _, cand = B.stage1(qc, bits, d, 40)
    start, step = U.ranges(x)
    _, i_u8, cand_u8 = BU.pipeline(q, center, bits, U.quantize_rows(x, start, step), start, step, 10, 40)
    assert np.array_equal(cand_u8, cand)

    def top(vals):
        cv = np.take_along_axis(vals, cand, axis=1)
        return np.take_along_axis(cand, np.lexsort((cand, -cv), axis=1)[:, :10], axis=1)
    c8, s8 = R8.quantize_rows(x)
    ov_u8 = BU.overlap(i_u8, gold)
    ov_sign = BU.overlap(top(B.sign_values(qc, bits, d)), gold)
    ov_fp8 = BU.overlap(top(R8.scores64(q, R8.dequantize(c8, s8))), gold)
    print(f"top-10 overlap with float64, centred bits, kp = 40: uint8 {ov_u8:.4f}, sign {ov_sign:.4f}, fp8 {ov_fp8:.4f}; "
          f"stage-1 recall {BU.overlap(cand, gold):.4f}")
    assert ov_u8 > ov_sign and ov_u8 >= ov_fp8
