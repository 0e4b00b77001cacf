"""The CPU reference of the binary-corpus scorer (tests/scorebits_ref.py) against itself, the ABI v19 bindings, and the argument
refusals of the Python surface that need no device."""
import numpy as np
import pytest
import torch

import scorebits_ref as B
from score8_ref import unit_corpus


def test_abi_v19_names_are_bound():
    from sgpt_amd import _lib
    assert _lib.SGPT_ABI_VERSION >= 19
    assert "sgpt_pack_sign_bits" in _lib.SIGNATURES and "sgpt_score_topk_bits" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sgpt_pack_sign_bits"][1]) == 8 and len(_lib.SIGNATURES["sgpt_score_topk_bits"][1]) == 18


@pytest.mark.parametrize("d", [1, 31, 32, 100, 768])
def test_agreement_is_the_sign_dot_product(d):
    """d - 2 * hamming equals <sign q, sign d> with signs +-1 over the true dimensions; pad bits are zero and cancel; the word
    population count and the 256-entry table agree."""
    q, c = unit_corpus(d, 300, d, 5)
    q, c = q.numpy(), c.numpy() - 0.01
    qb, cb = B.pack(q), B.pack(c)
    assert qb.shape == (5, B.ldb_of(d)) and cb.shape == (300, 4 * ((d + 31) // 32))
    assert np.array_equal(cb[:, :(d + 7) // 8], np.packbits(c > 0, axis=-1)) and not cb[:, (d + 7) // 8:].any()
    if d % 8:
        assert not (cb[:, d // 8] & ((1 << (8 - d % 8)) - 1)).any()          # the pad bits of the last true byte
    h = B.hamming(qb, cb)
    assert np.array_equal(h, B.hamming_words(qb, cb))
    sq, sc = np.where(q > 0, 1, -1), np.where(c > 0, 1, -1)
    assert np.array_equal(B.agreement(qb, cb, d), sq @ sc.T)
    assert np.array_equal(B.signs(cb, d), sc.astype(np.float64))
    assert np.array_equal(B.sign_values(q, cb, d), q.astype(np.float64) @ sc.T.astype(np.float64) / np.sqrt(np.float64(d)))


def test_pack_rule_on_special_values():
    x = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0, 3.0]], dtype=np.float32)
    assert np.unpackbits(B.pack(x), axis=-1)[0, :10].tolist() == [0, 0, 0, 1, 0, 1, 0, 1, 0, 1]
    assert np.unpackbits(B.pack(x, center=np.full(10, 2.0, dtype=np.float32)), axis=-1)[0, :10].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1]


def test_stage1_order_and_mode0_values():
    bits = np.zeros((6, 4), dtype=np.uint8)
    bits[[1, 4]] = 0xff                                       # documents 1 and 4 equal an all-positive query over d = 32
    bits[2, 0] = 0xf0
    a, i = B.stage1(np.ones((1, 32), dtype=np.float32), bits, 32, 4, idx_base=10)
    assert a.tolist() == [[32, 32, -24, -32]] and i.tolist() == [[11, 14, 12, 10]]
    assert B.mode0_values(a, 32).tolist() == [[1.0, 1.0, -0.75, -1.0]] and B.mode0_values(a, 32).dtype == np.float32


@pytest.fixture
def no_device(monkeypatch):
    """Whatever reaches for the device context stops there -- on any machine."""
    import sgpt_amd.runtime as RT
    import sgpt_amd.util as U

    class Reached(Exception):
        pass

    def stop(device=None):
        raise Reached
    monkeypatch.setattr(U, "get_context", stop)
    monkeypatch.setattr(RT, "get_context", stop)
    return Reached


def test_python_refusals_need_no_device(no_device):
    from sgpt_amd import BinaryCorpus, QuantizedCorpus, util
    emb = torch.zeros(4, 16)
    for bad in ("int8", "binary", "FP8", None):              # (unchanged: the new precision is spelled "ubinary")
        with pytest.raises(ValueError) as e:
            util.quantize_embeddings(emb, precision=bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="normalize=False"):
        util.quantize_embeddings(emb, precision="ubinary", normalize=False)
    with pytest.raises(no_device):                           # "ubinary" is accepted and goes on to the device
        util.quantize_embeddings(emb, precision="ubinary")
    with pytest.raises(no_device):
        util.quantize_embeddings(emb, precision="ubinary", center="mean")
    with pytest.raises(no_device):
        util.quantize_embeddings(emb, precision="ubinary", keep_fp8=True)
    with pytest.raises(ValueError, match="one query matrix"):  # a centre and an fp8 copy cannot share the call's one query matrix
        util.quantize_embeddings(emb, precision="ubinary", center="mean", keep_fp8=True)
    bc = BinaryCorpus(torch.zeros(4, 4, dtype=torch.uint8), 16)
    assert len(bc) == 4 and bc.nbytes == 16 and not isinstance(bc, QuantizedCorpus)
    fp8 = QuantizedCorpus(torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), normalized=True, dim=16)
    full = BinaryCorpus(torch.zeros(4, 4, dtype=torch.uint8), 16, center=torch.zeros(16), fp8=fp8)
    assert full.nbytes == 16 + 16 * 4 + (4 * 16 + 4 * 4)
    with pytest.raises(ValueError, match="bytes per row"):
        BinaryCorpus(torch.zeros(4, 4, dtype=torch.uint8), 33)
    with pytest.raises(ValueError, match="same rows"):
        BinaryCorpus(torch.zeros(5, 4, dtype=torch.uint8), 16, fp8=fp8)
    # what semantic_search re-scores with: fp8 only where the corpus has the copy and no centre
    plain8 = BinaryCorpus(torch.zeros(4, 4, dtype=torch.uint8), 16, fp8=fp8)
    assert [util._binary_rescore(c) for c in (bc, plain8, full)] == ["sign", "fp8", "sign"]
    q = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="top_k <= 1024"):
        util.semantic_search(q, BinaryCorpus(torch.zeros(2000, 4, dtype=torch.uint8), 16), top_k=1025)
    with pytest.raises(ValueError, match="sign bits carry no norms"):
        util.semantic_search(q, bc, score_function=util.dot_score)
    with pytest.raises(ValueError, match="sign bits carry no norms"):
        util.semantic_search(q, bc, score_function=lambda a, b: a @ b.T)
    with pytest.raises(no_device):                           # cos_sim goes on to the device
        util.semantic_search(q, bc, score_function=util.cos_sim)
