"""The CPU reference of the fp8 corpus scorer (tests/score8_ref.py) against itself, and the argument refusals of the Python surface
that need no device."""
import numpy as np
import pytest
import torch

import score8_ref as R

SEEDS = (1, 16, 64)          # the seeds of tests/test_gpu_score8.py (one per query count)


def test_decode_times_scale_round_trips_torch_cast():
    """Every code decodes to the value torch's float8_e4m3fn gives; quantise -> de-quantise reproduces torch's cast of row / scale; the
    scales are the tightest powers of two; every de-quantised value of a unit row is an f16 value."""
    allc = np.arange(256, dtype=np.uint8)
    v = R.decode_e4m3(allc)
    assert np.isnan(v[0x7f]) and np.isnan(v[0xff]) and np.isnan(v).sum() == 2
    assert v[0x7e] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x81] == -2.0 ** -9
    back = torch.from_numpy(np.nan_to_num(v).astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    ok = ~np.isnan(v) & (allc != 0x80)                      # (-0 encodes as 0x80 or 0x00: both zero)
    assert np.array_equal(back[ok], allc[ok])
    _, c = R.unit_corpus(3, 500, 128, 1)
    codes, scale = R.quantize_rows(c.numpy())
    assert np.all(np.log2(scale) == np.round(np.log2(scale)))
    amax = np.abs(c.numpy()).max(axis=1)
    assert np.all(amax / scale <= 448) and np.all(amax / scale > 224)
    deq = R.dequantize(codes, scale)
    want = (torch.from_numpy(c.numpy() / scale[:, None]).to(torch.float8_e4m3fn).to(torch.float64).numpy()) * scale[:, None].astype(np.float64)
    assert np.array_equal(deq, want)
    assert np.array_equal(deq.astype(np.float16).astype(np.float64), deq)        # exact in f16: the f16 scorer sees the same rows


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("d", [128, 768])
def test_fp32_accumulation_stays_inside_the_arithmetic_bound(seed, d):
    q, c = R.unit_corpus(seed, 300, d, 8)
    codes, scale = R.quantize_rows(c.numpy())
    rows = R.dequantize(codes, scale)
    q16 = q.to(torch.float16).numpy()
    ref = R.scores64(q16, rows)
    acc = np.zeros(ref.shape, dtype=np.float32)
    qf, rf = q16.astype(np.float32), rows.astype(np.float32)
    for i in range(d):                                       # sequential fp32 accumulation, k ascending
        acc = (acc + qf[:, i:i + 1] * rf[None, :, i]).astype(np.float32)
    assert np.all(np.abs(acc.astype(np.float64) - ref) <= R.arithmetic_bound(q16, rows))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("d", [128, 768])
def test_fp8_scores_stay_inside_the_quantisation_bound(seed, d):
    q, c = R.unit_corpus(seed, 300, d, 8)
    codes, scale = R.quantize_rows(c.numpy())
    s8 = R.scores64(q.numpy(), R.dequantize(codes, scale))
    s = q.numpy().astype(np.float64) @ c.numpy().astype(np.float64).T
    assert np.all(np.abs(s8 - s) <= R.quantisation_bound(q.numpy(), c.numpy(), scale))


def test_topk_tie_rule_and_nan_rows():
    s = np.array([[0.5, 2.0, 0.5, 0.5, 2.0], [1.0, 1.0, 1.0, 1.0, 1.0]])
    v, i = R.topk_lowest_index(s, 3, idx_base=10)
    assert i.tolist() == [[11, 14, 10], [10, 11, 12]] and v.tolist() == [[2.0, 2.0, 0.5], [1.0, 1.0, 1.0]]
    rows = np.ones((3, 8))
    rows[1, 2] = np.nan
    assert R.scores64(np.ones((2, 8), dtype=np.float16), rows).tolist() == [[8.0, -1.0, 8.0]] * 2


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
    from sgpt_amd import QuantizedCorpus, util
    emb = torch.zeros(4, 16)
    for bad in ("int8", "binary", "FP8", None):
        with pytest.raises(ValueError) as e:
            util.quantize_embeddings(emb, precision=bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(no_device):                           # "fp8" is accepted and goes on to the device
        util.quantize_embeddings(emb, precision="fp8")
    qc = QuantizedCorpus(torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), normalized=True)
    qd = QuantizedCorpus(torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), normalized=False)
    assert len(qc) == 4 and qc.nbytes == 4 * 16 + 4 * 4
    q = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="normalize=True"):
        util.semantic_search(q, qd, score_function=util.cos_sim)
    with pytest.raises(ValueError, match="normalize=False"):
        util.semantic_search(q, qc, score_function=util.dot_score)
    with pytest.raises(ValueError, match="arbitrary score function"):
        util.semantic_search(q, qc, score_function=lambda a, b: a @ b.T)
    with pytest.raises(no_device):                           # the matching pairs go on to the device
        util.semantic_search(q, qc, score_function=util.cos_sim)
    with pytest.raises(no_device):
        util.semantic_search(q, qd, score_function=util.dot_score)
