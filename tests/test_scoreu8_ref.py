"""CPU tests of the uint8 corpus reference (tests/scoreu8_ref.py) and of the Python surface's refusals: the format, the quantiser, the
query prologue, the two bounds, and what per-dimension ranges buy over fp8 on the anisotropic fixture."""
import json

import numpy as np
import pytest
import torch

import score8_ref as R8
import scoreu8_ref as R
from helpers import GOLDEN


def test_round_trip_of_all_256_codes():
    """Every code de-quantises to a value that quantises back to it, under ranges of very different magnitudes per column."""
    start = np.zeros(128, dtype=np.float32)
    step = np.zeros(128, dtype=np.float32)
    start[:5] = [-1.0, 0.25, -3e-3, 1000.0, -0.5]
    step[:5] = [2.0 / 255, 1e-4, 3e-5, 7.0, 1.0 / 255]
    codes = np.full((256, 128), 128, dtype=np.uint8)
    codes[:, :5] = np.arange(256, dtype=np.uint8)[:, None]
    rows32 = R.dequantize32(codes, start, step)
    assert np.array_equal(R.quantize_rows(rows32[:, :5], start, step), codes)
    assert np.array_equal(R.dequantize(codes, start, step)[:, 5:], np.zeros((256, 123)))       # pad columns: 0 + 128 * 0
    assert np.abs(R.dequantize(codes, start, step) - rows32).max() <= 2.0 ** -23 * 2785.0       # (fp32 rounding of the largest value)


def test_quantiser_clamps_zero_step_nan_and_padding():
    x = np.array([[0.0, 5.0, 1.0, np.nan, 0.5], [1.0, -5.0, 1.0, 0.3, 2.5], [127.5 / 256, 0.0, 1.0, 0.7, 1.5]], dtype=np.float32)
    start = np.zeros(128, dtype=np.float32)
    step = np.zeros(128, dtype=np.float32)
    start[:5] = [0.0, -1.0, 1.0, 0.0, 0.0]
    step[:5] = [1.0 / 256, 1.0 / 128, 0.0, 1.0 / 255, 1.0]           # (powers of two: the quotients below are exact)
    codes = R.quantize_rows(x, start, step)
    assert codes.shape == (3, 128) and codes.dtype == np.uint8
    assert codes[:, 0].tolist() == [0, 255, 128]              # 0, 256 clamped, and 127.5 rounds half to even
    assert codes[:, 1].tolist() == [255, 0, 128]              # outside the range: clamped
    assert codes[:, 2].tolist() == [128, 128, 128]            # step == 0
    assert codes[0, 3] == 128                                 # NaN element
    assert codes[:, 4].tolist() == [0, 2, 2]                  # 0.5 -> 0, 2.5 -> 2, 1.5 -> 2: round-half-even
    assert (codes[:, 5:] == 128).all()                        # pad columns
    s, t = R.ranges(x[:, [0, 1, 4]])
    assert s.shape == (128,) and s[:3].tolist() == [0.0, -5.0, 0.5] and np.array_equal(t[:3], np.float32([1, 10, 2]) / np.float32(255))
    assert (s[3:] == 0).all() and (t[3:] == 0).all()


def test_quantiser_case_of_the_gpu_test_has_few_near_half_elements():
    """The GPU test of the quantiser accepts either neighbour where the float64 quotient is within 1e-4 of a half-integer; for its seed
    such elements are at most 0.1 % of all (a uniform fraction gives 0.02 %), and numpy's fp32 differs from the float64 rule only there."""
    x = R.row_kernel_case()
    start, step = R.ranges(x[::3])
    t64 = R.quotient64(x, start, step)
    near = R.near_half(t64)
    print(f"{near.sum()} of {near.size} elements within 1e-4 of a half step ({near.mean():.2e})")
    assert near.mean() <= 1e-3
    live = np.isfinite(t64)
    want = np.where(live, np.clip(np.rint(np.where(live, t64, 0)), 0, 255), 128).astype(np.uint8)
    codes = R.quantize_rows(x, start, step)[:, :x.shape[1]]
    assert ((codes == want) | near).all() and (codes[:, 17] == 128).all()
    assert (codes == 0).any() and (codes == 255).any()        # ranges from every third row: the rest clamps


def test_prologue_properties():
    g = np.random.default_rng(5)
    d = 200
    x = g.standard_normal((50, d)).astype(np.float32) * np.geomspace(1e-3, 10, d).astype(np.float32)[None, :]
    start, step = R.ranges(x)
    q = g.standard_normal((7, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[3] = 0
    q[5] *= 1e-6
    q2, qscale, qbias = R.prepare_queries(q, start, step)
    assert q2.shape == (7, 256) and q2.dtype == np.float16 and (q2[:, d:] == 0).all()
    amax = np.abs(q2.astype(np.float64)).max(axis=1)
    live = [0, 1, 2, 4, 5, 6]
    assert np.all(amax[live] >= 1) and np.all(amax[live] < 2)
    assert amax[3] == 0 and qscale[3] == 1 and qbias[3] == 0 and (q2[3] == 0).all()
    m, e = np.frexp(qscale.astype(np.float64))
    assert np.all(m == 0.5)                                   # powers of two
    # the decomposition: qbias + qscale <q'', c> is <q, x^> up to the f16 rounding of q'' (relative 2^-11 per element)
    codes = R.quantize_rows(x, start, step)
    want = q.astype(np.float64) @ R.dequantize(codes, start, step)[:, :d].T
    got = R.exact_scores(q2, qscale, qbias, codes)
    slack = 2.0 ** -11 * qscale.astype(np.float64)[:, None] * R.abs_products(q2, codes) * (1 + 2.0 ** -10) + 1e-12
    assert np.all(np.abs(got - want) <= slack)


def test_kernel_arithmetic_stays_within_the_arithmetic_bound():
    """The kernel's arithmetic, modelled in numpy (fp32 accumulation over k slices, one fma), against the exact score of the same
    operands: within the derived bound, on unit rows at d = 768 and on a width that needs padding."""
    for seed, N, d, nq in ((7, 3000, 768, 16), (8, 1000, 100, 5)):
        q, c = R8.unit_corpus(seed, N, d, nq)
        q, c = q.numpy(), c.numpy()
        start, step = R.ranges(c)
        codes = R.quantize_rows(c, start, step)
        q2, qscale, qbias = R.prepare_queries(q, start, step)
        qb32 = qbias.astype(np.float32)
        exact = R.exact_scores(q2, qscale, qb32, codes)
        err = np.abs(R.kernel_model(q2, qscale, qb32, codes).astype(np.float64) - exact)
        bound = R.arithmetic_bound(q2, qscale, codes, exact, d)
        print(f"d={d}: max |model - exact| = {err.max():.3e}, smallest bound = {bound.min():.3e}")
        assert np.all(err <= bound)


def _fixture():
    fx = np.load(f"{GOLDEN}/scoring.npz")
    meta = json.loads(str(fx["es_json"]))
    cn = torch.nn.functional.normalize(torch.from_numpy(fx["es_corpus_emb"]), dim=1).numpy()
    qn = torch.nn.functional.normalize(torch.from_numpy(fx["es_query_emb"]), dim=1).numpy()
    return meta, qn, cn


def _overlap10(meta, scores):
    want = meta["results"]["cos_sim"]
    _, order = R.topk_lowest_index(scores, scores.shape[1])
    out = []
    for r, qid in enumerate(meta["queries"]):
        mine = [f"d{i}" for i in order[r].tolist() if f"d{i}" != qid][:10]
        ref10 = sorted(want[qid], key=want[qid].get, reverse=True)[:10]
        out.append(len(set(mine) & set(ref10)) / len(ref10))
    return float(np.mean(out))


def test_quantisation_bound_and_overlap_on_the_anisotropic_fixture():
    """tests/golden/scoring.npz es_* (700 x 96, 13 queries, a few channels carry the row): every score from the uint8 rows within
    sum |q_j| step_j / 2 of the fp32 rows' score, and the top-10 overlap with the fixture's ranking strictly above the fp8 reference's on
    the same rows (0.97 against 0.80)."""
    meta, qn, cn = _fixture()
    start, step = R.ranges(cn)
    codes = R.quantize_rows(cn, start, step)
    s64 = qn.astype(np.float64) @ cn.astype(np.float64).T
    su8 = qn.astype(np.float64) @ R.dequantize(codes, start, step)[:, :cn.shape[1]].T
    err = np.abs(su8 - s64)
    assert np.all(err <= R.quantisation_bound(qn, cn, start, step))
    c8, s8 = R8.quantize_rows(cn)
    sf8 = qn.astype(np.float64) @ R8.dequantize(c8, s8).T
    o_u8, o_f8 = _overlap10(meta, su8), _overlap10(meta, sf8)
    print(f"uint8: max |dcos| = {err.max():.3e}, top-10 overlap = {o_u8:.4f}; fp8: max |dcos| = {np.abs(sf8 - s64).max():.3e}, overlap = {o_f8:.4f}")
    assert o_u8 > o_f8
    # ranges from a calibration subset: the rest clamps, and the bound's clamp term covers it
    start_c, step_c = R.ranges(cn[::7])
    codes_c = R.quantize_rows(cn, start_c, step_c)
    err_c = np.abs(qn.astype(np.float64) @ R.dequantize(codes_c, start_c, step_c)[:, :cn.shape[1]].T - s64)
    assert (codes_c == 0).any() and (codes_c[:, :cn.shape[1]] == 255).any()
    assert np.all(err_c <= R.quantisation_bound(qn, cn, start_c, step_c))


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
    from sgpt_amd import QuantizedCorpus, Uint8Corpus, util
    emb = torch.zeros(4, 16)
    with pytest.raises(ValueError, match="'int8'") as e:       # the signed spelling stays refused, and says where to go
        util.quantize_embeddings(emb, precision="int8")
    assert '"uint8"' in str(e.value)
    for bad in ("UINT8", "binary", None):
        with pytest.raises(ValueError) as e:
            util.quantize_embeddings(emb, precision=bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(no_device):                           # "uint8" is accepted and goes on to the device
        util.quantize_embeddings(emb, precision="uint8")
    with pytest.raises(no_device):
        util.quantize_embeddings(emb, precision="uint8", ranges=np.stack([-np.ones(16), np.ones(16)]))
    with pytest.raises(no_device):
        util.quantize_embeddings(emb, precision="uint8", calibration_embeddings=emb[:2], normalize=False)
    for prec in ("fp8", "ubinary"):                          # the new keywords belong to "uint8"
        with pytest.raises(ValueError, match="belong to precision='uint8'"):
            util.quantize_embeddings(emb, precision=prec, ranges=np.zeros((2, 16)))
        with pytest.raises(ValueError, match="belong to precision='uint8'"):
            util.quantize_embeddings(emb, precision=prec, calibration_embeddings=emb)
    with pytest.raises(ValueError, match="belong to precision='ubinary'"):
        util.quantize_embeddings(emb, precision="uint8", center="mean")
    with pytest.raises(ValueError, match="belong to precision='ubinary'"):
        util.quantize_embeddings(emb, precision="uint8", keep_fp8=True)
    with pytest.raises(ValueError, match="not both"):
        util.quantize_embeddings(emb, precision="uint8", ranges=np.zeros((2, 16)), calibration_embeddings=emb)
    codes = torch.full((4, 128), 128, dtype=torch.uint8)
    codes[:, :16] = torch.arange(64, dtype=torch.uint8).reshape(4, 16) * 4
    uc = Uint8Corpus(codes, torch.zeros(128), torch.zeros(128), normalized=True, dim=16)
    ud = Uint8Corpus(codes, torch.zeros(128), torch.zeros(128), normalized=False, dim=16)
    assert len(uc) == 4 and uc.nbytes == 4 * 128 + 2 * 128 * 4 and uc.dim == 16 and not isinstance(uc, QuantizedCorpus)
    i8 = uc.codes_int8()
    assert i8.dtype == torch.int8 and i8.shape == (4, 16) and i8[0, :3].tolist() == [-128, -124, -120] and i8[3, 15].item() == 124
    with pytest.raises(ValueError, match="ld % 128"):
        Uint8Corpus(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(16), torch.zeros(16))
    with pytest.raises(ValueError, match="do not hold dim"):
        Uint8Corpus(codes, torch.zeros(128), torch.zeros(128), dim=129)
    with pytest.raises(ValueError, match="start and step"):
        Uint8Corpus(codes, torch.zeros(16), torch.zeros(128), dim=16)
    q = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="normalize=True"):
        util.semantic_search(q, ud, score_function=util.cos_sim)
    with pytest.raises(ValueError, match="normalize=False"):
        util.semantic_search(q, uc, score_function=util.dot_score)
    with pytest.raises(ValueError, match="arbitrary score function"):
        util.semantic_search(q, uc, score_function=lambda a, b: a @ b.T)
    with pytest.raises(no_device):                           # the matching pairs go on to the device
        util.semantic_search(q, uc, score_function=util.cos_sim)
    with pytest.raises(no_device):
        util.semantic_search(q, ud, score_function=util.dot_score)
