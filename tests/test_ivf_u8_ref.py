"""CPU: the numpy restatement of the IVF corpus over uint8 lists (tests/ivf_u8_ref.py) against brute force; IVFUint8Corpus validates what
it is given and refuses what its search does not serve before anything reaches for the device; the build refuses the precisions it does
not hold; the ABI carries the two entries."""
import os
import re

import numpy as np
import pytest
import torch

import ivf_ref as R
import ivf_u8_ref as R8
import scoreu8_ref as U

from sgpt_amd import _lib, util
from sgpt_amd.corpus import CORPUS_KINDS, CorpusBuilders, IVFCorpus, IVFUint8Corpus, Uint8Corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----
def test_search_over_every_list_is_brute_force_over_the_dequantised_rows():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((40, 16)).astype(np.float32)
    x[10:14] = x[10]                                     # four equal rows: equal codes, equal values
    q = np.stack([x[10], x[3] + 0.1]).astype(np.float32)
    start, step = U.ranges(x)
    offsets, perm = R.lists(rng.integers(0, 5, 40), 5)
    codes = U.quantize_rows(x, start, step)[perm]
    assert codes.shape == (40, 128) and (codes[:, 16:] == 128).all() and codes[:, :16].min() == 0 and codes[:, :16].max() == 255
    val, idx, cands = R8.search_u8(q, codes, start, step, perm, offsets, np.tile(np.arange(5), (2, 1)), 12)
    rows = start[None, :16].astype(np.float64) + codes[:, :16].astype(np.float64) * step[None, :16].astype(np.float64)
    s = q.astype(np.float64) @ rows.T                    # brute force, list-major positions
    for i in range(2):
        o = R.library_order(s[i], perm)[:12]
        # (two float64 sums of 16 terms in different orders: 16 * 2^-53 relative of sum |terms| < 1e2)
        assert np.array_equal(idx[i], perm[o]) and np.allclose(val[i], s[i][o], rtol=0, atol=1e-12) and len(cands[i]) == 40
    tied = idx[0][np.isin(idx[0], np.arange(10, 14))]
    assert len(tied) == 4 and (np.diff(tied) > 0).all()
    assert (np.abs(R8.values64(q, codes, start, step) - q.astype(np.float64) @ x[perm].astype(np.float64).T)
            <= U.quantisation_bound(q, x[perm], start, step) + 1e-12).all()
    # one probed list, idx_base, a running list
    v1, i1, c1 = R8.search_u8(q, codes, start, step, perm, offsets, np.full((2, 1), 2), 30, idx_base=100)
    n2 = offsets[3] - offsets[2]
    assert len(c1[0]) == n2 and (i1[:, n2:] == -1).all() and np.isinf(v1[:, n2:]).all() and (i1[:, :n2] >= 100).all()


def test_rounding_count_follows_the_lane_groups():
    # d -> ld, G, rounds: 8 -> 128, 8, 1; 136 -> 256, 16, 1; 264 -> 384, 32, 1; 768 -> 768, 64, 1; 1032 -> 1152, 64, 2; 2056 -> 2176, 64, 3
    assert [R8.lanes_per_row(U.ld_of(d)) for d in (8, 136, 264, 512, 768, 1032, 2056)] == [8, 16, 32, 32, 64, 64, 64]
    assert [R8.score_roundings(d) for d in (8, 136, 264, 768, 1032, 2056, 4096)] == [13, 13, 14, 15, 18, 22, 28]
    assert R.gamma(28) < 2e-6


def test_build_quantises_the_f16_rows_of_the_same_lists():
    x, _ = R.clustered_fixture(n=512, clusters=6, nq=2)
    c, codes, start, step, ids, offsets, rows16 = R8.build_u8(x, 4, 3, 0)
    c0, rows0, ids0, offsets0 = R.build(x, 4, 3, 0)
    assert np.array_equal(c, c0) and np.array_equal(ids, ids0) and np.array_equal(offsets, offsets0) and np.array_equal(rows16, rows0)
    assert codes.shape == (512, 128) and np.array_equal(codes, U.quantize_rows(rows16.astype(np.float32), start, step))
    assert np.array_equal(start[:128], rows16.astype(np.float32).min(axis=0))


# ---- IVFUint8Corpus: constructor validation, every refusal of check_search (device-free) ----
def _index(nlist=4, d=16, N=40, **kw):
    ld = (d + 127) // 128 * 128
    parts = dict(centroids=torch.zeros(nlist, d), codes=torch.zeros(N, ld, dtype=torch.uint8), start=torch.zeros(ld), step=torch.zeros(ld),
                 ids=torch.arange(N), offsets=torch.zeros(nlist + 1, dtype=torch.int64), max_list=N)
    parts.update(kw)
    return IVFUint8Corpus(**parts)


def test_ivf_uint8_corpus_holds_its_format():
    ix = _index()
    assert isinstance(ix, CORPUS_KINDS) and not isinstance(ix, IVFCorpus)
    assert len(ix) == 40 and ix.dim == 16 and ix.nlist == 4 and ix.nprobe == 4 and ix.data is ix.codes
    assert ix.centroids16.dtype == torch.float16 and tuple(ix.centroids16.shape) == (4, 16)
    assert ix.nbytes == 4 * 16 * 4 + 4 * 16 * 2 + 40 * 128 + 2 * 128 * 4 + 40 * 8 + 5 * 8
    view = ix.with_nprobe(2)
    assert type(view) is IVFUint8Corpus and view.nprobe == 2 and ix.nprobe == 4 and view.codes is ix.codes and view.centroids is ix.centroids
    assert _index(nlist=64, N=70).nprobe == 32
    u8 = ix.as_uint8_corpus()
    assert isinstance(u8, Uint8Corpus) and u8.codes is ix.codes and u8.start is ix.start and u8.step is ix.step and u8.dim == 16 and u8.normalized
    assert _index(d=136).codes.shape[1] == 256


@pytest.mark.parametrize("kw, text", [
    (dict(centroids=torch.zeros(4, 16, dtype=torch.float16)), "centroids are fp32"),
    (dict(centroids=torch.zeros(4, 12)), "d % 8 == 0"),
    (dict(codes=torch.zeros(40, 128, dtype=torch.int8)), "codes are uint8"),
    (dict(codes=torch.zeros(40, 128, dtype=torch.float16)), "codes are uint8"),
    (dict(codes=torch.zeros(40, 100, dtype=torch.uint8)), "ld % 128 == 0"),
    (dict(codes=torch.zeros(40, 256, dtype=torch.uint8), start=torch.zeros(256), step=torch.zeros(256)), "do not hold dim = 16"),
    (dict(dim=24), "do not hold dim = 24"),
    (dict(start=torch.zeros(16)), "start must be fp32 [128]"),
    (dict(step=torch.zeros(128, dtype=torch.float64)), "step must be fp32 [128]"),
    (dict(ids=torch.arange(39)), "ids must be int64 [40]"),
    (dict(ids=torch.arange(40, dtype=torch.int32)), "ids must be int64"),
    (dict(offsets=torch.zeros(4, dtype=torch.int64)), "offsets must be int64 [5]"),
    (dict(offsets=torch.zeros(5, dtype=torch.int32)), "offsets must be int64"),
    (dict(centroids16=torch.zeros(4, 8, dtype=torch.float16)), "centroids16 must be f16"),
    (dict(max_list=41), "max_list"),
    (dict(max_list=-1), "max_list"),
    (dict(nprobe=0), "nprobe"),
    (dict(nprobe=5), "nprobe"),
    (dict(nprobe=2.0), "nprobe"),
])
def test_ivf_uint8_corpus_refuses_a_bad_format(kw, text):
    with pytest.raises(ValueError, match=re.escape(text)) as e:
        _index(**kw)
    assert str(e.value).startswith("IVFUint8Corpus: ")


def test_check_search_refusals_are_device_free(monkeypatch):
    from sgpt_amd import runtime

    def no_device(*a, **k):
        raise AssertionError("a refusal reached for the device")
    monkeypatch.setattr(runtime, "get_context", no_device)
    ix = _index()
    q = torch.zeros(2, 16)
    assert ix.check_search(util.cos_sim, 1024) is True
    with pytest.raises(ValueError, match="over an IVFUint8Corpus scores with cos_sim only"):
        util.semantic_search(q, ix, score_function=util.dot_score)
    with pytest.raises(ValueError, match="cos_sim only"):
        util.semantic_search(q, ix, score_function=lambda a, b: a @ b.T)
    with pytest.raises(ValueError, match="top_k <= 1024, got 1025"):
        util.semantic_search(q, ix, top_k=1025)
    ix.nprobe = 9
    with pytest.raises(ValueError, match="IVFUint8Corpus: nprobe"):
        util.semantic_search(q, ix)
    for kw in (dict(rescore="fp8", rescore_multiplier=4), dict(rescore="sign", rescore_multiplier=2)):
        with pytest.raises(ValueError, match="BinaryCorpus only"):
            _index().score_topk(None, q, 1, 0, None, None, **kw)
    with pytest.raises(ValueError, match="dtype must be None"):
        _index().score_topk(None, q, 1, 0, None, torch.float16, "sign", 4)


def test_the_build_refuses_other_precisions_before_the_device(monkeypatch):
    from sgpt_amd import runtime

    def no_device(*a, **k):
        raise AssertionError("a refusal reached for the device")
    monkeypatch.setattr(runtime, "get_context", no_device)
    monkeypatch.setattr(util, "get_context", no_device)
    x = torch.zeros(64, 16)
    for build in (util.build_ivf_index, lambda *a, **k: CorpusBuilders.ivf_index(None, *a, **k)):      # (no Context: nothing of it is touched)
        with pytest.raises(ValueError, match="precision 'int8' is not built .* precision=\"uint8\""):
            build(x, nlist=4, precision="int8")
        with pytest.raises(ValueError, match="unknown precision 'fp8'"):
            build(x, nlist=4, precision="fp8")
        with pytest.raises(ValueError, match="ranges / calibration_embeddings belong to precision='uint8'"):
            build(x, nlist=4, ranges=torch.zeros(2, 16))
        with pytest.raises(ValueError, match="ranges / calibration_embeddings belong to precision='uint8'"):
            build(x, nlist=4, precision="f16", calibration_embeddings=x)
        with pytest.raises(ValueError, match="not both"):
            build(x, nlist=4, precision="uint8", ranges=torch.zeros(2, 16), calibration_embeddings=x)


# ---- the ABI ----
def test_abi_v27_declares_the_two_entries():
    assert _lib.SGPT_ABI_VERSION >= 27
    header = open(os.path.join(ROOT, "include", "sgpt_hip.h")).read()
    assert int(re.search(r"#define SGPT_ABI_VERSION (\d+)", header).group(1)) == _lib.SGPT_ABI_VERSION
    for name, nargs in (("sgpt_u8_gather_quantize_rows", 12), ("sgpt_ivf_search_u8", 23)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        proto = re.search(r"sgpt_status " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == nargs
    assert len(_lib.SIGNATURES["sgpt_ivf_search"][1]) == 20 and len(_lib.SIGNATURES["sgpt_gather_rows"][1]) == 9      # (the f16 entries stay)
