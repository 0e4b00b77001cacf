"""CPU: the numpy restatement of the IVF corpus (tests/ivf_ref.py) holds its own invariants; IVFCorpus validates what it is given and
refuses what its search does not serve before anything reaches for the device; the ABI carries the four entries."""
import os
import re

import numpy as np
import pytest
import torch

import ivf_ref as R

from sgpt_amd import _lib, util
from sgpt_amd.corpus import CORPUS_KINDS, IVFCorpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----
def test_lists_are_a_stable_partition():
    rng = np.random.default_rng(0)
    a = rng.integers(1, 6, 500)                          # lists 0 and 6 stay empty
    offsets, perm = R.lists(a, 7)
    assert offsets[0] == 0 and offsets[-1] == 500 and offsets[1] == 0 and offsets[6] == offsets[7]
    assert sorted(perm.tolist()) == list(range(500))
    for c in range(7):
        mine = perm[offsets[c]:offsets[c + 1]]
        assert (a[mine] == c).all() and (np.diff(mine) > 0).all()
    o2, p2 = R.lists(np.array([-5, 9, 2, 0]), 3)         # the clamp: -5 -> 0, 9 -> 2
    assert o2.tolist() == [0, 2, 2, 4] and p2.tolist() == [0, 3, 1, 2]


def test_centroids_are_unit_and_fall_back_to_prev():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    x[7] = 0
    offsets, perm = R.lists(np.r_[np.full(7, 1), 2, rng.integers(3, 5, 292)], 6)      # list 0 and 5 empty, list 2 = the zero row
    prev = rng.standard_normal((6, 16))
    c = R.centroids(x, perm, offsets, prev=prev)
    assert np.array_equal(c[[0, 2, 5]], prev[[0, 2, 5]])
    assert np.allclose(np.linalg.norm(c[[1, 3, 4]], axis=1), 1.0, atol=1e-12)
    raw = R.centroids(x, perm, offsets, normalize=False)
    assert np.array_equal(raw[1], x[:7].astype(np.float64).sum(axis=0)) and not raw[0].any() and not raw[2].any()
    b = R.centroid_bound(x, perm, offsets)
    assert (b[[1, 3, 4]] < 1e-3).all() and (b[[1, 3, 4]] > 0).all() and np.isinf(b[2]).all() and not b[[0, 5]].any()


def test_search_over_every_list_is_the_exact_search_and_ties_go_to_the_lowest_id():
    rng = np.random.default_rng(2)
    x = R.f16(rng.integers(-3, 4, (200, 8)))
    x[50:60] = x[50]                                     # ten equal rows
    q = x[[50, 3]].astype(np.float32)
    offsets, perm = R.lists(rng.integers(0, 5, 200), 5)
    probes = np.tile(np.arange(5), (2, 1))
    val, idx, cands = R.search(q, x[perm], perm, offsets, probes, 12)
    s = R.scores64(q, x)
    for i in range(2):
        o = R.library_order(s[i], np.arange(200))[:12]
        assert np.array_equal(idx[i], o) and np.array_equal(val[i], s[i][o]) and len(cands[i]) == 200
    tied = idx[0][np.isin(idx[0], np.arange(50, 60))]
    assert (np.diff(tied) > 0).all()
    # one probed list, more slots than rows: the tail is (-inf, -1); a running list and idx_base merge in
    v1, i1, _ = R.search(q, x[perm], perm, offsets, probes[:, :1], 100, idx_base=1000)
    n0 = offsets[1] - offsets[0]
    assert (i1[:, n0:] == -1).all() and np.isinf(v1[:, n0:]).all() and (i1[:, :n0] >= 1000).all()
    run = (np.full((2, 3), 1e9), np.array([[7, 5, 6]] * 2), 2)
    v2, i2, _ = R.search(q, x[perm], perm, offsets, probes, 3, run=run)
    assert i2[:, :2].tolist() == [[5, 7], [5, 7]] and (v2[:, :2] == 1e9).all()


def test_kmeans_is_deterministic_and_the_fixture_recalls():
    x, q = R.clustered_fixture(n=1024, clusters=12, nq=8)
    a, b = R.build(x, 8, 4, 0), R.build(x, 8, 4, 0)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    c, rows, ids, offsets = a
    assert np.allclose(np.linalg.norm(c.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(R.assign(rows, c), np.repeat(np.arange(8), np.diff(offsets)))
    exact = np.stack([R.library_order(r, np.arange(1024))[:10] for r in R.scores64(q, R.f16(x))])
    rec = [R.recall_at(R.search(q, rows, ids, offsets, R.probe_sets(q, R.f16(c), p), 10)[1], exact) for p in (1, 2, 4, 8)]
    assert rec == sorted(rec) and rec[-1] == 1.0 and rec[2] >= 0.9


def test_score_bound_counts_the_kernels_roundings():
    assert [R.score_roundings(d) for d in (8, 512, 520, 768, 4096)] == [10, 10, 12, 12, 24]
    assert R.gamma(10) < 6e-7


# ---- IVFCorpus: constructor validation, every refusal of check_search (device-free) ----
def _index(nlist=4, d=16, N=40, **kw):
    parts = dict(centroids=torch.zeros(nlist, d), rows=torch.zeros(N, d, dtype=torch.float16), ids=torch.arange(N),
                 offsets=torch.zeros(nlist + 1, dtype=torch.int64), max_list=N)
    parts.update(kw)
    return IVFCorpus(**parts)


def test_ivf_corpus_holds_its_format():
    ix = _index()
    assert isinstance(ix, CORPUS_KINDS) and len(ix) == 40 and ix.dim == 16 and ix.nlist == 4 and ix.nprobe == 4 and ix.data is ix.rows
    assert ix.centroids16.dtype == torch.float16 and tuple(ix.centroids16.shape) == (4, 16)
    assert ix.nbytes == 4 * 16 * 4 + 4 * 16 * 2 + 40 * 16 * 2 + 40 * 8 + 5 * 8
    view = ix.with_nprobe(2)
    assert view.nprobe == 2 and ix.nprobe == 4 and view.rows is ix.rows and view.centroids is ix.centroids
    assert _index(nlist=64, N=70).nprobe == 32


@pytest.mark.parametrize("kw, text", [
    (dict(centroids=torch.zeros(4, 16, dtype=torch.float16)), "centroids are fp32"),
    (dict(centroids=torch.zeros(4, 12), rows=torch.zeros(40, 12, dtype=torch.float16)), "d % 8 == 0"),
    (dict(centroids=torch.zeros(4, 4104), rows=torch.zeros(40, 4104, dtype=torch.float16)), "d <= 4096"),
    (dict(rows=torch.zeros(40, 16)), "rows are f16"),
    (dict(rows=torch.zeros(40, 24, dtype=torch.float16)), "rows are f16"),
    (dict(ids=torch.arange(39)), "ids must be int64"),
    (dict(ids=torch.arange(40, dtype=torch.int32)), "ids must be int64"),
    (dict(offsets=torch.zeros(4, dtype=torch.int64)), "offsets must be int64"),
    (dict(centroids16=torch.zeros(4, 8, dtype=torch.float16)), "centroids16 must be f16"),
    (dict(max_list=41), "max_list"),
    (dict(nprobe=0), "nprobe"),
    (dict(nprobe=5), "nprobe"),
    (dict(nprobe=2.0), "nprobe"),
])
def test_ivf_corpus_refuses_a_bad_format(kw, text):
    with pytest.raises(ValueError, match=re.escape(text)):
        _index(**kw)


def test_ivf_corpus_refuses_too_many_lists():
    with pytest.raises(ValueError, match="nlist <= 65536"):
        _index(nlist=65537, d=8, N=8)


def test_nprobe_is_capped_at_1024():
    ix = _index(nlist=2048, d=8, N=8)
    assert ix.with_nprobe(1024).nprobe == 1024
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        ix.with_nprobe(1025)


def test_check_search_refusals_are_device_free(monkeypatch):
    from sgpt_amd import runtime

    def no_device(*a, **k):
        raise AssertionError("a refusal reached for the device")
    monkeypatch.setattr(runtime, "get_context", no_device)
    ix = _index()
    q = torch.zeros(2, 16)
    assert ix.check_search(util.cos_sim, 1024) is True
    with pytest.raises(ValueError, match="cos_sim only"):
        util.semantic_search(q, ix, score_function=util.dot_score)
    with pytest.raises(ValueError, match="cos_sim only"):
        util.semantic_search(q, ix, score_function=lambda a, b: a @ b.T)
    with pytest.raises(ValueError, match="top_k <= 1024"):
        util.semantic_search(q, ix, top_k=1025)
    ix.nprobe = 9                                        # (the attribute is the caller's to set: checked again at search time)
    with pytest.raises(ValueError, match="nprobe"):
        util.semantic_search(q, ix)
    ix.nprobe = 0
    with pytest.raises(ValueError, match="nprobe"):
        util.semantic_search(q, ix)


def test_score_topk_refuses_rescore_and_dtype():
    ix = _index()
    for kw in (dict(rescore="fp8", rescore_multiplier=4), dict(rescore="sign", rescore_multiplier=2)):
        with pytest.raises(ValueError, match="BinaryCorpus only"):
            ix.score_topk(None, torch.zeros(1, 16), 1, 0, None, None, **kw)
    with pytest.raises(ValueError, match="dtype must be None"):
        ix.score_topk(None, torch.zeros(1, 16), 1, 0, None, torch.float16, "sign", 4)


# ---- the ABI ----
def test_abi_v26_declares_the_four_entries():
    assert _lib.SGPT_ABI_VERSION >= 26
    header = open(os.path.join(ROOT, "include", "sgpt_hip.h")).read()
    assert int(re.search(r"#define SGPT_ABI_VERSION (\d+)", header).group(1)) == _lib.SGPT_ABI_VERSION
    for name, nargs in (("sgpt_ivf_lists", 7), ("sgpt_ivf_centroids", 13), ("sgpt_gather_rows", 9), ("sgpt_ivf_search", 20)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        proto = re.search(r"sgpt_status " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == nargs
    assert int(re.search(r"#define SGPT_IVF_CHUNK (\d+)", header).group(1)) == _lib.SGPT_IVF_CHUNK == R.CHUNK
    assert "ivf.hip" in __import__("sgpt_amd.build", fromlist=["SOURCES"]).SOURCES
