"""CPU tests of the host side of sgpt_amd/evaluation.py: qrels / result packing, cut validation, output styles, surface."""
import inspect
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_pack_qrels_unknown_documents_count_in_R_and_never_match():
    from sgpt_amd.evaluation import ABSENT, pack_qrels
    pos_of = {"a": 0, "b": 1, "c": 2, "d": 3}
    qrels = {"q1": {"c": 2, "zz": 1, "a": 0, "yy": 3}, "q2": {"b": 1}}
    p = pack_qrels(qrels, ["q1", "q2"], pos_of)
    assert p.off.tolist() == [0, 4, 5] and p.off.dtype == np.int32
    assert p.pos.dtype == np.int64 and p.rel.dtype == np.int32 and p.ideal.dtype == np.int32
    # ascending positions, the two unknown documents last under a position no list holds
    assert p.pos[:4].tolist() == [0, 2, ABSENT, ABSENT] and ABSENT > 2 ** 62
    assert p.rel[:2].tolist() == [0, 2] and sorted(p.rel[2:4].tolist()) == [1, 3]
    assert p.ideal[:4].tolist() == [3, 2, 1, 0]
    assert p.R.tolist() == [3, 1]                      # zz and yy are relevant and absent: they count
    assert p.evaluated.tolist() == [True, True] and p.no_qrels == [] and p.no_relevant == []


def test_pack_qrels_reports_and_excludes_missing_and_R0_queries():
    from sgpt_amd.evaluation import pack_qrels
    pos_of = {"a": 0, "b": 1}
    qrels = {"q1": {"a": 1}, "q3": {"a": 0, "b": -1}, "q4": {}}
    p = pack_qrels(qrels, ["q1", "q2", "q3", "q4"], pos_of)
    assert p.no_qrels == ["q2"] and p.no_relevant == ["q3", "q4"]
    assert p.judged.tolist() == [True, False, True, True]
    assert p.evaluated.tolist() == [True, False, False, False]
    assert p.off.tolist() == [0, 1, 1, 3, 3]
    assert p.R.tolist() == [1, 0, 0, 0]                # grades <= 0 are judged, not relevant
    assert p.rel[1:3].tolist() == [0, -1] and p.ideal[1:3].tolist() == [0, -1]


def test_pack_qrels_binary_grades():
    from sgpt_amd.evaluation import pack_qrels
    p = pack_qrels({"q": {"a": 3, "b": 0, "c": -2, "d": 1}}, ["q"], {"a": 0, "b": 1, "c": 2, "d": 3}, binary=True)
    assert p.rel.tolist() == [1, 0, 0, 1] and p.ideal.tolist() == [1, 1, 0, 0] and p.R.tolist() == [2]


def test_k_values_validation():
    from sgpt_amd.evaluation import MAX_CUTS, check_k_values
    assert check_k_values([1, 3, 5, 10, 100, 1000]) == [1, 3, 5, 10, 100, 1000]
    assert check_k_values(np.array([2, 7])) == [2, 7]
    for bad in ([], [0, 1], [-1], [3, 1], [1, 1], [1.5], [True], list(range(1, MAX_CUTS + 2))):
        with pytest.raises(ValueError):
            check_k_values(bad)


def test_pack_results_orders_by_score_then_position_and_pads():
    from sgpt_amd.evaluation import pack_results
    pos_of = {"a": 0, "b": 1, "c": 2, "d": 3, "q2": 4}
    results = {"q1": {"d": 0.5, "b": 0.9, "a": 0.5, "c": 0.7},         # a and d tie: the lower position first
               "q2": {"q2": 1.0, "a": 0.25},                             # the query's own id is dropped
               "q3": {}}
    idx, val = pack_results(results, ["q1", "q2", "q3", "q4"], pos_of, 5)
    assert idx.dtype == np.int64 and val.dtype == np.float32 and idx.shape == val.shape == (4, 5)
    assert idx[0].tolist() == [1, 2, 0, 3, -1]
    assert val[0, :4].tolist() == [np.float32(0.9), np.float32(0.7), 0.5, 0.5] and val[0, 4] == -np.inf
    assert idx[1].tolist() == [0, -1, -1, -1, -1] and val[1, 0] == 0.25
    assert (idx[2:] == -1).all() and np.isneginf(val[2:]).all()
    idx2, _ = pack_results(results, ["q2"], pos_of, 2, ignore_identical_ids=False)
    assert idx2[0].tolist() == [4, 0]
    with pytest.raises(ValueError):
        pack_results(results, ["q1"], pos_of, 3)
    # ties are fp32 ties: two float64 scores that round to one fp32 value rank by position
    idx3, _ = pack_results({"q": {"b": 0.1 + 1e-12, "a": 0.1}}, ["q"], pos_of, 2)
    assert idx3[0].tolist() == [0, 1]


def _sums(k_values, hits, first, dcg, idcg, sp, R, packed):
    from sgpt_amd.evaluation import MetricSums
    return MetricSums(k_values, np.array(hits), np.array(first), np.array(dcg, np.float32), np.array(idcg, np.float32),
                      np.array(sp, np.float32), np.array(R), packed)


def test_beir_style_key_names_rounding_and_means_over_evaluated_queries():
    from sgpt_amd.evaluation import pack_qrels
    pos_of = {"a": 0, "b": 1, "c": 2}
    qrels = {"q1": {"a": 1, "b": 1, "c": 1}, "q2": {"a": 2}, "q4": {"a": 0}}
    packed = pack_qrels(qrels, ["q1", "q2", "q3", "q4"], pos_of)          # q3: no qrels; q4: R = 0
    s = _sums([1, 3], hits=[[1, 2], [0, 1], [1, 1], [0, 0]], first=[[1, 1], [0, 3], [1, 1], [0, 0]],
              dcg=[[1.0, 1.5], [0.0, 1.5], [9.0, 9.0], [0.0, 0.0]], idcg=[[1.0, 2.1309297], [3.0, 3.0], [0.0, 0.0], [0.0, 0.0]],
              sp=[[1.0, 5.0 / 3.0], [0.0, 1.0 / 3.0], [7.0, 7.0], [0.0, 0.0]], R=[3, 1, 0, 0], packed=packed)
    assert s.report == {"evaluated": 2, "no_qrels": 1, "no_relevant": 1}
    ndcg, _map, recall, precision = s.beir()
    assert list(ndcg) == ["NDCG@1", "NDCG@3"] and list(_map) == ["MAP@1", "MAP@3"]
    assert list(recall) == ["Recall@1", "Recall@3"] and list(precision) == ["P@1", "P@3"]
    assert ndcg == {"NDCG@1": 0.5, "NDCG@3": round((1.5 / 2.1309297 + 0.5) / 2, 5)}
    assert _map == {"MAP@1": round((1 / 3 + 0) / 2, 5), "MAP@3": round((5 / 9 + 1 / 3) / 2, 5)}
    assert recall == {"Recall@1": 0.16667, "Recall@3": 0.83333}
    assert precision == {"P@1": 0.5, "P@3": 0.5}
    for d in (ndcg, _map, recall, precision):
        assert all(v == round(v, 5) for v in d.values())
    assert s.custom("mrr") == {"MRR@1": 0.5, "MRR@3": 0.66667}
    with pytest.raises(ValueError):
        s.custom("hole")
    st = s.st()
    assert list(st) == ["accuracy@k", "precision@k", "recall@k", "ndcg@k", "mrr@k", "map@k"]
    assert st["accuracy@k"] == {1: 0.5, 3: 1.0}
    assert st["map@k"][1] == pytest.approx((1.0 / 1 + 0.0) / 2) and st["map@k"][3] == pytest.approx((5 / 9 + 1 / 3) / 2)


def test_surface_and_no_cpu_fallback():
    import torch
    from sgpt_amd import evaluation as E
    from sgpt_amd._lib import SgptHipError
    from sgpt_amd.beir import DenseRetrievalExactSearch
    assert callable(DenseRetrievalExactSearch.search_ranked)
    sig = inspect.signature(DenseRetrievalExactSearch.search_ranked)
    assert list(sig.parameters)[:5] == ["self", "corpus", "queries", "top_k", "score_function"]
    assert list(inspect.signature(DenseRetrievalExactSearch.search).parameters)[:6] == [
        "self", "corpus", "queries", "top_k", "score_function", "return_sorted"]
    r = E.EvaluateRetrieval(object(), k_values=[1, 10, 100])
    assert r.top_k == 100 and r.score_function == "cos_sim" and r.k_values == [1, 10, 100]
    assert E.EvaluateRetrieval().k_values == [1, 3, 5, 10, 100, 1000]
    for name in ("evaluate", "evaluate_custom", "evaluate_ranked"):
        assert isinstance(inspect.getattr_static(E.EvaluateRetrieval, name), staticmethod)
    with pytest.raises(ValueError):
        E.EvaluateRetrieval().retrieve({}, {})
    with pytest.raises(ValueError):
        E.EvaluateRetrieval.evaluate({"q": {"a": 1}}, {"q": {"a": 1.0}}, [3, 1])
    if not torch.cuda.is_available():
        with pytest.raises(SgptHipError):
            E.EvaluateRetrieval.evaluate({"q": {"a": 1}}, {"q": {"a": 1.0}}, [1])


def test_reference_fixture_is_data_and_self_consistent():
    fx = json.load(open(os.path.join(GOLDEN, "ir_metrics.json")))
    nq = len(fx["query_ids"])
    assert nq == 200 and len(fx["lists"]) == len(fx["score_num"]) == len(fx["relevant"]) == nq
    assert all(len(r) == 100 and len(set(s)) == 100 and s == sorted(s, reverse=True) for r, s in zip(fx["lists"], fx["score_num"]))
    assert all(1 <= len(rel) <= 20 for rel in fx["relevant"])
    assert sum(1 for r, rel in zip(fx["lists"], fx["relevant"]) if not set(r) & set(rel)) >= 3
    assert set(fx["metrics"]) == {"accuracy@k", "precision@k", "recall@k", "ndcg@k", "mrr@k", "map@k"}
