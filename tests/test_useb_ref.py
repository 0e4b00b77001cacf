"""CPU: the float64 restatement of the USEB definitions (tests/useb_ref.py) against the recorded outputs of the reference's
evaluators (tests/golden/useb_metrics.json) and directly against scikit-learn / scipy; the task-file loaders of
sgpt_amd/useb_eval.py on tiny files; the CSR construction (sentence de-duplication, skipped queries, R_extra)."""
import json
import os

import numpy as np
import pytest

import useb_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def f32(num, den):
    return (np.asarray(num, np.float32) / np.float32(den)).astype(np.float64)


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(GOLDEN, "useb_metrics.json")))


def test_group_ranking_and_metrics_match_the_reference(fx):
    assert len(fx["groups"]) >= 200
    ties = 0
    for g in fx["groups"]:
        scores = f32(g["num"], fx["groups_den"])
        ties += len(scores) - len(set(scores.tolist()))
        s = R.group_sums(scores, g["gold"])
        assert s["order"] == g["order"]
        assert abs(s["sp"] / s["R"] - g["map"]) < 1e-12 and float(s["hits1"]) == g["p@1"] and abs(s["hits5"] / 5.0 - g["p@5"]) < 1e-12
        assert abs(1.0 / s["first"] - g["mrr"]) < 1e-12
    assert ties > 1000                                                  # the fixture is about exact ties
    want = {k: float(np.mean([g[k] for g in fx["groups"]])) for k in ("map", "p@1", "p@5", "mrr")}
    got = R.askubuntu_metrics([(f32(g["num"], fx["groups_den"]), g["gold"]) for g in fx["groups"]])
    assert all(abs(got[k] - want[k]) < 1e-12 for k in want)


def test_pairs_match_the_reference_and_scipy_sklearn(fx):
    from scipy.stats import rankdata, spearmanr
    from sklearn.metrics import average_precision_score
    assert {p["name"] for p in fx["pairs"]} >= {"continuous", "two_decimals", "two_decimals_with_none", "all_equal"}
    for p in fx["pairs"]:
        pred = f32(p["num"], p["den"])
        is_para = [None if v < 0 else v for v in p["label"]]
        ap, rho = R.twitterpara_metrics(pred, is_para, p["gold"])
        assert abs(ap - p["ap"]) < 1e-12, p["name"]
        assert (p["spearman"] is None and np.isnan(rho)) or abs(rho - p["spearman"]) < 1e-12, p["name"]
        assert np.array_equal(R.rank2(pred), np.rint(2 * rankdata(pred)).astype(np.int64))
    rng = np.random.default_rng(3)
    for n, decimals in ((1, 3), (2, 0), (65, 1), (5000, 1), (5000, 6)):
        s = np.round(rng.standard_normal(n), decimals).astype(np.float32)
        lab = rng.integers(-1, 2, size=n)
        lab[0] = 1
        assert np.array_equal(R.rank2(s), np.rint(2 * rankdata(s.astype(np.float64))).astype(np.int64))
        used = lab >= 0
        assert abs(R.average_precision(s, lab) - average_precision_score(lab[used], s[used].astype(np.float64))) < 1e-12
        if n > 2:
            gold = rng.integers(0, 6, size=n) * 20
            assert abs(R.spearman(R.rank2(s), gold) - spearmanr(gold, s).correlation) < 1e-12
    assert R.average_precision([0.5, 0.25], [0, 0]) == 0.0                # no positive: undefined, reported as 0
    num, n_pos, n_used = R.ap_parts([3.0, 1.0, 2.0, 1.0], [1, 0, -1, 1])
    assert (n_pos, n_used) == (2, 3) and abs(num - (1.0 + 2.0 / 3.0)) < 1e-15


def test_cqadupstack_matches_the_reference(fx):
    c = fx["cqadupstack"]
    m, nd = R.cqadupstack_metrics(f32(c["num"], c["den"]), [set(r) for r in c["rel_cols"]], c["n_rel"])
    assert abs(m - c["map@100"]) < 1e-12 and abs(nd - c["ndcg@10"]) < 1e-12
    assert any(n == 0 for n in c["n_rel"]) and any(n > len(r) for n, r in zip(c["n_rel"], c["rel_cols"]))


def test_group_sums_definitions_on_a_worked_case():
    s = R.group_sums([0.5, float("nan"), 0.5, 2.0, -0.0, 0.0], [2, 3, 0, -1, 1, 0], R_extra=2, ideal=[3, 2, 1, 1, 0, -1])
    assert s["order"] == [3, 0, 2, 4, 5, 1]                             # ties keep the input order, -0 == +0, NaN last
    assert (s["hits1"], s["hits5"], s["first"], s["R"]) == (0, 2, 2, 5)
    assert abs(s["sp"] - (1 / 2 + 2 / 4 + 3 / 6)) < 1e-15
    assert abs(s["dcg"] - (2 / np.log2(3) + 1 / np.log2(5) + 3 / np.log2(7))) < 1e-15
    assert abs(s["idcg"] - (3 / np.log2(2) + 2 / np.log2(3) + 1 / np.log2(4) + 1 / np.log2(5))) < 1e-15
    empty = R.group_sums([], [], R_extra=1)
    assert empty["order"] == [] and empty["R"] == 1 and empty["sp"] == 0.0 and empty["first"] == 0
    x = np.array([3.0, 4.0])
    assert np.allclose(R.pair_scores(x, [[3.0, 4.0], [0.0, 0.0], [4.0, -3.0]], "cos"), [1.0, 0.0, 0.0])
    assert np.allclose(R.pair_scores(x, [[0.0, 0.0]], "neg_l2"), [-5.0]) and np.allclose(R.pair_scores(x, [[1.0, 1.0]], "dot"), [7.0])


# ---- loaders and CSR construction of sgpt_amd/useb_eval.py (host code: no GPU) -----------------------------------------------
def test_askubuntu_loader_and_csr(tmp_path):
    from sgpt_amd.useb_eval import AskUbuntuEvaluator, load_askubuntu
    (tmp_path / "text_tokenized.txt").write_text(
        "1\thow to boot \tbody one\n2\tgrub error\tbody two\n3\tgrub error\tbody three\n4\tusb stick\tbody four\n5\tno sound\tbody five\n")
    row = "1\t2 4\t2 3 4 5\t1.0 2.5 2.5 0.5\n"
    (tmp_path / "dev.txt").write_text(row)
    (tmp_path / "test.txt").write_text(row + "2\t\t1 3\t1.0 2.0\n" + "5\t1\t2 3\t1.0 2.0\n")
    pool, splits = load_askubuntu(str(tmp_path))
    assert pool["1"] == ("how to boot", "body one") and len(splits["valid"]) == 1
    assert splits["test"][0] == ("1", ["2", "4"], ["3", "4", "2", "5"])          # BM25 order, the tie keeps the file's order
    ev = AskUbuntuEvaluator(None, pool, {"test": splits["test"][:2]})
    t = ev.task("test")                                                          # the query without gold ids is skipped
    assert t.group_ids == ["1"] and t.grp_off.tolist() == [0, 4]
    assert t.sentences == ["how to boot", "grub error", "usb stick", "no sound"]  # "grub error" (ids 2 and 3) is one row
    assert t.q_row.tolist() == [0] and t.cand_row.tolist() == [1, 2, 1, 3] and t.cand_rel.tolist() == [0, 1, 1, 0]
    assert t.R_extra.tolist() == [0] and t.ideal_rel.tolist() == [1, 1, 0, 0] and t.ideal_off.tolist() == [0, 4]
    assert AskUbuntuEvaluator(None, pool, splits, "title_and_body")._sent("4") == "usb stick body four"
    with pytest.raises(ValueError, match="'5'"):
        AskUbuntuEvaluator(None, pool, splits).task("test")                      # gold id 1 is not in the list of query 5


def test_scidocs_loader_and_csr(tmp_path):
    from sgpt_amd.useb_eval import SciDocsEvaluator, load_scidocs
    data = {"corpus": {"q1": {"title": "graph kernels"}, "a": {"title": "deep nets"}, "b": {"title": None}, "c": {"title": "graph kernels"},
                       "q2": {"title": ""}, "e": {"title": "trees"}},
            "test": {"cite": {"q1": {"a": 1, "b": 1, "c": 0, "gone": 1, "e": 0}, "q2": {"a": 1}, "q3": {"a": 1}}}}
    (tmp_path / "data.json").write_text(json.dumps(data))
    ev = SciDocsEvaluator(None, load_scidocs(str(tmp_path)))
    t = ev.task(ev.data["test"]["cite"])
    assert t.group_ids == ["q1"]                                                 # q2 has an empty title, q3 is not in the corpus
    assert t.sentences == ["graph kernels", "trees", "deep nets"]                # candidates by descending id: e, c, a; c shares the query's row
    assert t.cand_row.tolist() == [1, 0, 2] and t.cand_rel.tolist() == [0, 0, 1]
    assert t.R_extra.tolist() == [2] and t.ideal_rel.tolist() == [1, 1, 1, 0, 0]  # b (no title) and gone (not in the corpus) count in R


def test_cqadupstack_and_twitterpara_loaders(tmp_path):
    from sgpt_amd.useb_eval import doubled_ranks, load_cqadupstack, load_pit, load_twitterurl, pearson
    (tmp_path / "corpus.json").write_text(json.dumps({"android": {"1": "a", "2": "b"}}))
    (tmp_path / "retrieval_split.json").write_text(json.dumps({"test": {"android": {"1": ["2"]}}, "valid": {"android": {}}}))
    corpus, split = load_cqadupstack(str(tmp_path))
    assert corpus["android"]["2"] == "b" and split["test"]["android"] == {"1": ["2"]}
    (tmp_path / "Twitter_URL_Corpus_test.txt").write_text("s one\ts two\t(5, 6)\turl\ns three\ts four\t(3, 6)\turl\ns five\ts six\t(0, 6)\turl\n")
    assert load_twitterurl(str(tmp_path)) == [("s one", "s two", 1, 100), ("s three", "s four", None, 60), ("s five", "s six", 0, 0)]
    (tmp_path / "test.data").write_text("7\ttopic\tsent a\tsent b\t4\tx\n8\ttopic\tsent c\tsent d\t2\tx\n")
    assert load_pit(str(tmp_path)) == [("sent a", "sent b", 1, 80), ("sent c", "sent d", 0, 40)]
    rng = np.random.default_rng(0)
    v = rng.integers(0, 6, size=500) * 20
    assert np.array_equal(doubled_ranks(v), R.rank2(v))
    a, b = rng.standard_normal(50), rng.standard_normal(50)
    assert abs(pearson(a, b) - np.corrcoef(a, b)[0, 1]) < 1e-12
