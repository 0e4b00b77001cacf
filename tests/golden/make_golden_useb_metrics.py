#!/usr/bin/env python3
"""Generate tests/golden/useb_metrics.json by running the reference's USEB evaluator functions on seeded inputs.

Runs only where the reference checkout is present (REF below).  askubuntu.py, twitterpara.py and cqadupstack.py are loaded from
their paths under a stub parent package (the package's own __init__ and scidocs.py need pytrec_eval, which is not installed);
scikit-learn, scipy, tqdm and transformers come from the environment.  Recorded:
  groups       rank_by_score orders on lists with exact score ties, and ap_score / reciprocal_rank of every list;
  pairs        sklearn's average_precision_score and scipy's spearmanr as twitterpara.py:110-117 calls them: continuous scores,
               scores with thousands of ties, rows with the label None;
  cqadupstack  CQADupStackEvaluator.compute_metrics on a score matrix without exact ties.
Scores are stored as integers: score = float32(num) / float32(den), exact in every consumer.

Before anything is written, every recorded value is compared with the float64 restatement the tests use (tests/useb_ref.py):
a mismatch of definitions shows here, on the CPU.  Only data is stored.

    python tests/golden/make_golden_useb_metrics.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
EV = f"{REF}/biencoder/useb/useb/useb/evaluators"
sys.path.insert(0, os.path.dirname(HERE))
import useb_ref as R  # noqa: E402


def load_evaluators():
    pkg = types.ModuleType("ref_useb")
    pkg.__path__ = []
    ev = types.ModuleType("ref_useb.evaluators")
    ev.__path__ = [EV]
    sys.modules.update({"ref_useb": pkg, "ref_useb.evaluators": ev})
    mods = {}
    for name in ("base", "askubuntu", "twitterpara", "cqadupstack"):
        spec = importlib.util.spec_from_file_location(f"ref_useb.evaluators.{name}", f"{EV}/{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def f32(num, den):
    return (np.asarray(num, np.float32) / np.float32(den)).astype(np.float64)


def main():
    mods = load_evaluators()
    au, tw, cq = mods["askubuntu"], mods["twitterpara"], mods["cqadupstack"]
    from scipy.stats import spearmanr
    from sklearn.metrics import average_precision_score
    assert tw.average_precision_score is average_precision_score and tw.spearmanr is spearmanr
    rng = np.random.default_rng(20240913)
    worst = 0.0

    groups = []
    for gi in range(240):
        n = int(rng.integers(5, 31))
        num = rng.integers(-12, 13, size=n)                                   # score = num / 8: few distinct values, many exact ties
        if gi % 7 == 0:
            num[:] = num[0]                                                   # every score equal: the input order survives
        gold = (rng.random(n) < 0.25).astype(int)
        if not gold.any():
            gold[int(rng.integers(0, n))] = 1
        cands = [str(i) for i in range(n)]
        scores = f32(num, 8).tolist()
        order = [int(c) for c in au.rank_by_score(cands, scores)]
        relevant = [c for c, g in zip(cands, gold) if g]
        pred = [str(i) for i in order]
        got = dict(au.ap_score(relevant, pred))
        got.update(au.reciprocal_rank(relevant, pred))
        want = R.group_sums(scores, gold.tolist())
        assert want["order"] == order, (gi, order, want["order"])
        mine = {"map": want["sp"] / want["R"], "p@1": float(want["hits1"]), "p@5": want["hits5"] / 5.0, "mrr": 1.0 / want["first"]}
        worst = max([worst] + [abs(float(got[k]) - mine[k]) for k in mine])
        groups.append({"num": num.tolist(), "gold": gold.tolist(), "order": order,
                       **{k: float(got[k]) for k in ("map", "p@1", "p@5", "mrr")}})

    pairs = []
    for name, n, den, with_none in (("continuous", 1500, 1000000, False), ("two_decimals", 3000, 100, False),
                                    ("two_decimals_with_none", 3000, 100, True), ("all_equal", 64, 100, True)):
        label5 = rng.integers(0, 6, size=n)                                   # the 0 .. 5 annotator counts of the two corpora
        num = np.clip(rng.normal(label5 / 5.0, 0.35) * den, -den, den).astype(np.int64)
        if name == "continuous":
            num = rng.permutation(2 * den)[:n] - den                          # distinct
        if name == "all_equal":
            num[:] = 37
        is_para = [None if (with_none and v == 3) else int(v > 3 if with_none else v >= 3) for v in label5]
        gold = (label5 * 20).tolist()
        pred = f32(num, den)
        keep = [i for i, v in enumerate(is_para) if v is not None]
        ap = float(average_precision_score(list(np.array(is_para)[keep]), list(pred[keep])))
        rho = float(spearmanr(gold, pred).correlation)
        my_ap, my_rho = R.twitterpara_metrics(pred, is_para, gold)
        worst = max(worst, abs(ap - my_ap), 0.0 if np.isnan(rho) and np.isnan(my_rho) else abs(rho - my_rho))
        pairs.append({"name": name, "num": num.tolist(), "den": den, "label": [-1 if v is None else v for v in is_para], "gold": gold,
                      "ap": ap, "spearman": None if np.isnan(rho) else rho})

    nq, nd, den = 40, 300, 100000
    num = np.stack([rng.permutation(den)[:nd] for _ in range(nq)])            # distinct within a row
    mtrx = f32(num, den)
    qids = [f"q{i}" for i in range(nq)]
    dids = [f"d{i}" for i in range(nd)]
    rel_docs = {}
    for qi, q in enumerate(qids):
        if qi % 13 == 5:
            rel_docs[q] = []                                                  # no duplicates: ndcg leaves the query out, map counts 0
            continue
        top = np.argsort(-mtrx[qi])
        inside = rng.choice(top[:60], size=int(rng.integers(0, 5)), replace=False) if qi % 13 != 7 else top[200:203]
        rel_docs[q] = [dids[int(c)] for c in inside] + [f"query-{qi}-{j}" for j in range(int(rng.integers(0, 3)))]   # some outside the pool
        if not rel_docs[q]:
            rel_docs[q] = [dids[int(top[3])]]
    rel_set = {q: set(v) for q, v in rel_docs.items()}
    m_ap, m_ndcg = cq.CQADupStackEvaluator.compute_metrics(None, mtrx, qids, dids, rel_docs, rel_set)
    col = {d: i for i, d in enumerate(dids)}
    rel_cols = [sorted(col[d] for d in rel_docs[q] if d in col) for q in qids]
    n_rel = [len(rel_docs[q]) for q in qids]
    my_ap, my_ndcg = R.cqadupstack_metrics(mtrx, [set(c) for c in rel_cols], n_rel)
    worst = max(worst, abs(float(m_ap) - my_ap), abs(float(m_ndcg) - my_ndcg))

    print(f"reference vs float64 restatement: max |diff| = {worst:.3e}")
    assert worst < 1e-12, "the definitions of tests/useb_ref.py differ from the reference's"

    out = {
        "source": "askubuntu.rank_by_score / ap_score / reciprocal_rank, twitterpara's average_precision_score + spearmanr calls, "
                  "CQADupStackEvaluator.compute_metrics of the reference (biencoder/useb/useb/useb/evaluators)",
        "groups_den": 8, "groups": groups, "pairs": pairs,
        "cqadupstack": {"num": num.tolist(), "den": den, "rel_cols": rel_cols, "n_rel": n_rel, "map@100": float(m_ap), "ndcg@10": float(m_ndcg)},
    }
    path = os.path.join(HERE, "useb_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
