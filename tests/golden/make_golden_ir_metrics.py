#!/usr/bin/env python3
"""Generate tests/golden/ir_metrics.json by running the reference's InformationRetrievalEvaluator.compute_metrics.

Runs only where the reference checkout is present (REF below).  The evaluator file is loaded directly from its path with
stub parent packages (its relative imports -- SentenceEvaluator, util.cos_sim / dot_score -- and tqdm are not needed by the two
functions that are called: compute_metrics and compute_dcg_at_k).  Inputs are seeded: 200 queries, ranked lists of 100
documents with distinct scores (the reference breaks ties by input order, this project by position), 1..20 relevant
documents per query (none with R = 0: the reference divides by it), a few queries whose relevant documents are never retrieved.

Before anything is written, the reference's output is compared with a float64 restatement of the definitions in
sgpt_amd/evaluation.py (binary grades): a mismatch of definitions shows here, on the CPU.  Only data is stored.

    python tests/golden/make_golden_ir_metrics.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ST = f"{REF}/biencoder/nli_msmarco/sentence-transformers/sentence_transformers"
K_VALUES = [1, 3, 5, 10, 100]


def load_evaluator():
    pkg = types.ModuleType("ref_st")
    pkg.__path__ = []
    ev = types.ModuleType("ref_st.evaluation")
    ev.__path__ = []
    ev.SentenceEvaluator = type("SentenceEvaluator", (), {})
    util = types.ModuleType("ref_st.util")
    util.cos_sim = util.dot_score = None
    tq = types.ModuleType("tqdm")
    tq.tqdm = tq.trange = None
    sys.modules.update({"ref_st": pkg, "ref_st.evaluation": ev, "ref_st.util": util})
    sys.modules.setdefault("tqdm", tq)
    spec = importlib.util.spec_from_file_location("ref_st.evaluation.InformationRetrievalEvaluator",
                                                  f"{ST}/evaluation/InformationRetrievalEvaluator.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.InformationRetrievalEvaluator


def restate(lists, relevant, k_values):
    """float64 restatement of sgpt_amd/evaluation.py's definitions, binary grades, "st" normalisation."""
    out = {n: {k: [] for k in k_values} for n in ("accuracy@k", "precision@k", "recall@k", "ndcg@k", "mrr@k", "map@k")}
    for docs, rel in zip(lists, relevant):
        R = len(rel)
        flags = np.array([d in rel for d in docs], dtype=np.float64)
        ranks = np.arange(1, len(docs) + 1, dtype=np.float64)
        first = int(np.argmax(flags)) + 1 if flags.any() else 0
        for k in k_values:
            f = flags[:k]
            hits = f.sum()
            out["accuracy@k"][k].append(float(hits > 0))
            out["precision@k"][k].append(hits / k)
            out["recall@k"][k].append(hits / R)
            out["mrr@k"][k].append(1.0 / first if 0 < first <= k else 0.0)
            dcg = (f / np.log2(ranks[:k] + 1)).sum()
            idcg = (1.0 / np.log2(np.arange(1, min(k, R) + 1) + 1.0)).sum()
            out["ndcg@k"][k].append(dcg / idcg)
            out["map@k"][k].append((f * np.cumsum(f) / ranks[:k]).sum() / min(k, R))
    return {n: {k: float(np.mean(v)) for k, v in d.items()} for n, d in out.items()}


def main():
    IRE = load_evaluator()
    rng = np.random.default_rng(20240607)
    nq, n_docs, depth = 200, 5000, 100
    qids = [f"q{i}" for i in range(nq)]
    lists, scores, relevant, score_num = [], [], [], []
    for qi in range(nq):
        docs = rng.choice(n_docs, size=depth, replace=False)
        num = np.sort(rng.permutation(100000)[:depth])[::-1]
        s = num.astype(np.float32) / np.float32(100000.0)                            # distinct fp32 scores, descending
        assert len(np.unique(s)) == depth
        score_num.append(num.tolist())
        R = int(rng.integers(1, 21))
        if qi % 40 == 7:                                   # relevant documents that are never retrieved
            pool = np.setdiff1d(np.arange(n_docs), docs)
            rel = rng.choice(pool, size=R, replace=False)
        else:                                              # some retrieved (biased to the head of the list), some not
            n_in = int(rng.integers(0, R + 1))
            w = 1.0 / np.arange(1, depth + 1)
            inside = rng.choice(docs, size=n_in, replace=False, p=w / w.sum())
            pool = np.setdiff1d(np.arange(n_docs), docs)
            rel = np.concatenate([inside, rng.choice(pool, size=R - n_in, replace=False)])
        lists.append([f"d{d}" for d in docs])
        scores.append(s)
        relevant.append({f"d{d}" for d in rel})

    ev = IRE.__new__(IRE)                                  # compute_metrics reads only these attributes
    ev.queries_ids = qids
    ev.queries = qids
    ev.relevant_docs = dict(zip(qids, relevant))
    ev.accuracy_at_k = ev.precision_recall_at_k = ev.mrr_at_k = ev.ndcg_at_k = ev.map_at_k = K_VALUES
    shuffled = []
    for docs, s in zip(lists, scores):                     # the reference sorts by score itself: hand the hits over shuffled
        perm = rng.permutation(depth)
        shuffled.append([{"corpus_id": docs[j], "score": float(s[j])} for j in perm])
    got = ev.compute_metrics(shuffled)
    got = {n: {int(k): float(v) for k, v in d.items()} for n, d in got.items()}
    assert abs(IRE.compute_dcg_at_k([1, 0, 1], 2) - 1.0) < 1e-12

    want = restate(lists, relevant, K_VALUES)
    worst = max(abs(got[n][k] - want[n][k]) for n in want for k in K_VALUES)
    print(f"reference vs float64 restatement: max |diff| = {worst:.3e}")
    assert worst < 1e-12, "the definitions of sgpt_amd/evaluation.py differ from the reference's"

    out = {
        "source": "InformationRetrievalEvaluator.compute_metrics of the reference (sentence_transformers/evaluation)",
        "k_values": K_VALUES,
        "n_docs": n_docs,
        "query_ids": qids,
        "lists": [[int(d[1:]) for d in docs] for docs in lists],                 # document numbers (id = "d<number>"), rank order
        "score_num": score_num,                                                  # score = float32(num) / float32(100000)
        "relevant": [sorted(int(d[1:]) for d in rel) for rel in relevant],
        "metrics": {n: {str(k): v for k, v in d.items()} for n, d in got.items()},
    }
    path = os.path.join(HERE, "ir_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
