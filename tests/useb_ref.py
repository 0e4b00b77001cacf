"""Test infrastructure: float64 restatement of the USEB evaluation definitions that csrc/useb_eval.hip and sgpt_amd/useb_eval.py
implement -- the reference of tests/test_gpu_useb_eval.py, pinned in tests/test_useb_ref.py against the recorded outputs of the
reference's evaluators (tests/golden/useb_metrics.json) and directly against scikit-learn and scipy.

Ranking of a group: descending score, equal scores to the lower position (Python's stable sorted(..., reverse=True)), NaN last.
Per group, with the ranked grades g_1 .. g_n (relevant: g > 0), hits@i = relevant among ranks 1 .. i:
  hits1, hits5 = hits@min(1, n), hits@min(5, n);  first = rank of the first relevant candidate (0: none)
  R = relevant candidates + R_extra;  sp = sum over relevant ranks i of hits@i / i
  dcg = sum_i max(g_i, 0) / log2(i + 1);  idcg = the same over the judged grades sorted descending
Pairs: rank2 = twice the tie-averaged ascending rank; AP = scikit-learn's average_precision_score (equal scores: one threshold)."""
import math

import numpy as np


def rank_order(scores):
    """-> group-local indices in rank order."""
    s = [float(v) for v in scores]
    return sorted(range(len(s)), key=lambda i: (math.isnan(s[i]), -s[i] if not math.isnan(s[i]) else 0.0))


def pair_scores(x, Y, mode):
    """float64 scores of row x against the rows of Y; mode "cos" | "dot" | "neg_l2"."""
    x, Y = np.asarray(x, np.float64), np.asarray(Y, np.float64).reshape(-1, len(x))
    if mode == "dot":
        return Y @ x
    if mode == "neg_l2":
        return -np.sqrt(((Y - x[None, :]) ** 2).sum(axis=1))
    if mode == "cos":
        return (Y @ x) / (np.maximum(np.linalg.norm(x), 1e-8) * np.maximum(np.linalg.norm(Y, axis=1), 1e-8))
    raise ValueError(mode)


def group_sums(scores, grades, R_extra=0, ideal=None):
    order = rank_order(scores)
    g = np.asarray([grades[i] for i in order], np.float64)
    n = len(g)
    rel = g > 0
    ranks = np.arange(1, n + 1, dtype=np.float64)
    cum = np.cumsum(rel)
    out = {"order": order, "hits1": int(rel[:1].sum()), "hits5": int(rel[:5].sum()),
           "first": int(np.argmax(rel)) + 1 if rel.any() else 0, "R": int(rel.sum()) + int(R_extra),
           "sp": float((rel * cum / ranks).sum()) if n else 0.0,
           "dcg": float((np.maximum(g, 0) / np.log2(ranks + 1)).sum()) if n else 0.0, "idcg": 0.0}
    if ideal is not None and len(ideal):
        ide = np.maximum(np.asarray(ideal, np.float64), 0)
        assert (np.diff(ide) <= 0).all(), "ideal grades must be sorted descending"
        out["idcg"] = float((ide / np.log2(np.arange(1, len(ide) + 1) + 1.0)).sum())
    return out


def rank2(scores):
    """Twice scipy.stats.rankdata(scores) (method 'average'), as exact integers."""
    s = np.asarray(scores, np.float64) + 0.0
    order = np.argsort(s, kind="stable")
    ss = s[order]
    n = len(s)
    start = np.r_[0, np.flatnonzero(ss[1:] != ss[:-1]) + 1] if n else np.zeros(0, np.int64)
    end = np.r_[start[1:], n] if n else np.zeros(0, np.int64)
    out = np.zeros(n, np.int64)
    for a, b in zip(start, end):
        out[order[a:b]] = a + b + 1                      # (a + 1) + b: first + last 1-based rank of the tie group
    return out


def ap_parts(scores, labels):
    """-> (numerator, n_pos, n_used) of the average precision over the rows with label >= 0."""
    s = np.asarray(scores, np.float64) + 0.0
    lab = np.asarray(labels, np.int64)
    used = lab >= 0
    s, pos = s[used], lab[used] > 0
    n_pos, n_used = int(pos.sum()), int(used.sum())
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], pos[order]
    num, tp_prev = 0.0, 0
    ends = np.r_[np.flatnonzero(s[1:] != s[:-1]) + 1, len(s)] if len(s) else []
    cum = np.cumsum(pos)
    for e in ends:
        tp = int(cum[e - 1])
        if tp > tp_prev:
            num += (tp - tp_prev) * tp / float(e)
        tp_prev = tp
    return num, n_pos, n_used


def average_precision(scores, labels):
    num, n_pos, _ = ap_parts(scores, labels)
    return num / n_pos if n_pos else 0.0


def pearson(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    den = math.sqrt(float((a * a).sum()) * float((b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


def spearman(pred_rank2, gold):
    """Spearman correlation from the doubled ranks of the predictions and the raw gold scores."""
    return pearson(pred_rank2, rank2(gold))


# ---- the four tasks, from per-group / per-pair scores ----------------------------------------------------------------------
def askubuntu_metrics(groups):
    """groups: [(scores, grades)] of the queries that have gold ids.  -> map, p@1, p@5, mrr (means over the groups)."""
    acc = {"map": [], "p@1": [], "p@5": [], "mrr": []}
    for scores, grades in groups:
        s = group_sums(scores, grades)
        if s["R"] == 0:
            raise ValueError("no gold id among the candidates")
        acc["map"].append(s["sp"] / s["R"])
        acc["p@1"].append(float(s["hits1"]))
        acc["p@5"].append(s["hits5"] / 5.0)
        acc["mrr"].append(1.0 / s["first"])
    return {k: float(np.mean(v)) for k, v in acc.items()}


def scidocs_metrics(groups):
    """groups: [(scores, grades, R_extra, ideal)].  trec_eval's map (sp / R, R over all judged relevant documents) and ndcg
    (dcg / idcg, full list); queries with R == 0 are left out of the means."""
    m, nd = [], []
    for scores, grades, R_extra, ideal in groups:
        s = group_sums(scores, grades, R_extra, ideal)
        if s["R"] == 0:
            continue
        m.append(s["sp"] / s["R"])
        nd.append(s["dcg"] / s["idcg"])
    return {"map": float(np.mean(m)) if m else 0.0, "ndcg": float(np.mean(nd)) if nd else 0.0}


def cqadupstack_metrics(score_mtrx, rel_cols, n_rel, map_k=100, ndcg_k=10):
    """score_mtrx [nq, nd]; rel_cols[q]: set of relevant columns; n_rel[q] = len(rel_docs) (may count documents outside the
    pool).  map@100: sp@100 / hits@100 over the retrieved list (0 without a hit), mean over all queries; ndcg@10 with an
    all-ones ideal of length n_rel, mean over the queries with n_rel > 0.  Lists without exactly tied scores."""
    aps, nds = [], []
    for q, row in enumerate(np.asarray(score_mtrx, np.float64)):
        order = rank_order(row)[:max(map_k, ndcg_k)]
        rel = np.array([c in rel_cols[q] for c in order], np.float64)
        r100 = rel[:map_k]
        hits = r100.sum()
        aps.append(float((r100 * np.cumsum(r100) / np.arange(1, len(r100) + 1)).sum() / hits) if hits else 0.0)
        if n_rel[q] > 0:
            r10 = rel[:ndcg_k]
            dcg = (r10 / np.log2(np.arange(1, len(r10) + 1) + 1.0)).sum()
            idcg = (1.0 / np.log2(np.arange(1, min(n_rel[q], ndcg_k) + 1) + 1.0)).sum()
            nds.append(float(dcg / idcg))
    return float(np.mean(aps)), float(np.mean(nds)) if nds else 0.0


def twitterpara_metrics(pred, is_para, gold):
    """pred scores, is_para in {1, 0, None}, gold scores -> (ap over the rows with a label, spearman over all rows)."""
    labels = [-1 if p is None else int(p) for p in is_para]
    return average_precision(pred, labels), spearman(rank2(pred), gold)
