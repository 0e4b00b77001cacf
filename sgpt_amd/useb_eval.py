"""The four USEB evaluators on the device (biencoder/useb/useb/useb/evaluators/{askubuntu,scidocs,cqadupstack,twitterpara}.py).

The reference drives every task through `semb_fn`: AskUbuntu and SciDocs call it once per query with 21 / ~31 sentences, copy
the embeddings to the host, score there and sort in Python.  Here a task is described before the first forward: the unique
sentences are encoded ONCE through `CustomEmbedder.encode_device` (token-budgeted bulk calls, embeddings stay on the device,
L2-normalised as base.py:34-35 does), the candidate groups become a CSR on the host, one call scores, ranks and reduces them
(include/sgpt_hip.h::sgpt_eval_groups / sgpt_eval_pairs / sgpt_eval_ranked), and what is left for the host is the
normalisation of per-group sums.  The encoder gives every sentence the same bits whatever batch it travels in (low-latency mode
off), so the embeddings are the ones `semb_fn` would have produced.  Results carry the reference's metric names.  No fallback:
without a GPU the calls raise SgptHipError.

  AskUbuntu    groups = query + its BM25 list (BM25-score order, stable); dot product of the embeddings; `map` averages the
               precisions over the relevant candidates FOUND IN THE LIST (the reference's ap_score), p@1, p@5 = hits5 / 5, mrr.
               The candidate ids of a list are taken to be distinct.  A query whose gold ids all miss the list: ValueError.
  SciDocs      per sub-task, groups = query + its judged documents that have a title, listed by descending document id (so
               equal scores break as trec_eval breaks them), scored twice (cosine, -L2).  map = sp / R with R over ALL judged
               relevant documents (R_extra: the ones without a title), ndcg = dcg / idcg over the full list.  The reference takes
               both from pytrec_eval, which is not a dependency here: they follow trec_eval's published definitions and are
               tested against a float64 restatement, not against a run of the reference.  Queries with R = 0 are left out of the
               means and counted in `report`, as sgpt_amd/evaluation.py does.
  CQADupStack  per forum: top-100 of the pool without the query ids (sgpt_score_topk), then sgpt_eval_ranked at cuts (10, 100):
               ndcg@10 = dcg@10 / idcg@10 with an all-ones ideal of length len(rel_docs); map@100 = sp@100 / hits@100, 0 without
               a hit (scikit-learn's AP over the retrieved list divides by the positives IN the list).  Exactly tied scores
               inside a top-100 list are one threshold for scikit-learn and separate ranks (lower pool position first) here.
  TwitterPara  cosine of the two embedding sets (sgpt_pairwise_scores), sgpt_eval_pairs for the doubled ranks and the AP
               numerator, Spearman as float64 Pearson of the doubled ranks on the host.

A re-ranker that scores elsewhere uses the same ranking and sums through `scores_in`:
    scores = torch.tensor(GPTRanker(model, tok).predict(pairs), device="cuda")      # pairs in the CSR's candidate order
    sums = get_context().eval_groups(task.grp_off, task.cand_rel, scores_in=scores)"""
import ast
import json
import logging
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)


# ---- task description: unique sentences + CSR of groups (host) -------------------------------------------------------------
@dataclass
class GroupTask:
    sentences: List[str]               # unique, stripped
    grp_off: np.ndarray                # int32 [G + 1]
    q_row: np.ndarray                  # int32 [G]: row of the group's query in `sentences`
    cand_row: np.ndarray               # int32: row of each candidate
    cand_rel: np.ndarray               # int32: grade of each candidate
    R_extra: np.ndarray                # int32 [G]: relevant judged documents that are not candidates
    ideal_off: np.ndarray              # int32 [G + 1]
    ideal_rel: np.ndarray              # int32: each group's judged grades, descending
    group_ids: List[str] = field(default_factory=list)


class SentencePool:
    """text -> row of the unique, stripped sentence (base.py:30 strips before the embedder sees a text)."""

    def __init__(self):
        self.row_of: Dict[str, int] = {}
        self.sentences: List[str] = []

    def row(self, text: str) -> int:
        t = text.strip()
        r = self.row_of.get(t)
        if r is None:
            r = self.row_of[t] = len(self.sentences)
            self.sentences.append(t)
        return r


def build_groups(groups: Sequence[Tuple[str, str, Sequence[str], Sequence[int], int, Sequence[int]]],
                 pool: Optional[SentencePool] = None) -> GroupTask:
    """groups: (group id, query text, candidate texts, candidate grades, R_extra, all judged grades).  Sentences are
    de-duplicated across the whole task; the judged grades are sorted descending for IDCG."""
    pool = pool or SentencePool()
    off, io = [0], [0]
    q_row, cand_row, cand_rel, R_extra, ideal, ids = [], [], [], [], [], []
    for gid, query, cands, grades, rx, judged in groups:
        if len(cands) != len(grades):
            raise ValueError(f"group {gid!r}: {len(cands)} candidates, {len(grades)} grades")
        ids.append(gid)
        q_row.append(pool.row(query))
        cand_row.extend(pool.row(c) for c in cands)
        cand_rel.extend(int(g) for g in grades)
        R_extra.append(int(rx))
        ideal.extend(sorted((int(g) for g in judged), reverse=True))
        off.append(len(cand_row))
        io.append(len(ideal))
    i32 = lambda a: np.asarray(a, dtype=np.int32)   # noqa: E731
    return GroupTask(pool.sentences, i32(off), i32(q_row), i32(cand_row), i32(cand_rel), i32(R_extra), i32(io), i32(ideal), ids)


def encode_unique(embedder, sentences: Sequence[str], normalize: bool = True):
    """Every sentence once, on the bulk path; fp32 [n, d] on the device (base.py:33-35: semb_fn, then F.normalize).  The token
    budget is the model's: SGPTModel.encode_ids cuts the list into length-sorted calls of at most max_tokens_per_call token rows,
    so the activation workspace stays bounded however many sentences a task has; only the [n, d] result grows with n."""
    from .runtime import get_context
    emb = embedder.encode_device(list(sentences))
    return get_context(emb.device).l2_normalize(emb) if normalize else emb


def group_sums(embedder, task: GroupTask, mode: str, normalize: bool = True, emb=None) -> Dict[str, np.ndarray]:
    """Encode (unless `emb` is given), one kernel call, the per-group sums as host arrays."""
    from .runtime import get_context
    if emb is None:
        emb = encode_unique(embedder, task.sentences, normalize)
    out = get_context(emb.device).eval_groups(task.grp_off, task.cand_rel, emb=emb, q_row=task.q_row, cand_row=task.cand_row, mode=mode,
                                              R_extra=task.R_extra, ideal_off=task.ideal_off, ideal_rel=task.ideal_rel)
    return {k: v.cpu().numpy() for k, v in out.items() if k not in ("scores", "order")}


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, dtype=np.float64), where=den > 0)


# ---- AskUbuntu ---------------------------------------------------------------------------------------------------------------
def load_askubuntu(datasets_dir: str):
    """text_tokenized.txt (qid \\t title \\t body) and dev.txt / test.txt (qid \\t gold ids \\t BM25 ids \\t BM25 scores).
    -> (pool {qid: (title, body)}, {"valid": [...], "test": [...]}) with entries (qid, gold ids, BM25 ids by descending score)."""
    pool = {}
    with open(os.path.join(datasets_dir, "text_tokenized.txt")) as f:
        for line in f:
            qid, title, body = line.split("\t")
            pool[qid] = (title.strip(), body.strip())
    splits = {}
    for name, fname in (("valid", "dev.txt"), ("test", "test.txt")):
        rows = []
        with open(os.path.join(datasets_dir, fname)) as f:
            for line in f:
                qid, gold, retrieved, scores = line.split("\t")
                retrieved = retrieved.split()
                scores = [float(s) for s in scores.strip().split()]
                ranked = [c for c, _ in sorted(zip(retrieved, scores), key=lambda kv: kv[1], reverse=True)]   # stable
                rows.append((qid, gold.split(), ranked))
        splits[name] = rows
    return pool, splits


class AskUbuntuEvaluator:
    name = "askubuntu"
    main_metric = "map_askubuntu_title"

    def __init__(self, embedder, pool: Dict[str, Tuple[str, str]], splits: Dict[str, list], text_components: str = "title"):
        if text_components not in ("title_and_body", "title", "body"):
            raise ValueError(f"text_components {text_components!r}")
        self.embedder, self.pool, self.splits, self.text_components = embedder, pool, splits, text_components

    @classmethod
    def from_dir(cls, embedder, datasets_dir: str = "data-eval/askubuntu", text_components: str = "title"):
        return cls(embedder, *load_askubuntu(datasets_dir), text_components=text_components)

    def _sent(self, qid: str) -> str:
        title, body = self.pool[qid]
        return {"title": title, "body": body, "title_and_body": " ".join([title, body])}[self.text_components]

    def task(self, eval_type: str) -> GroupTask:
        groups = []
        for qid, gold, ranked in self.splits[eval_type]:
            if not gold:
                continue
            gold_set = set(gold)
            if not gold_set & set(ranked):
                raise ValueError(f"askubuntu: none of the gold ids of query {qid!r} is in its candidate list")
            grades = [1 if c in gold_set else 0 for c in ranked]
            groups.append((qid, self._sent(qid), [self._sent(c) for c in ranked], grades, 0, grades))
        return build_groups(groups)

    def run(self, eval_type: str = "test", normalize: bool = True) -> Dict[str, float]:
        s = group_sums(self.embedder, self.task(eval_type), "dot", normalize)
        per = {"map": _ratio(s["sp"], s["R"]), "p@1": s["hits1"].astype(np.float64), "p@5": s["hits5"] / 5.0,
               "mrr": _ratio(1.0, s["first"])}
        return {f"{k}_askubuntu_{self.text_components}": float(v.mean()) if len(v) else 0.0 for k, v in per.items()}


# ---- SciDocs -----------------------------------------------------------------------------------------------------------------
def load_scidocs(datasets_dir: str) -> dict:
    """data.json: {"corpus": {pid: {"title": ...}}, "valid" / "test": {sub-task: {qid: {did: grade}}}}."""
    with open(os.path.join(datasets_dir, "data.json")) as f:
        return json.load(f)


class SciDocsEvaluator:
    name = "scidocs"
    main_metric = "map_scidocs_cosine_avg"

    def __init__(self, embedder, data: dict):
        self.embedder, self.data = embedder, data
        self.report: Dict[str, Dict[str, int]] = {}

    @classmethod
    def from_dir(cls, embedder, datasets_dir: str = "data-eval/scidocs"):
        return cls(embedder, load_scidocs(datasets_dir))

    def _title(self, pid: str) -> Optional[str]:
        entry = self.data["corpus"].get(pid)
        return None if entry is None else (entry["title"] or "")

    def task(self, qrel: Dict[str, Dict[str, int]], pool: Optional[SentencePool] = None) -> GroupTask:
        groups = []
        for qid, docs in qrel.items():
            query = self._title(qid)
            if not query:
                continue
            dids = sorted((d for d in docs if self._title(d)), reverse=True)          # descending id: trec_eval's tie-break
            grades = [int(docs[d]) for d in dids]
            r_extra = sum(1 for d, g in docs.items() if g > 0 and not self._title(d))
            groups.append((qid, query, [self._title(d) for d in dids], grades, r_extra, list(docs.values())))
        return build_groups(groups, pool)

    def run(self, eval_type: str = "test", normalize: bool = True) -> Dict[str, float]:
        qrels = self.data[eval_type]
        pool = SentencePool()
        tasks = {dname: self.task(qrel, pool) for dname, qrel in qrels.items()}           # one pool: every title encoded once
        emb = encode_unique(self.embedder, pool.sentences, normalize)
        results = {}
        for dname, task in tasks.items():
            for distance, mode in (("euclidean", "neg_l2"), ("cosine", "cos")):
                s = group_sums(self.embedder, task, mode, emb=emb)
                keep = s["R"] > 0
                self.report[f"{dname}_{distance}"] = {"evaluated": int(keep.sum()), "no_relevant": int((~keep).sum())}
                results[f"map_scidocs_{dname}_{distance}"] = float(_ratio(s["sp"], s["R"])[keep].mean()) if keep.any() else 0.0
                results[f"ndcg_scidocs_{dname}_{distance}"] = float(_ratio(s["dcg"], s["idcg"])[keep].mean()) if keep.any() else 0.0
        for metric in ("map", "ndcg"):
            for distance in ("euclidean", "cosine"):
                results[f"{metric}_scidocs_{distance}_avg"] = float(np.mean([results[f"{metric}_scidocs_{d}_{distance}"] for d in qrels]))
        return results


# ---- CQADupStack -------------------------------------------------------------------------------------------------------------
def load_cqadupstack(datasets_dir: str):
    """corpus.json {forum: {qid: text}} and retrieval_split.json {"valid" / "test": {forum: {qid: [duplicate ids]}}}."""
    with open(os.path.join(datasets_dir, "corpus.json")) as f:
        corpus = json.load(f)
    with open(os.path.join(datasets_dir, "retrieval_split.json")) as f:
        split = json.load(f)
    return corpus, split


def cqadupstack_from_ranked(idx, val, packed, has_rel, ctx=None, map_k: int = 100, ndcg_k: int = 10) -> Tuple[float, float]:
    """Ranked lists [nq, K] + packed qrels (grades 1) -> (mean map@map_k over all queries, mean ndcg@ndcg_k over the queries
    with has_rel): sgpt_eval_ranked at the two cuts, then the reference's normalisation (cqadupstack.py:95-127)."""
    from .evaluation import metric_sums
    s = metric_sums(idx, val, packed, [ndcg_k, map_k], check_order=False, ctx=ctx)
    ap = _ratio(s.sp[:, 1], s.hits[:, 1])                                         # positives IN the list; 0 without a hit
    ndcg = _ratio(s.dcg[:, 0], s.idcg[:, 0])[np.asarray(has_rel, bool)]
    return (float(ap.mean()) if len(ap) else 0.0), (float(ndcg.mean()) if len(ndcg) else 0.0)


class CQADupStackEvaluator:
    name = "cqadupstack"
    main_metric = "map@100_cqadupstack_avg"
    MAP_K, NDCG_K = 100, 10

    def __init__(self, embedder, corpus: Dict[str, Dict[str, str]], retrieval_split: dict, forum: str = "all"):
        if forum != "all" and forum not in corpus:
            raise ValueError(f"forum {forum!r}")
        self.embedder, self.corpus, self.retrieval_split = embedder, corpus, retrieval_split
        self.dnames = list(corpus) if forum == "all" else [forum]

    @classmethod
    def from_dir(cls, embedder, datasets_dir: str = "data-eval/cqadupstack", forum: str = "all"):
        return cls(embedder, *load_cqadupstack(datasets_dir), forum=forum)

    def forum_metrics(self, forum: str, eval_type: str, normalize: bool = True) -> Tuple[float, float]:
        import torch
        from .evaluation import pack_qrels
        from .runtime import get_context
        qrels = self.retrieval_split[eval_type][forum]
        qids = list(qrels)
        dids = [d for d in self.corpus[forum] if d not in qrels]                     # the pool without the queries
        pool = SentencePool()
        q_rows = [pool.row(self.corpus[forum][q]) for q in qids]
        d_rows = [pool.row(self.corpus[forum][d]) for d in dids]
        emb = encode_unique(self.embedder, pool.sentences, normalize)
        ctx = get_context(emb.device)
        q_emb = emb[torch.as_tensor(q_rows, dtype=torch.int64, device=emb.device)]
        d_emb = emb[torch.as_tensor(d_rows, dtype=torch.int64, device=emb.device)]
        val, idx, _ = ctx.score_topk(q_emb, d_emb, min(self.MAP_K, len(dids)))
        packed = pack_qrels({q: {d: 1 for d in rel} for q, rel in qrels.items()}, qids, {d: i for i, d in enumerate(dids)})
        return cqadupstack_from_ranked(idx, val, packed, [len(qrels[q]) > 0 for q in qids], ctx, self.MAP_K, self.NDCG_K)

    def run(self, eval_type: str = "test", normalize: bool = True) -> Dict[str, float]:
        results = {}
        for forum in self.dnames:
            results[f"map@100_cqadupstack_{forum}"], results[f"ndcg@10_cqadupstack_{forum}"] = self.forum_metrics(forum, eval_type, normalize)
        if len(self.dnames) > 1:
            results["map@100_cqadupstack_avg"] = float(np.mean([results[f"map@100_cqadupstack_{f}"] for f in self.dnames]))
            results["ndcg@10_cqadupstack_avg"] = float(np.mean([results[f"ndcg@10_cqadupstack_{f}"] for f in self.dnames]))
        return results


# ---- TwitterPara -------------------------------------------------------------------------------------------------------------
def _example(s1: str, s2: str, label: int):
    return s1, s2, (None if label == 3 else int(label > 3)), label * 20


def load_twitterurl(datasets_dir: str):
    """Twitter_URL_Corpus_test.txt: s1 \\t s2 \\t "(k, 6)" ...; label = k.  -> [(s1, s2, is_para in {1, 0, None}, gold score)]."""
    out = []
    with open(os.path.join(datasets_dir, "Twitter_URL_Corpus_test.txt")) as f:
        for line in f:
            items = line.strip().split("\t")
            out.append(_example(items[0], items[1], int(ast.literal_eval(items[2])[0])))
    return out


def load_pit(datasets_dir: str):
    """test.data: columns 2, 3 = the sentences, column 4 = the label."""
    out = []
    with open(os.path.join(datasets_dir, "test.data")) as f:
        for line in f:
            items = line.strip().split("\t")
            out.append(_example(items[2], items[3], int(items[4])))
    return out


def doubled_ranks(values) -> np.ndarray:
    """2 x scipy.stats.rankdata(values) (ties averaged) as exact integers: the host half of Spearman (gold scores)."""
    v = np.asarray(values, np.float64) + 0.0
    order = np.argsort(v, kind="stable")
    vs = v[order]
    start = np.r_[0, np.flatnonzero(vs[1:] != vs[:-1]) + 1]
    end = np.r_[start[1:], len(v)]
    out = np.empty(len(v), np.int64)
    out[order] = np.repeat(start + end + 1, end - start)
    return out


def pearson(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    den = float(np.sqrt((a * a).sum() * (b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


class TwitterParaEvaluator:
    name = "twitterpara"
    main_metric = "ap_twitter_avg"

    def __init__(self, embedder, datasets: Dict[str, list], dname: str = "all"):
        self.embedder, self.datasets = embedder, datasets
        self.dnames = ["twitterurl", "pit"] if dname == "all" else [dname]

    @classmethod
    def from_dir(cls, embedder, datasets_dir: str = "data-eval/twitterpara", dname: str = "all"):
        return cls(embedder, {"twitterurl": load_twitterurl(datasets_dir), "pit": load_pit(datasets_dir)}, dname)

    def dataset_metrics(self, data: list, normalize: bool = True) -> Tuple[float, float]:
        import torch
        from .runtime import get_context
        if not data:
            raise ValueError("twitterpara: empty dataset")
        pool = SentencePool()
        r1 = [pool.row(e[0]) for e in data]
        r2 = [pool.row(e[1]) for e in data]
        emb = encode_unique(self.embedder, pool.sentences, normalize)
        ctx = get_context(emb.device)
        a = emb[torch.as_tensor(r1, dtype=torch.int64, device=emb.device)]
        b = emb[torch.as_tensor(r2, dtype=torch.int64, device=emb.device)]
        pred = ctx.pairwise_scores(a, b, cosine=True)
        labels = np.asarray([-1 if e[2] is None else int(e[2]) for e in data], np.int32)
        out = ctx.eval_pairs(pred, labels)
        n_pos, ap_num = int(out["n_pos"].item()), float(out["ap_num"].item())
        ap = ap_num / n_pos if n_pos else 0.0                                          # undefined without a positive: 0
        return ap, pearson(out["rank2"].cpu().numpy(), doubled_ranks([e[3] for e in data]))

    def run(self, eval_type: Optional[str] = None, normalize: bool = True) -> Dict[str, float]:
        if eval_type == "valid":
            logger.warning("TwitterPara has no development set: evaluated on the test set")
        results = {}
        for dname in self.dnames:
            results[f"ap_twitter_{dname}"], results[f"spearman_twitter_{dname}"] = self.dataset_metrics(self.datasets[dname], normalize)
        if len(self.dnames) > 1:
            results["ap_twitter_avg"] = float(np.mean([results[f"ap_twitter_{d}"] for d in self.dnames]))
            results["spearman_twitter_avg"] = float(np.mean([results[f"spearman_twitter_{d}"] for d in self.dnames]))
        return results
