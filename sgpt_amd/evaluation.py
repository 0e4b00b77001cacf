"""Retrieval metrics (NDCG / MAP / Recall / P / MRR / Accuracy @ k) computed on the device.

  EvaluateRetrieval   <- beir.retrieval.evaluation.EvaluateRetrieval as biencoder/beir/beir_dense_retriever.py:440-446 uses it
  "st" style          <- sentence_transformers/evaluation/InformationRetrievalEvaluator.py:189-271 (compute_metrics)

The reference takes both from `beir` / `pytrec_eval`; neither is a dependency here.  Every metric is a host-side
normalisation of one kernel's per-query, per-cut sums (include/sgpt_hip.h::sgpt_eval_ranked): one definition, no CPU
metric code, and -- as everywhere in this package -- no fallback: without a GPU the calls raise SgptHipError.

Definitions.  Per query, with its ranked list r_1 .. r_n (descending score, ties to the lower corpus position), its judged
documents rel(d) (integer grades; relevant: rel > 0), R = the number of relevant judged documents (judged documents that
are not in the corpus count in R, as in trec_eval) and a cut k:
  hits@k = relevant documents among r_1 .. r_min(k, n);  P@k = hits@k / k;  Recall@k = hits@k / R;  Accuracy@k = [hits@k > 0]
  MRR@k  = 1 / (rank of the first relevant document) if that rank <= k, else 0
  DCG@k  = sum_{i <= min(k, n)} max(rel(r_i), 0) / log2(i + 1);  IDCG@k: the same over the judged grades sorted descending;
  NDCG@k = DCG@k / IDCG@k
  SP@k   = sum over relevant r_i, i <= min(k, n), of hits@i / i;  MAP@k = SP@k / R (trec `map_cut`); the "st" style divides
           by min(k, R) as InformationRetrievalEvaluator does.
Queries without a qrels entry and queries with R = 0 are left out of the means; how many is reported (`report`), the mean
is over the evaluated queries.  Ties are exactly equal fp32 scores; trec_eval's tie-break by document id string is not
reproduced."""
import logging
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

ABSENT = np.iinfo(np.int64).max        # position of a judged document that is not in the corpus: never in a ranked list
MAX_CUTS = 16                          # SGPT_EVAL_MAX_CUTS


@dataclass
class RankedLists:
    """What a search leaves on the device: row q = query_ids[q]; idx holds positions into corpus_ids (-1: padding)."""
    query_ids: List[str]
    corpus_ids: List[str]
    val: "torch.Tensor"        # noqa: F821  fp32 [nq, K]
    idx: "torch.Tensor"        # noqa: F821  int64 [nq, K]
    pos_of: Optional[Dict[str, int]] = None      # corpus id -> position (the search has built it already; else made on first use)

    def positions(self) -> Dict[str, int]:
        if self.pos_of is None:
            self.pos_of = {cid: i for i, cid in enumerate(self.corpus_ids)}
        return self.pos_of


@dataclass
class PackedQrels:
    """The qrels of `query_ids` as a CSR in position space (host arrays)."""
    off: np.ndarray            # int32 [nq + 1]
    pos: np.ndarray            # int64: judged positions, ascending within a query (ABSENT for documents outside the corpus)
    rel: np.ndarray            # int32: grade of each entry of pos
    ideal: np.ndarray          # int32: the query's grades sorted descending
    R: np.ndarray              # int32 [nq]: relevant (grade > 0) judged documents
    judged: np.ndarray         # bool [nq]: the query has a qrels entry
    no_qrels: List[str]        # queries without a qrels entry
    no_relevant: List[str]     # queries whose qrels entry holds no grade > 0

    @property
    def evaluated(self) -> np.ndarray:
        return self.judged & (self.R > 0)


def check_k_values(k_values: Sequence[int]) -> List[int]:
    """-> the cuts as a list of ints; ValueError unless they are 1 .. MAX_CUTS positive integers in strictly ascending order."""
    ks = list(k_values)
    if not 1 <= len(ks) <= MAX_CUTS:
        raise ValueError(f"k_values: between 1 and {MAX_CUTS} cuts, got {len(ks)}")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"k_values: positive integers, got {k!r}")
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"k_values must be strictly ascending, got {ks}")
    return [int(k) for k in ks]


def pack_qrels(qrels: Dict[str, Dict[str, int]], query_ids: Sequence[str], pos_of: Dict[str, int], binary: bool = False) -> PackedQrels:
    """Dict[qid, Dict[doc_id, grade]] -> CSR over `query_ids` in the position space `pos_of` (doc_id -> position).  Judged
    documents missing from pos_of keep their grade under the position ABSENT.  binary=True: grades become [grade > 0]."""
    off = np.zeros(len(query_ids) + 1, dtype=np.int64)
    pos_l, rel_l, ideal_l = [], [], []
    R = np.zeros(len(query_ids), dtype=np.int32)
    judged = np.zeros(len(query_ids), dtype=bool)
    no_qrels, no_relevant = [], []
    for qi, qid in enumerate(query_ids):
        entry = qrels.get(qid)
        if entry is None:
            no_qrels.append(qid)
            off[qi + 1] = off[qi]
            continue
        judged[qi] = True
        p = np.fromiter((pos_of.get(d, ABSENT) for d in entry), dtype=np.int64, count=len(entry))
        g = np.fromiter((int(v) for v in entry.values()), dtype=np.int64, count=len(entry))
        if binary:
            g = (g > 0).astype(np.int64)
        order = np.argsort(p, kind="stable")
        pos_l.append(p[order])
        rel_l.append(g[order])
        ideal_l.append(np.sort(g)[::-1])
        R[qi] = int((g > 0).sum())
        if R[qi] == 0:
            no_relevant.append(qid)
        off[qi + 1] = off[qi] + len(entry)
    if off[-1] >= 2 ** 31:
        raise ValueError("qrels: more than 2^31 judgements")
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)   # noqa: E731
    return PackedQrels(off.astype(np.int32), cat(pos_l, np.int64), cat(rel_l, np.int32), cat(ideal_l, np.int32), R, judged,
                       no_qrels, no_relevant)


def pack_results(results: Dict[str, Dict[str, float]], query_ids: Sequence[str], pos_of: Dict[str, int], K: int,
                 ignore_identical_ids: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Dict[qid, Dict[doc_id, score]] -> (idx int64 [nq, K], val fp32 [nq, K]): every row sorted by descending fp32 score, ties
    by ascending position, the tail padded with (-1, -inf).  K covers the longest list.  ignore_identical_ids: a document that
    carries the query's id is dropped, as beir's evaluate does.  A query missing from `results` gets an empty row."""
    idx = np.full((len(query_ids), K), -1, dtype=np.int64)
    val = np.full((len(query_ids), K), -np.inf, dtype=np.float32)
    for qi, qid in enumerate(query_ids):
        entry = results.get(qid)
        if not entry:
            continue
        docs = [d for d in entry if not (ignore_identical_ids and d == qid)]
        if len(docs) > K:
            raise ValueError(f"pack_results: query {qid!r} has {len(docs)} results, K = {K}")
        p = np.fromiter((pos_of[d] for d in docs), dtype=np.int64, count=len(docs))
        v = np.fromiter((entry[d] for d in docs), dtype=np.float32, count=len(docs))
        order = np.lexsort((p, -v))                       # primary key: -score; secondary: position
        idx[qi, : len(docs)] = p[order]
        val[qi, : len(docs)] = v[order]
    return idx, val


class MetricSums:
    """The kernel's per-query outputs on the host, and the two output styles made of them."""

    def __init__(self, k_values, hits, first, dcg, idcg, sp, R, packed: PackedQrels):
        self.k_values = list(k_values)
        self.hits, self.first = np.asarray(hits, np.int64), np.asarray(first, np.int64)
        self.dcg, self.idcg, self.sp = (np.asarray(a, np.float64) for a in (dcg, idcg, sp))
        self.R = np.asarray(R, np.int64)
        self.evaluated = packed.judged & (self.R > 0)
        self.report = {"evaluated": int(self.evaluated.sum()), "no_qrels": len(packed.no_qrels),
                       "no_relevant": len(packed.no_relevant)}

    def _mean(self, per_query: np.ndarray) -> List[float]:
        rows = per_query[self.evaluated]
        return rows.mean(axis=0).tolist() if len(rows) else [0.0] * len(self.k_values)

    def _safe(self, num, den):
        den = np.asarray(den, np.float64)
        return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, dtype=np.float64), where=den > 0)

    def per_query(self, st_map: bool = False) -> Dict[str, np.ndarray]:
        k = np.asarray(self.k_values, np.float64)[None, :]
        Rc = self.R[:, None].astype(np.float64)
        return {
            "ndcg": self._safe(self.dcg, self.idcg), "map": self._safe(self.sp, np.minimum(k, Rc) if st_map else Rc),
            "recall": self._safe(self.hits, Rc), "precision": self.hits / k, "accuracy": (self.hits > 0).astype(np.float64),
            "mrr": self._safe(1.0, self.first) * (self.first > 0),
        }

    def beir(self):
        pq = self.per_query()
        named = lambda name, key: {f"{name}@{k}": round(v, 5) for k, v in zip(self.k_values, self._mean(pq[key]))}   # noqa: E731
        return named("NDCG", "ndcg"), named("MAP", "map"), named("Recall", "recall"), named("P", "precision")

    def custom(self, metric: str) -> Dict[str, float]:
        if metric.lower() not in ("mrr", "mrr@k", "mrr_cut"):
            raise ValueError(f"evaluate_custom: metric {metric!r} is not served (mrr)")
        return {f"MRR@{k}": round(v, 5) for k, v in zip(self.k_values, self._mean(self.per_query()["mrr"]))}

    def st(self) -> Dict[str, Dict[int, float]]:
        pq = self.per_query(st_map=True)
        return {f"{name}@k": dict(zip(self.k_values, self._mean(pq[key])))
                for name, key in (("accuracy", "accuracy"), ("precision", "precision"), ("recall", "recall"), ("ndcg", "ndcg"),
                                  ("mrr", "mrr"), ("map", "map"))}


def metric_sums(idx, val, packed: PackedQrels, k_values: Sequence[int], check_order: bool = True, ctx=None) -> MetricSums:
    """idx / val [nq, K] (device tensors or host arrays) + packed qrels -> MetricSums through the kernel.  Lists shallower than
    the deepest cut are padded with (-1, -inf) columns: padding ends a list, so every sum is the one over min(k, n) ranks."""
    import torch
    from .runtime import get_context
    ks = check_k_values(k_values)
    ctx = ctx if ctx is not None else get_context(idx.device if isinstance(idx, torch.Tensor) and idx.is_cuda else None)
    idx = torch.as_tensor(idx).to(device=ctx.device, dtype=torch.int64)
    val = torch.as_tensor(val).to(device=ctx.device, dtype=torch.float32)
    nq, K = idx.shape
    if K < ks[-1]:
        pad_i = torch.full((nq, ks[-1]), -1, dtype=torch.int64, device=ctx.device)
        pad_v = torch.full((nq, ks[-1]), float("-inf"), dtype=torch.float32, device=ctx.device)
        pad_i[:, :K] = idx
        pad_v[:, :K] = val
        idx, val = pad_i, pad_v
    out = ctx.eval_ranked(idx, val, packed.off, packed.pos, packed.rel, packed.ideal, ks, check_order=check_order)
    host = {n: t.cpu().numpy() for n, t in out.items()}
    return MetricSums(ks, host["hits"], host["first"], host["dcg"], host["idcg"], host["sp"], host["R"], packed)


class EvaluateRetrieval:
    """beir's EvaluateRetrieval as the reference driver uses it (beir_dense_retriever.py:440-446), metrics by the HIP kernel.

        retriever = EvaluateRetrieval(DenseRetrievalExactSearch(model), k_values=[1, 3, 5, 10, 100, 1000])
        results = retriever.retrieve(corpus, queries)                                   # the reference's dict
        ndcg, _map, recall, precision = retriever.evaluate(qrels, results, retriever.k_values)
    or, when only the metrics are wanted (no D2H of the lists, no dict):
        ranked = retriever.retrieve_ranked(corpus, queries)
        ndcg, _map, recall, precision = retriever.evaluate_ranked(qrels, ranked, retriever.k_values)"""

    def __init__(self, retriever=None, k_values: List[int] = [1, 3, 5, 10, 100, 1000], score_function: str = "cos_sim"):
        self.k_values = k_values
        self.top_k = max(k_values)
        self.retriever = retriever
        self.score_function = score_function

    def retrieve(self, corpus: Dict[str, Dict[str, str]], queries: Dict[str, str], **kwargs) -> Dict[str, Dict[str, float]]:
        if not self.retriever:
            raise ValueError("Model/Technique has not been provided!")
        return self.retriever.search(corpus, queries, self.top_k, self.score_function, **kwargs)

    def retrieve_ranked(self, corpus: Dict[str, Dict[str, str]], queries: Dict[str, str], **kwargs) -> RankedLists:
        if not self.retriever:
            raise ValueError("Model/Technique has not been provided!")
        return self.retriever.search_ranked(corpus, queries, self.top_k, self.score_function, **kwargs)

    # -- device path --------------------------------------------------------------------------
    @staticmethod
    def ranked_sums(qrels: Dict[str, Dict[str, int]], ranked: RankedLists, k_values: List[int], binary: bool = False,
                    check_order: bool = True) -> MetricSums:
        packed = pack_qrels(qrels, ranked.query_ids, ranked.positions(), binary=binary)
        return metric_sums(ranked.idx, ranked.val, packed, k_values, check_order=check_order)

    @staticmethod
    def evaluate_ranked(qrels: Dict[str, Dict[str, int]], ranked: RankedLists, k_values: List[int], style: str = "beir",
                        return_report: bool = False, check_order: bool = True):
        """style "beir": (ndcg, _map, recall, precision), dicts keyed NDCG@k / MAP@k / Recall@k / P@k, rounded to 5 places;
        style "st": the dict of InformationRetrievalEvaluator.compute_metrics (binary relevance, its MAP variant).
        return_report=True appends {"evaluated", "no_qrels", "no_relevant"}: the query counts behind and beside the means."""
        if style not in ("beir", "st"):
            raise ValueError("style must be 'beir' or 'st'")
        sums = EvaluateRetrieval.ranked_sums(qrels, ranked, k_values, binary=style == "st", check_order=check_order)
        return EvaluateRetrieval._styled(sums, style, return_report)

    # -- dict path (drop-in) ------------------------------------------------------------------
    @staticmethod
    def results_sums(qrels: Dict[str, Dict[str, int]], results: Dict[str, Dict[str, float]], k_values: List[int],
                     ignore_identical_ids: bool = True, binary: bool = False, corpus_ids: Optional[Sequence[str]] = None) -> MetricSums:
        """The dict path: `results` packed into padded [nq, K] arrays (score descending, then position) and put through the
        same kernel.  Position space: `corpus_ids` when given (then equal scores rank as the search ranks them), else the
        document ids of results and qrels in sorted order."""
        ks = check_k_values(k_values)
        query_ids = list(results)
        if corpus_ids is None:
            seen = set()
            for qid in query_ids:
                seen.update(results[qid])
                seen.update(qrels.get(qid, ()))
            corpus_ids = sorted(seen)
        pos_of = {cid: i for i, cid in enumerate(corpus_ids)}
        K = max([ks[-1]] + [len(results[q]) for q in query_ids])
        idx, val = pack_results(results, query_ids, pos_of, K, ignore_identical_ids=ignore_identical_ids)
        packed = pack_qrels(qrels, query_ids, pos_of, binary=binary)
        return metric_sums(idx, val, packed, ks, check_order=True)

    @staticmethod
    def evaluate(qrels: Dict[str, Dict[str, int]], results: Dict[str, Dict[str, float]], k_values: List[int],
                 ignore_identical_ids: bool = True, style: str = "beir", return_report: bool = False,
                 corpus_ids: Optional[Sequence[str]] = None):
        if style not in ("beir", "st"):
            raise ValueError("style must be 'beir' or 'st'")
        sums = EvaluateRetrieval.results_sums(qrels, results, k_values, ignore_identical_ids, binary=style == "st", corpus_ids=corpus_ids)
        return EvaluateRetrieval._styled(sums, style, return_report)

    @staticmethod
    def evaluate_custom(qrels: Dict[str, Dict[str, int]], results, k_values: List[int], metric: str) -> Dict[str, float]:
        """metric "mrr" -> {MRR@k}.  `results`: the dict of retrieve(), or the RankedLists of retrieve_ranked()."""
        if metric.lower() not in ("mrr", "mrr@k", "mrr_cut"):
            raise ValueError(f"evaluate_custom: metric {metric!r} is not served (mrr)")
        sums = (EvaluateRetrieval.ranked_sums(qrels, results, k_values) if isinstance(results, RankedLists)
                else EvaluateRetrieval.results_sums(qrels, results, k_values))
        EvaluateRetrieval._log(sums)
        return sums.custom(metric)

    @staticmethod
    def _log(sums: MetricSums):
        rep = sums.report
        if rep["no_qrels"] or rep["no_relevant"]:
            logger.warning("Evaluated %d queries; left out of the means: %d without qrels, %d without a relevant document",
                           rep["evaluated"], rep["no_qrels"], rep["no_relevant"])

    @staticmethod
    def _styled(sums: MetricSums, style: str, return_report: bool):
        EvaluateRetrieval._log(sums)
        if style == "st":
            out = sums.st()
            return (out, sums.report) if return_report else out
        out = sums.beir()
        for group in out:
            for name, v in group.items():
                logger.info("%s: %.4f", name, v)
        return out + (sums.report,) if return_report else out
