"""-m gpu: the metrics kernel (csrc/eval.hip, sgpt_eval_ranked) and sgpt_amd/evaluation.py against a float64 restatement of
the metric definitions written below, and against the reference's InformationRetrievalEvaluator output (tests/golden/ir_metrics.json).

Bounds.  Integer outputs (hits, rank of the first relevant document, R) must be equal.  Float outputs must be within 1e-5
relative of the float64 value: a 1001-term fp32 sum of non-negative terms in a fixed tree order is good to about
log2(1001) x 2^-24 = 6e-7 relative, so 1e-5 leaves a factor of ~16 and still fails on any dropped or misplaced term (the
smallest term of DCG@1000 is 1 / log2(1001) = 0.1)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-5
K_ALL = [1, 3, 5, 10, 100, 1000]


def ref_sums(idx, off, pos, rel, ideal, k_values):
    """float64 restatement: per query and cut hits, first relevant rank (0 if beyond the cut), DCG, IDCG, SP; R per query."""
    nq, nk = idx.shape[0], len(k_values)
    hits, first = np.zeros((nq, nk), np.int64), np.zeros((nq, nk), np.int64)
    dcg, idcg, sp = (np.zeros((nq, nk), np.float64) for _ in range(3))
    R = np.zeros(nq, np.int64)
    for q in range(nq):
        grade = {int(p): int(g) for p, g in zip(pos[off[q]: off[q + 1]], rel[off[q]: off[q + 1]])}
        ide = np.asarray(ideal[off[q]: off[q + 1]], np.float64)
        R[q] = int((ide > 0).sum())
        row = idx[q]
        neg = np.nonzero(row < 0)[0]
        n = int(neg[0]) if len(neg) else len(row)                      # padding ends the list
        g = np.array([grade.get(int(p), 0) for p in row[:n]], np.float64)
        relv = g > 0
        ranks = np.arange(1, n + 1, dtype=np.float64)
        cum = np.cumsum(relv)
        f = int(np.argmax(relv)) + 1 if relv.any() else 0
        for j, k in enumerate(k_values):
            m = min(k, n)
            hits[q, j] = int(relv[:m].sum())
            first[q, j] = f if 0 < f <= k else 0
            dcg[q, j] = (np.maximum(g[:m], 0) / np.log2(ranks[:m] + 1)).sum()
            mi = min(k, len(ide))
            idcg[q, j] = (np.maximum(ide[:mi], 0) / np.log2(np.arange(1, mi + 1) + 1.0)).sum()
            sp[q, j] = (relv[:m] * cum[:m] / ranks[:m]).sum()
    return dict(hits=hits, first=first, dcg=dcg, idcg=idcg, sp=sp, R=R)


def make_case(rng, nq, K, n_corpus, big_query=None, tie_rows=True):
    """Random graded qrels (grades 0..3 and a few negatives) and ranked lists [nq, K] with -1 padding from position 0, from the
    middle, and none; exact score ties; optionally one query with 2000 judgements."""
    from sgpt_amd.evaluation import ABSENT
    idx = np.full((nq, K), -1, np.int64)
    val = np.full((nq, K), -np.inf, np.float32)
    off, pos_l, rel_l, ideal_l = [0], [], [], []
    for q in range(nq):
        mode = q % 5
        n = 0 if mode == 3 else (int(rng.integers(1, K)) if mode == 1 and K > 1 else K)
        n = min(n, n_corpus)
        docs = rng.choice(n_corpus, size=n, replace=False)
        s = np.sort(rng.standard_normal(n).astype(np.float32))[::-1].copy()
        if tie_rows and n > 4 and q % 2 == 0:                          # exact ties: runs of equal scores, positions ascending inside
            a = int(rng.integers(0, n - 3))
            b = min(n, a + int(rng.integers(2, 40)))
            s[a:b] = s[a]
            docs[a:b] = np.sort(docs[a:b])
        idx[q, :n], val[q, :n] = docs, s
        nj = 2000 if q == big_query else int(rng.integers(0, 40)) + (300 if q % 11 == 4 else 0)
        nj = min(nj, n_corpus)
        take_in = min(n, int(rng.integers(0, nj + 1)))
        inside = rng.choice(docs, size=take_in, replace=False) if take_in else np.zeros(0, np.int64)
        rest = np.setdiff1d(np.arange(n_corpus), docs)
        outside = rng.choice(rest, size=min(nj - take_in, len(rest)), replace=False)
        p = np.concatenate([inside, outside]).astype(np.int64)
        n_abs = int(rng.integers(0, 3))
        p = np.concatenate([np.sort(p), np.full(n_abs, ABSENT, np.int64)])
        g = rng.choice([-1, 0, 1, 2, 3], size=len(p), p=[0.05, 0.25, 0.4, 0.2, 0.1]).astype(np.int32)
        pos_l.append(p)
        rel_l.append(g)
        ideal_l.append(np.sort(g)[::-1])
        off.append(off[-1] + len(p))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt)    # noqa: E731
    return idx, val, np.array(off, np.int32), cat(pos_l, np.int64), cat(rel_l, np.int32), cat(ideal_l, np.int32)


def check_against_reference(got, want, tag):
    worst = {}
    for name in ("hits", "first", "R"):
        g = got[name].cpu().numpy().astype(np.int64)
        assert np.array_equal(g, want[name]), f"{tag}: {name} differs at {np.argwhere(g != want[name])[:5].tolist()}"
    for name in ("dcg", "idcg", "sp"):
        g = got[name].cpu().numpy().astype(np.float64)
        w = want[name]
        assert np.array_equal(w == 0, g == 0), f"{tag}: {name} zero pattern"
        relerr = np.abs(g - w) / np.where(w != 0, np.abs(w), 1.0)
        worst[name] = float(relerr.max()) if relerr.size else 0.0
    print(f"{tag}: max relative error dcg {worst['dcg']:.2e} idcg {worst['idcg']:.2e} sp {worst['sp']:.2e} (bound {RTOL:g})")
    for name, e in worst.items():
        assert e <= RTOL, f"{tag}: {name} off by {e:.3e} relative"


@pytest.mark.parametrize("nq", [1, 7, 1000])
@pytest.mark.parametrize("K", [11, 101, 1001])
def test_kernel_matches_float64_definitions(nq, K):
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(1000 * nq + K)
    idx, val, off, pos, rel, ideal = make_case(rng, nq, K, n_corpus=5000, big_query=(nq // 2 if nq > 1 else 0))
    ks = [k for k in K_ALL if k <= K]
    got = ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(val), off, pos, rel, ideal, ks, check_order=True)
    want = ref_sums(idx, off, pos, rel, ideal, ks)
    assert want["hits"].sum() > 0 or nq == 1
    check_against_reference(got, want, f"nq={nq} K={K}")
    # the same sums without the order check (asynchronous call; val is not read)
    got2 = ctx.eval_ranked(torch.from_numpy(idx), None, off, pos, rel, ideal, ks, check_order=False)
    for name in got:
        assert torch.equal(got[name], got2[name]), name


def test_cuts_that_are_not_the_default_and_a_cut_on_a_chunk_boundary():
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(5)
    idx, val, off, pos, rel, ideal = make_case(rng, 33, 300, n_corpus=800)
    ks = [2, 63, 64, 65, 128, 129, 191, 192, 256, 300]
    got = ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(val), off, pos, rel, ideal, ks)
    check_against_reference(got, ref_sums(idx, off, pos, rel, ideal, ks), "chunk-boundary cuts")


def _fixture():
    fx = json.load(open(os.path.join(GOLDEN, "ir_metrics.json")))
    qids = fx["query_ids"]
    corpus_ids = [f"d{i}" for i in range(fx["n_docs"])]
    results = {q: {f"d{d}": float(np.float32(n) / np.float32(100000.0)) for d, n in zip(docs, nums)}
               for q, docs, nums in zip(qids, fx["lists"], fx["score_num"])}
    qrels = {q: {f"d{d}": 1 for d in rel} for q, rel in zip(qids, fx["relevant"])}
    return fx, qids, corpus_ids, results, qrels


def test_reference_fixture_st_style():
    """The reference's InformationRetrievalEvaluator.compute_metrics output on seeded inputs, through the dict path and
    through device-resident lists."""
    from sgpt_amd.evaluation import EvaluateRetrieval, RankedLists
    fx, qids, corpus_ids, results, qrels = _fixture()
    ks = fx["k_values"]
    got = EvaluateRetrieval.evaluate(qrels, results, ks, style="st")
    idx = torch.tensor(fx["lists"], dtype=torch.int64, device="cuda:0")
    val = (torch.tensor(fx["score_num"], dtype=torch.float32) / torch.tensor(100000.0, dtype=torch.float32)).to("cuda:0")
    got_r, rep = EvaluateRetrieval.evaluate_ranked(qrels, RankedLists(qids, corpus_ids, val, idx), ks, style="st", return_report=True)
    assert rep == {"evaluated": 200, "no_qrels": 0, "no_relevant": 0}
    for g, tag in ((got, "dict path"), (got_r, "ranked path")):
        worst = 0.0
        for name, per_k in fx["metrics"].items():
            for k, w in per_k.items():
                v = g[name][int(k)]
                assert (w == 0) == (v == 0)
                worst = max(worst, abs(v - w) / (abs(w) if w else 1.0))
        print(f"reference fixture, {tag}: max relative error {worst:.2e} (bound {RTOL:g})")
        assert worst <= RTOL
    assert got == got_r


def test_beir_style_against_float64_definitions_with_left_out_queries():
    from sgpt_amd.evaluation import EvaluateRetrieval
    rng = np.random.default_rng(77)
    corpus_ids = [f"d{i}" for i in range(400)]
    results, qrels = {}, {}
    for q in range(60):
        docs = rng.choice(400, size=int(rng.integers(1, 120)), replace=False)
        results[f"q{q}"] = {f"d{d}": float(s) for d, s in zip(docs, rng.standard_normal(len(docs)).astype(np.float32))}
        if q % 9 == 3:
            continue                                                    # no qrels entry
        judged = np.concatenate([rng.choice(docs, size=min(len(docs), 4), replace=False), rng.choice(400, size=3)])
        qrels[f"q{q}"] = {f"d{d}": (0 if q % 9 == 5 else int(rng.integers(0, 4))) for d in judged}     # q % 9 == 5: R = 0
        qrels[f"q{q}"]["not-in-corpus"] = 0 if q % 9 == 5 else 2
    ks = [1, 3, 5, 10, 100, 1000]
    ndcg, _map, recall, precision, rep = EvaluateRetrieval.evaluate(qrels, results, ks, return_report=True, corpus_ids=corpus_ids + ["not-in-corpus-x"])
    acc = {n: {k: [] for k in ks} for n in ("NDCG", "MAP", "Recall", "P", "MRR")}
    pos_of = {c: i for i, c in enumerate(corpus_ids)}
    n_eval = 0
    for qid, res in results.items():
        if qid not in qrels or not any(g > 0 for g in qrels[qid].values()):
            continue
        n_eval += 1
        order = sorted(res, key=lambda d: (-np.float32(res[d]), pos_of[d]))
        g = np.array([qrels[qid].get(d, 0) for d in order], np.float64)
        ide = np.sort(np.array(list(qrels[qid].values()), np.float64))[::-1]
        R = (ide > 0).sum()
        relv, ranks = g > 0, np.arange(1, len(g) + 1, dtype=np.float64)
        f = int(np.argmax(relv)) + 1 if relv.any() else 0
        for k in ks:
            m, mi = min(k, len(g)), min(k, len(ide))
            acc["P"][k].append(relv[:m].sum() / k)
            acc["Recall"][k].append(relv[:m].sum() / R)
            acc["MAP"][k].append((relv[:m] * np.cumsum(relv)[:m] / ranks[:m]).sum() / R)
            acc["NDCG"][k].append((np.maximum(g[:m], 0) / np.log2(ranks[:m] + 1)).sum()
                                  / (np.maximum(ide[:mi], 0) / np.log2(np.arange(1, mi + 1) + 1.0)).sum())
            acc["MRR"][k].append(1.0 / f if 0 < f <= k else 0.0)
    assert rep == {"evaluated": n_eval, "no_qrels": sum(1 for q in results if q not in qrels),
                   "no_relevant": sum(1 for q in results if q in qrels) - n_eval}
    assert rep["no_qrels"] > 0 and rep["no_relevant"] > 0
    mrr = EvaluateRetrieval.evaluate_custom(qrels, results, ks, metric="mrr")
    for got, name in ((ndcg, "NDCG"), (_map, "MAP"), (recall, "Recall"), (precision, "P"), (mrr, "MRR")):
        assert list(got) == [f"{name}@{k}" for k in ks]
        for k in ks:
            w = float(np.mean(acc[name][k]))
            assert abs(got[f"{name}@{k}"] - w) <= 0.5e-5 + RTOL * abs(w), (name, k, got[f"{name}@{k}"], w)   # 5-place rounding + RTOL


def _texts(rng, n, lo, hi, tag):
    words = ["alpha", "beta", "gamma", "delta", "query", "doc", "paris", "atom", "cell", "gene", "?", "the", "of"]
    return [f"{tag}{i} " + " ".join(rng.choice(words, size=int(rng.integers(lo, hi))).tolist()) for i in range(n)]


@pytest.mark.parametrize("fn", ["cos_sim", "dot"])
def test_end_to_end_ranked_equals_dict_path(fn, tmp_path, monkeypatch):
    """evaluate_ranked(qrels, search_ranked(...)) == evaluate(qrels, search(...)) on a tiny synthetic model, with a query id
    that is also a corpus id (self-match rule) and top_k + 1 larger than the corpus."""
    from helpers import build_model, load_case
    from sgpt_amd.beir import CustomEmbedder, DenseRetrievalExactSearch
    from sgpt_amd.evaluation import EvaluateRetrieval
    from sgpt_amd.tokenization import SyntheticTokenizer
    monkeypatch.chdir(tmp_path)
    fx, cfg_kw, *_ = load_case("tiny_right")
    m = build_model(cfg_kw, int(fx["seed"]), float(fx["std"]), "fp32")
    tok = SyntheticTokenizer(cfg_kw["vocab_size"])
    emb = CustomEmbedder(model_name="synthetic/tiny-neo", model=m, tokenizer=tok, method="weightedmean", specb=True,
                         maxseqlen=40, dataset="unit")
    rng = np.random.default_rng(21)
    corpus = {f"d{i}": {"title": t.split(" ")[0], "text": t} for i, t in enumerate(_texts(rng, 90, 3, 40, "c"))}
    queries = {f"q{i}": t for i, t in enumerate(_texts(rng, 11, 2, 8, "u"))}
    queries["d3"] = "gene cell ?"                                       # id collides with a corpus id
    cids = list(corpus)
    qrels = {q: {cids[int(j)]: int(rng.integers(0, 3)) for j in rng.choice(90, size=6, replace=False)} for q in queries}
    qrels["d3"]["d3"] = 2                                               # the self-match is judged relevant and must never be a hit
    qrels["q0"]["gone"] = 1                                             # judged, not in the corpus
    del qrels["q1"]                                                     # a query without qrels
    retriever = EvaluateRetrieval(DenseRetrievalExactSearch(emb, corpus_chunk_size=32), k_values=[1, 3, 5, 10, 100, 1000],
                                  score_function=fn)
    results = retriever.retrieve(corpus, queries)
    ranked = retriever.retrieve_ranked(corpus, queries)
    assert ranked.val.is_cuda and ranked.idx.shape == (len(queries), 90) and ranked.query_ids == list(queries)
    assert all(len(v) == (89 if q == "d3" else 90) for q, v in results.items()) and "d3" not in results["d3"]
    # search() is search_ranked + assemble_results
    from sgpt_amd.beir import assemble_results
    assert results == assemble_results(ranked.query_ids, ranked.corpus_ids, ranked.val.cpu().numpy(), ranked.idx.cpu().numpy())
    a = retriever.evaluate(qrels, results, retriever.k_values, return_report=True, corpus_ids=ranked.corpus_ids)
    b = retriever.evaluate_ranked(qrels, ranked, retriever.k_values, return_report=True)
    assert a == b
    assert a[4] == {"evaluated": len(queries) - 1, "no_qrels": 1, "no_relevant": 0}
    assert a[2]["Recall@1000"] < 1.0 and a[0]["NDCG@10"] > 0.0          # "gone" and the self-match keep recall below 1
    assert retriever.evaluate(qrels, results, retriever.k_values) == b[:4]          # position space from the ids alone: no ties here
    assert retriever.evaluate_custom(qrels, results, [1, 10], "mrr") == retriever.evaluate_custom(qrels, ranked, [1, 10], "mrr")
    st_a = retriever.evaluate(qrels, results, [1, 10, 100], style="st", corpus_ids=ranked.corpus_ids)
    assert st_a == retriever.evaluate_ranked(qrels, ranked, [1, 10, 100], style="st")


def test_check_order_and_argument_errors_are_status_codes():
    from sgpt_amd import get_context
    from sgpt_amd.evaluation import EvaluateRetrieval, RankedLists
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(3)
    idx, val, off, pos, rel, ideal = make_case(rng, 9, 130, n_corpus=500, tie_rows=False)
    ok = ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(val), off, pos, rel, ideal, [1, 10, 100])
    bad_val = val.copy()
    full = [q for q in range(9) if idx[q, -1] >= 0][0]
    bad_val[full, 70], bad_val[full, 100] = val[full, 100], val[full, 70]          # one row handed over in scrambled order
    with pytest.raises(ValueError, match="not sorted by descending score"):
        ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(bad_val), off, pos, rel, ideal, [1, 10, 100])
    # a break beyond the deepest cut is still found; without the check the same call succeeds
    with pytest.raises(ValueError, match="not sorted"):
        ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(bad_val), off, pos, rel, ideal, [1, 10])
    again = ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(bad_val), off, pos, rel, ideal, [1, 10, 100], check_order=False)
    assert all(torch.equal(ok[n], again[n]) for n in ok)
    for ks, msg in (([10, 1], "strictly ascending"), ([0, 1], "positive"), ([1, 131], "deeper than the lists"), ([], "cuts"),
                    (list(range(1, 18)), "cuts")):
        with pytest.raises(ValueError, match=msg):
            ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(val), off, pos, rel, ideal, ks)
    with pytest.raises(ValueError):
        ctx.eval_ranked(torch.from_numpy(idx), torch.from_numpy(val), off[:-1], pos, rel, ideal, [1])
    # the Python surface checks the order by default
    ranked = RankedLists([f"q{i}" for i in range(9)], [f"d{i}" for i in range(500)], torch.from_numpy(bad_val).cuda(), torch.from_numpy(idx).cuda())
    qrels = {f"q{i}": {f"d{int(p)}": 1 for p in idx[i, :3] if p >= 0} for i in range(9)}
    with pytest.raises(ValueError, match="not sorted"):
        EvaluateRetrieval.evaluate_ranked(qrels, ranked, [1, 10])
    # an empty set of queries is a valid call
    empty = ctx.eval_ranked(torch.zeros((0, 5), dtype=torch.int64), torch.zeros((0, 5)), np.zeros(1, np.int32), pos[:0], rel[:0], ideal[:0], [1, 5])
    assert empty["hits"].shape == (0, 2) and empty["R"].shape == (0,)
