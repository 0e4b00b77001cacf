"""-m gpu: csrc/useb_eval.hip (sgpt_eval_groups, sgpt_eval_pairs) and sgpt_amd/useb_eval.py against the float64 restatement
of tests/useb_ref.py, against scikit-learn / scipy, and against the recorded outputs of the reference's evaluators
(tests/golden/useb_metrics.json).

Bounds.  Rank orders and integer outputs (hits1, hits5, first, R, rank2, n_pos, n_used) must be equal.  sp / dcg / idcg within
1e-5 relative: the bound and reasoning of tests/test_gpu_eval.py (a <= 1024-term fp32 sum of non-negative terms in a fixed tree
order is good to ~log2(1024) x 2^-24 = 6e-7).  Scores from embeddings within 1e-5 x max(1, |x||y|) of float64 (fp32 tree sum
over d <= 4096 terms: ~12 x 2^-24 x sum|terms|).  The AP numerator is accumulated in fp64 on the device (include/sgpt_hip.h):
AP within 1e-12 relative of scikit-learn; Spearman from rank2 within 1e-12 of scipy.  End to end: 1e-5 relative per metric."""
import json
import os

import numpy as np
import pytest
import torch

import useb_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-5
SIZES = [0, 1, 2, 20, 63, 64, 65, 1000, 1024]


def f32(num, den):
    return np.asarray(num, np.float32) / np.float32(den)


def close(got, want, tol, tag):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, tag
    assert np.array_equal(got == 0, want == 0), f"{tag}: zero pattern"
    err = float((np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)).max()) if got.size else 0.0
    print(f"{tag}: max relative error {err:.2e} (bound {tol:g})")
    assert err <= tol, f"{tag}: off by {err:.3e} relative"


def csr(groups):
    """groups: dicts with grades, R_extra, ideal (+ scores or rows) -> host CSR arrays."""
    off = np.cumsum([0] + [len(g["grades"]) for g in groups])
    io = np.cumsum([0] + [len(g["ideal"]) for g in groups])
    cat = lambda key, dt: np.concatenate([np.asarray(g[key], dt) for g in groups] + [np.zeros(0, dt)])   # noqa: E731
    return off, cat("grades", np.int32), np.asarray([g["R_extra"] for g in groups], np.int32), io, cat("ideal", np.int32)


def check_groups(out, groups, off, ref_scores, tag):
    """Kernel outputs against useb_ref.group_sums of `ref_scores[g]` (the scores the ranking is defined on)."""
    want = [R.group_sums(s, g["grades"], g["R_extra"], g["ideal"]) for s, g in zip(ref_scores, groups)]
    order = out["order"].cpu().numpy()
    for gi, w in enumerate(want):
        assert order[off[gi]: off[gi + 1]].tolist() == w["order"], f"{tag}: order of group {gi} (size {off[gi + 1] - off[gi]})"
    for name in ("hits1", "hits5", "first", "R"):
        assert out[name].cpu().numpy().tolist() == [w[name] for w in want], f"{tag}: {name}"
    for name in ("sp", "dcg", "idcg"):
        close(out[name].cpu().numpy(), [w[name] for w in want], RTOL, f"{tag} {name}")
    return want


def make_group(rng, n, kind):
    num = rng.integers(-40, 41, size=n)                                 # score = num / 8: exact ties in every larger group
    if kind == "all_equal":
        num[:] = 5
    grades = rng.choice([-1, 0, 1, 2, 3], size=n, p=[0.1, 0.4, 0.3, 0.1, 0.1])
    if kind == "all_relevant":
        grades[:] = 2
    if kind == "none_relevant":
        grades[:] = rng.choice([-1, 0], size=n)
    extra = rng.choice([-1, 0, 1, 3], size=int(rng.integers(0, 4)))     # judged documents that are not candidates
    scores = f32(num, 8)
    if kind == "special" and n >= 6:
        scores[[0, 1, 2, 3, 4]] = [np.nan, -np.inf, -0.0, 0.0, np.inf]
    return {"scores": scores, "grades": grades.astype(np.int32), "R_extra": int((extra > 0).sum()),
            "ideal": np.sort(np.concatenate([grades, extra]))[::-1]}


def test_groups_from_given_scores_every_size_and_kind():
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(11)
    groups = [make_group(rng, n, kind) for n in SIZES for kind in ("plain", "all_equal", "all_relevant", "none_relevant", "special")]
    perm = rng.permutation(len(groups))
    mixed = [groups[i] for i in perm]
    for tag, sel in [("all sizes, mixed", mixed)] + [(f"size {n} alone", [g for g in groups if len(g["grades"]) == n]) for n in SIZES]:
        off, rel, rx, io, ideal = csr(sel)
        scores = np.concatenate([g["scores"] for g in sel] + [np.zeros(0, np.float32)])
        out = ctx.eval_groups(off, rel, scores_in=torch.from_numpy(scores), R_extra=rx, ideal_off=io, ideal_rel=ideal)
        want = check_groups(out, sel, off, [g["scores"] for g in sel], tag)
        assert np.array_equal(out["scores"].cpu().numpy(), scores, equal_nan=True)
        assert sum(w["R"] for w in want) > 0 or tag == "size 0 alone"
    # without IDCG inputs and without R_extra
    off, rel, rx, io, ideal = csr(mixed)
    scores = torch.from_numpy(np.concatenate([g["scores"] for g in mixed]))
    bare = ctx.eval_groups(off, rel, scores_in=scores)
    full = ctx.eval_groups(off, rel, scores_in=scores, R_extra=rx, ideal_off=io, ideal_rel=ideal)
    assert torch.equal(bare["sp"], full["sp"]) and torch.equal(bare["order"], full["order"]) and not bare["idcg"].any()
    assert torch.equal(bare["R"] + torch.from_numpy(rx).cuda(), full["R"])
    # an empty call
    empty = ctx.eval_groups(np.zeros(1, np.int32), np.zeros(0, np.int32), scores_in=torch.zeros(0))
    assert empty["sp"].shape == (0,) and empty["order"].shape == (0,)


def test_groups_of_more_than_1024_candidates_are_refused():
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    with pytest.raises(ValueError, match="1025"):
        ctx.eval_groups(np.array([0, 3, 1028]), np.zeros(1028, np.int32), scores_in=torch.zeros(1028))
    with pytest.raises(ValueError):
        ctx.eval_groups(np.array([0, 3]), np.zeros(3, np.int32), emb=torch.zeros(4, 8), q_row=[0], cand_row=[1, 2, 3], mode="l1")


def spread_rows(rng, n, d, scale=2.0):
    """Query row + n candidate rows of norm `scale` whose cosines to the query are evenly spaced in [-0.9, 0.9]."""
    q = rng.standard_normal(d)
    q *= scale / np.linalg.norm(q)
    cos = rng.permutation(np.linspace(-0.9, 0.9, n))
    u = rng.standard_normal((n, d))
    u -= (u @ q)[:, None] * q[None, :] / (q @ q)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    y = scale * (cos[:, None] * q[None, :] / scale + np.sqrt(1 - cos ** 2)[:, None] * u)
    return np.concatenate([q[None, :], y]).astype(np.float32)


@pytest.mark.parametrize("d", [768, 2048, 4096])
@pytest.mark.parametrize("mode", ["cos", "dot", "neg_l2"])
def test_groups_from_embeddings(mode, d):
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(d + len(mode))
    blocks, groups, q_row, cand_row, ref_scores, base = [], [], [], [], [], 0
    for n_unique in (1, 18, 60, 100, 300):
        rows = spread_rows(rng, n_unique, d)
        s64 = R.pair_scores(rows[0], rows[1:], mode)
        scale = max(1.0, float(np.linalg.norm(rows[0].astype(np.float64)) * np.linalg.norm(rows[1:].astype(np.float64), axis=1).max()))
        # the condition on the INPUTS, checked on the float64 scores before any GPU result is looked at: rounding cannot reorder them
        assert n_unique == 1 or np.diff(np.sort(s64)).min() >= 1e-3 * scale, (mode, d, n_unique)
        dup = rng.integers(0, n_unique, size=max(1, n_unique // 8))      # exact ties: the same row listed twice
        local = rng.permutation(np.concatenate([np.arange(n_unique), dup]))
        grades = rng.choice([-1, 0, 1, 2], size=len(local), p=[0.1, 0.4, 0.3, 0.2]).astype(np.int32)
        groups.append({"grades": grades, "R_extra": int(rng.integers(0, 3)), "ideal": np.sort(np.concatenate([grades, [2, 1]]))[::-1]})
        q_row.append(base)
        cand_row.append(base + 1 + local)
        ref_scores.append(s64[local])
        blocks.append(rows)
        base += len(rows)
    emb = torch.from_numpy(np.concatenate(blocks))
    off, rel, rx, io, ideal = csr(groups)
    assert off[-1] > 64 and np.diff(off).max() <= 1024
    out = ctx.eval_groups(off, rel, emb=emb, q_row=q_row, cand_row=np.concatenate(cand_row), mode=mode, R_extra=rx, ideal_off=io, ideal_rel=ideal)
    got = out["scores"].cpu().numpy().astype(np.float64)
    e64 = emb.numpy().astype(np.float64)
    worst = 0.0
    for gi in range(len(groups)):
        y = e64[cand_row[gi]]
        bound = np.maximum(1.0, np.linalg.norm(e64[q_row[gi]]) * np.linalg.norm(y, axis=1))
        worst = max(worst, float((np.abs(got[off[gi]: off[gi + 1]] - ref_scores[gi]) / bound).max()))
        # the same row listed twice: the same bits
        seg = out["scores"].cpu().numpy()[off[gi]: off[gi + 1]]
        for r in np.unique(cand_row[gi]):
            assert len(set(seg[cand_row[gi] == r].view(np.int32).tolist())) == 1
    print(f"{mode} d={d}: max |score - float64| / max(1, |x||y|) = {worst:.2e} (bound 1e-5)")
    assert worst <= 1e-5
    check_groups(out, groups, off, ref_scores, f"{mode} d={d}")


def pair_case(rng, n, kind):
    gold5 = rng.integers(0, 6, size=n)
    s = rng.standard_normal(n).astype(np.float32) * 0.3 + (gold5 / 5.0).astype(np.float32)
    if kind == "two_decimals":
        s = np.round(s, 2).astype(np.float32)
    if kind == "all_equal":
        s[:] = np.float32(0.25)
    lab = (gold5 > 3).astype(np.int32)
    if kind == "left_out":
        s = np.round(s, 1).astype(np.float32)
        lab[gold5 == 3] = -1
        lab[0] = 1
    if kind == "no_positive":
        lab[:] = 0
    if n > 4 and kind == "continuous":
        s[1], s[2] = np.float32(-0.0), np.float32(0.0)                   # one tie group for scipy and for the kernel
    return s, lab, gold5 * 20


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 100003, 2 ** 20])
def test_pairs_against_scipy_and_sklearn(n):
    from scipy.stats import rankdata, spearmanr
    from sklearn.metrics import average_precision_score
    from sgpt_amd import get_context
    from sgpt_amd.useb_eval import doubled_ranks, pearson
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(n)
    for kind in ("continuous", "two_decimals", "all_equal", "left_out", "no_positive"):
        s, lab, gold = pair_case(rng, n, kind)
        out = ctx.eval_pairs(torch.from_numpy(s), lab)
        rank2 = out["rank2"].cpu().numpy()
        s64 = s.astype(np.float64)
        assert np.array_equal(rank2, np.rint(2 * rankdata(s64)).astype(np.int64)), (n, kind)
        used = lab >= 0
        n_pos, n_used, ap_num = int(out["n_pos"].item()), int(out["n_used"].item()), float(out["ap_num"].item())
        assert (n_pos, n_used) == (int((lab > 0).sum()), int(used.sum())), (n, kind)
        if n_pos == 0:
            assert ap_num == 0.0                                           # AP undefined without a positive: reported as 0
        else:
            want = float(average_precision_score(lab[used], s64[used]))
            assert abs(ap_num / n_pos - want) <= 1e-12 * want, (n, kind, ap_num / n_pos, want)
        if n >= 3 and kind != "all_equal" and len(set(gold.tolist())) > 1:
            rho = pearson(rank2, doubled_ranks(gold))
            assert abs(rho - float(spearmanr(gold, s64).correlation)) <= 1e-12, (n, kind)
        if kind == "two_decimals" and n >= 1000:
            assert n - len(np.unique(s)) > n // 2                          # thousands of ties


def test_pairs_nan_and_empty_input():
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    s = torch.linspace(0, 1, 3000)
    ok = ctx.eval_pairs(s, torch.ones(3000, dtype=torch.int32))
    assert ok["rank2"].cpu().tolist() == list(range(2, 6002, 2))
    s[1234] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ctx.eval_pairs(s, torch.ones(3000, dtype=torch.int32))
    empty = ctx.eval_pairs(torch.zeros(0), torch.zeros(0, dtype=torch.int32))
    assert empty["rank2"].shape == (0,) and int(empty["n_pos"].item()) == 0 and float(empty["ap_num"].item()) == 0.0
    with pytest.raises(ValueError):
        ctx.eval_pairs(torch.zeros(4), torch.zeros(3, dtype=torch.int32))


def test_reference_fixture_through_the_kernels():
    """Every value recorded from the reference's evaluators (tests/golden/useb_metrics.json), reproduced by the kernels."""
    from sgpt_amd import get_context
    from sgpt_amd.evaluation import pack_qrels
    from sgpt_amd.useb_eval import cqadupstack_from_ranked, doubled_ranks, pearson
    ctx = get_context("cuda:0")
    fx = json.load(open(os.path.join(GOLDEN, "useb_metrics.json")))
    groups = fx["groups"]
    off = np.cumsum([0] + [len(g["num"]) for g in groups])
    scores = np.concatenate([f32(g["num"], fx["groups_den"]) for g in groups])
    out = ctx.eval_groups(off, np.concatenate([g["gold"] for g in groups]), scores_in=torch.from_numpy(scores))
    order = out["order"].cpu().numpy()
    for gi, g in enumerate(groups):
        assert order[off[gi]: off[gi + 1]].tolist() == g["order"], gi        # rank_by_score, exact ties included
    h = {k: out[k].cpu().numpy().astype(np.float64) for k in ("sp", "R", "hits1", "hits5", "first")}
    close(h["sp"] / h["R"], [g["map"] for g in groups], RTOL, "fixture ap_score map")
    assert h["hits1"].tolist() == [g["p@1"] for g in groups]
    assert np.allclose(h["hits5"] / 5.0, [g["p@5"] for g in groups], rtol=0, atol=1e-15)
    assert np.allclose(1.0 / h["first"], [g["mrr"] for g in groups], rtol=0, atol=1e-15)
    for p in fx["pairs"]:
        pred = f32(p["num"], p["den"])
        o = ctx.eval_pairs(torch.from_numpy(pred), np.asarray(p["label"], np.int32))
        ap = float(o["ap_num"].item()) / int(o["n_pos"].item())
        assert abs(ap - p["ap"]) <= 1e-12 * p["ap"], p["name"]
        rho = pearson(o["rank2"].cpu().numpy(), doubled_ranks(p["gold"]))
        assert (p["spearman"] is None and np.isnan(rho)) or abs(rho - p["spearman"]) <= 1e-12, p["name"]
    c = fx["cqadupstack"]
    mtrx = torch.from_numpy(f32(c["num"], c["den"]))
    val, idx = ctx.topk(mtrx, 100)
    nq, nd = mtrx.shape
    qids, dids = [f"q{i}" for i in range(nq)], [f"d{i}" for i in range(nd)]
    qrels = {q: {**{dids[j]: 1 for j in cols}, **{f"out{q}-{j}": 1 for j in range(n - len(cols))}}
             for q, cols, n in zip(qids, c["rel_cols"], c["n_rel"])}
    packed = pack_qrels(qrels, qids, {d: i for i, d in enumerate(dids)})
    m_ap, m_ndcg = cqadupstack_from_ranked(idx, val, packed, np.asarray(c["n_rel"]) > 0, ctx)
    close([m_ap, m_ndcg], [c["map@100"], c["ndcg@10"]], RTOL, "fixture cqadupstack")


def test_geometry_independence():
    """The same groups in another order and split over two calls: identical bits."""
    from sgpt_amd import get_context
    ctx = get_context("cuda:0")
    rng = np.random.default_rng(5)
    d = 768
    emb = torch.from_numpy(rng.standard_normal((600, d)).astype(np.float32)).cuda()
    groups = []
    for n in (3, 20, 64, 65, 300, 1, 1024, 20, 0, 90):
        groups.append({"rows": rng.integers(0, 600, size=n), "q": int(rng.integers(0, 600)), "grades": rng.integers(-1, 3, size=n).astype(np.int32),
                       "R_extra": 1, "ideal": np.sort(rng.integers(0, 3, size=n + 2))[::-1]})

    def run(sel, mode):
        off, rel, rx, io, ideal = csr(sel)
        rows = np.concatenate([g["rows"] for g in sel] + [np.zeros(0, np.int64)])
        out = ctx.eval_groups(off, rel, emb=emb, q_row=[g["q"] for g in sel], cand_row=rows, mode=mode, R_extra=rx, ideal_off=io, ideal_rel=ideal)
        res = []
        for gi in range(len(sel)):
            per = {k: out[k][off[gi]: off[gi + 1]].cpu() for k in ("scores", "order")}
            per.update({k: out[k][gi].cpu() for k in ("hits1", "hits5", "first", "R", "sp", "dcg", "idcg")})
            res.append(per)
        return res

    for mode in ("cos", "dot", "neg_l2"):
        base = run(groups, mode)
        perm = rng.permutation(len(groups))
        shuffled = run([groups[i] for i in perm], mode)
        first, second = run(groups[:3], mode), run(groups[3:], mode)           # the first call holds no group above 64
        for gi in range(len(groups)):
            for other in (shuffled[int(np.flatnonzero(perm == gi)[0])], (first + second)[gi]):
                for k, v in base[gi].items():
                    assert torch.equal(v, other[k]), (mode, gi, k)


# ---- end to end on the tiny synthetic model ---------------------------------------------------------------------------------
WORDS = ["alpha", "beta", "gamma", "delta", "query", "doc", "paris", "atom", "cell", "gene", "?", "the", "of", "grub", "boot", "usb"]


def _texts(rng, n, lo, hi, tag):
    return [f"{tag}{i} " + " ".join(rng.choice(WORDS, size=int(rng.integers(lo, hi))).tolist()) for i in range(n)]


@pytest.fixture(scope="module")
def embedder():
    from helpers import build_model, load_case
    from sgpt_amd.tokenization import SyntheticTokenizer
    from sgpt_amd.useb import CustomEmbedder
    fx, cfg_kw, *_ = load_case("tiny_right")
    m = build_model(cfg_kw, int(fx["seed"]), float(fx["std"]), "fp32")
    old = m.ctx.set_low_latency(False)
    yield CustomEmbedder(m, SyntheticTokenizer(cfg_kw["vocab_size"]), method="weightedmean", maxseqlen=40)
    m.ctx.set_low_latency(old)


def _semb(embedder, texts):
    """The reference's route for one batch: semb_fn on the stripped texts, F.normalize (base.py:26-37)."""
    from sgpt_amd.useb import make_semb_fn
    raw = make_semb_fn(embedder)([t.strip() for t in texts])
    return raw, torch.nn.functional.normalize(raw, dim=-1).numpy().astype(np.float64)


def _agree(got, want, tag):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in want:
        print(f"{tag} {k}: device {got[k]:.6f} reference route {want[k]:.6f}")
        assert abs(got[k] - want[k]) <= RTOL * abs(want[k]) and (want[k] != 0 or got[k] == 0), (tag, k, got[k], want[k])


def test_end_to_end_askubuntu(embedder):
    from sgpt_amd.useb_eval import AskUbuntuEvaluator, encode_unique
    rng = np.random.default_rng(31)
    titles = _texts(rng, 70, 2, 9, "t")
    pool = {str(i): (t, f"body {i} " + t) for i, t in enumerate(titles)}
    rows = []
    for q in range(14):
        cands = [str(c) for c in rng.choice(70, size=20, replace=False) if c != q]
        gold = [] if q == 5 else [cands[int(j)] for j in rng.choice(len(cands), size=3, replace=False)] + ["not-retrieved"]
        rows.append((str(q), gold, cands))
    ev = AskUbuntuEvaluator(embedder, pool, {"test": rows})
    got = ev.run("test")
    task = ev.task("test")
    bulk = encode_unique(embedder, task.sentences, normalize=False).cpu()
    groups = []
    for gi, (qid, gold, cands) in enumerate(r for r in rows if r[1]):
        raw, e = _semb(embedder, [pool[qid][0]] + [pool[c][0] for c in cands])
        rows_g = [int(task.q_row[gi])] + task.cand_row[task.grp_off[gi]: task.grp_off[gi + 1]].tolist()
        assert torch.equal(raw, bulk[rows_g]), f"bulk and per-group embeddings of query {qid} differ"       # bit-equal
        groups.append((e[1:] @ e[0], [1 if c in set(gold) else 0 for c in cands]))
    want = {f"{k}_askubuntu_title": v for k, v in R.askubuntu_metrics(groups).items()}
    _agree(got, want, "askubuntu")
    assert 0 < got["map_askubuntu_title"] < 1


def test_end_to_end_scidocs(embedder):
    from sgpt_amd.useb_eval import SciDocsEvaluator
    rng = np.random.default_rng(32)
    titles = _texts(rng, 90, 2, 9, "p")
    corpus = {f"p{i:03d}": {"title": (None if i % 17 == 3 else ("" if i % 17 == 4 else t))} for i, t in enumerate(titles)}
    data = {"corpus": corpus, "test": {}}
    for dname in ("cite", "cocite", "coview", "coread"):
        qrel = {}
        for q in rng.choice(90, size=8, replace=False):
            docs = {f"p{int(j):03d}": int(rng.integers(0, 2)) for j in rng.choice(90, size=30, replace=False) if j != q}
            docs["gone"] = 1
            qrel[f"p{int(q):03d}"] = docs
        qrel["p000"] = {f"p{j:03d}": 0 for j in range(10, 20)}                 # R = 0: left out of the means
        data["test"][dname] = qrel
    ev = SciDocsEvaluator(embedder, data)
    got = ev.run("test")
    want = {}
    for dname, qrel in data["test"].items():
        per = {"euclidean": [], "cosine": []}
        for qid, docs in qrel.items():
            if not corpus[qid]["title"]:
                continue
            dids = sorted((x for x in docs if x in corpus and corpus[x]["title"]), reverse=True)
            _, e = _semb(embedder, [corpus[qid]["title"]] + [corpus[x]["title"] for x in dids])
            grades = [docs[x] for x in dids]
            r_extra = sum(1 for x, g in docs.items() if g > 0 and x not in dids)
            ideal = sorted(docs.values(), reverse=True)
            per["euclidean"].append((R.pair_scores(e[0], e[1:], "neg_l2"), grades, r_extra, ideal))
            per["cosine"].append((R.pair_scores(e[0], e[1:], "cos"), grades, r_extra, ideal))
        for dist, groups in per.items():
            m = R.scidocs_metrics(groups)
            want[f"map_scidocs_{dname}_{dist}"], want[f"ndcg_scidocs_{dname}_{dist}"] = m["map"], m["ndcg"]
    for metric in ("map", "ndcg"):
        for dist in ("euclidean", "cosine"):
            want[f"{metric}_scidocs_{dist}_avg"] = float(np.mean([want[f"{metric}_scidocs_{dn}_{dist}"] for dn in data["test"]]))
    _agree(got, want, "scidocs")
    assert ev.report["cite_cosine"]["no_relevant"] >= 1 and 0 < got["map_scidocs_cosine_avg"] < 1


def test_end_to_end_cqadupstack(embedder):
    from sgpt_amd.useb_eval import CQADupStackEvaluator
    rng = np.random.default_rng(33)
    corpus, split = {}, {"test": {}}
    for forum, n in (("android", 150), ("gis", 60)):
        corpus[forum] = {f"{forum}{i}": t for i, t in enumerate(_texts(rng, n, 2, 10, forum[0]))}
        ids = list(corpus[forum])
        qrels = {}
        for q in rng.choice(n, size=9, replace=False):
            qrels[ids[int(q)]] = [ids[int(j)] for j in rng.choice(n, size=int(rng.integers(0, 5)), replace=False) if j != q]
        split["test"][forum] = qrels
    got = CQADupStackEvaluator(embedder, corpus, split).run("test")
    want = {}
    for forum, qrels in split["test"].items():
        dids = [x for x in corpus[forum] if x not in qrels]
        _, qe = _semb(embedder, [corpus[forum][q] for q in qrels])
        _, de = _semb(embedder, [corpus[forum][x] for x in dids])
        mtrx = qe @ de.T
        top = np.sort(mtrx, axis=1)[:, ::-1][:, :100]
        assert np.abs(np.diff(top, axis=1)).min() > 0                         # no ties inside a list: the documented difference does not arise
        col = {x: i for i, x in enumerate(dids)}
        m, nd = R.cqadupstack_metrics(mtrx, [{col[x] for x in rel if x in col} for rel in qrels.values()], [len(rel) for rel in qrels.values()])
        want[f"map@100_cqadupstack_{forum}"], want[f"ndcg@10_cqadupstack_{forum}"] = m, nd
    want["map@100_cqadupstack_avg"] = float(np.mean([want[f"map@100_cqadupstack_{f}"] for f in corpus]))
    want["ndcg@10_cqadupstack_avg"] = float(np.mean([want[f"ndcg@10_cqadupstack_{f}"] for f in corpus]))
    _agree(got, want, "cqadupstack")


def test_end_to_end_twitterpara(embedder):
    from sgpt_amd.useb_eval import TwitterParaEvaluator
    rng = np.random.default_rng(34)
    datasets = {}
    for dname, n in (("twitterurl", 120), ("pit", 70)):
        s = _texts(rng, 60, 2, 9, dname[0])
        data = []
        for _ in range(n):
            a, b = rng.choice(60, size=2, replace=False)
            label = int(rng.integers(0, 7 if dname == "twitterurl" else 6))
            data.append((s[int(a)], s[int(b)] + " ", None if label == 3 else int(label > 3), label * 20))
        datasets[dname] = data
    got = TwitterParaEvaluator(embedder, datasets).run()
    want = {}
    for dname, data in datasets.items():
        _, e1 = _semb(embedder, [x[0] for x in data])
        _, e2 = _semb(embedder, [x[1] for x in data])
        pred = (e1 * e2).sum(1) / (np.maximum(np.linalg.norm(e1, axis=1), 1e-8) * np.maximum(np.linalg.norm(e2, axis=1), 1e-8))
        want[f"ap_twitter_{dname}"], want[f"spearman_twitter_{dname}"] = R.twitterpara_metrics(pred, [x[2] for x in data], [x[3] for x in data])
    want["ap_twitter_avg"] = float(np.mean([want[f"ap_twitter_{x}"] for x in datasets]))
    want["spearman_twitter_avg"] = float(np.mean([want[f"spearman_twitter_{x}"] for x in datasets]))
    _agree(got, want, "twitterpara")
