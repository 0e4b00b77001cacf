#!/usr/bin/env python3
"""Evaluation leg of a BEIR run at the driver's depth, host dict path against device path, from the same device lists.

  nq = 1000 queries, K = 1001 entries per list, 1 M corpus ids, ~8 judged documents per query.
  (a) dict path as it stood before sgpt_amd/evaluation.py: run_val.cpu(), run_idx.cpu(), beir.assemble_results, then a
      plain-Python metric loop over the dict (NDCG / MAP / Recall / P at the six cuts);
  (b) EvaluateRetrieval.evaluate_ranked on the device lists (qrels packing, the kernel with its order check, D2H of the sums,
      the host normalisation).
Both in one process, alternating, warm, every window closed by a device synchronise; median and spread of --reps windows.
--profile-only runs (b)'s kernel call a few times and nothing else, for a `rocprofv3 --kernel-trace --stats` run.

    python scripts/eval_bench.py [--reps 20] [--out profiles/eval_device_vs_host.txt]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgpt_amd import get_context                                   # noqa: E402
from sgpt_amd.beir import assemble_results                         # noqa: E402
from sgpt_amd.evaluation import EvaluateRetrieval, RankedLists     # noqa: E402

K_VALUES = [1, 3, 5, 10, 100, 1000]


def python_metrics(qrels, results, k_values):
    """The consumer of the dict on the host: sort, then the sums of the metric definitions, per query."""
    ndcg, _map, recall, prec = ({k: 0.0 for k in k_values} for _ in range(4))
    n = 0
    for qid, res in results.items():
        rel = qrels.get(qid)
        if not rel:
            continue
        R = sum(1 for g in rel.values() if g > 0)
        if R == 0:
            continue
        n += 1
        order = sorted(res.items(), key=lambda kv: -kv[1])
        ideal = sorted((g for g in rel.values() if g > 0), reverse=True)
        hits, dcg, sp, j = 0, 0.0, 0.0, 0

        def record(k, hits, dcg, sp):
            idcg = sum(v / math.log2(r + 2) for r, v in enumerate(ideal[:k]))
            ndcg[k] += dcg / idcg
            _map[k] += sp / R
            recall[k] += hits / R
            prec[k] += hits / k
        for i, (doc, _) in enumerate(order, start=1):
            g = rel.get(doc, 0)
            if g > 0:
                hits += 1
                dcg += g / math.log2(i + 1)
                sp += hits / i
            if j < len(k_values) and i == k_values[j]:
                record(k_values[j], hits, dcg, sp)
                j += 1
        for k in k_values[j:]:                    # cuts deeper than the list
            record(k, hits, dcg, sp)
    return tuple({f"{name}@{k}": round(v / max(n, 1), 5) for k, v in d.items()}
                 for name, d in (("NDCG", ndcg), ("MAP", _map), ("Recall", recall), ("P", prec)))


def make_inputs(nq, K, n_corpus, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ctx = get_context("cuda:0")
    # distinct corpus positions per row: a random start and a stride coprime to the corpus size
    start = torch.randint(0, n_corpus, (nq, 1), generator=g)
    stride = 10 * torch.randint(1, 1000, (nq, 1), generator=g) + 1          # coprime to 10^6
    idx = ((start + stride * torch.arange(K)[None, :]) % n_corpus).to(torch.int64)
    val = torch.sort(torch.rand((nq, K), generator=g), dim=1, descending=True).values
    corpus_ids = [f"doc{i}" for i in range(n_corpus)]
    query_ids = [f"q{i}" for i in range(nq)]
    rng = np.random.default_rng(seed)
    qrels = {}
    for qi, qid in enumerate(query_ids):
        inside = idx[qi, rng.choice(K, size=5, replace=False)].tolist()
        outside = rng.integers(0, n_corpus, size=3).tolist()
        qrels[qid] = {corpus_ids[p]: int(rng.integers(1, 3)) for p in inside + outside}
    return ctx, RankedLists(query_ids, corpus_ids, val.to(ctx.device), idx.to(ctx.device)), qrels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=1001)
    ap.add_argument("--corpus", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    ctx, ranked, qrels = make_inputs(a.nq, a.k, a.corpus)
    sync = lambda: torch.cuda.synchronize(ctx.device)     # noqa: E731

    if a.profile_only:
        from sgpt_amd.evaluation import pack_qrels
        packed = pack_qrels(qrels, ranked.query_ids, ranked.positions())
        for _ in range(10):
            ctx.eval_ranked(ranked.idx, ranked.val, packed.off, packed.pos, packed.rel, packed.ideal, K_VALUES, check_order=True)
        sync()
        return

    def host_path():
        res = assemble_results(ranked.query_ids, ranked.corpus_ids, ranked.val.cpu().numpy(), ranked.idx.cpu().numpy())
        t1 = time.perf_counter()
        out = python_metrics(qrels, res, K_VALUES)
        return out, t1

    def device_path():
        return EvaluateRetrieval.evaluate_ranked(qrels, ranked, K_VALUES)

    want, _ = host_path()
    got = device_path()
    agree = max(abs(x[k] - y[k]) for x, y in zip(want, got) for k in x)
    ta, ta_dict, tb = [], [], []
    for _ in range(a.reps):
        sync()
        t0 = time.perf_counter()
        _, t1 = host_path()
        sync()
        t2 = time.perf_counter()
        device_path()
        sync()
        t3 = time.perf_counter()
        ta.append((t2 - t0) * 1e3)
        ta_dict.append((t1 - t0) * 1e3)
        tb.append((t3 - t2) * 1e3)
    q = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))   # noqa: E731
    lines = [
        f"eval_bench: nq={a.nq} K={a.k} corpus={a.corpus} cuts={K_VALUES} reps={a.reps} ({torch.cuda.get_device_name(0)})",
        "ms per evaluation, median [min .. max]; alternating windows in one process, each closed by a device synchronise",
        "(a) host: D2H of the lists + assemble_results + Python metric loop : %.2f [%.2f .. %.2f]" % q(ta),
        "    of which D2H + assemble_results (the dict)                     : %.2f [%.2f .. %.2f]" % q(ta_dict),
        "(b) device: evaluate_ranked (pack qrels, kernel + order check, sums): %.2f [%.2f .. %.2f]" % q(tb),
        f"NDCG@10 host {want[0]['NDCG@10']} device {got[0]['NDCG@10']}; largest difference over all 24 figures {agree:.1e}",
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
