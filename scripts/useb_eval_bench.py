#!/usr/bin/env python3
"""AskUbuntu-shaped USEB evaluation, the per-query `semb_fn` route against the device evaluator, same model, same task.

  400 queries x 20 candidates over a pool of 5 000 sentences (8 .. 24 tokens), SGPT-125M shape, synthetic weights, f16.
  (a) the route the reference's evaluator takes through `make_semb_fn`: per query one 21-sentence embedder call, `.cpu()`,
      F.normalize, host matmul, Python sort and ap_score / reciprocal_rank arithmetic (askubuntu.py:131-157);
  (b) sgpt_amd.useb_eval.AskUbuntuEvaluator.run: every unique sentence encoded once, one sgpt_eval_groups call, host means.
Both in one process, alternating, warm, every window closed by a device synchronise; median and spread of --reps windows.
The four metrics of the two routes must agree to 1e-5 relative (asserted before anything is timed).

    python scripts/useb_eval_bench.py [--reps 7] [--out profiles/useb_eval_device_vs_host.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgpt_amd import SGPTConfig, SGPTModel, synthetic_weights                  # noqa: E402
from sgpt_amd.tokenization import SyntheticTokenizer                           # noqa: E402
from sgpt_amd.useb import CustomEmbedder, make_semb_fn                         # noqa: E402
from sgpt_amd.useb_eval import AskUbuntuEvaluator                              # noqa: E402


def make_task(n_pool, n_queries, n_cand, seed=0):
    rng = np.random.default_rng(seed)
    vocab = [f"w{i}" for i in range(3000)]
    pool = {str(i): (f"s{i} " + " ".join(rng.choice(vocab, size=int(rng.integers(7, 24))).tolist()), "") for i in range(n_pool)}
    rows = []
    for q in rng.choice(n_pool, size=n_queries, replace=False):
        cands = [str(c) for c in rng.choice(n_pool, size=n_cand + 1, replace=False) if c != q][:n_cand]
        gold = [cands[int(j)] for j in rng.choice(n_cand, size=int(rng.integers(1, 5)), replace=False)]
        rows.append((str(int(q)), gold, cands))
    return pool, rows


def per_query_route(semb_fn, pool, rows):
    acc = {"map": [], "p@1": [], "p@5": [], "mrr": []}
    for qid, gold, cands in rows:
        embs = torch.nn.functional.normalize(semb_fn([pool[qid][0]] + [pool[c][0] for c in cands]), dim=-1)
        scores = torch.matmul(embs[0:1], embs[1:].t()).squeeze(0).tolist()
        ranked = [c for c, _ in sorted(zip(cands, scores), key=lambda kv: kv[1], reverse=True)]
        rel = set(gold)
        hits, precisions, first = 0, [], 0
        for i, c in enumerate(ranked, start=1):
            if c in rel:
                hits += 1
                precisions.append(hits / i)
                first = first or i
            if i == 1:
                p1 = hits / 1
            if i == 5:
                p5 = hits / 5
        acc["map"].append(float(np.mean(precisions)))
        acc["p@1"].append(p1)
        acc["p@5"].append(p5)
        acc["mrr"].append(1.0 / first)
    return {f"{k}_askubuntu_title": float(np.mean(v)) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=5000)
    ap.add_argument("--queries", type=int, default=400)
    ap.add_argument("--cands", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = SGPTConfig(vocab_size=50257, max_position_embeddings=2048, hidden_size=768, num_layers=12, num_heads=12, window_size=256)
    model = SGPTModel(cfg, synthetic_weights(cfg, seed=0), device="cuda:0", dtype="f16", precision="plain")
    model.ctx.set_low_latency(False)                                  # every batch size gives a sentence the same bits
    emb = CustomEmbedder(model, SyntheticTokenizer(cfg.vocab_size), method="weightedmean", maxseqlen=128)
    semb_fn = make_semb_fn(emb)
    pool, rows = make_task(a.pool, a.queries, a.cands)
    ev = AskUbuntuEvaluator(emb, pool, {"test": rows})
    sync = lambda: torch.cuda.synchronize(model.device)               # noqa: E731

    want, got = per_query_route(semb_fn, pool, rows), ev.run("test")
    worst = max(abs(got[k] - want[k]) / abs(want[k]) for k in want)
    assert set(got) == set(want) and worst <= 1e-5, (got, want)
    ta, tb = [], []
    for _ in range(a.reps):
        sync()
        t0 = time.perf_counter()
        per_query_route(semb_fn, pool, rows)
        sync()
        t1 = time.perf_counter()
        ev.run("test")
        sync()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    n_unique = len(ev.task("test").sentences)
    q = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))   # noqa: E731
    lines = [
        f"useb_eval_bench: {a.queries} queries x {a.cands} candidates, pool {a.pool} ({n_unique} unique sentences in the task), "
        f"SGPT-125M shape f16, synthetic weights, reps={a.reps} ({torch.cuda.get_device_name(0)})",
        "ms per evaluation (tokenisation included on both sides), median [min .. max]; alternating windows in one process, each closed "
        "by a device synchronise",
        "(a) per query: semb_fn on 21 sentences, .cpu(), host matmul, Python sort + metric : %.1f [%.1f .. %.1f]" % q(ta),
        "(b) AskUbuntuEvaluator.run: unique sentences once, one sgpt_eval_groups call      : %.1f [%.1f .. %.1f]" % q(tb),
        "metrics (a) " + " ".join(f"{k.split('_')[0]}={v:.6f}" for k, v in want.items()),
        "metrics (b) " + " ".join(f"{k.split('_')[0]}={v:.6f}" for k, v in got.items()) + f"; largest relative difference {worst:.1e}",
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
