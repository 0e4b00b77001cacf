"""CPU tests of the score + top-k schedule for the uint8 corpus (sgpt_amd/csrc/score_plan.h, SCORE_CORPUS_U8): it plans like the fp8
corpus -- the 64-row tile, the sampled / filtered schedule -- with the any-N launches and the tail folding of the binary corpus.
tests/score_plan_u8_dump.cpp is built with the host compiler, as tests/test_score_plan.py builds its own."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "score_plan_u8_dump.cpp")
WS_ORDER = ["sc", "tv0", "tv1", "ti0", "ti1", "sav_v", "sav_i", "qpad", "cand_v", "cand_i", "cand_cnt", "th_v", "th_i", "thr", "qscale", "qbias"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++) to build tests/score_plan_u8_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("score_plan_u8") / "score_plan_u8_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    return [json.loads(line) for line in r.stdout.splitlines()]


def _align(v, a):
    return (v + a - 1) // a * a


def test_u8_plans_over_the_grid(plans):
    """nq {1, 16, 64} x N {1, 255, 256, 257, 1000, 262 221, 1 000 000} x d {128, 768} x k {1, 11, 100, 1001} x running list."""
    u8 = [p for p in plans if p["u8"]]
    assert len(u8) == 3 * 7 * 2 * 4 * 2
    n_filt = n_sampled = n_fold = n_doubling = 0
    for p in u8:
        nq, N, d, k = p["nq"], p["N"], p["d"], p["k"]
        ctx = (nq, N, d, k, p["n_run"])
        # planned like fp8: the 64-row tile of padded query rows; like bits: every launch takes any number of documents
        assert p["fast"] and p["nq_pad"] == 64 and p["pad_queries"] and p["any_n"] and not p["top2"], ctx
        pos = p["first"]
        if not p["filt"]:
            assert p["chunks"] == [] and p["first"] == 0 and p["rest"] == N, ctx
        else:
            assert k <= 1024 and N >= 2 * p["chunk"] and p["chunks"], ctx
            n_filt += 1
            n_sampled += p["sampled"]
            n_doubling += not p["sampled"]
        spans = [(0, p["first"])] if p["first"] else []
        for i, (doc0, ln, fold, n_valid, tail_launch) in enumerate(p["chunks"]):
            last = i == len(p["chunks"]) - 1
            assert doc0 == pos and ln > 0 and ln % 256 == 0, ctx
            assert not tail_launch, ctx                       # no launch of its own for a ragged tail
            if fold:
                # the launch counts the documents that exist: len whole-tile documents + the < 256 behind them
                assert last and N % 256 and n_valid == ln + N % 256 and doc0 + n_valid == N, ctx
                n_fold += 1
            else:
                assert n_valid == 0, ctx
            count = n_valid if fold else ln
            assert count < 2 ** 31, ctx                       # GemmArgs.N is an int
            spans.append((doc0, doc0 + count))
            pos = doc0 + count
        if p["rest"]:
            spans.append((N - p["rest"], N))
        # every document is visited exactly once across first / chunks / rest
        assert spans[0][0] == 0 and spans[-1][1] == N and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (ctx, spans)
        assert not p["filt"] or p["rest"] == 0, ctx
        # the sample's rows are in range, at an odd stride
        if p["sampled"]:
            assert k <= 64 and p["S"] >= 256 and (p["S"] - 1) * p["s_stride"] < N, ctx
            assert p["s_stride"] == 1 or p["s_stride"] % 2 == 1, ctx
        else:
            assert p["S"] == 0, ctx
        assert p["fresh_list"] == (p["sampled"] and p["n_run"] == 0), ctx
        assert p["cap"] <= 2048 and len(p["chunks"]) <= p["n_flags"], ctx
        # ws2: 256-aligned regions back to back, nothing overlaps, nothing is left over
        off = 0
        for name in WS_ORDER:
            o, b = p["ws"][name]
            assert o == off and o % 256 == 0 and b % 256 == 0, (ctx, name)
            off += b
        assert off == p["total"], ctx
        ws = {name: p["ws"][name][1] for name in WS_ORDER}
        assert ws["qpad"] == 64 * d * 2 and ws["qscale"] == ws["qbias"] == 256, ctx       # the tile of pre-scaled f16 rows, 64 floats each
        assert ws["sc"] == _align(nq * max(p["S"], p["fchunk"], p["chunk"]) * 4, 256), ctx
    # the grid reaches the sampled schedule (k <= 64), the doubling one (64 < k <= 1024), and folded tails in both
    assert n_filt == n_sampled + n_doubling and n_sampled >= 24 and n_doubling >= 12 and n_fold >= 12


def test_the_schedule_at_the_sizes_the_gpu_tests_use(plans):
    """N = 262 144 + 77 is the smallest shard the planner filters at nq = 16 (chunk 131 072): the tail rides in the last filtered launch."""
    p = next(p for p in plans if p["u8"] and (p["nq"], p["N"], p["d"], p["k"], p["n_run"]) == (16, 262221, 128, 11, 0))
    assert p["filt"] and p["sampled"] and p["chunks"][-1][2] == 1 and p["chunks"][-1][0] + p["chunks"][-1][3] == 262221
    p = next(p for p in plans if p["u8"] and (p["nq"], p["N"], p["d"], p["k"], p["n_run"]) == (16, 1000, 128, 11, 0))
    assert not p["filt"] and p["rest"] == 1000


def test_other_kinds_carry_no_u8_regions(plans):
    """The two new regions have 0 bytes for every other corpus kind and sit behind the old ones: their layouts and totals stand."""
    others = [p for p in plans if not p["u8"]]
    assert len(others) > 500
    for p in others:
        assert p["ws"]["qscale"][1] == 0 and p["ws"]["qbias"][1] == 0, p
        assert p["ws"]["qscale"][0] == p["ws"]["qbias"][0] == p["total"] == p["ws"]["thr"][0] + p["ws"]["thr"][1], p
