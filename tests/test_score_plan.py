"""CPU tests of the score + top-k schedule (sgpt_amd/csrc/score_plan.h): the planner is plain C++, so tests/score_plan_dump.cpp is built
with the host compiler and its plans are (1) compared field for field with tests/golden/score_plans.json -- recorded from the
schedule as it stood inside score_topk_impl before it became a function of its own -- and (2) checked over a grid of shapes for the
properties the launches rely on."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "score_plan_dump.cpp")
GOLDEN = os.path.join(HERE, "golden", "score_plans.json")
WS_ORDER = ["sc", "tv0", "tv1", "ti0", "ti1", "sav_v", "sav_i", "qpad", "cand_v", "cand_i", "cand_cnt", "th_v", "th_i", "thr"]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++) to build tests/score_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    return exe


def _plans(exe, args=(), stdin=""):
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, check=True)
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_plans_equal_the_recorded_schedule(dump):
    with open(GOLDEN) as f:
        want = json.load(f)
    lines = "".join(f"{w['nq']} {w['N']} {w['d']} {w['k']} {w['kind']} {w['pred']} {w['n_run']}\n" for w in want)
    got = _plans(dump, stdin=lines)
    assert len(got) == len(want) >= 60
    for g, w in zip(got, want):
        shape = {f: w[f] for f in ("nq", "N", "d", "k", "kind", "pred", "n_run")}
        assert g.keys() == w.keys(), shape
        for field in w:
            assert g[field] == w[field], (shape, field)
    # the benchmark's pass (1000 queries x 1 M x 768, k = 11): the sample at an odd stride, then TWO filtered launches, the second with
    # the shard's tail folded -- the number the schedule's comment quotes
    bench = next(w for w in want if (w["nq"], w["N"], w["d"], w["k"], w["kind"]) == (1000, 1_000_000, 768, 11, "16"))
    assert (bench["S"], bench["s_stride"], bench["top2"]) == (15_360, 65, 1) and [c[1] for c in bench["chunks"]] == [524_288, 475_648]


def _align(v, a):
    return (v + a - 1) // a * a


def _foldable(M, N, K):      # gemm_score_tail_foldable's shape arithmetic (score_plan.h: score_tail_foldable_shape)
    return M >= 256 and M % 256 == 0 and N % 256 == 0 and N >= 512 and K % 64 == 0 and K >= 128 and M < N


def test_plan_properties_over_the_grid(dump):
    """nq x N x d x k x corpus kind x predicated x running list (score_plan_dump.cpp --grid): what the launches and the workspace carve
    rely on.  Each assertion names the contract it comes from."""
    plans = _plans(dump, ["--grid"])
    assert len(plans) > 40_000
    n_filt = n_fold = n_tail = n_bits_fold = 0
    for p in plans:
        nq, N, d, k, kind = p["nq"], p["N"], p["d"], p["k"], p["kind"]
        ctx = (nq, N, d, k, kind, p["pred"], p["n_run"])
        n256, tail = N // 256 * 256, N % 256
        chunks = p["chunks"]
        # the schedule covers [0, N) once, in order: materialised first chunk (k > 64) | filtered chunks | trailing materialise-and-select
        # (the sample of the sampled schedule covers nothing: "the filtered chunks below re-score the sampled documents like any other")
        if not p["filt"]:
            assert chunks == [] and p["first"] == 0 and p["rest"] == N and not p["sampled"], ctx
        else:
            # filt: k <= 1024, no whole-call predicate, whole 256-document chunks, N >= 2 chunk -- so at least one filtered chunk runs
            assert k <= 1024 and not p["pred"] and p["fast"] and p["chunk"] % 256 == 0 and N >= 2 * p["chunk"] and chunks, ctx
            assert (p["first"] == 0) == bool(p["sampled"]) and p["first"] % 256 == 0, ctx
            n_filt += 1
        pos = p["first"]
        for i, (doc0, ln, fold, n_valid, tail_launch) in enumerate(chunks):
            last = i == len(chunks) - 1
            assert doc0 == pos, ctx
            # whole 256-document tiles: score64_kernel / the fp8 byte tile (launch_score64q8) / the 256x256 kernel take N % 256 == 0 (common.h: Score8Args,
            # "64 padded f16 query rows x 256 documents"; gemm.hip: shape256).  A binary corpus folds an exact tail on top (common.h:
            # launch_scorebits, "g.N documents (any number, bounds-checked)"): then n_valid, not len, is the launch's count
            assert ln > 0 and ln % 256 == 0, ctx
            assert ln + 256 < 2 ** 31, ctx                         # GemmArgs.N is an int, a folded launch has N = len + 256
            assert not (fold and tail_launch), ctx
            if fold or tail_launch:
                # "the < 256 trailing documents ride in the last chunk's launch" | "ragged tail (< 256 documents): filtered against the same
                # thresholds by the small-tile kernel" -- either way only behind the last whole tile, and only if there is a tail
                assert last and 0 < tail and doc0 + ln == n256, ctx
            if fold:
                # GemmArgs.n_valid (common.h): "documents [n_valid, N) of the last column tile do not exist" -- honoured by the 256x256
                # kernel alone, hence the one predicate; the Hamming tile counts exactly
                assert kind == "bits" or _foldable(p["nq_pad"], ln + 256, d), ctx
                assert n_valid == ln + tail, ctx
                n_fold += 1
                n_bits_fold += kind == "bits"
            else:
                assert n_valid == 0, ctx
            n_tail += tail_launch
            pos = N if (fold or tail_launch) else doc0 + ln
            if last:
                assert pos == N, ctx                               # (a filtered pass leaves nothing: its last chunk "takes what is left")
        assert pos + p["rest"] == N and (not p["filt"] or p["rest"] == 0), ctx
        # the sample: whole tiles ("S % 256 == 0" is what EPI_SCORE_TOP2 asks, 8 floats per 256-document tile), inside the shard's whole
        # tiles at its stride, and "an ODD stride: ... the structure a sample must not resonate with"
        if p["sampled"]:
            assert k <= 64 and p["S"] > 0 and p["S"] % 256 == 0 and p["S"] * p["s_stride"] <= n256, ctx
            assert p["s_stride"] == 1 or p["s_stride"] % 2 == 1, ctx
        else:
            assert p["S"] == 0 and p["s_stride"] == 1 and not p["top2"], ctx
        assert not p["top2"] or p["nq_pad"] >= 256, ctx            # EPI_SCORE_TOP2: "256x256 kernel only" (common.h)
        assert p["fresh_list"] == (p["sampled"] and p["n_run"] == 0), ctx
        # query rows: the 64-row tile for short batches, else whole 256-row tiles ("the query rows padded to a multiple of 256")
        assert p["nq_pad"] == (64 if p["fast"] and nq <= 64 else _align(nq, 256)), ctx
        assert p["cap"] <= 2048, ctx                               # "the merge sorts the candidates in 2048 LDS slots"
        # one overflow flag per filtered chunk
        assert p["n_flags"] >= 1 and len(chunks) <= p["n_flags"], ctx
        # ws2: 256-aligned regions back to back, nothing overlaps, nothing is left over
        off = 0
        for name in WS_ORDER:
            o, b = p["ws"][name]
            assert o == off and o % 256 == 0 and b % 256 == 0, (ctx, name)
            off += b
        assert off == p["total"], ctx
        ws = {name: p["ws"][name][1] for name in WS_ORDER}
        # the score tile serves the sample (S columns), a fallback piece (fchunk) and a materialised chunk (chunk)
        assert p["fchunk"] >= p["chunk"], ctx
        assert ws["sc"] == _align(nq * max(p["S"], p["fchunk"], p["chunk"]) * 4, 256), ctx
        assert ws["tv0"] == ws["tv1"] == ws["sav_v"] == _align(nq * k * 4, 256) and ws["ti0"] == ws["ti1"] == ws["sav_i"] == _align(nq * k * 8, 256), ctx
        assert ws["qpad"] == (_align(p["nq_pad"] * d * 2, 256) if p["fast"] and kind != "bits" else 0), ctx
        if p["filt"]:
            assert ws["cand_v"] == _align(nq * p["cap"] * 4, 256) and ws["cand_i"] == _align(nq * p["cap"] * 8, 256), ctx
            assert ws["cand_cnt"] == _align((p["nq_pad"] + p["n_flags"]) * 4, 256), ctx      # counters + per-chunk overflow flags
        else:
            assert ws["cand_v"] == ws["cand_i"] == ws["cand_cnt"] == 0, ctx
        assert (ws["th_v"], ws["th_i"], ws["thr"]) == ((ws["tv0"], ws["ti0"], _align(nq * 4, 256)) if p["sampled"] else (0, 0, 0)), ctx
    # the grid reaches every kind of chunk
    assert n_filt > 1000 and n_fold > 100 and n_tail > 100 and n_bits_fold > 100
