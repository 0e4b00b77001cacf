"""CPU test of the cut of a bulk encode call into two chains (sgpt_amd/csrc/encode_split.h: encode_split_point): the function is plain
C++, so tests/encode_split_dump.cpp is built with the host compiler under AddressSanitizer + UBSan and run over random length lists;
every answer is checked against the rule restated here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "encode_split_dump.cpp")
TILE, ALIGN = 256, 8


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++) to build tests/encode_split_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("encode_split") / "encode_split_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    return exe


def _cuts(exe, layouts):
    text = "".join(f"{T} {len(off)} {' '.join(map(str, off))}\n" for T, off in layouts)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    assert len(got) == len(layouts)
    return got


def _want(T, off):
    """The rule: the sequence start nearest T / 2 that is a multiple of 256 rows and lies in [T / 3, 2 T / 3]; the lower of two equally
    near ones; (0, 0) when there is none."""
    B = len(off) - 1
    cands = [(abs(2 * off[b] - T), off[b], b) for b in range(1, B) if off[b] % TILE == 0 and T <= 3 * off[b] <= 2 * T]
    return min(cands)[1:] if cands else (0, 0)


def _layout(rng, B, lo, hi):
    lens = rng.integers(lo, hi + 1, size=B)
    off = np.concatenate([[0], np.cumsum((lens + ALIGN - 1) // ALIGN * ALIGN)])
    return int((off[-1] + TILE - 1) // TILE * TILE), [int(v) for v in off]


def test_cut_follows_the_rule_over_random_length_lists(dump):
    rng = np.random.default_rng(5)
    layouts = []
    for _ in range(400):        # U{16..128}: most packs have an aligned start somewhere, fewer of them in the middle third
        layouts.append(_layout(rng, int(rng.integers(2, 400)), 16, 128))
    for _ in range(100):        # long sequences: few starts, often none that qualifies
        layouts.append(_layout(rng, int(rng.integers(2, 12)), 200, 2048))
    for B in (2, 3, 7, 64, 175, 1024):     # fixed 128-token sequences: every second start is aligned
        layouts.append((B * 128 + (-B * 128) % TILE, [128 * b for b in range(B + 1)]))
    got = _cuts(dump, layouts)
    n_cut = n_none = 0
    for (T, off), (row, seq) in zip(layouts, got):
        assert (row, seq) == _want(T, off), (T, off[:8], row, seq)
        if row:
            n_cut += 1
            B = len(off) - 1
            assert off[seq] == row and row % TILE == 0            # on a sequence start, on a row tile
            assert 0 < seq < B and 0 < row < T                    # both chains hold sequences and rows
            assert T <= 3 * row <= 2 * T
        else:
            n_none += 1
    assert n_cut > 100 and n_none > 100        # the lists exercise both answers


def test_layouts_that_must_not_be_cut(dump):
    cases = [
        (256, [0, 128]),                                   # one sequence
        (1024, [0, 504, 1016]),                            # no aligned start at all
        (3072, [0, 256, 512, 768, 2560, 3072]),            # aligned starts only outside the middle third (768 < 1024, 2560 > 2048)
        (2560, [0, 256, 2304, 2560]),                      # ... on both sides
        (1024, [0, 512, 512, 1024]),                       # not ascending
        (1024, [0, 512, 1536]),                            # runs past T
        (1024, [8, 512, 1024]),                            # does not start at row 0
    ]
    assert _cuts(dump, cases) == [(0, 0)] * len(cases)


def test_edges_of_the_middle_third_and_ties(dump):
    cases = [
        (768, [0, 256, 512, 768]),         # both ends of [T / 3, 2 T / 3] are starts, equally near: the lower
        (1024, [0, 512, 1024]),            # exactly T / 2, two sequences
        (1536, [0, 512, 1024, 1536]),      # T / 3 and 2 T / 3 exactly
        (1280, [0, 256, 768, 1280]),       # 768 (dist 256) qualifies, 256 < T / 3 does not
    ]
    assert _cuts(dump, cases) == [(256, 1), (512, 1), (512, 1), (768, 2)]
