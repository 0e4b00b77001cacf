"""No GPU: tests/lmhead_ref.py -- the reference, the case table and the bound of tests/test_gpu_lmhead.py -- and the proof that
the table can fail: a numpy emulation of the chunk loop of sgpt_lm_logprobs (fp32 logits by gemm_ref.fp32_chain) stays inside
the bound as it is, and leaves it by more than 4x, produces NaN or writes a guard entry with each of seven defects."""
import re
from pathlib import Path

import numpy as np
import pytest

import gemm_ref as G
import lmhead_ref as L
import rowops_ref as R

ROOT = Path(__file__).resolve().parent.parent
SMALL = [c for c in L.CASES if c.V < 1000]
EMULATED = ("chunks-n5", "chunks-n1024", "chunks-n1025", "bias-n1025")     # the clean emulation; the defects run on the last two


def test_layout_mirrors_the_three_lines_of_the_entry():
    """R, rows_bytes, ldv (and lg_bytes) are read out of csrc/encode.hip as text and evaluated on the table's shapes: a change of
    the layout shows up here before test_stale_pad_columns stops meaning anything."""
    src = (ROOT / "sgpt_amd" / "csrc" / "encode.hip").read_text()
    body = src[src.index("sgpt_status sgpt_lm_logprobs("):]
    assert re.search(r"const long ldv = \(V \+ 3\) / 4 \* 4;", body)
    assert re.search(r"const int R = n < 1024 \? n : 1024;", body)
    assert re.search(r"rows_bytes = align_up\(\(size_t\)R \* dm \* 4, 256\), lg_bytes = align_up\(\(size_t\)R \* ldv \* 4, 256\);", body)
    assert re.search(r"float\* rows = \(float\*\)c->ws2;\s*float\* logits = \(float\*\)\(\(char\*\)c->ws2 \+ rows_bytes\);", body)
    assert L.layout(5, 128, 211) == (5, 2560, 212, 4352)
    assert L.layout(2049, 384, 257) == (1024, 1024 * 384 * 4, 260, 1024 * 260 * 4)
    assert L.layout(1025, 128, 50257) == (1024, 524288, 50260, 1024 * 50260 * 4)
    # the stale-pad test: vocab 260 and vocab 257 share d and ldv, so every logits element has one address in both calls
    assert L.layout(1025, 128, 260) == L.layout(1025, 128, 257) and L.layout(1025, 128, 257).ldv - 257 == 3
    assert L.chunks(3109) == [(0, 1024), (1024, 1024), (2048, 1024), (3072, 37)]
    assert L.chunks(1024) == [(0, 1024)] and L.chunks(1025) == [(0, 1024), (1024, 1)] and L.chunks(5) == [(0, 5)]


def test_case_table_and_the_kernel_of_every_chunk():
    """Every n of the issue at V = 211, the bias cases, and which (kernel, order) each chunk launches by the mirror of the launch
    rule.  V_SUPER is the SMALLEST V % 4 != 0 whose full chunk takes the 128x128 tile; the one-row tail there is 149 64x64 tiles
    in run order, and the tail on 64x64 tiles in supertile order with MT == 1 is the real vocabulary's."""
    assert sorted(c.n for c in L.CASES if c.name.startswith("chunks-")) == sorted(L.NS)
    assert [len(L.chunks(n)) for n in L.NS] == [1, 1, 1, 1, 2, 2, 3, 4]
    for c in L.CASES:
        assert tuple(L.chunk_variants(c.n, c.V, c.d)) == c.variants, c.name
        assert c.d % 128 == 0 and L.layout(c.n, c.d, c.V).ldv % 4 == 0
        assert c.patterns == (L.PATTERNS if c.V == 211 and c.n in (1025, 2049) else L.PATTERNS[:1])
    for V in range(L.V_SUPER - 200, L.V_SUPER):
        assert V % 4 == 0 or G.linear_variant("fp32", 0, False, 1024, V, 64)[0] != "rs128", V
    assert L.V_SUPER % 4 != 0 and G.linear_variant("fp32", 0, False, 1024, L.V_SUPER, 64) == ("rs128", "supertile")
    assert L.case("real-n1025").variants[1] == ("rs64", "supertile") and (1 + 63) // 64 == 1          # MT == 1
    assert L.case("bias-n2049").head == "bias" and L.layout(1, 384, 257).ldv == 260


@pytest.mark.parametrize("pattern", L.PATTERNS)
def test_row_patterns_leave_nan_in_every_row_they_do_not_select(pattern):
    for n in (1025, 2049):
        ref = L.reference(f"chunks-n{n}", "gauss", pattern)
        sel = np.zeros(ref.T_pad, bool)
        sel[ref.row_idx] = True
        assert ref.T_pad % 32 == 0 and ref.row_idx.min() >= 0 and ref.row_idx.max() < ref.T_pad and len(ref.row_idx) == n
        assert np.isnan(ref.hidden[~sel]).all() and np.isfinite(ref.hidden[sel]).all()
        if pattern != "random-small":
            assert (~sel).any()
        if pattern == "spans":
            assert (np.diff(ref.row_idx) > 0).all() and (np.diff(ref.row_idx) > 1).sum() > n // 14
        if pattern == "reversed":
            assert (np.diff(ref.row_idx) < 0).all()
        if pattern == "random-small":
            assert ref.T_pad < n and len(np.unique(ref.row_idx)) < n
        if pattern == "random-large":
            assert ref.T_pad > n and len(np.unique(ref.row_idx)) < n
        if pattern == "repeat":
            assert len(np.unique(ref.row_idx)) == 1


def test_reference_is_the_plain_formula_and_targets_hit_the_edges():
    """row_stats works in row blocks and never holds the logits: here against the one-line formula, and against the oracle's
    fp32 log_softmax."""
    from oracle import sgpt_oracle as O
    for name in ("chunks-n1025", "bias-n1025"):
        ref = L.reference(name, "gauss", "spans")
        x = ref.hidden[ref.row_idx].astype(np.float64) @ ref.W.astype(np.float64).T
        if ref.bias is not None:
            x = x + ref.bias.astype(np.float64)
        lp, am = R.logprob_rows(x, ref.case.V, ref.targets)
        assert np.abs(lp - ref.lp).max() < 1e-12 and np.array_equal(am, ref.am)
        top2 = np.sort(x, axis=1)[:, -2:]
        assert np.abs((top2[:, 1] - top2[:, 0]) - ref.gap).max() < 1e-12
        assert np.abs(O.log_softmax(x)[np.arange(len(lp)), ref.targets] - lp).max() < 1e-4
        assert 2.0 < x.std() < 4.0, "logits have a standard deviation near 3"
        tg = ref.targets
        assert (tg == 0).sum() >= len(tg) // 8 and (tg == ref.case.V - 1).sum() >= len(tg) // 8 and (tg == ref.am).sum() >= len(tg) // 8
        E = G.bound(ref.hidden[ref.row_idx], ref.W, ref.bias, None, ref.case.d).max(axis=1)
        assert np.array_equal(E, ref.E)
        assert np.array_equal(ref.bound, 2 * ref.E + L.logprob_bound(ref.case.V, L.logit_at(ref.hidden, ref.row_idx, ref.W, ref.bias, tg) - x.max(axis=1)))


@pytest.mark.parametrize("c", L.CASES, ids=lambda c: c.name)
def test_greedy_condition_of_the_gaussian_inputs(c):
    """A condition on the inputs alone: at most 1 % of a run's rows have a float64 top-two gap within 2 max_j E."""
    for kind, pattern in L.runs(c):
        if kind == "gauss" and pattern != "repeat":
            ref = L.reference(c.name, kind, pattern)
            assert np.isfinite(ref.lp).all() and (ref.bound > 0).all()
            assert L.greedy_left_out(ref).mean() <= L.GREEDY_LEFT_OUT_MAX, (c.name, pattern)
    if "repeat" in c.patterns:                             # one row n times: none or all of the rows, so the seed must give none
        assert not L.greedy_left_out(L.reference(c.name, "gauss", "repeat")).any()


@pytest.mark.parametrize("c", [c for c in L.CASES if "exact" in c.operands], ids=lambda c: c.name)
def test_exact_operands_are_exact(c):
    """Multiples of 2^-3 in [-1, 1]: every logit is a multiple of 2^-6 below 2^9 + 1 -- float32 and float64 agree, whatever the
    order of the sum (here: k ascending and descending in groups of 4, on the small vocabularies).  The duplicated LM-head
    rows are the strict maximum of the rows built for them, and the float64 argmax (first maximum) is the lower one."""
    ref = L.reference(c.name, "exact", c.patterns[0])
    x32 = L.exact_logits(ref)                              # asserts float32(float64 logits) == float64 logits
    assert np.isnan(x32[:, c.V:]).all() and x32.shape[1] == L.layout(c.n, c.d, c.V).ldv
    x = x32[:, :c.V].astype(np.float64)
    assert np.array_equal(x * 64, np.round(x * 64)) and np.abs(x).max() <= c.d + 1
    if c.V < 1000 and c.n <= 1025:
        a = ref.hidden[ref.row_idx]
        for rev in (False, True):
            y = G.fp32_chain(a, ref.W, 4, reverse=rev)
            y = y if ref.bias is None else y + ref.bias[None, :]
            assert np.array_equal(y, x32[:, :c.V])
    j1, j2 = L.DUP[c.V]
    assert j1 < j2 and np.array_equal(ref.W[j1], ref.W[j2]) and (c.V == 257) == (j1 // 64 == j2 // 64)
    hit = np.flatnonzero(x[:, j1] == c.d + (ref.bias is not None))
    assert len(hit) >= max(1, len(np.unique(ref.row_idx)) // L.DUP_EVERY) and (ref.am[hit] == j1).all()
    rest = np.delete(x[hit], [j1, j2], axis=1)
    assert (rest.max(axis=1) < x[hit, j1]).all() and np.array_equal(x[hit, j1], x[hit, j2])


@pytest.mark.parametrize("name", EMULATED)
def test_emulation_without_a_defect_stays_inside_the_bound(name):
    ref = L.reference(name, "gauss", "spans")
    lp, greedy = L.emulate(ref.hidden, ref.row_idx, ref.W, ref.bias, ref.targets)
    r = L.worst_ratio(lp, ref)
    print(f"lmhead: emulation {name}: worst error / bound = {r:.3f}")
    assert r <= 1.0 and not L.defect_seen(lp, ref)
    assert (lp[ref.case.n:] == L.SENTINEL).all() and (greedy[ref.case.n:] == -7).all()
    keep = ~L.greedy_left_out(ref)
    assert np.array_equal(greedy[:ref.case.n][keep], ref.am[keep])


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_every_defect_is_seen(defect):
    """One defect at a time in the emulated chunk loop: NaN, or a row more than 4x outside its bound, or a written guard entry,
    in at least one of the two cases (the margin of the project's GEMM reference tests)."""
    seen = {}
    for name in ("chunks-n1025", "bias-n1025"):
        ref = L.reference(name, "gauss", "spans")
        lp, _ = L.emulate(ref.hidden, ref.row_idx, ref.W, ref.bias, ref.targets, defect)
        seen[name] = L.defect_seen(lp, ref)
    print(f"lmhead: defect '{defect}': {seen}")
    assert any(seen.values())
    if defect != "bias dropped":
        assert all(seen.values())                          # (a tied head has no bias to drop)
