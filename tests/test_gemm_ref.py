"""CPU: the infrastructure of tests/test_gpu_linear_edges.py (tests/gemm_ref.py) on its own -- the float64 reference against a
triple loop, torch.float64 and torch's / HF's GELU formulas; the launch mirror against the shape table (every branch of the
register-staged kernel reached, every case showing the edge it is listed for); the derived bound against an fp32 chain in numpy
(room below it) and against a dropped 16-byte k-chunk (no room to hide one)."""
import math

import numpy as np
import pytest
import torch

import gemm_ref as G

DTYPES = ["bf16", "f16", "fp32"]
SMALL = [c for c in G.CASES if c.kernel == "rs64-deep"]          # the cases an fp32 chain in numpy can walk


def _epis(c, dtype):
    """(epi, out16) combinations sgpt_linear accepts for the case."""
    out = [(0, False)] + ([(0, True)] if dtype != "fp32" else [])
    if c.N % 4 == 0:
        out += [(1, dtype != "fp32"), (9, dtype != "fp32"), (2, False)]
        if c.M % 128 == 0 and dtype != "fp32":
            out.append((4, True))
    return out


# ---------------------------------------------------------------- the launch mirror and the shape table --------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_cases_reach_every_branch_of_the_register_staged_kernel(dtype):
    reached = {}
    for c in G.CASES:
        K = G.case_k(c, dtype)
        for epi, out16 in _epis(c, dtype):
            for policy in (0, 1):
                got = G.linear_variant(dtype, epi, out16, c.M, c.N, K, tile_policy=policy, low_latency=c.ll)
                assert got == (c.kernel, c.order), f"{c.name} {dtype} epi {epi} policy {policy}: {got}, listed as {(c.kernel, c.order)}"
            reached.setdefault(got, set()).add(c.name)
        if c.ll:        # mode off: one group
            assert G.linear_variant(dtype, 0, False, c.M, c.N, K, low_latency=False) == ("rs64-deep", "run")
    for k in sorted(reached):
        print(f"{dtype} {k[0]:>9} / {k[1]:<9}: {' '.join(sorted(reached[k]))}")
    assert set(reached) == {("rs64-deep", "run"), ("rs64", "supertile"), ("rs128", "run"), ("rs128", "supertile"), ("rs64-kg2", "run")}
    # the blocks of the large cases as problems of their own: the other tile size, the other k-step
    for name in G.BLOCK_CASES:
        K = G.case_k(G.case(name), dtype)
        for epi in (0, 1, 2, 9):
            assert G.linear_variant(dtype, epi, False, G.BLOCK_M, G.BLOCK_N, K) == ("rs64-deep", "run")
        assert G.kstep_of("rs64-deep", dtype) == 2 * G.kstep_of(G.case(name).kernel, dtype)


def test_mirror_on_the_shapes_of_test_gpu_linear():
    """The classification the shape list of tests/test_gpu_linear.py gets (aligned shapes: 256d or the 64x64 tile, never 128x128)."""
    assert G.linear_variant("bf16", 0, True, 4096, 2304, 128)[0] == "256d"               # 144 tiles > 128
    assert G.linear_variant("bf16", 1, True, 4096, 2304, 128) == ("rs64", "supertile")    # gelu: few; t128 = 576 < 600
    assert G.linear_variant("f16", 2, False, 16384, 1536, 768)[0] == "256d"
    assert G.linear_variant("f16", 0, True, 2048, 768, 3072) == ("rs64-deep", "run")      # t128 = 96
    assert G.linear_variant("f16", 0, True, 1024, 768, 768, tile_policy=1)[0] == "256d"
    assert G.linear_variant("f16", 2, False, 512, 768, 3072, low_latency=True) == ("rs64-kg2", "run")
    assert G.linear_variant("f16", 2, False, 1024, 768, 2112, low_latency=True) == ("rs64-deep", "run")   # 17 steps
    assert G.linear_variant("fp32", 9, False, 32, 512, 128) == ("rs64-deep", "run")
    assert G.linear_variant("fp32", 0, False, 4096, 4096, 256) == ("rs128", "supertile")  # fp32 never takes 256d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_each_case_shows_the_edge_it_is_listed_for(c, dtype):
    K = G.case_k(c, dtype)
    kernel, order = G.linear_variant(dtype, 0, False, c.M, c.N, K, low_latency=c.ll)
    assert kernel != "256d"
    B, BK = G.tile_of(kernel), G.kstep_of(kernel, dtype)
    assert BK in ((32, 64) if dtype == "fp32" else (64, 128))
    MT, NT = -(-c.M // B), -(-c.N // B)
    assert K % (4 if dtype == "fp32" else 8) == 0
    assert ("M" in c.edges) == (c.M % B != 0)
    assert ("N" in c.edges) == (c.N % B != 0)
    if "N" in c.edges and c.N % 4 == 0:
        assert c.N % B in (4, 60)                      # a last column tile one vector wide, or one vector short of full
    assert ("K" in c.edges) == (K % BK != 0)
    if "order" in c.edges:
        assert order == "supertile" and (MT % 8 != 0 or NT % 8 != 0 or MT == 1)
    assert (order == "supertile") == (MT * NT > 512)
    if kernel == "rs64-kg2":                           # group 1's last step is the partial one
        nk = -(-K // BK)
        assert nk % 2 == 0 and K % BK != 0 and K > (nk - 1) * BK > (nk // 2) * BK


def test_first_rows_take_every_value_and_every_corner():
    first = [c for c in G.CASES if c.name.startswith("k1-")]
    second = [c for c in G.CASES if c.name.startswith("kt-")]
    assert {c.M for c in first} == {1, 63, 65, 130} and {c.N for c in first} == {4, 60, 68, 132}
    assert {(c.M > 64, c.N > 64) for c in first} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.M, c.N) for c in second} == {(65, 68), (65, 132), (130, 68), (130, 132)}
    assert {c.K16 for c in second} == {136, 200} and {c.K32 for c in second} == {68, 100, 132}
    assert G.CASES[-1].tag == "last" and G.CASES[-1].N % 2 == 1


# ---------------------------------------------------------------- linear_ref -------------------------------------------------

def test_linear_ref_against_a_triple_loop():
    rng = np.random.default_rng(1)
    M, N, K = 3, 5, 4
    a, w = rng.standard_normal((M, K)), rng.standard_normal((N, K))
    bias, resid = rng.standard_normal(N), rng.standard_normal((M, N))
    u = np.zeros((M, N))
    for m in range(M):
        for n in range(N):
            for k in range(K):
                u[m, n] += a[m, k] * w[n, k]
            u[m, n] += bias[n]
    assert np.abs(G.linear_ref(a, w, bias, None, 0) - u).max() < 1e-14
    assert np.abs(G.linear_ref(a, w, None, None, 0) - (u - bias)).max() < 1e-14
    assert np.abs(G.linear_ref(a, w, bias, resid, 2) - (u + resid)).max() < 1e-14
    assert G.linear_ref(a, w, bias, None, 4).shape == (N, M) and np.abs(G.linear_ref(a, w, bias, None, 4) - u.T).max() < 1e-14
    for m in range(M):
        for n in range(N):
            x = u[m, n]
            assert abs(G.linear_ref(a, w, bias, None, 9)[m, n] - 0.5 * x * (1 + math.erf(x / math.sqrt(2)))) < 1e-14
            t = math.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3))
            assert abs(G.linear_ref(a, w, bias, None, 1)[m, n] - 0.5 * x * (1 + t)) < 1e-14
    assert np.array_equal(G.split_ref(a, w, bias, 1), G.linear_ref(a, w, bias, None, 1))
    with pytest.raises(ValueError):
        G.split_ref(a, w, bias, 2)


@pytest.mark.parametrize("c", [c for c in G.CASES if c.M * c.N * c.K16 <= 2e8], ids=lambda c: c.name)
def test_linear_ref_against_torch_float64(c):
    x = G.make_inputs(c, "f16")
    a, w, b, r = (torch.from_numpy(x[k]) for k in ("a64", "w64", "bias64", "resid64"))
    u = a @ w.T + b
    scale = float(u.abs().max()) + 1.0
    assert np.abs(G.linear_ref(x["a64"], x["w64"], x["bias64"], None, 0) - u.numpy()).max() < 1e-13 * scale
    assert np.abs(G.linear_ref(x["a64"], x["w64"], x["bias64"], x["resid64"], 2) - (u + r).numpy()).max() < 1e-13 * scale
    want = torch.nn.functional.gelu(u)                                               # erf form
    assert np.abs(G.linear_ref(x["a64"], x["w64"], x["bias64"], None, 9) - want.numpy()).max() < 1e-13 * scale
    want = 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * torch.pow(u, 3.0))))   # HF NewGELUActivation
    assert np.abs(G.linear_ref(x["a64"], x["w64"], x["bias64"], None, 1) - want.numpy()).max() < 1e-13 * scale
    assert np.abs(G.linear_ref(x["a64"], x["w64"], x["bias64"], None, 1)
                  - torch.nn.functional.gelu(u, approximate="tanh").numpy()).max() < 1e-13 * scale


def test_gelu_slope_constant():
    u = np.linspace(-8, 8, 160001)
    for f in (G.gelu_new, G.gelu_erf):
        assert np.abs(np.gradient(f(u), u)).max() < G.GELU_SLOPE
    assert all(abs(float(G.gelu_erf(np.array([x]))[0]) - 0.5 * x * (1 + math.erf(x / math.sqrt(2)))) < 1e-15 for x in (-6.0, -1.3, 0.2, 3.0))


# ---------------------------------------------------------------- the bound ---------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_fp32_chain_stays_under_a_quarter_of_the_bound(c, dtype):
    """The inputs leave the bound room: an fp32 chain of the MFMA's shape, k ascending and k descending, is within bound / 4 of
    the float64 value everywhere -- so an element beyond the bound on the GPU is the kernel's."""
    x = G.make_inputs(c, dtype)
    ref = G.linear_ref(x["a64"], x["w64"], None, None, 0)
    bnd = G.bound(x["a64"], x["w64"], None, None, x["K"])
    assert (bnd > 0).all()
    group = 4 if dtype == "fp32" else 32
    worst = 0.0
    for rev in (False, True):
        got = G.fp32_chain(x["a64"], x["w64"], group, reverse=rev).astype(np.float64)
        worst = max(worst, float((np.abs(got - ref) / bnd).max()))
    print(f"{c.name} {dtype}: fp32 chain error / bound = {worst:.4f}")
    assert worst < 0.25
    # with bias and residual added in fp32 (epi 2)
    full = (G.fp32_chain(x["a64"], x["w64"], group) + (x["bias64"].astype(np.float32)[None, :] + x["resid64"].astype(np.float32))).astype(np.float32)
    err = np.abs(full.astype(np.float64) - G.linear_ref(x["a64"], x["w64"], x["bias64"], x["resid64"], 2))
    assert (err < 0.25 * G.bound(x["a64"], x["w64"], x["bias64"], x["resid64"], x["K"])).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_a_dropped_k_chunk_is_detectable(c, dtype):
    """One 16-byte chunk of one row of A zeroed (what a wrong tail guard or a skipped step does) moves some element of that row by
    more than 4 x the bound -- with bias and residual in the bound, and for the first, a middle and the last chunk of K."""
    x = G.make_inputs(c, dtype)
    K, epc = x["K"], (4 if dtype == "fp32" else 8)
    for m, k0 in ((0, 0), (c.M // 2, (K // epc // 2) * epc), (c.M - 1, K - epc)):
        a_row, w = x["a64"][m:m + 1], x["w64"]
        bnd = G.bound(a_row, w, x["bias64"], x["resid64"][m:m + 1], K)
        cut = a_row.copy()
        cut[:, k0:k0 + epc] = 0.0
        moved = np.abs(a_row @ w.T - cut @ w.T)
        assert (moved > 4.0 * bnd).any(), f"row {m}, chunk at k = {k0}: moved at most {float((moved / bnd).max()):.2f} x the bound"


# ---------------------------------------------------------------- the persistent 256x256 kernel: tile walk and case table --------

def _all_tiles_once(M, N, cu_cap):
    L = G.tiles256(M, N, G.NCU256, cu_cap)
    seen = [t for run in L.runs for t in run]
    n = (M // 256) * (N // 256)
    assert len(seen) == n == len(set(seen)), f"{M} x {N}, cap {cu_cap}: {len(seen)} visits of {len(set(seen))} tiles, {n} exist"
    assert all(0 <= m0 < M and 0 <= n0 < N and m0 % 256 == 0 and n0 % 256 == 0 for m0, n0 in seen)
    assert L.skipped == L.tiles_total - n and len(L.runs) == L.grid
    return L


def test_tiles256_visits_every_tile_exactly_once():
    """The arithmetic of launch256d / tile_coords: for every AT x BT in 1..90 x 1..20 and the tile counts of the case table, both
    orientations, every workgroup cap: the union of the workgroups' runs is every tile exactly once.  A failure here is a finding
    about tile_coords (this function mirrors it line by line), not about the mirror's caller."""
    shapes = {(at, bt) for at in range(1, 91) for bt in range(1, 21)} | {(c.M // 256, c.N // 256) for c in G.CASES256}
    shapes |= {(b, a) for a, b in shapes}
    both = set()
    for mt, nt in sorted(shapes):
        for cap in (0, 8, 24, 96):
            L = _all_tiles_once(mt * 256, nt * 256, cap)
            both.add(L.balanced)
            assert L.grid % 8 == 0 and L.grid <= (cap if cap else G.NCU256)      # the XCD interleave of the tile order
    assert both == {True, False}


def test_tiles256_pins():
    """The mirror against values worked out by hand from launch256d."""
    L = G.tiles256(19200, 3584, 256)
    assert (L.balanced, L.m_major, L.AT, L.BT, L.tiles_total, L.grid, L.skipped) == (False, True, 75, 14, 1344, 256, 294)
    # workgroup 0 of 256: tiles 0, 256, 512 = XCD 0, local 0 / 32 (band 0, the column group of 6: ng 1) / 64 (band 1, r = 8: A-tile 8 * 5)
    assert L.runs[0][:3] == [(0, 0), (0, 8 * 256), (40 * 256, 0)]
    # 8 workgroups: workgroup 0 walks XCD 0's local list -- 8 columns of A-tile 0, then A-tile 8
    assert G.tiles256(19200, 3584, 256, 8).runs[0][:9] == [(0, 256 * j) for j in range(8)] + [(8 * 256, 0)]
    L = G.tiles256(2048, 768, 256, 8)
    assert L.balanced and L.grid == 8 and L.runs[1] == [(256, 0), (256, 256), (256, 512)]
    L = G.tiles256(768, 2048, 256, 8)
    assert not L.m_major and not L.deep_a and L.runs[1] == [(0, 256), (256, 256), (512, 256)]
    assert G.tiles256(2048, 768, 256, 100).grid == 24 and G.tiles256(8448, 2304, 256, 100).grid == 96 and G.tiles256(8448, 2304, 256, 7).grid == 256
    assert G.tiles256(256, 256, 256).grid == 8 and [len(r) for r in G.tiles256(256, 256, 256).runs] == [1] + [0] * 7
    assert not G.tiles256(87552, 768, 256).balanced and G.tiles256(87296, 768, 256).balanced       # 1026 / 1023 tiles: 4 * ncu = 1024


def test_cases256_reach_every_branch_of_the_tile_walk():
    launches = {c.name: G.launch_of(c) for c in G.CASES256}
    assert {L.balanced for L in launches.values()} == {True, False}
    assert {L.m_major for L in launches.values()} == {True, False}
    assert {(L.balanced, L.m_major) for L in launches.values()} == {(True, True), (True, False), (False, True), (False, False)}
    sup = [launches[n] for n in G.SUPER_ROWS]
    assert all(not L.balanced and L.skipped > 0 for L in sup) and launches["super-m"].skipped == 294
    assert launches["super-3"].BT < 8 and launches["super-m"].BT % 8 == 6 and launches["super-m"].AT % 32 != 0
    lens = {n: {len(r) for r in L.runs} for n, L in launches.items()}
    assert 0 in lens["single"] and 1 in lens["single"]
    assert lens["uneven"] == {2, 3} and lens["two-tile"] == {2} and lens["grid-8448x2304"] == {1, 2}
    assert any(max(v) >= 3 for v in lens.values()) and any(len(v) > 1 and min(v) > 0 for v in lens.values())
    for deep_a in (True, False):                       # every ring state: nk % 6 on a run of several tiles
        res = {(c.K // 64) % 6 for c in G.CASES256 if c.tag == "ring" and launches[c.name].deep_a == deep_a
               and min(len(r) for r in launches[c.name].runs) >= 3}
        assert res == set(range(6)), (deep_a, res)
    assert launches["cap24"].grid == launches["cap100"].grid == 24
    for c in G.CASES256:
        L = launches[c.name]
        lens_ = sorted({len(r) for r in L.runs})
        print(f"{c.name}: {L.AT} x {L.BT} tiles, {'balanced' if L.balanced else 'supertile'}, grid {L.grid}, "
              f"tiles per workgroup {' / '.join(f'{n} ({sum(len(r) == n for r in L.runs)} wg)' for n in lens_)}, skipped slots {L.skipped}")


@pytest.mark.parametrize("c", G.CASES256, ids=lambda c: c.name)
def test_cases256_take_the_256_kernel_under_their_policy(c):
    epis = [(2, False), (4, True)] + ([(0, True), (1, True), (9, True)] if c.tag in ("ring", "small", "cap") else [])
    for dtype in ("bf16", "f16"):
        for epi, out16 in epis:
            assert G.linear_variant(dtype, epi, out16, c.M, c.N, c.K, tile_policy=c.policy) == ("256d", "persistent"), (c.name, epi)
    if c.tag in ("ring", "cap") or c.name in ("uneven", "two-tile"):      # the bit-invariance partner: the register-staged kernel
        assert G.linear_variant("f16", 0, True, c.M, c.N, c.K, tile_policy=0)[0] != "256d"
    assert c.M % 256 == 0 and c.N % 256 == 0 and c.K % 64 == 0 and c.K >= 128


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["ringA-k128", "ringA-k448", "ringW-k128", "ringW-k448"])
def test_a_stale_slot_and_a_wrong_prefetch_are_detectable(name, dtype):
    """What the carry-over between tiles can get wrong, in float64, on the second tile of workgroup 0's run (uniform inputs of
    make_inputs, unchanged): (1) its k-step 1 reads the deep operand's ring slot as it was three steps earlier -- a k-step of the
    PREVIOUS tile (a slot the run-ahead DMA did not refill); (2) its k-step 0, fetched during the previous tile's last steps, comes
    from the previous tile's operand rows (s_nxt / d_nxt taken from the wrong tile).  Either moves at least a quarter of the tile's
    elements by more than 4 x the tolerance of tests/test_gpu_linear_256.py (16-bit store with bias; bias + residual in fp32),
    while an fp32 chain of the true inputs stays under a quarter of the accumulation bound alone."""
    from gemm_gpu_util import tolerance
    c = G.case(name)
    x = G.make_inputs(c, dtype)
    L = G.launch_of(c)
    (pm0, pn0), (m0, n0) = L.runs[0][0], L.runs[0][1]
    nk = c.K // 64
    a, w = x["a64"], x["w64"]
    A1, W1, A0, W0 = a[m0:m0 + 256], w[n0:n0 + 256], a[pm0:pm0 + 256], w[pn0:pn0 + 256]
    true = G.product(A1, W1)
    g_old = nk * 1 + 1 - 3                              # the global k-step whose data the deep slot of (tile 1, step 1) held before
    assert g_old // nk == 0
    ko = (g_old % nk) * 64
    if L.deep_a:
        stale = true + G.product(A0[:, ko:ko + 64] - A1[:, 64:128], W1[:, 64:128])
    else:
        stale = true + G.product(A1[:, 64:128], W0[:, ko:ko + 64] - W1[:, 64:128])
    wrong = true - G.product(A1[:, :64], W1[:, :64]) + G.product(A0[:, :64], W0[:, :64])
    bias, resid = x["bias64"][n0:n0 + 256], x["resid64"][m0:m0 + 256, n0:n0 + 256]
    s = G.abs_product(A1, W1)
    for epi, out16, r in ((0, True, None), (2, False, resid)):
        ref = G.epilogue(true, bias, r, epi)
        tol = tolerance(dtype, epi, out16, ref, G.bound_from(s, bias, r, c.K))
        for what, bad in (("stale deep slot", stale), ("prefetch from the previous tile", wrong)):
            frac = float((np.abs(bad - true) > 4.0 * tol).mean())
            print(f"{name} {dtype} epi {epi} {what}: {frac:.3f} of the tile beyond 4 x the tolerance")
            assert frac >= 0.25, f"{what}, epi {epi}: only {frac:.3f} of the tile's elements leave 4 x the tolerance"
    bm, bn = G.BLOCK_M, G.BLOCK_N
    bnd = G.bound(a[:bm], w[:bn], None, None, c.K)
    ref = G.product(a[:bm], w[:bn])
    worst = max(float((np.abs(G.fp32_chain(a[:bm], w[:bn], 32, reverse=rev).astype(np.float64) - ref) / bnd).max()) for rev in (False, True))
    print(f"{name} {dtype}: fp32 chain error / bound = {worst:.4f}")
    assert worst < 0.25


# ---------------------------------------------------------------- the query-sized kernels: launcher mirror and case table --------

QIDS = dict(ids=lambda c: c.name)


def test_q_depth_rule_pins():
    """The mirror against values worked out by hand from q_chunks / q_depth_rule / q_class of csrc/qgemm.hip."""
    chunks = [G.q_chunks(bm, bn, False, kd) for bm, bn, kd in G.Q_TILES]
    assert chunks == [3, 2, 3, 3, 4, 6, 8]
    assert [G.q_depth_rule(ch, True) for ch in chunks] == [6, 6, 6, 6, 6, 3, 2]
    assert [G.q_depth_rule(ch, False) for ch in chunks] == [4, 4, 4, 4, 4, 2, 2]
    assert [G.q_chunks(bm, bn, True, 128) for bm, bn in G.Q_LN_TILES] == [1, 2, 2]
    assert G.q_class((32, 32, 128), False, 768) == 6 and G.q_class((32, 32, 128), False, 512) == 4
    assert G.q_class((32, 32, 128), False, 3072) == 6                                   # nk = 24: both divide, the deeper ring wins
    assert G.q_class((32, 32, 128), False, 640) == 0 and G.q_class((32, 16, 256), False, 768) == 0 and G.q_class((32, 16, 256), False, 128) == 0
    assert G.q_class((128, 64, 128), False, 384) == 6 and G.q_class((128, 64, 128), False, 256) == 4 and G.q_class((128, 64, 128), False, 768) == 6
    # 128x128: D = 2 in both classes, so q_class answers 6 whenever it answers: the class-4 instantiation is never launched
    assert {G.q_class((128, 128, 128), False, 128 * nk) for nk in range(1, 65)} == {0, 6}


def test_q_pick_pins_on_the_shapes_of_test_gpu_linear():
    """What the cost rule picks at 256 CUs for the shapes tests/test_gpu_linear.py runs (its docstring cites this): no ragged row tile,
    no 64x32 tile, and only the depths listed."""
    seen = set()
    for M, N, K in [(32, 768, 768), (32, 768, 3072), (96, 2304, 768), (352, 768, 3072), (512, 3072, 768), (1024, 768, 768), (2304, 768, 3072),
                    (2816, 2304, 768), (160, 1024, 1024), (64, 4096, 4096), (448, 2048, 8192)]:
        for epi, ns in [(G.EPI_STORE, 0), (G.EPI_GELU, 0), (G.EPI_RESID, 0)] + ([(G.EPI_QKV, N // 3 * 2)] if N % 96 == 0 else []):
            L = G.q_launch(M, N, K, epi, ns)
            assert L is not None
            if L.bm > 32:
                assert M % L.bm == 0, (M, N, K, epi, L.bm)
            seen.add((L.bm, L.bn, L.D))
    assert seen == {(32, 16, 6), (32, 32, 6), (32, 32, 4), (32, 64, 6), (64, 64, 6), (64, 64, 4), (128, 64, 3), (128, 128, 2)}, sorted(seen)


@pytest.mark.parametrize("c", G.CASESQ, **QIDS)
def test_casesq_get_the_tile_depth_and_group_they_state(c):
    epis = [(G.EPI_QKV, c.n_split), (G.EPI_GELU, 0)] + ([] if c.ln else [(G.EPI_STORE, 0), (G.EPI_RESID, 0)])
    for epi, ns in epis:
        L = G.q_launch(c.M, c.N, c.K, epi, ns, c.ln, c.tile)
        assert L is not None, f"{c.name} epi {epi}: not served"
        assert (L.bm, L.bn, L.kd, L.D, L.group) == (c.bm, c.bn, c.kd, c.D, c.group), f"{c.name} epi {epi}: {L[:6]}"
        assert c.K // c.kd >= L.D and (c.K // c.kd) % L.D == 0 and L.lds <= G.Q_LDS_LIMIT
        assert L.cls == (6 if L.D in (6, 3) or (c.bm, c.bn) == (128, 128) else 4)
        assert G.Q_TILES[c.tile - 1][:2] == (c.bm, c.bn) if not c.ln else G.Q_LN_TILES[c.tile - 1] == (c.bm, c.bn)
        if not c.ln:                                   # a forced tile does not read the CU count
            assert G.q_launch(c.M, c.N, c.K, epi, ns, False, c.tile, ncu=304)[:6] == L[:6]
    if c.ln:                                           # the partner of the bit comparison: the same tile without the prologue
        P = G.q_launch(c.M, c.N, c.K, G.EPI_QKV, c.n_split, False, G.Q_LN_AS_PLAIN[c.tile])
        assert P is not None and (P.bm, P.bn) == (c.bm, c.bn)


@pytest.mark.parametrize("c", G.CASESQ, **QIDS)
def test_casesq_show_the_edges_they_are_listed_for(c):
    L = G.launch_q(c)
    nk = c.K // c.kd
    assert c.K % c.kd == 0 and c.M % 32 == 0 and c.N % c.bn == 0 and c.n_split % c.bn == 0 and 0 < c.n_split < c.N
    assert ("ragged" in c.edges) == (c.M % c.bm != 0)
    assert ("one-tile" in c.edges) == (c.M < c.bm)
    assert ("one-group" in c.edges) == (nk == c.D) and ("long-ring" in c.edges) == (nk in (2 * c.D, 3 * c.D)) and nk in (c.D, 2 * c.D, 3 * c.D)
    assert ("short-run" in c.edges) == (L.R < 8)
    if "uneven-run" in c.edges:
        assert L.c0 >= 1 and L.rem != 0
    elif c.tag == "plain":
        assert L.R < 8
    last = L.NT - (L.NG - 1) * L.group
    assert ("short-last" in c.edges) == (last < L.group)
    split_tile = c.n_split // c.bn                      # the first V tile
    assert ("split-inside" in c.edges) == (split_tile % L.group != 0)
    assert ("bias3" in c.edges) == (L.group * c.bn > 2 * G.QNT)
    if c.tag == "ln-group":
        assert L.group > 1 and L.MT * L.NG <= G.NCU256 < L.MT * L.NT
    # both q | k and V tiles exist, on either side of a tile boundary
    assert 0 < split_tile < L.NT


def test_casesq_cover_what_the_suite_is_for():
    plain = [c for c in G.CASESQ if c.tag == "plain"]
    assert {(c.tile, c.D) for c in plain} == {(1, 6), (1, 4), (2, 6), (2, 4), (3, 6), (3, 4), (4, 6), (4, 4), (5, 6), (5, 4), (6, 3), (6, 2), (7, 2)}
    for k, bm, bn, kd, cls, D, k_one, k_long in G.Q_PLAIN:
        rows = [c for c in plain if (c.tile, c.D) == (k, D)]
        assert {c.K for c in rows} == {k_one, k_long} and k_one // kd == D and k_long // kd in (2 * D, 3 * D)
        assert G.q_class((bm, bn, kd), False, k_one) == cls == G.q_class((bm, bn, kd), False, k_long)
        for K in (k_one, k_long):
            at_k = [c for c in rows if c.K == K]
            assert {c.M for c in at_k} == set(G.Q_ROWS[bm])
            assert any("short-run" in c.edges for c in at_k) and any("uneven-run" in c.edges for c in at_k)
            if bm > 32:
                assert any("ragged" in c.edges for c in at_k) and any("uneven-run" in c.edges and "ragged" in c.edges for c in at_k)
            if bm == 64:
                assert any("ragged" not in c.edges for c in at_k)
            if bm == 128:
                assert any("one-tile" in c.edges for c in at_k)
    ln = [c for c in G.CASESQ if c.tag == "ln"]
    assert {(c.tile, c.K) for c in ln} == {(t, d) for t in (1, 2, 3) for d in (512, 768, 1024)} - {(3, 1024)}
    assert {c.M for c in ln if c.bm == 64} == {96, 160} and all("ragged" in c.edges for c in ln if c.bm == 64)
    assert {c.M for c in ln if c.bm == 32} == {32, 96}
    tile, M, N, d, ns = G.Q_LN_REFUSED
    assert G.q_launch(M, N, d, G.EPI_QKV, ns, True, tile) is None and G.q_launch(M, N, d, G.EPI_QKV, ns, True, 0) is not None
    assert G.q_launch(M, N, 768, G.EPI_QKV, ns, True, tile) is not None
    grp = {c.name: c for c in G.CASESQ if c.tag == "ln-group"}
    assert grp["lng-32x32-128x2144"].group == 2 and G.launch_q(grp["lng-32x32-128x2144"]).NG == 34
    assert "ragged" in grp["lng-64x64-160x5568"].edges and grp["lng-32x64-4096x2112"].group * 64 == 1088
    assert len({c.name for c in G.CASESQ}) == len(G.CASESQ)


def test_q_refusals_of_a_forced_tile():
    assert G.q_launch(32, 128, 768, G.EPI_STORE, force=5) is None                  # M <= 32 on a 64-row tile
    assert G.q_launch(96, 96, 768, G.EPI_STORE, force=5) is None                   # N % 64
    assert G.q_launch(96, 128, 768, G.EPI_STORE, force=1) is None                  # 256-element stages: K / 256 = 3
    assert G.q_launch(96, 128, 768, G.EPI_QKV, 32, force=5) is None                # n_split off the tile boundary
    assert G.q_launch(96, 192, 768, G.EPI_QKV, 128, True, force=4) is None         # the prologue has three candidates
    assert G.q_launch(48, 128, 768, G.EPI_STORE) is None and G.q_launch(32, 128, 640, G.EPI_STORE) is None


def _covers_once(M, N, bm, bn, group):
    MT, NT, NG, R, c0, rem, grid, blocks = G.q_blocks(M, N, bm, bn, group)
    live = [b for b in blocks if b is not None]
    assert len(live) == R == len(set(live)) and set(live) == {(mt, ng) for mt in range(MT) for ng in range(NG)}
    assert grid == len(blocks) and grid % 8 == 0 and grid - R < 8
    # XCD x = blocks x, x + 8, ...: a contiguous run of the column-group-major list, of c0 or c0 + 1 workgroups
    for x in range(8):
        run = [ng * MT + mt for mt, ng in (b for b in blocks[x::8] if b is not None)]
        assert run == list(range(run[0], run[0] + len(run))) if run else R < 8
        assert len(run) == c0 + (1 if x < rem else 0)
    tiles = sorted(t for mt, ng in live for t in range(ng * group, min(NT, ng * group + group)))
    assert tiles == sorted(list(range(NT)) * MT)        # every column tile of every row tile in exactly one group


def test_q_workgroup_list_covers_every_tile_group_once():
    for c in G.CASESQ:
        _covers_once(c.M, c.N, c.bm, c.bn, c.group)
    for MT in (1, 2, 3, 5, 8, 128):                     # R around the multiples of 8
        for R in list(range(1, 42)) + [255, 256, 257]:
            if R % MT == 0:
                for group in (1, 2, 3):
                    NG = R // MT
                    for NT in {NG * group, NG * group - (group - 1)}:
                        _covers_once(MT * 32, NT * 32, 32, 32, group)


# ---------------------------------------------------------------- the fp8 MFMA kernel: tile walk, case table, exact operands ------

Q8IDS = dict(ids=lambda c: c.name)
Q8_SMALL = [c for c in G.CASES256Q if c.tag != "grid"]
# the ring positions a tile can start from: tile i of a run starts at sd = i nk mod 3, so nk % 3 == 0 always starts from 0
Q8_RING_STATES = {(0, 0), (0, 1), (1, 1), (2, 1), (0, 2), (2, 2), (1, 2)}         # (sd at the start of a tile, nk % 3)


def test_tiles256q_visits_every_tile_exactly_once():
    """launch256q / tile_coords of gemm256q_kernel: the supertile walk at every size, never the balanced one; the union of the
    workgroups' runs is every tile exactly once for every AT x BT in 1..40 x 1..12, both orientations, every cap."""
    shapes = {(at, bt) for at in range(1, 41) for bt in range(1, 13)} | {(c.M // 256, c.N // 256) for c in G.CASES256Q}
    shapes |= {(b, a) for a, b in shapes}
    for mt, nt in sorted(shapes):
        for cap in G.CAPQ + (96,):
            L = G.tiles256q(mt * 256, nt * 256, G.NCU256, cap)
            seen = [t for run in L.runs for t in run]
            assert not L.balanced and len(seen) == mt * nt == len(set(seen)), (mt, nt, cap)
            assert all(0 <= m0 < mt * 256 and 0 <= n0 < nt * 256 for m0, n0 in seen)
            assert L.skipped == L.tiles_total - mt * nt and L.grid % 8 == 0 and L.grid <= (cap // 8 * 8 if 8 <= cap < G.NCU256 else G.NCU256)
            assert L.deep_a == (mt >= nt) == L.m_major
            slots = G.slots256q(mt * 256, nt * 256, G.NCU256, cap)
            assert [[s for s in r if s is not None] for r in slots] == L.runs


def test_tiles256q_pins():
    """The mirror against values worked out by hand from launch256q."""
    L = G.tiles256q(2048, 768, 256, 8)                 # AT 8, BT 3: one band of 4 x 8 x 3 = 96 slots; XCD b's first three are (b, 0 .. 2)
    assert (L.tiles_total, L.grid, L.skipped) == (96, 8, 72) and L.runs[1] == [(256, 0), (256, 256), (256, 512)]
    L = G.tiles256q(768, 2048, 256, 8)
    assert not L.m_major and not L.deep_a and L.runs[1] == [(0, 256), (256, 256), (512, 256)]
    assert [G.tiles256q(2048, 768, 256, cap).grid for cap in G.CAPQ] == [96, 8, 24, 96]
    L = G.tiles256q(256, 256, 256)                     # 32 slots for one tile
    assert (L.tiles_total, L.grid) == (32, 32) and [len(r) for r in L.runs] == [1] + [0] * 31
    L = G.tiles256q(2304, 2304, 256, 8)                # BT 9: column groups of 8 and 1; A-tile 8 belongs to XCD 0
    assert L.tiles_total == 288 and [len(r) for r in L.runs] == [18] + [9] * 7
    assert L.runs[0] == [(0, 256 * j) for j in range(8)] + [(2048, 256 * j) for j in range(8)] + [(0, 2048), (2048, 2048)]
    assert L.runs[3] == [(768, 256 * j) for j in range(9)]
    L = G.tiles256q(8192, 2304, 256)
    assert (L.tiles_total, L.grid, L.skipped) == (288, 256, 0) and sorted(len(r) for r in L.runs) == [1] * 224 + [2] * 32


def test_cases256q_reach_every_branch_of_the_tile_walk():
    launches = {c.name: G.launch_of_q8(c) for c in G.CASES256Q}
    for deep_a in (True, False):
        states = set()
        for c in G.CASES256Q:
            L = launches[c.name]
            if c.tag == "ring" and L.deep_a == deep_a:
                nk = c.K // 128
                assert c.K % 256 == 0 and L.grid == 8 and all(len(r) == 3 for r in L.runs)
                states |= {((i * nk) % 3, nk % 3) for r in L.runs for i in range(len(r))}
        assert states == Q8_RING_STATES, (deep_a, states)
    assert {(L.deep_a, L.m_major) for L in launches.values()} == {(True, True), (False, False)}
    for tag in ("ring", "grid"):
        assert {launches[c.name].deep_a for c in G.CASES256Q if c.tag == tag} == {True, False}
    L = launches["q8-uneven"]
    assert sorted(len(r) for r in L.runs) == [0, 0, 0, 4, 4, 4, 4, 4]                  # three of eight workgroups exit at once
    assert [len(r) for r in launches["q8-single"].runs].count(1) == 1 and sum(map(len, launches["q8-single"].runs)) == 1
    c = G.case("q8-groups")
    slots = G.slots256q(c.M, c.N, G.NCU256, c.cu_cap)
    def interior_gap(r):
        live = [i for i, s in enumerate(r) if s is not None]
        return any(s is None for s in r[live[0]:live[-1]])
    assert all(interior_gap(r) for r in slots) and launches["q8-groups"].BT == 9       # a skipped slot between two tiles of a run
    # the look-up of the tile after the next one runs past the end: in every run of two tiles or more, at its last but one tile
    assert all(len(r) >= 2 for c in G.CASES256Q if c.tag in ("ring", "groups") for r in launches[c.name].runs)
    assert {tuple(sorted({len(r) for r in launches[n].runs})) for n in ("q8-grid-m", "q8-grid-n")} == {(1, 2)}
    assert [G.launch_of_q8(G.case("q8-cap"), cu_cap=cap).grid for cap in G.CAPQ] == [96, 8, 24, 96]
    assert all(c.K % 256 == 0 and c.M % 256 == 0 and c.N % 256 == 0 for c in G.CASES256Q)
    assert len({c.name for c in G.CASES + G.CASES256 + G.CASES256Q + G.CASESQ}) == len(G.CASES + G.CASES256 + G.CASES256Q + G.CASESQ)


@pytest.mark.parametrize("c", G.CASES256Q, **Q8IDS)
def test_exact_operands_have_distinct_slabs_and_small_sums(c):
    """Per operand, the 256 x 128-byte slabs of any two different (row tile, k-step) pairs differ -- so do the (A slab, W slab)
    pairs of any two (tile, k-step) -- the codes are integers e4m3 holds exactly, and |acc| <= EXACT_ACC_MAX."""
    a, w = G.exact_codes(c.M, c.N, c.K)
    assert a.min() == -4 and a.max() == 4 and w.min() == -6 and w.max() == 6
    for x in (a, w):
        back = torch.from_numpy(x.astype(np.float32)).to(torch.float8_e4m3fn).float().numpy()
        assert np.array_equal(back, x)
    for x, rows in ((a, c.M), (w, c.N)):
        slabs = {x[r0:r0 + 256, k0:k0 + 128].astype(np.int8).tobytes() for r0 in range(0, rows, 256) for k0 in range(0, c.K, 128)}
        assert len(slabs) == (rows // 256) * (c.K // 128)
    acc = a.astype(np.float32) @ w.astype(np.float32).T                              # integers below 2^24: exact in fp32 too
    assert float(np.abs(acc).max()) <= G.EXACT_ACC_MAX and 24 * c.K <= 18432
    assert 8 * G.EXACT_ACC_MAX < 2 ** 15
    if c.tag != "grid":
        assert np.array_equal(acc.astype(np.float64), G.exact_case(c.name)["acc"])


@pytest.mark.parametrize("c", Q8_SMALL, **Q8IDS)
def test_exact_epilogue_values_are_exact_in_fp32(c):
    """Every intermediate the epilogues form from the exact operands is an fp32 number: the scaled accumulator, with the bias, and
    with bias + residual, for every scale variant; the gelu set-up keeps u >= 16, u / out_scale <= 448 and at GELU_EXACT_MARGIN
    from every rounding boundary of e4m3, and gelu_new(u) = u in float64."""
    x = G.exact_case(c.name)
    f32 = lambda v: np.array_equal(v.astype(np.float32).astype(np.float64), v)
    for variant, (rows, a_scalar) in G.SCALE_VARIANTS.items():
        v = G.exact_scaled(x, variant)
        assert float(np.abs(v).max()) < 2 ** 15 - 16
        assert f32(v) and f32(v + x["bias"][None, :]) and f32(x["bias"][None, :] + x["resid"]) and f32(v + (x["bias"][None, :] + x["resid"]))
        bias, out_scale, u = G.gelu_exact_setup(x["acc"], x["sa"] if rows else None, x["sw"], a_scalar)
        assert f32(bias) and f32(u) and np.array_equal(v + bias[None, :], u)
        assert float(u.min()) >= 16.0 and float(u.max()) <= 448.0 * out_scale and math.log2(out_scale) == round(math.log2(out_scale))
        assert np.array_equal(G.gelu_new(u), u)
        margin = float(G.e4m3_tie_distance(u / out_scale).min())
        print(f"{c.name} {variant}: u in [{u.min():.4g}, {u.max():.4g}], out_scale {out_scale:g}, distance to a rounding boundary >= 2^{math.log2(margin):.2f}")
        assert margin >= G.GELU_EXACT_MARGIN


def test_e4m3_tie_distance():
    v = np.array([1.0, 1.0625, 1.125, 17.0, 18.0, 448.0, 2.0 ** -9, 1.5 * 2.0 ** -9])
    assert np.allclose(G.e4m3_tie_distance(v), [0.03125, 0.0, 0.0625 / 1.125, 0.0, 1.0 / 18.0, 16.0 / 448.0, 0.5, 0.0])
    assert len(G.e4m3_values()) == 127 and G.e4m3_values()[-1] == 448.0


@pytest.mark.parametrize("c", [c for c in G.CASES256Q if c.tag in ("ring", "uneven", "groups", "grid")], **Q8IDS)
def test_a_slab_from_the_wrong_tile_or_a_stale_slot_changes_the_exact_result(c):
    """What the carry-over between the tiles of a run can get wrong, as integers, for every pair of consecutive tiles of two
    workgroups' runs and every k-step of the later tile: (1) the A slab or (2) the W slab of that k-step comes from the previous
    tile of the run; (3) the deep operand's slab is the one its ring slot held three global k-steps earlier (a slot the run-ahead
    DMA did not refill: for the first k-steps of a tile a slab of the PREVIOUS tile).  Each changes more than nine tenths of the
    tile's integer sums -- the condition under which torch.equal on the GPU sees the fault with certainty."""
    a, w = G.exact_codes(c.M, c.N, c.K)
    L = G.launch_of_q8(c)
    nk = c.K // 128
    runs = [r for r in L.runs if len(r) >= 2]
    assert runs
    for run in (runs[0], runs[-1]):
        for i in range(1, len(run)):
            (pm0, pn0), (m0, n0) = run[i - 1], run[i]
            A1, W1, A0, W0 = a[m0:m0 + 256], w[n0:n0 + 256], a[pm0:pm0 + 256], w[pn0:pn0 + 256]
            for kt in range(nk):
                ks = slice(kt * 128, kt * 128 + 128)
                moved = {"A from the previous tile": (A0[:, ks] - A1[:, ks]) @ W1[:, ks].T,
                         "W from the previous tile": A1[:, ks] @ (W0[:, ks] - W1[:, ks]).T}
                g = i * nk + kt - 3                     # global k-step of the run whose deep slab the ring slot held before
                D_old = (A0, W0)[not L.deep_a] if g < i * nk else (A1, W1)[not L.deep_a]
                go = slice((g % nk) * 128, (g % nk) * 128 + 128)
                if L.deep_a:
                    moved["stale deep slot"] = (D_old[:, go] - A1[:, ks]) @ W1[:, ks].T
                else:
                    moved["stale deep slot"] = A1[:, ks] @ (D_old[:, go] - W1[:, ks]).T
                for what, d in moved.items():
                    if (pm0 == m0 and what.startswith("A")) or (pn0 == n0 and what.startswith("W")):
                        continue                        # the neighbour shares this operand's rows: the same slab
                    frac = float((d != 0).mean())
                    assert frac > 0.9, f"{c.name} tile {i} of a run, k-step {kt}, {what}: only {frac:.3f} of the sums change"
