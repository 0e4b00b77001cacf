"""Test infrastructure: the projection GEMM with its fused epilogues (include/sgpt_hip.h::sgpt_linear / sgpt_linear_split) in
float64 numpy, a derived error bound for any fp32 accumulation of the same products, a Python mirror of the launch rule of
csrc/gemm.hip and of the tile walk of its persistent 256x256 kernel, the same for the fp8 MFMA kernel (csrc/gemm256q.hip) with
operands whose sums are exact, a mirror of the launcher and workgroup list of the query-sized kernels (csrc/qgemm.hip), and the
shape tables of tests/test_gpu_linear_edges.py, tests/test_gpu_linear_256.py, tests/test_gpu_linear_fp8.py and
tests/test_gpu_linear_query.py.  Checked without a GPU by tests/test_gemm_ref.py.

Operands are the exact values of the already rounded inputs (16-bit x 16-bit and fp32 x fp32 products are taken as the float64
product of the stored values), so the only error a kernel may show is that of its fp32 accumulation, of the epilogue function
and of the one rounding to the output format."""
import functools
import math
from collections import namedtuple

import numpy as np

EPI_STORE, EPI_GELU, EPI_RESID, EPI_VT, EPI_GELU_ERF = 0, 1, 2, 4, 9
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
GELU_SLOPE = 1.13                                     # max |gelu'| of both GELUs (1.1290 at u = 1.41): an error of the sum through the function


def _erf(x):
    """float64 erf, vectorised (torch's; tests/test_gemm_ref.py pins it to math.erf -- np.vectorize(math.erf) takes seconds on
    the large cases)."""
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu_new(u):
    """HF NewGELUActivation (gelu_new): 0.5 u (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3)))."""
    u = np.asarray(u, np.float64)
    return 0.5 * u * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def gelu_erf(u):
    """HF GELUActivation ("gelu"): 0.5 u (1 + erf(u / sqrt 2))."""
    u = np.asarray(u, np.float64)
    return 0.5 * u * (1.0 + _erf(u / math.sqrt(2.0)))


def product(a, w):
    """a w^T in float64 (the part of linear_ref worth computing once per case)."""
    return np.asarray(a, np.float64) @ np.asarray(w, np.float64).T


def epilogue(u, bias, resid, epi):
    """The epilogue of sgpt_linear on the float64 product u [M, N]."""
    if bias is not None:
        u = u + np.asarray(bias, np.float64)[None, :]
    if epi == EPI_STORE:
        return u
    if epi == EPI_GELU:
        return gelu_new(u)
    if epi == EPI_GELU_ERF:
        return gelu_erf(u)
    if epi == EPI_RESID:
        return np.asarray(resid, np.float64) + u
    if epi == EPI_VT:
        return np.ascontiguousarray(u.T)
    raise ValueError(f"epi {epi}")


def linear_ref(a, w, bias, resid, epi):
    """float64 value of sgpt_linear: a [M, K], w [N, K], bias [N] or None, resid [M, N] or None.
    epi 0: a w^T (+ bias); 1: gelu_new(a w^T + bias); 9: gelu_erf(a w^T + bias); 2: resid + a w^T + bias;
    4: (a w^T (+ bias))^T, shape [N, M]."""
    return epilogue(product(a, w), bias, resid, epi)


def split_ref(a, w, bias, epi):
    """sgpt_linear_split (epi 0 | 1 | 4): the float64 value v that hi = round16(v) and lo = round16(v - hi) reproduce together."""
    if epi not in (EPI_STORE, EPI_GELU, EPI_VT):
        raise ValueError(f"epi {epi}")
    return linear_ref(a, w, bias, None, epi)


def abs_product(a, w):
    """|a| |w|^T in float64: the magnitude sum under the bound."""
    return np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(w, np.float64)).T


def bound_from(s, bias, resid, K):
    """bound() from a precomputed s = abs_product(a, w)."""
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    if resid is not None:
        s = s + np.abs(np.asarray(resid, np.float64))
    return (K + 4) * 2.0 ** -23 * s


def bound(a, w, bias, resid, K):
    """Per-element bound [M, N] on |fp32 result - float64 value| of resid + a w^T + bias computed as an fp32 chain of ANY order:
    (K + 4) 2^-23 S with S = |a| |w|^T + |bias| + |resid| -- the gamma_n bound of a sum of n = K products plus the bias, the
    residual and the scale factors of the epilogue (4 more roundings).  Unit roundoff 2^-23, not 2^-24: the MFMA's internal
    adds are not documented to round to nearest.  Derived, not measured: nothing of the kernel enters but fp32 accumulation."""
    return bound_from(abs_product(a, w), bias, resid, K)


def fp32_chain(a, w, group, reverse=False):
    """a w^T the way an fp32 MFMA chain forms it, in numpy: float32 products, `group` of them summed in float32 per step (32 for
    the 16x16x32 16-bit instruction, 4 for 16x16x4 fp32), the step added to a float32 accumulator; k ascending, or descending
    with reverse=True.  Returns float32 [M, N].  For small shapes (a Python loop over K)."""
    a32, w32 = np.asarray(a, np.float32), np.asarray(w, np.float32)
    K = a32.shape[1]
    ks = list(range(K))
    if reverse:
        ks.reverse()
    acc = np.zeros((a32.shape[0], w32.shape[0]), np.float32)
    for s0 in range(0, K, group):
        part = np.zeros_like(acc)
        for k in ks[s0:s0 + group]:
            part = (part + a32[:, k, None] * w32[None, :, k]).astype(np.float32)
        acc = (acc + part).astype(np.float32)
    return acc


# ---------------------------------------------------------------- the launch rule of csrc/gemm.hip, default build ----------------
FEW_TILES, DEEP_TILES, KG16_MIN = 128, 512, 6        # SGPT_FEW_TILES, SGPT_DEEP_TILES, SGPT_KG16_MIN


def linear_variant(dtype, epi, out16, M, N, K, tile_policy=0, low_latency=False):
    """(kernel, block order) that sgpt_linear launches: a mirror of launch_gemm16<> and launch<> in csrc/gemm.hip.
    dtype 'bf16' | 'f16' | 'fp32'; out16 is accepted for symmetry with the entry (no rule depends on it today).
    kernel: '256d' (256x256 LDS-DMA tiles), 'rs128' (register-staged, 128x128, 64-element k-steps), 'rs64' (64x64, 64-element
    k-steps), 'rs64-deep' (64x64, 128-element k-steps), 'rs64-kg2' (the same with two k-groups).  order: 'run' (at most 512
    tiles: each XCD a contiguous run of the tile list), 'supertile' (8 x 8 supertiles per XCD), 'persistent' for 256d.
    A change of the rule in gemm.hip must change this function and the shape table with it: test_gemm_ref.py fails until then."""
    del out16
    gelu = epi in (EPI_GELU, EPI_GELU_ERF)
    if dtype != "fp32":
        few = tile_policy != 1 and (M // 256) * (N // 256) <= (255 if gelu else FEW_TILES)
        shape256 = M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 128
        if shape256 and not few:
            return "256d", "persistent"
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    small = t128 < (600 if K <= 1024 else 300)
    B = 64 if small else 128
    MT, NT = (M + B - 1) // B, (N + B - 1) // B
    order = "run" if MT * NT <= 512 else "supertile"
    if not small:
        return "rs128", order
    if MT * NT > DEEP_TILES:
        return "rs64", order
    nk16 = -(-K // (16 * (4 if dtype == "fp32" else 8)))      # 128-element (fp32: 64-element) k-steps
    if low_latency and nk16 % 2 == 0 and nk16 // 2 >= KG16_MIN:
        return "rs64-kg2", order
    return "rs64-deep", order


def tile_of(kernel):
    return {"rs128": 128, "rs64": 64, "rs64-deep": 64, "rs64-kg2": 64, "256d": 256}[kernel]


def kstep_of(kernel, dtype):
    """Elements of K per k-step of a register-staged kernel: 8 (deep: 16) chunks of 16 bytes."""
    chunks = 16 if kernel in ("rs64-deep", "rs64-kg2") else 8
    return chunks * (4 if dtype == "fp32" else 8)


# ---------------------------------------------------------------- shapes of tests/test_gpu_linear_edges.py -----------------------
# K16 / K32: the reduction length with 16-bit / fp32 operands.  edges: what the shape is listed for -- 'M' (M % tile != 0),
# 'N' (N % tile != 0, a multiple of 4 left over unless N % 4 != 0), 'K' (K % k-step != 0), 'order' (MT % 8 != 0, NT % 8 != 0 or
# MT == 1 under the supertile order).  ll: low-latency mode (k-groups) on.  tag: which test of the GPU file owns the case.
Case = namedtuple("Case", "name M N K16 K32 kernel order edges ll tag")


def _c(name, M, N, K16, K32, kernel, order, edges, ll=False, tag="epi"):
    return Case(name, M, N, K16, K32, kernel, order, frozenset(edges.split()), ll, tag)


CASES = [
    # a single partial k-step: every M and N once, every (below / above one tile) x (below / above one tile) corner
    _c("k1-1x4", 1, 4, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-63x132", 63, 132, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-65x60", 65, 60, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-130x68", 130, 68, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-1x132", 1, 132, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-130x4", 130, 4, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-63x60", 63, 60, 8, 4, "rs64-deep", "run", "M N K"),
    _c("k1-65x68", 65, 68, 8, 4, "rs64-deep", "run", "M N K"),
    # full 128-element (fp32: 64-element) steps and a tail
    _c("kt-65x68", 65, 68, 136, 68, "rs64-deep", "run", "M N K"),
    _c("kt-65x132", 65, 132, 200, 100, "rs64-deep", "run", "M N K"),
    _c("kt-130x68", 130, 68, 200, 132, "rs64-deep", "run", "M N K"),
    _c("kt-130x132", 130, 132, 136, 68, "rs64-deep", "run", "M N K"),
    # M % 128 == 0: the same with the transposed store (epi 4) among the epilogues
    _c("vt-128x60", 128, 60, 8, 4, "rs64-deep", "run", "N K"),
    _c("vt-128x68", 128, 68, 200, 100, "rs64-deep", "run", "N K"),
    _c("vt-256x132", 256, 132, 136, 68, "rs64-deep", "run", "N K"),
    # 64-element steps, supertile order with MT = 25, NT = 23 (the last column tile 4 wide)
    _c("st64-1540x1412", 1540, 1412, 72, 36, "rs64", "supertile", "M N K order"),
    # 128x128 tiles: supertile order with 25 x 25 tiles; run order with a long k-loop and a tail (t128 = 320)
    _c("st128-3100x3076", 3100, 3076, 72, 36, "rs128", "supertile", "M N K order"),
    _c("run128-2500x1924", 2500, 1924, 1032, 1028, "rs128", "run", "M N K"),
    # k-groups with a tail (group 1's last step is the partial one), and the control with an odd step count
    _c("kg2-130x68", 130, 68, 1528, 764, "rs64-kg2", "run", "M N K", ll=True, tag="kgroup"),
    _c("kg1-130x68", 130, 68, 1400, 700, "rs64-deep", "run", "M N K", ll=True, tag="kgroup"),
    # the LM head: one row tile, N % 4 == 1 (epi 0 only)
    _c("lmhead-37x50257", 37, 50257, 768, 768, "rs64", "supertile", "M N order", tag="oddn"),
    # odd N with a 16-bit output: 8-byte vector stores that are not 8-byte aligned (the last test of the GPU file)
    _c("odd-65x1001", 65, 1001, 136, 136, "rs64-deep", "run", "M N K", tag="last"),
]

# the block of the large cases that is also computed as a problem of its own (bit invariance across tile sizes and k-steps)
BLOCK_M, BLOCK_N = 130, 68
BLOCK_CASES = ("st128-3100x3076", "run128-2500x1924", "st64-1540x1412")


# ---------------------------------------------------------------- the persistent 256x256 kernel: launch256d and tile_coords ------
Launch256 = namedtuple("Launch256", "balanced m_major deep_a AT BT tiles_total grid skipped runs")


@functools.lru_cache(maxsize=8)
def _tile_list256(MT, NT, ncu, gm, gn, may_balance=True):
    """tile_coords of gemm256d_kernel for every tile index below tiles_total: (m0, n0), or None where it returns false.
    may_balance=False: tile_coords of gemm256q_kernel (csrc/gemm256q.hip), which has the supertile branch alone."""
    m_major = MT >= NT
    AT, BT = (MT, NT) if m_major else (NT, MT)
    GM, GN = (gm if gm > 0 else 4), (gn if gn > 0 else 8)
    balanced = may_balance and AT * BT <= 4 * ncu              # launch256d
    R = AT * BT
    c0, rem = R >> 3, R & 7
    tiles_total = 8 * ((R + 7) >> 3) if balanced else ((AT + 7) // 8 + GM - 1) // GM * GM * 8 * BT
    per_band = GM * BT

    def tile_coords(tile):
        xcd = tile & 7
        if balanced:
            l = tile >> 3
            if l >= c0 + (1 if xcd < rem else 0):
                return None
            gi = xcd * c0 + (xcd if xcd < rem else rem) + l
            at = gi // BT
            bt = gi - at * BT
        else:
            local = tile >> 3
            band, inb = local // per_band, local % per_band
            ng = inb // (GM * GN)
            g = BT - ng * GN if BT - ng * GN < GN else GN
            r = inb - ng * GM * GN
            at, bt = xcd + 8 * (band * GM + r // g), ng * GN + r % g
            if at >= AT:
                return None
        return ((at if m_major else bt) * 256, (bt if m_major else at) * 256)

    return balanced, m_major, AT, BT, tuple(tile_coords(t) for t in range(tiles_total))


def tiles256(M, N, ncu, cu_cap=0, gm=4, gn=8):
    """A line-by-line mirror of launch256d<> and of tile_coords in gemm256d_kernel (csrc/gemm.hip): the launch of an M x N problem
    (multiples of 256) on a device of ncu CUs under the per-ctx workgroup cap cu_cap.  runs[b] is the ordered list of (m0, n0)
    workgroup b visits -- tile = b, b + grid, ... below tiles_total, the slots tile_coords refuses skipped (`skipped` of them in
    all).  deep_a is what launch_gemm16 passes for sgpt_linear (M >= N; the EPI_QKV launch always passes true)."""
    ncu = ncu // 8 * 8
    balanced, m_major, AT, BT, coords = _tile_list256(M // 256, N // 256, ncu, gm, gn)
    tiles_total = len(coords)
    cus = cu_cap // 8 * 8 if 8 <= cu_cap < ncu else ncu
    grid = tiles_total if tiles_total < cus else cus
    runs = [[c for c in coords[b::grid] if c is not None] for b in range(grid)]
    return Launch256(balanced, m_major, M >= N, AT, BT, tiles_total, grid, sum(c is None for c in coords), runs)


# ---------------------------------------------------------------- shapes of tests/test_gpu_linear_256.py -------------------------
# 16-bit operands only (fp32 never takes the 256x256 kernel); written for a device of NCU256 CUs.  policy: the tile policy of the
# launch (1 = force 256x256 tiles).  tag: 'ring' (every epilogue; a run of several tiles at every nk % 6), 'small' (every
# epilogue: single / uneven / two-tile), 'grid' and 'super' (in-place residual and transposed store only), 'cap' (bit invariance).
NCU256 = 256
Case256 = namedtuple("Case256", "name M N K policy cu_cap tag")
RING_K = (128, 192, 256, 320, 384, 448)                # nk = 2 .. 7: every nk % 6
CASES256 = (
    [Case256(f"ringA-k{K}", 2048, 768, K, 1, 8, "ring") for K in RING_K]           # deep A: 24 tiles, 3 per workgroup
    + [Case256(f"ringW-k{K}", 768, 2048, K, 1, 8, "ring") for K in RING_K]         # deep W (M < N)
    + [
        Case256("single", 256, 256, 128, 1, 0, "small"),                            # R = 1: seven of eight workgroups exit at once
        Case256("uneven", 1280, 1024, 192, 1, 8, "small"),                          # R = 20: runs of 3 and 2 tiles
        Case256("two-tile", 1024, 1024, 128, 1, 8, "small"),                        # the n2tile lookup runs past the end
        Case256("grid-8448x2304", 8448, 2304, 192, 0, 0, "grid"),                   # 297 tiles on 256 workgroups: 2 and 1
        Case256("super-m", 19200, 3584, 128, 0, 0, "super"),                        # AT 75 / BT 14: ragged bands, 294 skipped slots
        Case256("super-n", 3584, 19200, 128, 0, 0, "super"),                        # m_major == false
        Case256("super-3", 87552, 768, 128, 0, 0, "super"),                         # AT 342 / BT 3: BT < GN
        Case256("cap24", 2048, 768, 320, 1, 24, "cap"),
        Case256("cap100", 2048, 768, 320, 1, 100, "cap"),                           # 100 rounds down to 96
    ]
)
SUPER_ROWS = ("super-m", "super-n", "super-3")


def launch_of(c, ncu=NCU256, cu_cap=None):
    return tiles256(c.M, c.N, ncu, c.cu_cap if cu_cap is None else cu_cap)


# ---------------------------------------------------------------- the fp8 MFMA kernel: launch256q and its tile_coords ------------
def tiles256q(M, N, ncu, cu_cap=0, gm=4, gn=8):
    """The same mirror for launch256q<> and tile_coords of gemm256q_kernel (csrc/gemm256q.hip): the supertile walk (GM 4 / GN 8) at
    every size -- the kernel has no balanced branch -- under the per-ctx workgroup cap; deep_a = M >= N (launch256q)."""
    ncu = ncu // 8 * 8
    balanced, m_major, AT, BT, coords = _tile_list256(M // 256, N // 256, ncu, gm, gn, False)
    tiles_total = len(coords)
    cus = cu_cap // 8 * 8 if 8 <= cu_cap < ncu else ncu
    grid = tiles_total if tiles_total < cus else cus
    runs = [[c for c in coords[b::grid] if c is not None] for b in range(grid)]
    return Launch256(balanced, m_major, M >= N, AT, BT, tiles_total, grid, sum(c is None for c in coords), runs)


def slots256q(M, N, ncu, cu_cap=0):
    """Per workgroup, the slots it looks at in order -- (m0, n0), or None for a slot tile_coords refuses (the walk of tiles256q
    with the refused slots kept: a None between two tiles is a skipped slot in the interior of a run)."""
    L = tiles256q(M, N, ncu, cu_cap)
    coords = _tile_list256(M // 256, N // 256, ncu // 8 * 8, 4, 8, False)[4]
    return [list(coords[b::L.grid]) for b in range(L.grid)]


# ---------------------------------------------------------------- shapes of tests/test_gpu_linear_fp8.py -------------------------
# fp8 (e4m3) operands, every K a multiple of 256; nk = K / 128 k-steps.  A workgroup carries the deep ring position sd (mod 3)
# from tile to tile: tile i of a run starts from sd = i nk mod 3.  tag: 'ring' (24 tiles on 8 workgroups, runs of 3: with
# nk % 3 = 2, 1, 0 the tiles of a run start from every sd), 'uneven' (three of eight workgroups without a tile), 'single',
# 'groups' (BT = 9 > GN: a second column group of width 1, skipped slots between the valid tiles of a run), 'cap' (bit invariance
# under the cap), 'grid' (no cap: 288 slots on a device of 256 CUs, runs of 2 and 1 -- the only rows that depend on the CU count).
Case256Q = namedtuple("Case256Q", "name M N K cu_cap tag")
RINGQ_K = (256, 512, 768)
CAPQ = (0, 8, 24, 100)                                 # 100 rounds down to 96
CASES256Q = (
    [Case256Q(f"q8-ringA-k{K}", 2048, 768, K, 8, "ring") for K in RINGQ_K]          # deep A (M >= N)
    + [Case256Q(f"q8-ringW-k{K}", 768, 2048, K, 8, "ring") for K in RINGQ_K]        # deep W
    + [
        Case256Q("q8-uneven", 1280, 1024, 256, 8, "uneven"),
        Case256Q("q8-single", 256, 256, 256, 0, "single"),
        Case256Q("q8-groups", 2304, 2304, 256, 8, "groups"),
        Case256Q("q8-cap", 2048, 768, 512, 0, "cap"),
        Case256Q("q8-grid-m", 8192, 2304, 512, 0, "grid"),
        Case256Q("q8-grid-n", 2304, 8192, 512, 0, "grid"),
    ]
)


def launch_of_q8(c, ncu=NCU256, cu_cap=None):
    return tiles256q(c.M, c.N, ncu, c.cu_cap if cu_cap is None else cu_cap)


# Exact operands.  Small-integer e4m3 codes: every product is an integer and every sum of them is exact in fp32 whatever its order,
# so the output of the kernel is ONE value per element and a k-step taken from a stale ring slot or from another tile fails
# torch.equal with certainty.  |a| <= 4, |w| <= 6: |acc| <= 24 K <= 18 432 (K <= 768) for any such codes; the pattern below keeps
# |acc| <= EXACT_ACC_MAX = 2^11 (tests/test_gemm_ref.py computes it for every case).  Row scales 2^-4 .. 2^2, channel scales
# 2^-3 .. 2^1, a_scalar 1 or 2^-2: every scaled value is at most 8 EXACT_ACC_MAX = 2^14 < 2^15 -- the threshold of the f16 range
# tracker -- and a multiple of 2^-9 with at most 11 + 9 significant bits; with the integer bias and residual added (|.| <= 13)
# it still has fewer than 24: every intermediate of every epilogue is exact in fp32, and the 16-bit stores round an exact value once.
# The pattern is a multiplicative hash of (row, k) folded to -4 .. 4 (a) and -6 .. 6 (w).  The periodic pattern of
# test_gpu_fp8mfma.py::test_linear_fp8_layout_probe, (5 m + 3 k) % 9 - 4 and (7 n + 11 k) % 13 - 6, does not serve here: its
# 256 x 128-byte slabs repeat -- A after 3 k-steps and after 9 row tiles, and the slab of (row tile 3, k-step 0) is that of (row
# tile 0, k-step 1) -- so a k-step read from the ring slot of three steps earlier would go unseen.  Linear patterns whose
# strides depend on the tile and the k-step have distinct slabs but resonate (|acc| up to 3 000 at K = 768); the hash has
# distinct slabs and accumulators of about six standard deviations of a random sum at most.
EXACT_ACC_MAX = 2048


def _hash_codes(R, K, p, q, mod):
    r, k = np.arange(R, dtype=np.uint64)[:, None], np.arange(K, dtype=np.uint64)[None, :]
    h = (((r * np.uint64(p)) ^ (k * np.uint64(q))) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(16)) % np.uint64(mod)).astype(np.int64) - mod // 2


def exact_codes(M, N, K):
    """(a [M, K] in -4 .. 4, w [N, K] in -6 .. 6) as int64 numpy: the small integers above."""
    return _hash_codes(M, K, 73856093, 19349663, 9), _hash_codes(N, K, 83492791, 50331653, 13)


def exact_scales(M, N):
    """Row scales 2^((m % 7) - 4) and channel scales 2^((n % 5) - 3), float64."""
    return 2.0 ** ((np.arange(M) % 7) - 4), 2.0 ** ((np.arange(N) % 5) - 3)


def exact_bias_resid(M, N):
    """Integer bias [N] (period 11, -5 .. 5) and residual [M, N] (period 17 along both axes, -8 .. 8), float64."""
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    return (np.arange(N) % 11 - 5).astype(np.float64), ((3 * m + 5 * n) % 17 - 8).astype(np.float64)


SCALE_VARIANTS = {"row": (True, 1.0), "scalar": (False, 0.25), "both": (True, 0.25)}      # (a_scale per row?, a_scalar)


@functools.lru_cache(maxsize=2)
def exact_case(name):
    """The exact operands of a CASES256Q row and their integer product acc [M, N] in float64 (computed once per case)."""
    c = case(name)
    a, w = exact_codes(c.M, c.N, c.K)
    sa, sw = exact_scales(c.M, c.N)
    bias, resid = exact_bias_resid(c.M, c.N)
    return dict(c=c, a=a, w=w, sa=sa, sw=sw, bias=bias, resid=resid, acc=product(a, w))


def exact_scaled(x, variant):
    """acc sa[m] a_scalar sw[n] of a scale variant, float64 (exact: powers of two)."""
    rows, a_scalar = SCALE_VARIANTS[variant]
    v = x["acc"] * (x["sw"] * a_scalar)[None, :]
    return v * x["sa"][:, None] if rows else v


def e4m3_values():
    """The 127 non-negative finite e4m3fn values, ascending."""
    import torch
    return torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()


def e4m3_tie_distance(v):
    """|v - the nearest rounding boundary of e4m3fn| / |v| for 0 < v <= 448 (float64 array): how far, relatively, a value is from
    the point where a last-bit difference of the epilogue's arithmetic could move its code."""
    vals = e4m3_values()
    ties = 0.5 * (vals[1:] + vals[:-1])
    i = np.clip(np.searchsorted(ties, v), 1, len(ties) - 1)
    return np.minimum(np.abs(v - ties[i - 1]), np.abs(v - ties[i])) / np.abs(v)


GELU_EXACT_MARGIN = 2.0 ** -19                          # 16 fp32 ulps


def gelu_exact_setup(acc, sa, sw, a_scalar):
    """Bias [N] and out_scale for the exact test of the gelu -> e4m3 epilogue on the integer product acc [M, N] under row scales sa
    (None = 1), channel scales sw and a_scalar.  With s[n] = sw[n] a_scalar: bias[n] = s[n] (C[n] + 2^-5), C[n] an integer, so that
    u = acc sa sw a_scalar + bias = s[n] t,  t = acc sa[m] + C[n] + 2^-5  >= 512:
      * u >= 16: z of gelu_new_fast is below -300, exp2 gives 0 and gelu_new(u) = u but for the last bit of rcp(1.0);
      * t is an odd multiple of 2^-5 in [2^9, 2^14) (while |acc sa| < 7 900; the tests compute the distance): it has at least 15 significant bits, a rounding
        boundary of e4m3 has 5, and the nearest one is at least 2^-5 away: 2^-19 relative = GELU_EXACT_MARGIN, 16 ulps of fp32 --
        no last-bit difference of rcp or exp2 moves a code;
      * u is exact in fp32 (19 bits) and u / out_scale <= 448 with out_scale the smallest such power of two.
    A bias per COLUMN cannot make every u / out_scale exactly representable in e4m3 (3 mantissa bits: the product would have to
    take 16 values); the distance to the boundaries is the property that protects the codes, and tests check the computed one.
    Returns (bias float64 [N], out_scale, u float64 [M, N])."""
    v = acc * (1.0 if sa is None else sa[:, None])
    vmax = float(np.abs(v).max())
    C = 512 + math.ceil(vmax) + 16 * (np.arange(acc.shape[1]) % 3)
    s = sw * a_scalar
    bias = s * (C + 2.0 ** -5)
    u = (v + (C + 2.0 ** -5)[None, :]) * s[None, :]
    out_scale = 2.0 ** math.ceil(math.log2(float(u.max()) / 448.0))
    return bias, out_scale, u


# ---------------------------------------------------------------- the query-sized kernels: the launcher of csrc/qgemm.hip --------
# A line-by-line mirror of q_chunks, q_depth_rule, q_class, q_pick_plain, q_plan_ln, qgemm_shape_ok, qgemm_ln_ok and of the
# workgroup list at the top of qgemm_kernel.  A change of a rule in qgemm.hip must change the function here and the table CASESQ
# with it: tests/test_gemm_ref.py fails until then.
EPI_QKV = 7                                            # sgpt_linear_query: q | k row-major, V^T (common.h GemmEpi)
QNT = 512                                              # threads per workgroup (8 waves)
QGEMM_MAX_ROWS = 4096
Q_LDS_LIMIT = 160 * 1024
Q_TILES = ((32, 16, 256), (32, 32, 128), (32, 64, 128), (64, 32, 128), (64, 64, 128), (128, 64, 128), (128, 128, 128))   # bm, bn, kd
Q_LN_TILES = ((32, 32), (32, 64), (64, 64))            # kd = 128
Q_LN_AS_PLAIN = {1: 2, 2: 3, 3: 5}                     # forced prologue tile -> the forced plain tile of the same (bm, bn)


def q_chunks(bm, bn, ln_a, kd):
    """16-byte chunks per thread and ring stage of a tile."""
    return ((0 if ln_a else bm) + bn) * kd * 2 // (QNT * 16)


def q_depth_rule(ch, six):
    """Ring stages in flight in registers."""
    if ch >= 8:
        return 2
    if six:
        return 6 if ch * 6 <= 24 else 3
    return 4 if ch * 4 <= 16 else 2


def q_class(tile, ln_a, K):
    """Depth class of tile (bm, bn, kd) at this K: 6 -> the SIX kernels, 4 -> the others, 0 -> not served."""
    bm, bn, kd = tile
    if K % kd:
        return 0
    nk = K // kd
    ch = q_chunks(bm, bn, ln_a, kd)
    d6, d4 = q_depth_rule(ch, True), q_depth_rule(ch, False)
    ok6, ok4 = nk % d6 == 0, nk % d4 == 0
    if ok6 and (not ok4 or d6 >= d4):
        return 6
    return 4 if ok4 else 0


def q_pick_plain(M, N, K, epi, n_split, ncu, force=0):
    """Index into Q_TILES of the tile a plain launch takes (force: only candidate force - 1), or -1."""
    best, best_cost = -1, 0
    for i, tl in enumerate(Q_TILES):
        bm, bn, _ = tl
        if force > 0 and i != force - 1:
            continue
        if N % bn or not q_class(tl, False, K):
            continue
        if epi == EPI_QKV and (n_split % bn or bn < 16):
            continue
        if bm > 32 and M <= 32:
            continue
        tiles = ((M + bm - 1) // bm) * (N // bn)
        rounds = (tiles + ncu - 1) // ncu
        cost = rounds * (bm + bn)
        if best < 0 or cost < best_cost or (cost == best_cost and bm * bn > Q_TILES[best][0] * Q_TILES[best][1]):
            best, best_cost = i, cost
    return best


def q_plan_ln(M, N, d, epi, n_split, ncu, force=0):
    """(bm, bn, group, LDS bytes) of a launch with the LayerNorm prologue, or None."""
    if d % 128 or N % 32:
        return None
    nk = d // 128
    if nk % 6 != 0 and nk % 4 != 0:
        return None
    best, best_cost = None, 0
    for ci, (bm, bn) in enumerate(Q_LN_TILES):
        if force > 0 and ci != force - 1:
            continue
        if N % bn or (epi == EPI_QKV and n_split % bn):
            continue
        if bm > 32 and M <= 32:
            continue
        mt, nt = (M + bm - 1) // bm, N // bn
        gq = max(1, (mt * nt + ncu - 1) // ncu)
        while mt * ((nt + gq - 1) // gq) > ncu:
            gq += 1
        lds = nk * bm * 256 + 2 * bn * 256 + gq * bn * 4
        if lds > Q_LDS_LIMIT:
            continue
        cost = (6200 if bm == 32 else 9400) + gq * nk * (250 if bn == 32 else 350 if bm == 32 else 440)
        if best is None or cost < best_cost:
            best, best_cost = (bm, bn, gq, lds), cost
    return best


def qgemm_shape_ok(M, N, K, epi, n_split, ncu):
    if M <= 0 or M > QGEMM_MAX_ROWS or M % 32 or K < 128 or N % 16:
        return False
    if epi == EPI_QKV and (n_split % 32 or n_split <= 0 or n_split >= N or N % 32):
        return False
    if epi not in (EPI_STORE, EPI_QKV, EPI_GELU, EPI_RESID):
        return False
    return q_pick_plain(M, N, K, epi, n_split, ncu) >= 0


def qgemm_ln_ok(M, N, d, epi, n_split, ncu):
    if M <= 0 or M > QGEMM_MAX_ROWS or M % 32 or epi not in (EPI_QKV, EPI_GELU):
        return False
    if epi == EPI_QKV and (n_split % 32 or n_split <= 0 or n_split >= N):
        return False
    if d not in (768, 1024, 512):
        return False
    return q_plan_ln(M, N, d, epi, n_split, ncu) is not None


QLaunch = namedtuple("QLaunch", "bm bn kd D cls group lds MT NT NG R c0 rem grid blocks")


def q_blocks(M, N, bm, bn, group):
    """The workgroup list of qgemm_kernel: (MT, NT, NG, R, c0, rem, grid, blocks); blocks[b] = (mt, ng) of block index b -- row tile
    mt, column group ng (column tiles ng * group .. below NT) -- or None where the block returns at once."""
    MT, NT = (M + bm - 1) // bm, N // bn
    NG = (NT + group - 1) // group
    R = MT * NG
    c0, rem = R >> 3, R & 7
    grid = 8 * ((R + 7) // 8)
    blocks = []
    for b in range(grid):
        xcd, local = b & 7, b >> 3
        if local >= c0 + (1 if xcd < rem else 0):
            blocks.append(None)
            continue
        gi = xcd * c0 + (xcd if xcd < rem else rem) + local
        ng = gi // MT
        blocks.append((gi - ng * MT, ng))
    return MT, NT, NG, R, c0, rem, grid, blocks


def q_launch(M, N, K, epi, n_split=0, ln=False, force=0, ncu=NCU256):
    """What launch_qgemm does with the problem on a device of ncu CUs (force: sgpt_ctx_set_query_tile): a QLaunch, or None where the
    entry answers "not served".  ln: the LayerNorm prologue (K = d)."""
    if ln:
        if not qgemm_ln_ok(M, N, K, epi, n_split, ncu):
            return None
        pl = q_plan_ln(M, N, K, epi, n_split, ncu, force)
        if pl is None:
            return None
        bm, bn, group, lds = pl
        kd = 128
        D = q_depth_rule(q_chunks(bm, bn, True, kd), (K // 128) % 6 == 0)
        cls = 6 if (K // 128) % 6 == 0 else 4
        lds_launch = (K // kd) * bm * kd * 2 + group * bn * 4 + 2 * bn * kd * 2          # qlaunch
        assert lds_launch == lds
    else:
        if not qgemm_shape_ok(M, N, K, epi, n_split, ncu):
            return None
        i = q_pick_plain(M, N, K, epi, n_split, ncu, force)
        if i < 0:
            return None
        bm, bn, kd = Q_TILES[i]
        cls = q_class(Q_TILES[i], False, K)
        D = q_depth_rule(q_chunks(bm, bn, False, kd), cls == 6)
        group, lds = 1, 2 * (bm + bn) * kd * 2
    return QLaunch(bm, bn, kd, D, cls, group, lds, *q_blocks(M, N, bm, bn, group))


# ---------------------------------------------------------------- shapes of tests/test_gpu_linear_query.py -----------------------
# Written for a device of NCU256 CUs (only `group` of the prologue cases depends on it: a forced tile does not).  tile: the forced
# candidate (sgpt_ctx_set_query_tile).  bm bn kd D: what the mirror must give.  group: column tiles per workgroup (prologue; 1 for
# the plain kernels).  edges, each checked by tests/test_gemm_ref.py:
#   ragged      M % bm != 0 (clamped loads, predicated stores)         one-tile    M < bm: the only row tile is ragged
#   one-group   K / kd == D: the re-arm loop never runs                 long-ring   K / kd == 2 D or 3 D
#   short-run   R = MT NG < 8: some XCDs have no workgroup              uneven-run  R = 8 c0 + rem, c0 >= 1, rem != 0
#   short-last  the last column group has fewer than `group` tiles      split-inside  n_split falls inside a column group
#   bias3       more than 1024 bias floats per workgroup (the third bias loop)
# tag: 'plain' | 'ln' (every forced prologue tile at d = 512 / 768 / 1024) | 'ln-group' (group > 1).
CaseQ = namedtuple("CaseQ", "name M N K n_split ln tile bm bn kd D group edges tag")

# forced tile, bm, bn, kd, depth class, D, K with one ring group (K / kd == D), a longer K (2 D or 3 D)
# (128x128: 8 chunks per stage, D = 2 whatever the class, and q_class answers 6 for every K it serves -- its class-4
#  instantiation is never launched: no row for it)
Q_PLAIN = (
    (1, 32, 16, 256, 6, 6, 1536, 3072), (1, 32, 16, 256, 4, 4, 1024, 2048),
    (2, 32, 32, 128, 6, 6, 768, 1536), (2, 32, 32, 128, 4, 4, 512, 1024),
    (3, 32, 64, 128, 6, 6, 768, 1536), (3, 32, 64, 128, 4, 4, 512, 1024),
    (4, 64, 32, 128, 6, 6, 768, 1536), (4, 64, 32, 128, 4, 4, 512, 1024),
    (5, 64, 64, 128, 6, 6, 768, 1536), (5, 64, 64, 128, 4, 4, 512, 1024),
    (6, 128, 64, 128, 6, 3, 384, 1152), (6, 128, 64, 128, 4, 2, 256, 512),
    (7, 128, 128, 128, 6, 2, 256, 768),
)
Q_ROWS = {32: (32, 96), 64: (96, 64), 128: (160, 64)}                # bm -> M: whole tiles; a whole and a ragged, one whole; ragged, one ragged
Q_COLS = {16: ((64, 32), (160, 96)), 32: ((64, 32), (288, 192)), 64: ((128, 64), (576, 384)), 128: ((256, 128), (1152, 768))}   # bn -> (N, n_split): 2 (bn 16: 4) and 9 (10) column tiles


def _plain_cases():
    out = []
    for k, bm, bn, kd, cls, D, k_one, k_long in Q_PLAIN:
        for K in (k_one, k_long):
            for M in Q_ROWS[bm]:
                for N, ns in Q_COLS[bn]:
                    MT, NT = -(-M // bm), N // bn
                    R = MT * NT
                    e = {"one-group" if K // kd == D else "long-ring"}
                    if M % bm:
                        e.add("ragged")
                    if M < bm:
                        e.add("one-tile")
                    if R < 8:
                        e.add("short-run")
                    elif R & 7:
                        e.add("uneven-run")
                    out.append(CaseQ(f"q{bm}x{bn}-c{cls}-{M}x{N}x{K}", M, N, K, ns, False, k, bm, bn, kd, D, 1, frozenset(e), "plain"))
    return out


def _ln(name, M, N, d, ns, tile, bm, bn, D, group, edges, tag="ln"):
    return CaseQ(name, M, N, d, ns, True, tile, bm, bn, 128, D, group, frozenset(edges.split()), tag)


def _ln_cases():
    out = []
    for d, six in ((512, False), (768, True), (1024, False)):
        for tile, (bm, bn) in enumerate(Q_LN_TILES, 1):
            if (bm, bn, d) == (64, 64, 1024):                        # 128 KiB of A panel + 32 KiB of ring + bias > 160 KiB: refused (Q_LN_REFUSED)
                continue
            D = 6 if six else 4                                       # 1 or 2 chunks per stage: the full depth of either class
            for M in ((32, 96) if bm == 32 else (96, 160)):
                R = -(-M // bm) * (192 // bn)
                e = ("one-group" if d // 128 == D else "long-ring") + (" ragged" if M % bm else "") + (" short-run" if R < 8 else " uneven-run" if R & 7 else "")
                out.append(_ln(f"ln{bm}x{bn}-d{d}-{M}", M, 192, d, 128, tile, bm, bn, D, 1, e))
    return out


CASESQ = _plain_cases() + _ln_cases() + [
    # two column tiles per workgroup, 34 groups, the last of one tile; q | k ends at tile 45 = the second tile of group 22
    _ln("lng-32x32-128x2144", 128, 2144, 768, 1440, 1, 32, 32, 6, 2, "one-group short-last split-inside", "ln-group"),
    # the same on the 64-row tile with a ragged last row tile: 3 x 87 tiles, 44 groups, q | k ends at tile 57 = the second of group 28
    _ln("lng-64x64-160x5568", 160, 5568, 768, 3648, 3, 64, 64, 6, 2, "one-group ragged short-last split-inside uneven-run", "ln-group"),
    # 17 column tiles = 1088 bias floats per workgroup; the second group has 16; q | k ends at tile 22, inside it
    _ln("lng-32x64-4096x2112", 4096, 2112, 512, 1408, 2, 32, 64, 4, 17, "one-group short-last split-inside bias3", "ln-group"),
]
Q_LN_REFUSED = (3, 96, 192, 1024, 128)                 # forced tile, M, N, d, n_split: 64x64 at d = 1024 needs more than 160 KiB of LDS


def launch_q(c, epi=None, ncu=NCU256):
    """q_launch of a CASESQ row (epi: EPI_QKV with the row's n_split by default for a prologue row, EPI_STORE for a plain one)."""
    if epi is None:
        epi = EPI_QKV if c.ln else EPI_STORE
    return q_launch(c.M, c.N, c.K, epi, c.n_split if epi == EPI_QKV else 0, c.ln, c.tile, ncu)



def case(name):
    return next(c for c in CASES + CASES256 + CASES256Q + CASESQ if c.name == name)


def case_k(c, dtype):
    if isinstance(c, (Case256, Case256Q, CaseQ)):
        return c.K
    return c.K32 if dtype == "fp32" else c.K16


def round_to(x, dtype):
    """x (float64 / float32 numpy) rounded once to the operand format; returns (torch tensor of that format, float64 numpy of the
    same values)."""
    import torch
    t = torch.from_numpy(np.asarray(x, np.float32)).to({"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}[dtype])
    return t, t.double().numpy()


def make_inputs(c, dtype, seed=0):
    """Operands of case c: a ~ U(-2, 2), w ~ U(-0.4, 0.4) rounded to the operand format, bias ~ U(-1, 1) and resid ~ U(-2, 2) in
    fp32.  Returns a dict of torch CPU tensors (a, w, bias, resid) and their float64 values (a64, w64, bias64, resid64).
    The scales keep a dropped 16-byte k-chunk far above the bound and an fp32 chain far below it (tests/test_gemm_ref.py)."""
    import torch
    K = case_k(c, dtype)
    rng = np.random.default_rng([seed, c.M, c.N, K])
    a, a64 = round_to(rng.uniform(-2, 2, size=(c.M, K)), dtype)
    w, w64 = round_to(rng.uniform(-0.4, 0.4, size=(c.N, K)), dtype)
    bias = torch.from_numpy(rng.uniform(-1, 1, size=c.N).astype(np.float32))
    resid = torch.from_numpy(rng.uniform(-2, 2, size=(c.M, c.N)).astype(np.float32))
    return dict(a=a, w=w, bias=bias, resid=resid, a64=a64, w64=w64, bias64=bias.double().numpy(), resid64=resid.double().numpy(), K=K)
