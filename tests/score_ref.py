"""Test infrastructure of tests/test_gpu_score_f64.py (not a test module; checked without a GPU by tests/test_score_ref.py): the
scorer -- sgpt_scores, sgpt_score_topk over fp32 / bf16 / f16 rows -- in float64 numpy, its derived bound, operands whose sums are
exact, the table of shapes that reaches every scorer launch, and the checkers the GPU tests apply to what the kernels return.

Reference: the float64 product of the operands as stored (already rounded to the format), so the only error a kernel may show is that
of its fp32 accumulation.  A NaN score is -1 for sgpt_score_topk (EPI_SCORE: isnan(acc) ? -1 : acc) and stays NaN for sgpt_scores.
Bound: gemm_ref.bound(a, w, None, None, K) = (K + 4) 2^-23 |a| |w|^T, the gamma_n bound of an fp32 chain of any order; nothing
measured enters it.  Order: score8_ref.topk_lowest_index, value descending, ties to the lowest index.

Legs (the launches of csrc/score.hip::score_tile and of the filtered schedule, csrc/gemm.hip::launch_gemm16):
  A  nq <= 64 on a served width: launch_score64 over the whole 256-document tiles, the < 256 trailing documents on the register-staged
     kernel with the unpadded query rows
  B  256x256 LDS-DMA kernel, EPI_SCORE, padded query rows M < N = 768: documents streamed (deep_a false); tail as in A
  C  the same with M >= N: queries streamed (deep_a true)
  D  the second chunk of a two-chunk materialised pass: one 256x256 launch over na + 256 documents, GemmArgs.n_valid = nc
  E  register-staged throughout: 16-bit rows with d < 128 or d % 64 != 0, fp32 rows
  F  the filtered schedule (EPI_SCORE_FILTER, the EPI_SCORE_TOP2 sample, the fold of the last chunk, the 64-row tile's tail launch)
  G  sgpt_scores: EPI_STORE with an fp32 output on the register-staged tiles
With N <= 1024 and k = N the materialise-and-select path returns every score of the launch: legs A to E check every element."""
import functools
from collections import namedtuple

import numpy as np
import torch

import gemm_ref as G
import score8_ref as R8

BIG_BASE = 2 ** 33 + 5                                 # an idx_base no 32-bit index arithmetic survives
FILLER = 131072                                        # leg D: documents of the first chunk (ScorePlan.chunk)
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
F16 = ("f16", "bf16")

# ---------------------------------------------------------------- the table of legs ---------------------------------------------
# fmts: the operand formats the case runs in.  big: the exact run takes idx_base = BIG_BASE and the Gaussian run 0 (else the other
# way round).  plan: the fields of tests/score_plan_dump.cpp's line for (nq, N, d, k) that tests/test_score_ref.py asserts; `chunks`
# as [doc0, len, fold_tail, n_valid, tail_launch] lists.
Case = namedtuple("Case", "name leg nq N d k fmts big plan")


def _plan(fast, nq_pad, chunk, **kw):
    p = dict(fast=fast, nq_pad=nq_pad, filt=0, sampled=0, top2=0, chunk=chunk, first=0, chunks=[])
    p.update(kw)
    return p


def _topk_cases():
    out = []
    for i, (nq, d) in enumerate(((1, 128), (33, 192), (64, 320), (64, 768))):
        out.append(Case(f"A-nq{nq}-d{d}", "A", nq, 805, d, 805, F16, i % 2 == 1, _plan(1, 64, 808, rest=805)))
    for i, (nq, d) in enumerate((nq, d) for nq in (65, 256, 300) for d in (128, 192)):
        out.append(Case(f"B-nq{nq}-d{d}", "B", nq, 805, d, 805, F16, i % 2 == 0, _plan(1, 256 if nq <= 256 else 512, 808, rest=805)))
    out.append(Case("C-nq1000-d320", "C", 1000, 805, 320, 805, F16, True, _plan(1, 1024, 808, rest=805)))
    out.append(Case("D-nq100-nc549", "D", 100, FILLER + 549, 128, 549, F16, False, _plan(1, 256, FILLER, rest=FILLER + 549)))
    out.append(Case("D-nq300-nc805", "D", 300, FILLER + 805, 128, 805, F16, True, _plan(1, 512, FILLER, rest=FILLER + 805)))
    for i, d in enumerate((8, 72, 200)):
        out.append(Case(f"E-nq50-d{d}", "E", 50, 805, d, 805, F16, i % 2 == 0, _plan(0, 256, 808, rest=805)))
    for i, (nq, d) in enumerate(((1, 4), (50, 100), (130, 768))):
        out.append(Case(f"E-fp32-nq{nq}-d{d}", "E", nq, 805, d, 805, ("fp32",), i % 2 == 1, _plan(0, 256, 808, rest=805)))
    return out


CASES = _topk_cases()
CASES_F = [
    Case("F-nq2048-k10", "F", 2048, 32805, 128, 10, F16, False,
         _plan(1, 2048, 16384, filt=1, sampled=1, top2=1, rest=0, chunks=[[0, 32768, 1, 32805, 0]])),
    Case("F-nq2048-k100", "F", 2048, 32805, 128, 100, F16, True,
         _plan(1, 2048, 16384, filt=1, first=8192, rest=0, chunks=[[8192, 8192, 0, 0, 0], [16384, 16384, 1, 16421, 0]])),
    Case("F-nq16-k10", "F", 16, 262181, 128, 10, F16, True,
         _plan(1, 64, 131072, filt=1, sampled=1, rest=0, chunks=[[0, 262144, 0, 0, 1]])),
]
# leg G: sgpt_scores(a [na, d], b [nb, d]) -> fp32 [na, ldo]
CaseG = namedtuple("CaseG", "name na nb d fmts")
# (the last shape of either list: 25 x 25 = 625 tiles of 128x128 in the supertile order, ragged in M, N and K -- the smaller shapes all take 64x64 tiles)
CASES_G = ([CaseG(f"G-{na}x{nb}-d{d}", na, nb, d, F16) for na, nb, d in ((1, 5, 8), (50, 37, 72), (130, 257, 768), (300, 1000, 200), (3100, 3076, 72))]
           + [CaseG(f"G-fp32-{na}x{nb}-d{d}", na, nb, d, ("fp32",)) for na, nb, d in ((1, 5, 4), (50, 37, 100), (130, 257, 768), (3100, 3076, 36))])
# NaN variants: (case, format, NaN document rows (index within the checked documents: a whole tile, the tail), NaN query row or None)
NAN_VARIANTS = (("A-nq33-d192", "f16", (300, 790), None), ("B-nq65-d128", "bf16", (300, 790), None),
                ("D-nq100-nc549", "f16", (300, 530), None), ("B-nq300-d192", "f16", (), 7))


def case(name):
    return next(c for c in CASES + CASES_F + CASES_G if c.name == name)


def doc0_of(c):
    """The first document whose score a leg checks: leg D returns the documents behind the filler, every other leg all of them."""
    return FILLER if c.leg == "D" else 0


def idx_base_of(c, kind):
    return BIG_BASE if c.big == (kind == "exact") else 0


# ---------------------------------------------------------------- operands -------------------------------------------------------
# Exact operands.  v = 2 h + o: h the small-integer hash of gemm_ref.exact_codes (queries -4 .. 4, documents -6 .. 6: asymmetric), o = 1
# at ONE position of every aligned 8-element k-slice s -- position s % 4, so neighbouring slices differ and a 4-element fp32 slice has
# it too -- and 0 elsewhere.  Then
#   * every operand is an integer of magnitude <= 13 (leg D queries: <= 19): a bf16 and an f16 value;
#   * sum |q_i c_i| <= 768 * 9 * 13 < 2^17: every partial sum of every order is an exact fp32 integer, the float64 value bit for bit;
#   * the sum over a slice of q_i c_i is ODD (one odd x odd product, the others even): dropping or doubling the slice changes the score
#     of the row against every document by an odd number; a slice read from the neighbouring k offset pairs the odd element with an
#     even one -- an even slice sum instead of an odd one.  Never zero.
def _odd_mask(d):
    k = np.arange(d)
    return ((k % 8) == (k // 8) % 4).astype(np.int64)


def _sign_pattern(d):
    k = np.arange(d, dtype=np.uint64)
    return np.where(((k * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(1), 1, -1).astype(np.int64)


def exact_operands(nq, N, d, filler=0):
    """(q [nq, d], c [N, d]) int64.  filler > 0 (leg D): the queries carry + 10 u (u a fixed sign pattern: sign(q_i) = u_i, 1 <= |q_i| <= 19)
    and documents [0, filler) are - u m with 7 <= m <= 12 of the slice's parity: every product of a query with a filler row is
    negative, so a filler score is at most - 7 sum |q_i|."""
    hq, hc = G.exact_codes(nq, N, d)
    odd = _odd_mask(d)[None, :]
    q, c = 2 * hq + odd, 2 * hc + odd
    if filler:
        u = _sign_pattern(d)[None, :]
        q = q + 10 * u
        c[:filler] = -u * (8 + 2 * ((hc[:filler] + 6) % 3) - odd)
    return q, c


def gauss_operands(seed, nq, N, d, filler=0):
    """(q, c) fp32 torch: unit queries, unit rows around a common offset (score8_ref.unit_corpus).  filler > 0 (leg D): the queries
    carry + 4 u (u a unit vector), documents [0, filler) are - 4 u + e / 2 (e unit rows): by Cauchy-Schwarz a filler score is at most
    -16 + 4 + 1 / 2 + 2 = -9.5 and a signal score at least -5."""
    q, c = R8.unit_corpus(seed, N, d, nq)
    if filler:
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        u = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1)
        q = q + 4 * u
        c[:filler] = -4 * u + 0.5 * torch.nn.functional.normalize(torch.randn(filler, d, generator=g), dim=1)
    return q, c


def seed_of(c):
    return 7919 * "ABCDEFG".index(getattr(c, "leg", "G")) + (c.nq + c.d if hasattr(c, "nq") else c.na + c.nb + c.d)


def rounded(x, fmt):
    """x (integer / float numpy or an fp32 torch tensor) rounded once to the operand format: (torch tensor, float64 numpy)."""
    t = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, np.float32))).to(TORCH[fmt])
    return t, t.double().numpy()


@functools.lru_cache(maxsize=4)
def operands(name, fmt, kind):
    """(q, c, q64, c64) of a case: torch CPU tensors of the format and their float64 values.  kind 'exact' | 'gauss'."""
    c = case(name)
    nq, N = (c.na, c.nb) if isinstance(c, CaseG) else (c.nq, c.N)
    filler = FILLER if getattr(c, "leg", "") == "D" else 0
    q, rows = exact_operands(nq, N, c.d, filler) if kind == "exact" else gauss_operands(seed_of(c), nq, N, c.d, filler)
    (qt, q64), (ct, c64) = rounded(q, fmt), rounded(rows, fmt)
    return qt, ct, q64, c64


def with_nan(t, rows, col=5):
    """A copy of the operand tensor with a NaN in column `col` (the last one of a narrower row) of each of `rows`."""
    t = t.clone()
    for r in rows:
        t[r, min(col, t.shape[1] - 1)] = float("nan")
    return t


# ---------------------------------------------------------------- reference and bound --------------------------------------------
def scores64(q64, c64, nan_to_m1):
    """float64 scores [nq, N]; an operand row with a NaN gives NaN in its row / column, or -1 (sgpt_score_topk)."""
    bad = np.isnan(q64).any(axis=1)[:, None] | np.isnan(c64).any(axis=1)[None, :]
    s = np.nan_to_num(q64, nan=0.0) @ np.nan_to_num(c64, nan=0.0).T
    s[bad] = -1.0 if nan_to_m1 else np.nan
    return s


def bound(q64, c64):
    return G.bound(np.nan_to_num(q64, nan=0.0), np.nan_to_num(c64, nan=0.0), None, None, q64.shape[1])


def topk(scores, k, idx_base=0):
    return R8.topk_lowest_index(scores, k, idx_base)


# ---------------------------------------------------------------- checkers: what the GPU tests assert ----------------------------
# val fp32 [nq, k], idx int64 [nq, k] (numpy), n: what sgpt_score_topk returned.  ref, bnd: float64 [nq, nc] over the nc documents the
# leg checks, document j of them being index idx_base + doc0 + j.  Every comparison is written so that a NaN fails it.
def check_exact(val, idx, n, ref, k, first_idx):
    """Exact operands: values bit-equal to the float64 scores, indices in the lowest-index order, n == k."""
    wv, wi = topk(ref, k, first_idx)
    assert n == k, f"n = {n}, k = {k}"
    assert val.dtype == np.float32 and idx.dtype == np.int64
    assert np.array_equal(idx, wi), f"{int((idx != wi).sum())} indices differ from the lowest-index order"
    assert np.array_equal(val.astype(np.float64), wv), f"{int((val.astype(np.float64) != wv).sum())} values differ from the float64 scores"
    return 0.0


def check_bounded(val, idx, n, ref, bnd, k, first_idx):
    """Gaussian operands: every row a permutation of the documents, every value within the bound of its document's float64 score,
    values non-increasing with equal neighbours in ascending index order.  Returns the worst error / bound."""
    assert n == k == ref.shape[1], f"n = {n}, k = {k}, documents = {ref.shape[1]}"
    assert val.dtype == np.float32 and idx.dtype == np.int64
    rel = idx - first_idx
    assert np.array_equal(np.sort(rel, axis=1), np.broadcast_to(np.arange(k), rel.shape)), "a row is no permutation of the documents"
    v = val.astype(np.float64)
    err, lim = np.abs(v - np.take_along_axis(ref, rel, axis=1)), np.take_along_axis(bnd, rel, axis=1)
    ok = err <= lim
    assert ok.all(), f"{int((~ok).sum())} scores outside the bound, the worst at {float(np.nanmax(err / lim)):.3g} bounds"
    assert (v[:, 1:] <= v[:, :-1]).all(), "values increase along a row"
    tie = v[:, 1:] == v[:, :-1]
    assert (rel[:, 1:][tie] > rel[:, :-1][tie]).all(), "equal scores not in ascending index order"
    return float((err / np.where(lim > 0, lim, 1.0)).max())


SENT32 = 0x7FC12345                                    # gemm_gpu_util's fp32 sentinel


def check_scores(out_bits, nb, ref, bnd, exact):
    """Leg G.  out_bits: the int32 image [na, ldo] of the output rows, written over the sentinel.  Every element within the bound (exact
    operands: bit-equal), NaN exactly where the reference has it, the pad columns unwritten.  Returns the worst error / bound."""
    assert (out_bits[:, nb:] == SENT32).all(), "a store into the pad columns"
    body = np.ascontiguousarray(out_bits[:, :nb])
    assert (body != SENT32).all(), "an element of the output was left unwritten"
    got = body.view(np.float32).astype(np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN is not exactly in the rows / columns of the NaN operands"
    err = np.abs(got - ref)[~nan]
    if exact:
        assert (err == 0).all(), f"{int((err != 0).sum())} values differ from the float64 scores"
    assert (err <= bnd[~nan]).all(), f"{int((err > bnd[~nan]).sum())} scores outside the bound"
    return float((err / np.where(bnd[~nan] > 0, bnd[~nan], 1.0)).max()) if err.size else 0.0


# ---------------------------------------------------------------- leg F: the filtered schedule -----------------------------------
def filtered_reference(q64, c64, kmax, block=256):
    """(values, indices) [nq, kmax] of the float64 top-kmax in the lowest-index order, computed in blocks of query rows."""
    ct = torch.from_numpy(np.ascontiguousarray(c64.T))
    tv, ti = [], []
    for r0 in range(0, q64.shape[0], block):
        v, i = torch.topk(torch.from_numpy(q64[r0:r0 + block]) @ ct, kmax, dim=1)
        v, i = v.numpy(), i.numpy()
        order = np.lexsort((i, -v), axis=1)
        tv.append(np.take_along_axis(v, order, axis=1))
        ti.append(np.take_along_axis(i, order, axis=1))
    return np.concatenate(tv), np.concatenate(ti)


def pair_ref(q64, c64, idx, block=256):
    """(float64 score, bound) [nq, m] of query r against documents idx[r, :]."""
    K = q64.shape[1]
    s, a = np.empty(idx.shape), np.empty(idx.shape)
    for r0 in range(0, idx.shape[0], block):
        rows = c64[idx[r0:r0 + block]]
        s[r0:r0 + block] = np.einsum("rd,rmd->rm", q64[r0:r0 + block], rows)
        a[r0:r0 + block] = np.einsum("rd,rmd->rm", np.abs(q64[r0:r0 + block]), np.abs(rows))
    return s, (K + 4) * 2.0 ** -23 * a


def ambiguous_rows(q64, c64, top_v, top_i, k):
    """bool [nq]: the float64 k-th and (k + 1)-th scores differ by less than twice the larger of their bounds."""
    _, b = pair_ref(q64, c64, top_i[:, k - 1:k + 1])
    return top_v[:, k - 1] - top_v[:, k] < 2 * b.max(axis=1)


def check_filtered(val, idx, n, q64, c64, top_v, top_i, k, idx_base):
    """Every returned value within the bound of the float64 score of its index; the returned set of a non-ambiguous row is the float64
    top-k, an ambiguous row may swap documents whose float64 scores are closer than twice the larger bound (tests/test_gpu_score8.py).
    Returns (worst error / bound, share of ambiguous rows)."""
    assert n == k and val.shape == idx.shape == (q64.shape[0], k)
    got = idx - idx_base
    assert ((got >= 0) & (got < c64.shape[0])).all(), "an index outside the corpus"
    ref, lim = pair_ref(q64, c64, got)
    err = np.abs(val.astype(np.float64) - ref)
    assert (err <= lim).all(), f"{int((~(err <= lim)).sum())} scores outside the bound"
    amb = ambiguous_rows(q64, c64, top_v, top_i, k)
    for r in range(got.shape[0]):
        g, w = set(got[r].tolist()), set(top_i[r, :k].tolist())
        assert len(g) == k, f"row {r}: a document returned twice"
        if g == w:
            continue
        assert amb[r], f"row {r}: not the float64 top-{k}, and the row is not ambiguous"
        extra, missing = np.array(sorted(g - w)), np.array(sorted(w - g))
        (se, be), (sm, bm) = pair_ref(q64[r:r + 1], c64, extra[None, :]), pair_ref(q64[r:r + 1], c64, missing[None, :])
        close = np.abs(se[0][:, None] - sm[0][None, :]) < 2 * np.maximum(be[0][:, None], bm[0][None, :])
        assert close.all(), f"row {r}: a swap between scores further apart than twice the bound"
    return float((err / lim).max()), float(amb.mean())


def topical_corpus(seed, N, d, nq):
    """Leg F's operands, fp32 torch: N // 256 topics (unit centres); query r is a unit row 0.6 away from the centre of topic r % topics,
    document n a unit row of topic n % topics at cosine t ~ U(0, 0.9) to its centre.  A query's best ~256 documents are those of its
    topic, their scores spread over ~0.75: neighbours in the ranking lie ~3e-3 apart at every k, far above the bound (~1e-5), so few
    rows are ambiguous.  score8_ref.unit_corpus does not serve here: the scores of a query against rows around ONE offset are normal
    with sigma 0.04, the k-th and (k + 1)-th of 32 805 of them lie sigma / (k sqrt(2 ln(N / k))) ~ 1.2e-4 apart at k = 100, and 15 % of
    the rows are ambiguous whatever the seed (2 % at k = 10)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    nrm, topics = torch.nn.functional.normalize, N // 256
    centre = nrm(torch.randn(topics, d, generator=g), dim=1)
    q = nrm(centre[torch.arange(nq) % topics] + 0.6 * nrm(torch.randn(nq, d, generator=g), dim=1), dim=1)
    t = torch.rand(N, 1, generator=g) * 0.9
    c = nrm(t * centre[torch.arange(N) % topics] + (1 - t * t).sqrt() * nrm(torch.randn(N, d, generator=g), dim=1), dim=1)
    return q, c


F_SEED = 1                                             # tests/test_score_ref.py asserts the 5 % cap of ambiguous rows for it
F_KMAX = 101


@functools.lru_cache(maxsize=2)
def filtered_case(nq, N, d, fmt):
    """Operands and the float64 top-101 of the leg F cases of one shape and format (the k = 10 and k = 100 cases share them)."""
    q, c = topical_corpus(F_SEED, N, d, nq)
    (qt, q64), (ct, c64) = rounded(q, fmt), rounded(c, fmt)
    top_v, top_i = filtered_reference(q64, c64, F_KMAX)
    return qt, ct, q64, c64, top_v, top_i
