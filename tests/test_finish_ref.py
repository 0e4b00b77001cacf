"""CPU: the float64 references of the embedding-finishing kernel tests (tests/finish_ref.py) against independent implementations
-- the oracle's fp32 restatements of the reference code (pool, normalize, pairwise_cos_sim, dot_score), torch in float64, torch's
own fp32 -> bf16 / f16 casts, and the golden vectors the reference itself produced (scoring.npz nrm / pcs, extras.npz lm_ref) --
and, for every shape and input family tests/test_gpu_finish.py runs, the fp32 emulation of the kernel's own summation order
inside the bound the GPU test asserts.  A bound the emulation breaks is wrong and is fixed here, never loosened on the GPU."""
import os

import numpy as np
import pytest
import torch

import finish_ref as F
from oracle import sgpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TORCH16 = {"bf16": torch.bfloat16, "f16": torch.float16}


ratio = F.ratio


def test_ratio_lets_nothing_non_finite_through():
    assert ratio([0.0, 1.0], [0.0, 2.0]) == 0.5 and ratio([0.0], [0.0]) == 0.0 and ratio([1e-30], [0.0]) == np.inf
    for bad in (np.nan, np.inf):
        assert ratio([0.0, bad], [1.0, 1.0]) == np.inf and ratio([0.0, 0.0], [1.0, bad]) == np.inf
    assert not max(0.0, ratio([np.nan], [1.0])) <= 1.0


# ================================================================================================== the references, pinned
@pytest.mark.parametrize("S", [1, 3, 33])
def test_pool_reference_vs_oracle_every_mask_kind(S):
    rng = np.random.default_rng(S)
    h = rng.standard_normal((6, S, 24)).astype(np.float32)
    mask = F.pool_masks(S)
    assert mask[0].all() and mask[1].sum() == 1 and mask[2, S - 1] == 1 and mask[2].sum() == 1 and not mask[5].any()
    if S >= 3:
        assert mask[3, 0] == 0 and mask[3, S - 1] == 0 and mask[3].any() and mask[4, 1] == 0 and mask[4, 2] == 1
    pw = rng.uniform(0.5, 1.5, S + 7).astype(np.float32)
    for mode in ("weightedmean", "mean", "learntmean"):
        want = O.pool(h, mask, mode, position_weights=pw)
        got = F.pool(h, mask, mode, pos_weights=pw)
        assert np.abs(got - want).max() < 2e-6 * np.abs(want).max() + 1e-6, mode
        assert (got[5] == 0).all() and (F.pool_bound(h, mask, mode, pw)[5] == 0).all()      # the all-zero mask: exact zeros
        assert np.array_equal(F.emulate_pool(h, mask, mode, pw)[5], np.zeros(24, np.float32))
    # lasttoken: the oracle's row, the all-zero mask giving row 0 (rowops_ref.pool_padded gives zeros there); cls: row 0
    assert np.array_equal(F.pool(h, mask, "lasttoken"), O.pool(h, mask, "lasttoken").astype(np.float64))
    assert np.array_equal(F.pool(h, mask, "lasttoken")[5], h[5, 0].astype(np.float64))
    assert np.array_equal(F.pool(h, mask, "lasttoken")[3], h[3, np.nonzero(mask[3])[0][-1]].astype(np.float64))
    assert np.array_equal(F.pool(h, mask, "cls"), h[:, 0].astype(np.float64))
    with pytest.raises(ValueError):
        F.pool(h, mask, "max")


def test_pool_reference_vs_the_reference_codes_learntmean_fixture():
    fx = np.load(os.path.join(GOLDEN, "extras.npz"))
    got = F.pool(fx["lm_hidden"], fx["lm_mask"], "learntmean", pos_weights=fx["lm_pw"])
    assert np.abs(got - fx["lm_ref"]).max() < 2e-6
    err = np.abs(F.emulate_pool(fx["lm_hidden"], fx["lm_mask"], "learntmean", fx["lm_pw"]) - got)
    assert ratio(err, F.pool_bound(fx["lm_hidden"], fx["lm_mask"], "learntmean", fx["lm_pw"])) <= 1.0


def test_l2_reference_vs_torch_oracle_and_the_fixture():
    for n, d, fam in [(5, 100, "plain"), (4, 65, "offset"), (5, 64, "huge"), (5, 772, "tiny"), (5, 3, "zero_row"), (4, 768, "clamp_row")]:
        x = F.l2_inputs(n, d, fam)
        ref = F.l2_normalize(x)
        t64 = torch.nn.functional.normalize(torch.from_numpy(x).double(), p=2, dim=1).numpy()
        assert np.abs(ref - t64).max() <= 1e-15 * max(1.0, np.abs(ref).max()), fam
        if fam not in ("tiny", "clamp_row"):                # the oracle squares in fp32: rows this small underflow there
            assert np.abs(ref - O.normalize(x)).max() < 1e-6, fam
    x = F.l2_inputs(5, 64, "zero_row")
    assert (F.l2_normalize(x)[-1] == 0).all() and (F.l2_bound(x)[-1] == 0).all()
    x = F.l2_inputs(5, 64, "clamp_row")
    assert abs(np.sqrt((x[-1].astype(np.float64) ** 2).sum()) - 2e-14) < 1e-20
    assert np.array_equal(F.l2_normalize(x)[-1], x[-1].astype(np.float64) / 1e-12)          # under the clamp: x / 1e-12
    fx = np.load(os.path.join(GOLDEN, "scoring.npz"))
    assert np.abs(F.l2_normalize(fx["a"]) - fx["nrm"]).max() < 1e-6


def test_pairwise_reference_vs_oracle_and_the_fixture():
    fx = np.load(os.path.join(GOLDEN, "scoring.npz"))
    a, b = fx["a"][:37], fx["b"]
    cos, _ = F.pairwise(a, b, cosine=True)
    dot, _ = F.pairwise(a, b, cosine=False)
    assert np.abs(cos - fx["pcs"]).max() < 1e-6
    assert np.abs(cos - O.pairwise_cos_sim(a, b)).max() < 1e-6
    assert np.abs(dot - np.diagonal(O.dot_score(a, b))).max() < 1e-4
    t = torch.nn.functional.cosine_similarity(torch.from_numpy(a).double(), torch.from_numpy(b).double(), dim=1).numpy()
    assert np.abs(cos - t).max() < 1e-14
    a, b, zeros = F.pairwise_inputs(5, 65)
    assert zeros == [1, 2, 3] and not a[1].any() and not b[2].any() and not a[3].any() and not b[3].any() and a[0].any()
    cos, cb = F.pairwise(a, b, cosine=True)
    assert (cos[zeros] == 0).all() and (cb[zeros] == 0).all() and 0 < abs(cos[4]) < 0.021       # the clamp row: a / 1e-12, small but there
    assert np.array_equal(F.emulate_pairwise(a, b, True)[zeros], np.zeros(3, np.float32))


# ========================================================================================================= 16-bit rounding
def torch_bits(x, fmt):
    return torch.from_numpy(x).to(TORCH16[fmt]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("fmt", F.FMTS16)
def test_round16_is_torchs_cast_bit_for_bit(fmt):
    rng = np.random.default_rng(16)
    rand_bits = rng.integers(0, 2 ** 32, 300000, dtype=np.uint64).astype(np.uint32).view(np.float32)     # every exponent, NaNs too
    near = (rng.standard_normal(100000) * np.exp2(rng.integers(-30, 18, 100000))).astype(np.float32)
    for x in (F.cvt_table(fmt), rand_bits, near) + tuple(F.cvt_inputs(n, fmt) for n in F.CVT_NUMEL[:4]):
        got, want = F.round16(x, fmt), torch_bits(x, fmt)
        assert F.same16(got, want, fmt)
        nan = np.isnan(x)
        assert np.array_equal(np.isnan(F.widen16(got, fmt)), nan)
        assert np.array_equal(got[~nan], want[~nan])
    v = F.widen16(np.arange(65536, dtype=np.uint16), fmt)                                   # every 16-bit value is a fixed point
    assert F.same16(F.round16(v, fmt), np.arange(65536, dtype=np.uint16), fmt)
    assert not F.same16(np.uint16([1, 2]), np.uint16([1, 3]), fmt) and not F.same16(np.uint16([F.NAN16[fmt]]), np.uint16([0]), fmt)
    assert F.same16(np.uint16([F.NAN16[fmt]]), np.uint16([F.NAN16[fmt] | 1 | 0x8000]), fmt)


def test_cvt_table_holds_the_edges():
    t = F.cvt_table("f16")
    r = dict(zip(t.tolist(), F.round16(t, "f16").tolist()))
    assert r[65504.0] == 0x7BFF and r[float(np.float32(65519.996))] == 0x7BFF and r[65520.0] == 0x7C00 and r[-65520.0] == 0xFC00
    assert r[2.0 ** -25] == 0 and r[float(np.float32(2.0 ** -25 * (1 + 2.0 ** -23)))] == 1 and r[2.0 ** -24] == 1      # tie to even: 0
    assert r[1.5 * 2.0 ** -24] == 2 and r[2.5 * 2.0 ** -24] == 2 and r[2.0 ** -14] == 0x0400                            # ties to even: 2, 2
    assert r[float(np.float32(2.0 ** -14 - 2.0 ** -25))] == 0x0400                                                      # rounds UP into the normals
    assert r[1.0 + 2.0 ** -11] == 0x3C00 and r[1.0 + 3 * 2.0 ** -11] == 0x3C02 and r[float(np.float32(1 + 2.0 ** -11 + 2.0 ** -23))] == 0x3C01
    t = F.cvt_table("bf16")
    b = dict(zip(t.view(np.uint32).tolist(), F.round16(t, "bf16").tolist()))
    assert b[0x7F7F0000] == 0x7F7F and b[0x7F7F7FFF] == 0x7F7F and b[0x7F7F8000] == 0x7F80 and b[0x7F7FFFFF] == 0x7F80
    assert b[0x00008000] == 0 and b[0x00008001] == 1 and b[0x00018000] == 2 and b[0x007FFFFF] == 0x0080 and b[0x80018000] == 0x8002
    assert b[0x3F808000] == 0x3F80 and b[0x3F818000] == 0x3F82 and b[0x3F808001] == 0x3F81
    assert (b[0x7F800001] & 0x7FFF) > 0x7F80 and (b[0xFF80FFFF] & 0x7FFF) > 0x7F80 and b[0xFF80FFFF] & 0x8000      # a NaN stays a NaN
    for fmt in F.FMTS16:
        t = F.cvt_table(fmt)
        assert t.dtype == np.float32 and t.shape[0] < 255 and np.isnan(t).sum() == 5 and np.isinf(t).sum() == 2
        sub = np.abs(t[np.isfinite(t)]) < 2.0 ** -126
        assert (sub & (t[np.isfinite(t)] != 0)).sum() >= 10                                  # fp32 subnormals are in it
        x = F.cvt_inputs(2097152 + 3, fmt)
        assert x.shape == (2097155,) and np.array_equal(x[:t.shape[0]].view(np.uint32), t.view(np.uint32)) and np.isnan(x[-1])


# ============================================================================================================ crest factor
@pytest.mark.parametrize("fmt", F.FMTS16)
def test_row_crest_reference(fmt):
    d = 64
    onehot = np.zeros((3, d), np.float32)
    onehot[1, 5] = -3.0
    assert F.row_crest(F.round16(onehot, fmt), fmt) == np.sqrt(d)                            # all the energy in one entry: sqrt(d)
    assert F.row_crest(F.round16(np.full((2, d), -0.75, np.float32), fmt), fmt) == 1.0       # a flat row: 1
    assert F.row_crest(F.crest_inputs(5, d, fmt, kind="zeros"), fmt) == 0.0 == F.emulate_row_crest(F.crest_inputs(5, d, fmt, kind="zeros"), fmt)
    bits = F.crest_inputs(5, d, fmt, pad=6)
    assert bits.shape == (5, d + 6) and (bits[:, d:] == F.NAN16[fmt]).all()
    v = torch.from_numpy(F.widen16(bits[:, :d], fmt)).double()
    assert not v[0].any() and torch.isinf(v[1]).any()
    per_row = v.abs().max(dim=1).values / (v * v).mean(dim=1).sqrt()
    assert float(per_row[2:].max()) == float(per_row[4])                                     # the spike row wins ...
    assert abs(F.row_crest(bits[:, :d], fmt) - float(per_row[4])) < 1e-12                    # ... rows 0 (zero) and 1 (inf) are skipped
    assert 6.0 < float(per_row[4]) <= 8.0
    only_bad = bits[:2, :d]
    assert F.row_crest(only_bad, fmt) == 0.0 == F.emulate_row_crest(only_bad, fmt)


# ============================================================ the emulations inside the bounds, on every input of the GPU file
@pytest.mark.parametrize("S", F.POOL_S)
@pytest.mark.parametrize("d", F.POOL_D)
def test_pool_emulation_is_inside_the_bound(d, S):
    worst = 0.0
    for fmt in F.POOL_FMTS:
        h, bits, mask, pw = F.pool_inputs(d, S, fmt)
        assert h.shape == (6, S, d) and pw.shape[0] > S and 0.5 <= pw.min() and pw.max() <= 1.5
        assert (np.abs(h[mask == 0]) >= 5e4).all() and np.isfinite(h).all()                 # large finite values sit under the mask
        if bits is not None:
            assert np.array_equal(F.round16(h, fmt), bits)                                   # h holds values of the format
        for mode in F.POOL_WEIGHTED:
            ref, bound = F.pool(h, mask, mode, pw), F.pool_bound(h, mask, mode, pw)
            assert np.isfinite(ref).all() and np.abs(ref).max() < 100.0                     # no trace of the masked values
            emu = F.emulate_pool(h, mask, mode, pw)
            assert not emu[5].any()
            worst = max(worst, ratio(np.abs(emu - ref), bound))
        for mode in ("lasttoken", "cls"):
            assert np.array_equal(F.emulate_pool(h, mask, mode).astype(np.float64), F.pool(h, mask, mode))
    print(f"finish: emulated pool d={d} S={S}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n", F.ROW_N)
@pytest.mark.parametrize("d", F.ROW_D)
def test_l2_emulation_is_inside_the_bound(d, n):
    worst = 0.0
    for fam in F.l2_families(d):
        x = F.l2_inputs(n, d, fam)
        assert np.isfinite(x).all() and np.isfinite(x.astype(np.float64) ** 2).all()
        ref, bound = F.l2_normalize(x), F.l2_bound(x)
        emu = F.emulate_l2(x)
        assert np.isfinite(emu).all()
        if fam == "zero_row":
            assert not emu[-1].any()
        worst = max(worst, ratio(np.abs(emu - ref), bound))
    print(f"finish: emulated l2 n={n} d={d}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n", F.ROW_N)
@pytest.mark.parametrize("d", F.ROW_D)
def test_pairwise_emulation_is_inside_the_bound(d, n):
    a, b, zeros = F.pairwise_inputs(n, d)
    for cosine in (False, True):
        ref, bound = F.pairwise(a, b, cosine)
        emu = F.emulate_pairwise(a, b, cosine)
        assert not emu[zeros].any()
        r = ratio(np.abs(emu - ref), bound)
        print(f"finish: emulated pairwise {'cos' if cosine else 'dot'} n={n} d={d}: worst error / bound = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("fmt", F.FMTS16)
@pytest.mark.parametrize("n", F.CREST_N)
@pytest.mark.parametrize("d", F.CREST_D)
def test_crest_emulation_is_inside_the_bound(d, n, fmt):
    for pad in (0, 6):
        bits = F.crest_inputs(n, d, fmt, pad=pad)[:, :d]
        ref = F.row_crest(bits, fmt)
        assert 1.0 <= ref <= np.sqrt(d) + 1e-9
        assert ratio(abs(F.emulate_row_crest(bits, fmt) - ref), F.crest_rel_bound(d) * ref) <= 1.0


def test_crest_of_fp32_rows_emulation_is_inside_the_bound_and_the_rounding_matters():
    """The fp32 input of the GPU file's Context.row_crest check: rounded to f16 first, then the crest."""
    x = F.crest_fp32_inputs()
    bits = F.round16(x, "f16")
    assert not np.array_equal(F.widen16(bits, "f16"), x)                                      # not f16 values
    ref, bound = F.row_crest(bits, "f16"), F.crest_rel_bound(130) * F.row_crest(bits, "f16")
    assert ratio(abs(F.emulate_row_crest(bits, "f16") - ref), bound) <= 1.0
    v = x.astype(np.float64)
    unrounded = (np.abs(v).max(axis=1) / np.sqrt((v * v).mean(axis=1))).max()
    assert 6.0 < ref < unrounded and ratio(abs(unrounded - ref), bound) > 100.0                # skipping the rounding is far outside


def test_a_wrong_kernel_is_outside_the_bounds():
    """What the bounds are for: the errors the GPU file must catch are far outside them."""
    x = F.l2_inputs(5, 100, "clamp_row")
    wrong = x / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)), 1e-6)           # clamp 1e-6
    assert ratio(np.abs(wrong - F.l2_normalize(x)), F.l2_bound(x)) > 1e3
    h, _, mask, pw = F.pool_inputs(64, 33, "f32")
    w = np.arange(33, dtype=np.float64)                                                                    # weight t instead of t + 1
    t0 = (w[:, None] * h[0].astype(np.float64)).sum(axis=0) / w.sum()
    assert ratio(np.abs(t0 - F.pool(h, mask, "weightedmean")[0]), F.pool_bound(h, mask, "weightedmean")[0]) > 1e3
    a, b, _ = F.pairwise_inputs(5, 100)
    ref, bound = F.pairwise(a, b, True)
    half = (F.l2_normalize(a) * b.astype(np.float64)).sum(axis=1)                                          # cosine dividing by |a| only
    assert ratio(np.abs(half - ref)[:1], bound[:1]) > 1e3
    x = np.float32([1.0 + 2.0 ** -8 + 2.0 ** -9])                                                                      # truncation instead of RNE
    assert F.round16(x, "bf16")[0] == 0x3F81 and (x.view(np.uint32) >> 16)[0] == 0x3F80
