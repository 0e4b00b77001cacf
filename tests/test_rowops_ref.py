"""CPU: the float64 references of the GPU row-kernel tests (tests/rowops_ref.py) against independent implementations -- the
oracle's fp32 restatements of the reference code (layer_norm, pool, the rotary step of gptj_forward, log_softmax), torch in
float64, and the golden vectors the reference itself produced (tiny_left / tiny_right embeddings, the learntmean fixture of
extras.npz, the Pooling config pooling_weightedmean_128.json) -- and the error bounds against fp32 implementations on the CPU."""
import json
import os

import numpy as np
import pytest
import torch

import rowops_ref as R
from oracle import sgpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("d", R.LN_WIDTHS)
def test_layernorm_reference_and_the_fp32_unit(d, family):
    x, g, b = R.ln_inputs(9, d, family, seed=d)
    ref, mean, rstd = R.layernorm(x, g, b, 1e-5, stats=True)
    t64 = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (d,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-5)
    assert np.abs(ref - t64.numpy()).max() < 1e-12 * max(1.0, np.abs(ref).max())
    # two independent fp32 implementations sit inside the unit B the GPU test allows four of
    B = R.layernorm_unit(x, g, ref, mean, rstd)[:, None]
    t32 = torch.nn.functional.layer_norm(torch.from_numpy(x), (d,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert (np.abs(t32 - ref) / B).max() < 2.0
    assert (np.abs(O.layer_norm(x, g, b, 1e-5) - ref) / B).max() < 2.0
    # the bound is not slack by orders of magnitude either: fp32 really is a sizeable fraction of B away
    assert (np.abs(t32 - ref) / B).max() > 0.02


@pytest.mark.parametrize("fmt,dt", [("f16", torch.float16), ("bf16", torch.bfloat16)])
def test_ulp16_is_the_spacing_of_the_format(fmt, dt):
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(20000) * np.exp(rng.uniform(-12, 8, 20000))).astype(np.float32)
    v = np.concatenate([v, np.float32([1.0, 2.0, 0.5, 1.999, 2.0 ** -14, 2.0 ** -15, 3.0e-7])])
    err = np.abs(torch.from_numpy(v).to(dt).double().numpy() - v.astype(np.float64)) / R.ulp16(v, fmt)
    assert err.max() <= 0.5 and err.max() > 0.49
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -16], dtype=dt)
    nxt = torch.nextafter(t, torch.full_like(t, 100.0))
    assert np.array_equal((nxt.double() - t.double()).numpy(), R.ulp16(t.double().numpy(), fmt))


def oracle_modes(n_pw):
    return [("weightedmean", None), ("mean", None), ("lasttoken", None), ("learntmean", n_pw)]


@pytest.mark.parametrize("side", ["left", "right"])
def test_pool_reference_vs_oracle_padded_and_packed_forms(side):
    rng = np.random.default_rng(7)
    B, S, d = 6, 41, 24
    lens = [1, 2, 7, 33, 41, 16]
    h = rng.standard_normal((B, S, d)).astype(np.float32)
    mask = np.zeros((B, S), dtype=np.int64)
    for i, n in enumerate(lens):
        mask[i, (S - n if side == "left" else 0):(S if side == "left" else n)] = 1
    pw = rng.uniform(0.5, 1.5, S).astype(np.float32)
    rows, off, ln, pl = R.pack_padded(h, mask)
    assert (pl == ([S - n for n in lens] if side == "left" else [0] * B)).all()
    for mode, _ in oracle_modes(S):
        want = O.pool(h, mask, mode, position_weights=pw)                       # fp32 restatement of Pooling.py
        padded = R.pool_padded(h, mask, mode, pos_weights=pw)
        packed = R.lnf_pool(rows, off, ln, pl, mode, pos_weights=pw)
        assert np.abs(padded - want).max() < 2e-6 * np.abs(want).max() + 1e-6, mode
        assert np.abs(packed - padded).max() < 1e-13, mode
        for nrm in (False, True):
            a = R.lnf_pool(rows, off, ln, pl, mode, pos_weights=pw, normalize=nrm)
            b = R.pool_padded(h, mask, mode, pos_weights=pw, normalize=nrm)
            assert np.abs(a - b).max() < 1e-13
            if nrm:
                assert np.abs(a - O.normalize(want)).max() < 1e-5
    # the learntmean index clamp: a table shorter than the padded length repeats its last weight
    short = pw[:S - 9]
    ext = np.concatenate([short, np.full(9, short[-1], np.float32)])
    assert np.array_equal(R.lnf_pool(rows, off, ln, pl, "learntmean", pos_weights=short), R.lnf_pool(rows, off, ln, pl, "learntmean", pos_weights=ext))
    # the fused final LayerNorm = LayerNorm of every row, then the pooling
    g, b = rng.standard_normal(d).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    fused = R.lnf_pool(rows, off, ln, pl, "weightedmean", ln=(g, b, 1e-5))
    assert np.abs(fused - R.lnf_pool(R.layernorm(rows, g, b, 1e-5), off, ln, pl, "weightedmean")).max() < 1e-13
    assert np.abs(fused - O.pool(O.layer_norm(h, g, b, 1e-5), mask, "weightedmean")).max() < 1e-5
    # an empty sequence pools to zeros, and the rows between sequences are never read
    gap = np.full((rows.shape[0] + 5, d), np.nan, dtype=np.float32)
    gap[5:] = rows
    z = R.lnf_pool(gap, np.concatenate([off + 5, [0]]), np.concatenate([ln, [0]]), np.concatenate([pl, [3]]), "mean", normalize=True)
    assert np.isfinite(z).all() and (z[-1] == 0).all() and np.abs(z[:-1] - R.pool_padded(h, mask, "mean", normalize=True)).max() < 1e-13


@pytest.mark.parametrize("tag", ["tiny_left", "tiny_right"])
def test_pool_reference_vs_the_reference_codes_own_embeddings(tag):
    """emb_* of the golden files = the reference's Pooling.forward on HF hidden states, configured as
    pooling_weightedmean_128.json (the reference's own Pooling.save output) says."""
    cfg = json.load(open(os.path.join(GOLDEN, "pooling_weightedmean_128.json")))
    fx = np.load(os.path.join(GOLDEN, f"{tag}.npz"))
    h, mask = fx["last_hidden"], fx["mask"]
    assert cfg["pooling_mode_weightedmean_tokens"] and cfg["word_embedding_dimension"] == h.shape[2]
    rows, off, ln, pl = R.pack_padded(h, mask)
    assert (pl > 0).any() == (tag == "tiny_left")
    for mode in ("weightedmean", "mean", "lasttoken"):
        assert np.abs(R.lnf_pool(rows, off, ln, pl, mode) - fx[f"emb_{mode}"]).max() < 5e-6, mode
        assert np.abs(R.pool_padded(h, mask, mode) - fx[f"emb_{mode}"]).max() < 5e-6, mode


def test_learntmean_reference_vs_the_reference_codes_fixture():
    fx = np.load(os.path.join(GOLDEN, "extras.npz"))
    rows, off, ln, pl = R.pack_padded(fx["lm_hidden"], fx["lm_mask"])
    assert np.abs(R.lnf_pool(rows, off, ln, pl, "learntmean", pos_weights=fx["lm_pw"]) - fx["lm_ref"]).max() < 2e-6
    assert np.abs(R.pool_padded(fx["lm_hidden"], fx["lm_mask"], "learntmean", pos_weights=fx["lm_pw"]) - fx["lm_ref"]).max() < 2e-6


@pytest.mark.parametrize("H,dh,rot", [(2, 256, 64), (12, 64, 64), (4, 128, 32)])
def test_rope_reference_vs_the_oracles_rotary_step(H, dh, rot):
    from sgpt_amd.model import rotary_tables
    rng = np.random.default_rng(H + rot)
    S, max_pos, dm = 11, 64, H * dh
    sin, cos = rotary_tables(max_pos, rot)
    so, co = O.rotary_tables(max_pos, rot)
    assert np.array_equal(sin, so) and np.array_equal(cos, co)
    assert (sin[0] == 0).all() and (cos[0] == 1).all()
    buf = rng.standard_normal((S, 3 * dm)).astype(np.float32)
    pos = rng.permutation(max_pos)[:S]
    pos[:3] = [0, max_pos - 1, 5]
    got = R.rope(buf, pos, sin, cos, H, dh, rot, k_off=dm)
    # gptj_forward's lines: rot * cos + rotate_every_two(rot) * sin with the tables repeat-interleaved (HF:gptj:64-67,197-210)
    s2, c2 = np.repeat(sin[pos], 2, axis=1)[:, None, :].astype(np.float64), np.repeat(cos[pos], 2, axis=1)[:, None, :].astype(np.float64)
    want = buf.astype(np.float64).copy()
    for base in (0, dm):
        t = want[:, base:base + dm].reshape(S, H, dh).copy()
        r = t[..., :rot]
        t[..., :rot] = r * c2 + O._rotate_every_two(r) * s2
        want[:, base:base + dm] = t.reshape(S, dm)
    assert np.abs(got - want).max() < 1e-14
    assert np.array_equal(got[:, 2 * dm:], buf[:, 2 * dm:].astype(np.float64))          # V untouched
    assert np.array_equal(got[0], buf[0].astype(np.float64))                              # position 0: the identity
    assert not np.array_equal(got[1, :rot], buf[1, :rot].astype(np.float64))
    part = R.rope(buf, pos, sin, cos, H, dh, rot, k_off=dm, T=S - 1)
    assert np.array_equal(part[S - 1], buf[S - 1].astype(np.float64)) and np.array_equal(part[:S - 1], got[:S - 1])


def test_embed_reference_vs_the_oracles_first_line():
    cfg = O.NeoConfig(vocab_size=97, max_position_embeddings=40, hidden_size=32, num_layers=0, num_heads=2)
    w = O.synth_weights(cfg, seed=2)
    rng = np.random.default_rng(2)
    ids, pos = rng.integers(0, 97, 23), rng.integers(0, 40, 23)
    want = w["wte.weight"][ids] + w["wpe.weight"][pos]                                  # gptneo_forward, HF:gpt_neo:462-463
    assert np.array_equal(R.embed(ids, pos, w["wte.weight"], w["wpe.weight"]).astype(np.float32), want)
    assert np.array_equal(R.embed(ids, None, w["wte.weight"]), w["wte.weight"][ids].astype(np.float64))


def test_logprob_reference_vs_oracle_and_torch():
    rng = np.random.default_rng(5)
    n, V, ld = 9, 211, 256
    x = np.full((n, ld), np.nan, dtype=np.float32)
    x[:, :V] = rng.standard_normal((n, V)).astype(np.float32) * 3
    x[1, :V] = 0.25                                                                       # all equal: -log V, greedy 0
    x[2, [3, 67, 200]] = 20.0                                                             # duplicated maximum: the lowest index
    x[3, 5:9] = -np.inf
    x[4, :V] += np.float32(1e4)
    tg = rng.integers(0, V, n)
    tg[3] = 100
    lp, am = R.logprob_rows(x, V, tg)
    want = O.log_softmax(x[:, :V])
    assert np.abs(lp - want[np.arange(n), tg]).max() < 2e-5
    t64 = torch.log_softmax(torch.from_numpy(x[:, :V]).double(), dim=-1).numpy()
    assert np.abs(lp - t64[np.arange(n), tg]).max() < 1e-12
    untied = [0, 3, 4, 5, 6, 7, 8]
    assert np.array_equal(am[untied], torch.from_numpy(x[untied, :V]).double().argmax(dim=-1).numpy())
    assert abs(lp[1] + np.log(V)) < 1e-12 and am[1] == 0 and am[2] == 3
