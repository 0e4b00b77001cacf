"""-m gpu: sgpt_lm_logprobs (csrc/encode.hip) -- the cross-encoder scorer behind crossencoder.loglikelihood_tokens and
GPTRanker.predict -- past one 1024-row chunk, against the float64 reference and the DERIVED bound of tests/lmhead_ref.py.

The entry takes `hidden` from the caller, so no forward pass is involved: one-layer models carry the LM head (GPT-Neo: tied to
wte.weight; GPT-J: lm_head.weight + lm_head.bias), and every row of `hidden` that no row_idx entry selects holds NaN.  What the
stand-alone tests of the GEMM (test_gpu_linear_edges.py) and of the log-softmax (test_gpu_rowops.py) cannot see and these can:
the gather, the chunk offsets of row_idx / targets / out, the leading dimension handed from the GEMM to the log-softmax, the
128x128 supertile leg and the one-row tail chunks at a large vocabulary, the bias of an untied head, and the reuse of the
context's workspace between chunks and calls.  tests/test_lmhead_ref.py shows on the CPU that the case table reaches those
legs and that seven defects of the chunk loop leave the bound by more than 4x.

Widths are 128 and 384: sgpt_model_load accepts d_model % 128 == 0 only, so no model of width 64 or 320 exists to carry a head.

Two kinds of operands.  EXACT (multiples of 2^-3 in [-1, 1]: every logit is exact in fp32 whatever the tile, k-step or order):
the result equals, bit for bit, ctx.logprob_rows on the logits built on the host, and does not depend on n, chunk position or
row order.  GAUSSIAN (logits of standard deviation 3): |lp - ref| <= 2 max_j E[i, j] + B[i], nothing measured.

RECORD -- 2026-10-21, MI355X, 46 passed in 4.5 s (every line of the run: profiles/lm_head_tests.txt).  No defect was found: every
exact run is bit-equal, every Gaussian run uses under 1 % of its bound (the gamma_n bound of an fp32 chain is far above what a
sum of 128 .. 384 products really loses; a wrong row is some 1000 bounds away).
worst error / bound, Gaussian operands (rows left out of the greedy comparison, per cent, after the slash):
  chunks n=1 0.002/0  n=5 0.001/0  n=1023 0.006/0.10  n=1024 0.006/0.10  n=2048 0.006/0.15  n=3109 0.008/0.10
  chunks n=1025  spans 0.005/0  reversed 0.005/0  random-small 0.006/0  random-large 0.006/0.10  repeat 0.003/0
  chunks n=2049  spans 0.007/0.10  reversed 0.007/0  random-small 0.007/0  random-large 0.005/0.05  repeat 0.004/0
  bias n=1025 0.002/0.59  n=2049 0.003/0.54      super n=1025 0.007/0      real n=1025 0.005/0      stale pad columns 0.002
worst error / B, exact operands (the log-softmax kernel alone, E = 0): 0.000 (n=1) .. 0.267 (bias n=2049)."""
import numpy as np
import pytest
import torch

import lmhead_ref as L
from oracle import sgpt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def report(what, ratio, left_out=None):
    tail = "" if left_out is None else f", rows left out of the greedy comparison = {100.0 * left_out:.2f} %"
    print(f"lmhead: {what}: worst error / bound = {ratio:.3f}{tail}")
    return ratio


# ---------------------------------------------------------------------------------------------------------------- models
_models = {}


def head_model(V, d, head, W, bias, ctx=None, key=None):
    """The smallest model the loader accepts (one layer, d_ffn 128, heads of 64) around the LM head (W, bias), fp32."""
    from sgpt_amd import SGPTConfig, SGPTModel
    if key is not None and key in _models:
        return _models[key]
    if head == "tied":
        kw = dict(vocab_size=V, max_position_embeddings=32, hidden_size=d, num_layers=1, num_heads=d // 64, intermediate_size=128,
                  window_size=8)
        w = dict(O.synth_weights(O.NeoConfig(**kw), seed=1, std=0.02))
        w["wte.weight"] = W
        cfg = SGPTConfig(**kw)
    else:
        kw = dict(vocab_size=V, n_positions=32, n_embd=d, n_layer=1, n_head=d // 64, rotary_dim=32, n_inner=128)
        w = dict(O.synth_weights_gptj(O.GPTJConfig(**kw), seed=1, std=0.02))
        w["lm_head.weight"], w["lm_head.bias"] = W, bias
        cfg = SGPTConfig.from_hf_dict(dict(kw, model_type="gptj"))
    m = SGPTModel(cfg, w, device=DEV, dtype="fp32", ctx=ctx)
    if key is not None:
        _models[key] = m
    return m


def model_of(ref):
    c = ref.case
    return head_model(c.V, c.d, c.head, ref.W, ref.bias, key=(c.V, c.d, c.head, ref.kind))


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def call(m, ref, sl=slice(None), greedy=True, hidden=None):
    hid = dev(ref.hidden) if hidden is None else hidden
    return m.lm_logprobs(hid, ref.row_idx[sl], ref.targets[sl], return_greedy=True) if greedy else (
        m.lm_logprobs(hid, ref.row_idx[sl], ref.targets[sl]), None)


RUNS = [(c.name, kind, pat) for c in L.CASES for kind, pat in L.runs(c)]
ids = lambda r: "-".join(r)     # noqa: E731


# ============================================================================================================ exact operands
@pytest.mark.parametrize("run", [r for r in RUNS if r[1] == "exact"], ids=ids)
def test_exact_operands_give_the_bits_of_logprob_rows_on_host_logits(run):
    """Every logit is exact in fp32, so gather + GEMM + bias + ldv + chunk offsets must reproduce ctx.logprob_rows on the logits
    matrix built on the host ([n, ldv], NaN behind column V) bit for bit -- log-probabilities and greedy tokens.  Greedy is
    exact too: it is the float64 argmax, and the LOWER of the two identical LM-head rows where they are the maximum.  The
    stand-alone kernel is tied to float64 elsewhere; here lp is also within its bound B of the float64 value (E = 0)."""
    ref = L.reference(*run)
    m, c = model_of(ref), ref.case
    lp, gr = call(m, ref)
    want_lp, want_gr = m.ctx.logprob_rows(dev(L.exact_logits(ref)), dev(ref.targets), V=c.V)
    assert torch.isfinite(lp).all(), "a NaN row of hidden, a pad column or a row of another chunk was read"
    assert torch.equal(lp, want_lp), f"{int((lp != want_lp).sum())} of {c.n} rows differ, first at {int((lp != want_lp).nonzero()[0])}"
    assert torch.equal(gr, want_gr)
    assert np.array_equal(gr.cpu().numpy(), ref.am)
    j1 = L.DUP[c.V][0]
    assert (ref.am == j1).sum() >= 1 and (gr.cpu().numpy()[ref.am == j1] == j1).all()
    assert report(f"{ids(run)} (B alone)", float((np.abs(lp.double().cpu().numpy() - ref.lp) / ref.B).max())) <= 1.0
    lp2, none = call(m, ref, greedy=False)                                     # out_greedy = NULL
    assert none is None and torch.equal(lp2, lp)


@pytest.mark.parametrize("name", ["chunks-n2049", "bias-n2049"])
def test_bits_do_not_depend_on_n_chunk_position_or_row_order(name):
    """Exact operands: the 2049-row call against the same rows in three calls (700 + 700 + 649: every row at another position of
    another chunk) and against one call with row_idx and targets permuted."""
    ref = L.reference(name, "exact", "spans")
    m, hid = model_of(ref), dev(ref.hidden)
    lp, gr = call(m, ref, hidden=hid)
    parts = [call(m, ref, sl=slice(a, b), hidden=hid) for a, b in ((0, 700), (700, 1400), (1400, 2049))]
    assert torch.equal(torch.cat([p[0] for p in parts]), lp) and torch.equal(torch.cat([p[1] for p in parts]), gr)
    perm = np.random.default_rng(5).permutation(ref.case.n)
    lp_p, gr_p = m.lm_logprobs(hid, ref.row_idx[perm], ref.targets[perm], return_greedy=True)
    assert torch.equal(lp_p, lp[dev(perm)]) and torch.equal(gr_p, gr[dev(perm)])


# ========================================================================================================= gaussian operands
@pytest.mark.parametrize("run", [r for r in RUNS if r[1] == "gauss"], ids=ids)
def test_gaussian_operands_against_float64_under_the_derived_bound(run):
    """|lp - ref| <= 2 max_j E[i, j] + B[i] (lmhead_ref.reference): E = gemm_ref.bound of an fp32 chain of any order, B the bound of
    the log-softmax kernel; a wrong row moves lp by O(1), hundreds of bounds.  Greedy equals the float64 argmax on every row whose
    float64 top-two gap exceeds 2 max_j E (at most 1 % of the rows fall out: test_lmhead_ref.py); on the others the chosen token's
    float64 logit is within 2 max_j E of the maximum."""
    ref = L.reference(*run)
    m = model_of(ref)
    lp, gr = call(m, ref)
    out = L.greedy_left_out(ref)
    assert out.mean() <= L.GREEDY_LEFT_OUT_MAX
    got = lp.cpu().numpy()
    assert np.isfinite(got).all(), "a NaN row of hidden, a pad column or a row of another chunk was read"
    ratio = np.abs(got.astype(np.float64) - ref.lp) / ref.bound
    assert report(ids(run), float(ratio.max()), float(out.mean())) <= 1.0, f"row {int(ratio.argmax())} of {ref.case.n}"
    g = gr.cpu().numpy().astype(np.int64)
    assert g.min() >= 0 and g.max() < ref.case.V
    assert np.array_equal(g[~out], ref.am[~out])
    if out.any():
        top = L.logit_at(ref.hidden, ref.row_idx, ref.W, ref.bias, ref.am)
        assert (top[out] - L.logit_at(ref.hidden, ref.row_idx, ref.W, ref.bias, g)[out] <= 2.0 * ref.E[out]).all()
    lp2, none = call(m, ref, greedy=False)
    assert none is None and torch.equal(lp2, lp)


def test_nothing_is_written_or_read_past_n():
    """The raw entry on buffers with 1024 guard entries behind n = 1025: the guard outputs keep their sentinel (the defect "tail
    chunk with the previous chunk's row count" of test_lmhead_ref.py writes there), the guard indices select a NaN row in range."""
    ref = L.reference("chunks-n1025", "gauss", "spans")
    m, n = model_of(ref), ref.case.n
    nan_row = int(np.flatnonzero(np.isnan(ref.hidden[:, 0]))[0])
    ri = dev(np.concatenate([ref.row_idx, np.full(L.CHUNK, nan_row, np.int32)]))
    tg = dev(np.concatenate([ref.targets, np.zeros(L.CHUNK, np.int32)]))
    out = torch.full((n + L.CHUNK,), float(L.SENTINEL), dtype=torch.float32, device=DEV)
    gr = torch.full((n + L.CHUNK,), -7, dtype=torch.int32, device=DEV)
    hid = dev(ref.hidden)
    st = m.ctx.lib.sgpt_lm_logprobs(m.handle, hid.data_ptr(), ri.data_ptr(), tg.data_ptr(), n, out.data_ptr(), gr.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == 0
    assert (out[n:] == float(L.SENTINEL)).all() and (gr[n:] == -7).all(), "entries behind n were written"
    assert L.worst_ratio(out.cpu().numpy()[:n], ref) <= 1.0


# ============================================================================================================ workspace reuse
@pytest.fixture()
def fresh_ctx():
    """A context of its own: its workspace starts empty, so the growth and the stale columns below are this test's doing."""
    from sgpt_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def test_workspace_growth_between_calls(fresh_ctx):
    """n = 5, n = 2049 (the workspace is freed and allocated again, larger), n = 5: the first and the third call return the same
    bits, and the second is right."""
    small, big = L.reference("chunks-n5", "gauss", "spans"), L.reference("chunks-n2049", "gauss", "spans")
    m = head_model(211, 128, "tied", small.W, None, ctx=fresh_ctx)
    try:
        a = call(m, small)
        b = call(m, big)
        c = call(m, small)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        assert L.worst_ratio(a[0].cpu().numpy(), small) <= 1.0 and L.worst_ratio(b[0].cpu().numpy(), big) <= 1.0
    finally:
        m.close()


def test_stale_pad_columns_of_the_logits_chunk(fresh_ctx):
    """The logits chunk lives in the context's workspace, so its pad columns [V, ldv) keep what the last call left there.  Two
    untied heads on one context with the same d and the same ldv = 260: vocab 260, whose bias puts 1e30 into columns 257 .. 259
    of every logits row, then vocab 257 with the same n -- by lmhead_ref.layout (pinned to the entry's three lines by
    test_lmhead_ref.py) every logits element has the same address in both calls, so the second call's pad columns hold 1e30.
    It must still equal its float64 reference, and no greedy token may be >= 257.  This check is only as strong as that layout:
    if the entry placed or sized its buffers otherwise, the second call might never see the first call's columns."""
    ref = L.reference("bias-n1025", "gauss", "spans")
    n, d = ref.case.n, ref.case.d
    assert L.layout(n, d, 260) == L.layout(n, d, 257)
    rng = np.random.default_rng(260)
    W260 = np.vstack([ref.W, (rng.standard_normal((3, d)) * (3.0 / np.sqrt(d))).astype(np.float32)])
    b260 = np.concatenate([ref.bias, np.full(3, 1e30, np.float32)])
    m260 = head_model(260, d, "bias", W260, b260, ctx=fresh_ctx)
    m257 = head_model(257, d, "bias", ref.W, ref.bias, ctx=fresh_ctx)
    try:
        hid = dev(ref.hidden)
        lp0, gr0 = m260.lm_logprobs(hid, ref.row_idx, ref.targets, return_greedy=True)
        assert (gr0 == 257).all(), "1e30 + logit is 1e30 in fp32 in all three columns: the first of them is the greedy token"
        assert torch.isfinite(lp0).all() and (lp0 < -1e29).all()
        lp, gr = m257.lm_logprobs(hid, ref.row_idx, ref.targets, return_greedy=True)
        assert int(gr.max()) < 257, "a stale pad column was read"
        assert report("stale pad columns, vocab 260 then 257", L.worst_ratio(lp.cpu().numpy(), ref)) <= 1.0
        out = L.greedy_left_out(ref)
        assert np.array_equal(gr.cpu().numpy()[~out], ref.am[~out])
    finally:
        m260.close(); m257.close()


# ================================================================================================================ end to end
def test_loglikelihood_tokens_with_more_than_1024_continuation_rows_in_one_call(monkeypatch):
    """crossencoder.loglikelihood_tokens on 150 requests of 8 .. 12 continuation tokens: one lm_logprobs call of more than 1024
    rows, against the oracle at the tolerance of test_crossencoder_* (relative 1e-3 over max(1, |want|)), and against the same
    requests scored with max_tokens_per_call = 512, where no call reaches 1024 rows."""
    from sgpt_amd import SGPTConfig, SGPTModel
    from sgpt_amd.crossencoder import loglikelihood_tokens
    kw = dict(vocab_size=211, max_position_embeddings=64, hidden_size=128, num_layers=2, num_heads=2, window_size=8)
    cfg = O.NeoConfig(**kw)
    w = O.synth_weights(cfg, seed=81, std=0.08)
    rng = np.random.default_rng(81)
    reqs = [(("c", "q"), rng.integers(0, 211, size=int(rng.integers(3, 14))).tolist(), rng.integers(0, 211, size=int(rng.integers(8, 13))).tolist())
            for _ in range(150)]
    want = np.asarray(O.loglikelihood_tokens(w, cfg, reqs, 48, 2))
    m = SGPTModel(SGPTConfig(**kw), w, device=DEV, dtype="fp32")
    rows_per_call = []
    inner = m.lm_logprobs
    monkeypatch.setattr(m, "lm_logprobs", lambda h, r, t, **k: (rows_per_call.append(len(r)), inner(h, r, t, **k))[1])
    try:
        got = np.asarray(loglikelihood_tokens(reqs, m, 48, instruction_len=2))
        assert rows_per_call == [sum(len(r[2]) for r in reqs)] and rows_per_call[0] > 1024
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-3
        del rows_per_call[:]
        small = np.asarray(loglikelihood_tokens(reqs, m, 48, instruction_len=2, max_tokens_per_call=512))
        assert len(rows_per_call) > 1 and max(rows_per_call) < 1024
        assert np.max(np.abs(small - got) / np.maximum(1.0, np.abs(want))) < 1e-3
    finally:
        m.close()


# ================================================================================================================== refusals
def test_lm_logprobs_refuses_bad_arguments_on_the_host():
    """SGPTModel.lm_logprobs looks at its arguments before it uploads them: each refusal names the argument, nothing is launched
    (the raw entry does not clamp row_idx and is never given an index out of range here)."""
    ref = L.reference("chunks-n5", "gauss", "spans")
    m = model_of(ref)
    hid = dev(ref.hidden)
    ri, tg, T = ref.row_idx.tolist(), ref.targets.tolist(), ref.T_pad
    bad = [
        ("hidden must be an fp32 tensor", lambda: m.lm_logprobs(hid.half(), ri, tg)),
        ("hidden must be an fp32 tensor", lambda: m.lm_logprobs(hid[0], ri, tg)),
        ("hidden must be an fp32 tensor", lambda: m.lm_logprobs(ref.hidden, ri, tg)),
        ("hidden is on cpu", lambda: m.lm_logprobs(hid.cpu(), ri, tg)),
        ("hidden has width 64, d_model is 128", lambda: m.lm_logprobs(hid[:, :64], ri, tg)),
        ("row_idx is empty", lambda: m.lm_logprobs(hid, [], [])),
        ("targets has 4 entries, row_idx 5", lambda: m.lm_logprobs(hid, ri, tg[:4])),
        (f"row_idx outside \\[0, {T}\\)", lambda: m.lm_logprobs(hid, ri[:4] + [T], tg)),
        (f"row_idx outside \\[0, {T}\\)", lambda: m.lm_logprobs(hid, [-1] + ri[1:], tg)),
    ]
    for msg, fn in bad:
        with pytest.raises(ValueError, match="lm_logprobs: " + msg):
            fn()
    assert m.lm_logprobs(hid, ri[:4] + [T - 1], tg).shape == (5,)              # the last row of hidden is in range
    assert L.worst_ratio(m.lm_logprobs(hid, np.asarray(ri, np.int64), torch.tensor(tg)).cpu().numpy(), ref) <= 1.0
