"""-m gpu: SGPTModel(attention="bidirectional") -- a Llama / Mistral / Qwen model after sgpt_model_set_attention(0) -- against HF
LlamaModel / Qwen2Model run without their causal mask (tests/golden/tiny_*_bidir.npz, recipe make_golden_bidir.py), with and without
pooling from token 3 on; isolation on the packed axis; the default path's bits; the refusals of the device path.

Bars: those tests/test_gpu_llama.py and tests/test_gpu_qwen.py hold the causal fixture of the same shape to -- fp32 1e-3 on every hidden
state and pooled vector; f16 1e-3 and bf16 8e-3 on the L2-normalised pooled vectors (max abs) and on their cosine matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import build_model, load_case, maxabs
from test_llama_bidir_ref import MODES, TAGS, load_bidir_case

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3
TOL_F16 = 1e-3
BAR16 = {"f16": TOL_F16, "bf16": 8 * TOL_F16}
# the causal fixture of each bidirectional one: same shape, same recipe family (its own seed)
CAUSAL_TWIN = {"tiny_llama_bidir": "tiny_llama", "tiny_llama_g4_bidir": "tiny_llama_g4", "tiny_llama_dh128_bidir": "tiny_llama_dh128",
               "tiny_qwen2_bidir": "tiny_qwen2"}

_models = {}


def bidir_model(tag, dtype):
    from sgpt_amd import SGPTModel
    if (tag, dtype) not in _models:
        fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
        _models[(tag, dtype)] = SGPTModel(cfg, w, device="cuda:0", dtype=dtype, attention="bidirectional")
    return _models[(tag, dtype)]


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def last_error(m) -> str:
    return (m.ctx.lib.sgpt_last_error(m.ctx.handle) or b"").decode()


class chains:
    """`with chains(m, n, min_rows):` -- the context's encode-chain setting for the block"""
    def __init__(self, m, n, min_rows):
        self.ctx, self.n, self.min_rows = m.ctx, n, min_rows

    def __enter__(self):
        self.old = self.ctx.set_encode_chains(self.n, self.min_rows)

    def __exit__(self, *exc):
        self.ctx.set_encode_chains(self.old, 0)


# ---- parity ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_bidirectional_forward_fp32_vs_hf_golden(tag):
    fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
    m = bidir_model(tag, "fp32")
    assert m.attention == "bidirectional"
    for sfx, kw in (("", {}), ("_from", dict(pool_from=int(fx["pool_from"])))):
        for mode in MODES:
            got = m.encode_ids(seqs, mode=mode, **kw).cpu().numpy()
            err = maxabs(got, fx[f"emb_{mode}{sfx}"])
            print(f"{tag} fp32 {mode}{sfx}: max|emb - ref| = {err:.3e}")
            assert np.isfinite(got).all() and err < TOL_FP32, (tag, mode, sfx)
            if sfx and mode != "lasttoken":
                assert not got[0].any(), "pool_from beyond a 1-token sequence: the empty range is a zero row"
    want = fx["hidden"]
    worst = 0.0
    for li in range(cfg.num_layers + 1):                         # hidden_states[li] per token, as HF numbers them
        hid = m.token_embeddings(seqs, layer_idx=li)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            e = maxabs(hid[i].cpu().numpy(), want[li, a:b])
            worst = max(worst, e)
            assert e < TOL_FP32, (tag, li, i)
    print(f"{tag} fp32 hidden states: max|h - ref| = {worst:.3e}")
    # with encode chains enabled the same encode gives the same bits (this family's blocks run as one chain: nothing is cut)
    base = m.encode_ids(seqs, mode="mean", pool_from=3)
    n0 = m.ctx.encode_chain_calls()
    with chains(m, 2, 32):
        assert torch.equal(m.encode_ids(seqs, mode="mean", pool_from=3), base)
    assert m.ctx.encode_chain_calls() == n0


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_bidirectional_forward_16bit_vs_hf_golden(tag, dtype):
    fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
    m = bidir_model(tag, dtype)
    bar = BAR16[dtype]
    for sfx, kw in (("", {}), ("_from", dict(pool_from=int(fx["pool_from"])))):
        for mode in MODES:
            got = m.encode_ids(seqs, mode=mode, **kw).cpu().numpy()
            ref = fx[f"emb_{mode}{sfx}"]
            assert np.isfinite(got).all()
            err = maxabs(_norm(got), _norm(ref))
            dcos = maxabs(_norm(got) @ _norm(got).T, _norm(ref) @ _norm(ref).T)
            print(f"{tag} {dtype} {mode}{sfx}: max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dcos:.3e} (bar {bar:.0e})")
            assert err < bar and dcos < bar, (tag, mode, sfx)
            gn = m.encode_ids(seqs, mode=mode, normalize=True, **kw).cpu().numpy()
            assert maxabs(gn, _norm(got)) < 1e-6
            if sfx and mode != "lasttoken":
                assert not got[0].any() and not gn[0].any()
    base = m.encode_ids(seqs, mode="weightedmean", pool_from=3)
    with chains(m, 2, 32):
        assert torch.equal(m.encode_ids(seqs, mode="weightedmean", pool_from=3), base)
    assert m.range_flags(reset=False) == 0


@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_every_hidden_state_pooled_from_a_token_on(dtype):
    """sgpt_encode_layers_pool_from: the L + 1 pooled hidden states over the rows behind token 3."""
    import llama_bidir_ref as B
    fx, hf, cfg, w, seqs, cuts = load_bidir_case("tiny_llama_bidir")
    m = bidir_model("tiny_llama_bidir", dtype)
    want = fx["hidden"].astype(np.float64)
    for mode in MODES:
        ref = np.stack([[B.pool_range(want[li, a:b], mode, 3) for a, b in zip(cuts[:-1], cuts[1:])] for li in range(cfg.num_layers + 1)])
        layers, mean = m.encode_packed_layers(m.pack(seqs, pool_from=3), mode=mode, per_layer=True)
        layers, mean = layers.cpu().numpy(), mean.cpu().numpy()
        if dtype == "fp32":
            assert maxabs(layers, ref) < TOL_FP32 and maxabs(mean, ref.mean(0)) < TOL_FP32
        else:
            for li in range(cfg.num_layers + 1):
                assert maxabs(_norm(layers[li]), _norm(ref[li])) < TOL_F16, (mode, li)
        assert torch.equal(m.encode_ids_all_layers(seqs, mode=mode, pool_from=3), torch.from_numpy(mean).cuda())


# ---- the default path keeps its bits ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp32", "f16", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_default_and_switched_back_models_keep_the_causal_bits(tag, dtype):
    """A default-constructed model reproduces the causal fixture of its shape at that fixture's bar, and a model switched 0 -> 1 gives the
    bits of a model on which set_attention was never called."""
    from sgpt_amd import SGPTModel
    from test_llama_ref import load_llama_case
    from test_qwen_ref import load_qwen_case
    twin = CAUSAL_TWIN[tag]
    fx, hf, cfg, w, seqs, cuts = (load_qwen_case if "qwen" in twin else load_llama_case)(twin)
    fresh = SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    assert fresh.attention == "causal"
    want = {mode: fresh.encode_ids(seqs, mode=mode) for mode in MODES}
    hid = fresh.token_embeddings(seqs)
    for mode in MODES:
        got, ref = want[mode].cpu().numpy(), fx[f"emb_{mode}"]
        if dtype == "fp32":
            assert maxabs(got, ref) < TOL_FP32
        else:
            assert maxabs(_norm(got), _norm(ref)) < BAR16[dtype]
    switched = SGPTModel(cfg, w, device="cuda:0", dtype=dtype, attention="bidirectional")
    moved = switched.encode_ids(seqs, mode="mean")
    assert not torch.equal(moved[1:], want["mean"][1:]), "the bidirectional mode computed the causal embeddings"
    assert torch.equal(moved[0], want["mean"][0])                 # one token: one key either way
    switched.set_attention("causal")
    assert switched.attention == "causal"
    for mode in MODES:
        assert torch.equal(switched.encode_ids(seqs, mode=mode), want[mode]), (tag, dtype, mode)
    for a, b in zip(switched.token_embeddings(seqs), hid):
        assert torch.equal(a, b)
    assert torch.equal(switched.encode_ids(seqs, mode="mean", pool_from=0), want["mean"])          # all-zero pool_lo: the old pool's bits
    fresh.close()
    switched.close()


# ---- isolation on the packed axis ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_bidirectional_sequences_do_not_see_their_neighbours(dtype):
    fx, hf, cfg, w, seqs, cuts = load_bidir_case("tiny_llama_g4_bidir")
    m = bidir_model("tiny_llama_g4_bidir", dtype)
    rng = np.random.default_rng(5)
    a = [seqs[1], seqs[3], seqs[2]]                               # 7 (an alignment row behind it), 70, 64 rows
    b = [seqs[1], rng.integers(3, 200, size=70).tolist(), seqs[2]]
    pa, pb = m.pack(a, pool_from=2), m.pack(b, pool_from=2)
    assert pa.off_host.tolist() == pb.off_host.tolist()
    ea, ha = m.encode_packed(pa, mode="weightedmean", return_hidden=True)
    eb, hb = m.encode_packed(pb, mode="weightedmean", return_hidden=True)
    off = pa.off_host.tolist()
    for i in (0, 2):
        assert torch.equal(ea[i], eb[i]) and torch.equal(ha[off[i]:off[i] + len(a[i])], hb[off[i]:off[i] + len(a[i])]), i
    assert not torch.equal(ea[1], eb[1])
    # and a sequence encoded alone equals its row of the batch
    for i, s in enumerate(a):
        assert torch.equal(m.encode_ids([s], mode="weightedmean", pool_from=2)[0], ea[i]), i


# ---- pool_from in a call that runs as two chains ---------------------------------------------------------------------------------------

def test_pool_from_is_offset_per_chain():
    """A GPT-Neo bulk call cut into two chains pools every sequence from its own pool_lo entry: the bits of the one-chain call."""
    fx, cfg_kw, *_ = load_case("cfg1_125m_32x64")
    m = build_model(cfg_kw, int(fx["seed"]), float(fx["std"]), "f16")
    rng = np.random.default_rng(41)
    seqs = [rng.integers(0, 50256, size=128).tolist() for _ in range(176)]
    pf = rng.integers(0, 140, size=176).tolist()
    pb = m.pack(seqs, pool_from=pf)
    assert pb.T_pad == 22528 and pb.pool_lo is not None
    n0 = m.ctx.encode_chain_calls()
    with chains(m, 2, 8704):
        on = m.encode_packed(pb, mode="weightedmean", normalize=True)
    assert m.ctx.encode_chain_calls() - n0 == 1
    with chains(m, 1, 8704):
        off = m.encode_packed(pb, mode="weightedmean", normalize=True)
        everything = m.encode_packed(m.pack(seqs), mode="weightedmean", normalize=True)
    assert torch.equal(on, off)
    emptied = [i for i, p in enumerate(pf) if p >= 128]
    assert emptied and all(not on[i].any() for i in emptied)
    assert not torch.equal(on[100:], everything[100:])             # the second chain's sequences did read their entries


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_device_path_refusals():
    from sgpt_amd import EncodeGraph, SGPTConfig, SGPTModel
    from sgpt_amd.model import synthetic_bert_weights, synthetic_weights
    from test_llama_ref import load_llama_case
    kw = dict(vocab_size=60, max_position_embeddings=64, hidden_size=128, num_layers=1, num_heads=2, intermediate_size=128)
    neo_cfg = SGPTConfig(window_size=8, **kw)
    neo = SGPTModel(neo_cfg, synthetic_weights(neo_cfg, seed=3), device="cuda:0", dtype="bf16", precision="plain")
    bert_cfg = SGPTConfig(model_type="bert", window_size=0, attention_layers=["global"], **kw)
    bert = SGPTModel(bert_cfg, synthetic_bert_weights(bert_cfg, seed=3), device="cuda:0", dtype="bf16")
    e = "sgpt_model_set_attention: the attention mode belongs to SGPT_ARCH_LLAMA models; %s"
    for m, why in ((neo, "SGPT_ARCH_GPTNEO stays causal"), (bert, "SGPT_ARCH_BERT is bidirectional by architecture")):
        for causal in (0, 1):
            assert m.ctx.lib.sgpt_model_set_attention(m.handle, causal) == -1 and last_error(m) == e % why
        with pytest.raises(ValueError, match="sgpt_model_set_attention"):
            m.set_attention("bidirectional")
    seqs = [[5, 6, 7, 8, 9], [10, 11]]
    want = neo.encode_ids(seqs, mode="mean")
    assert torch.isfinite(want).all() and neo.attention == "causal" and bert.attention == "bidirectional"
    # a Mistral descriptor that applies its window
    fx, hf, cfg, w, mseqs, cuts = load_llama_case("tiny_mistral_window")
    win = SGPTModel(cfg, w, device="cuda:0", dtype="f16")
    before = win.encode_ids(mseqs, mode="mean")
    assert win.ctx.lib.sgpt_model_set_attention(win.handle, 0) == -1
    assert last_error(win) == ("sgpt_model_set_attention: bidirectional attention with an applied sliding window (window 16 on a layer of "
                               "this model) is not built")
    assert win.ctx.lib.sgpt_model_set_attention(win.handle, 2) == -1 and last_error(win) == "sgpt_model_set_attention: causal 0 | 1"
    assert win.ctx.lib.sgpt_model_set_attention(win.handle, 1) == 0
    assert torch.equal(win.encode_ids(mseqs, mode="mean"), before), "a refused switch changed the model"
    with pytest.raises(ValueError, match="applied sliding window"):
        SGPTModel(cfg, w, device="cuda:0", dtype="f16", attention="bidirectional")
    # the library's own refusal of a range with cls / learntmean, whatever the Python host checked first
    pb = bert.pack(seqs, pool_from=1)
    o = torch.zeros((2, 128), device="cuda")
    for m, mode, msg in ((bert, 4, "not cls or learntmean"), (neo, 3, "not cls or learntmean")):
        st = m.ctx.lib.sgpt_encode_pool_from(m.handle, pb.ids.data_ptr(), pb.pos.data_ptr(), pb.seq_off.data_ptr(), pb.seq_len.data_ptr(),
                                             pb.pad_left.data_ptr(), pb.B, pb.T_pad, pb.max_alloc, mode, 1, 1, 0, o.data_ptr(), None, None,
                                             pb.pool_lo.data_ptr(), None)
        assert st == -1 and msg in last_error(m), last_error(m)
    with pytest.raises(ValueError, match="pool_from"):
        bert.encode_packed(pb, mode="cls")
    assert torch.isfinite(bert.encode_packed(pb, mode="mean")).all()
    # EncodeGraph: neither feature is captured
    bi = bidir_model("tiny_llama_bidir", "f16")
    with pytest.raises(ValueError, match="EncodeGraph: a model with attention='bidirectional' is not captured"):
        EncodeGraph(bi, [[5, 6, 7]])
    with pytest.raises(ValueError, match="EncodeGraph: pool_from is not captured"):
        EncodeGraph(neo, seqs, pool_from=1)
    g = EncodeGraph(neo, seqs, mode="mean")                        # what it did before, it still does
    assert torch.equal(g.replay(), want)
    del g
    for m in (neo, bert, win):
        m.close()
