"""CPU: the Llama / Mistral family's host side -- the float64 reference of tests/llama_ref.py against HF LlamaModel / MistralModel's
recorded values (tests/golden/tiny_llama*.npz, tiny_mistral_window.npz, recipe make_golden_llama.py), config parsing, state-dict
mapping, BOS / EOS framing, the rotary tables and the sliding_window rule.

Tolerance of the reference check, derived as tests/test_bert_ref.py derives its own.  The fixture is HF's fp32 forward, the
reference float64, so the difference is fp32 rounding alone (u = 2^-24); one fp32 row operation is held to 32 u |ref| against
float64 (tests/test_rowops_ref.py).  A block of this family chains NINE fp32 stages on every element -- RMSNorm-1, the Q | K | V
projection, the rotary rotation, softmax . V, out-projection + residual, RMSNorm-2, the gate | up projection, silu(gate) * up, the
down-projection + residual (the residual adds do not shrink an absolute error) -- and the final RMSNorm and the pooling are two
more: (9 L + 2) * 32 u * max|hidden|."""
import hashlib
import json
import os

import numpy as np
import pytest

import llama_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
TAGS = ["tiny_llama", "tiny_llama_dh128", "tiny_llama_g4", "tiny_mistral_window"]
MODES = ("mean", "weightedmean", "lasttoken")


def load_llama_case(tag):
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights
    fx = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    hf = json.loads(str(fx["cfg"]))
    cfg = SGPTConfig.from_hf_dict(hf)
    w = synthetic_llama_weights(cfg, seed=int(fx["seed"]))
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(fx["weights_sha256"]), "synthetic_llama_weights no longer produces the fixture's weights"
    lens = fx["seq_lens"].tolist()
    cuts = np.cumsum([0] + lens)
    seqs = [fx["ids"][a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    return fx, hf, cfg, w, seqs, cuts


_ref_cache = {}


def ref_forward(tag):
    """The float64 hidden states of a fixture's sequences, computed once per session and shared (read-only)."""
    if tag not in _ref_cache:
        fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
        _ref_cache[tag] = R.forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta,
                                    cfg.window_size)
    return _ref_cache[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_llama_ref_reproduces_hf(tag):
    fx, hf, cfg, w, seqs, cuts = load_llama_case(tag)
    L = cfg.num_layers
    assert [len(s) for s in seqs] == [1, 7, 64, 70, 130] and hf["max_position_embeddings"] == 160
    hs = ref_forward(tag)
    want = fx["hidden"].astype(np.float64)                       # [L + 1, rows, d]
    assert want.shape[0] == L + 1
    bound = (9 * L + 2) * 32 * U32 * float(np.abs(want).max())
    worst = 0.0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        worst = max(worst, float(np.abs(hs[i] - want[:, a:b]).max()))
        for mode in MODES:
            worst = max(worst, float(np.abs(R.pool(hs[i][-1], mode) - fx[f"emb_{mode}"][i]).max()))
    print(f"{tag}: max|llama_ref - HF| = {worst:.3e} (bound {bound:.3e})")
    assert worst < bound


def test_the_window_fixture_needs_its_window():
    """tiny_mistral_window: without the window (or with one key more) the reference leaves the recorded values by far more than rounding."""
    fx, hf, cfg, w, seqs, cuts = load_llama_case("tiny_mistral_window")
    assert cfg.window_size == 16 and set(cfg.attention_layers) == {"local"}
    want = fx["hidden"].astype(np.float64)[:, cuts[4]:cuts[5]]
    for window in (0, 17):
        got = R.forward(w, seqs[4:], cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, window)[0]
        assert np.abs(got - want).max() > 1e-3, window


LLAMA_CFG = dict(model_type="llama", vocab_size=32000, hidden_size=4096, num_hidden_layers=32, num_attention_heads=32,
                 num_key_value_heads=8, intermediate_size=14336, max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=500000.0,
                 hidden_act="silu", attention_bias=False, mlp_bias=False)


def test_config_accepts_llama_and_mistral_and_rejects_what_is_not_built():
    from sgpt_amd.model import SGPTConfig
    c = SGPTConfig.from_hf_dict(LLAMA_CFG)
    assert (c.model_type, c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.intermediate_size, c.vocab_size) == \
        ("llama", 4096, 32, 32, 8, 14336, 32000)
    assert c.layer_norm_epsilon == 1e-5 and c.rope_theta == 500000.0 and c.window_size == 0 and set(c.attention_layers) == {"global"}
    small = {k: v for k, v in LLAMA_CFG.items() if k not in ("num_key_value_heads", "rope_theta", "rms_norm_eps")}
    c = SGPTConfig.from_hf_dict(small)
    assert c.num_kv_heads == 32 and c.rope_theta == 10000.0 and c.layer_norm_epsilon == 1e-6          # HF's defaults
    assert SGPTConfig.from_hf_dict(dict(LLAMA_CFG, head_dim=128)).hidden_size == 4096
    assert SGPTConfig.from_hf_dict(dict(LLAMA_CFG, rope_scaling=None)).model_type == "llama"
    assert SGPTConfig.from_hf_dict(dict(LLAMA_CFG, rope_scaling={"rope_type": "default"})).model_type == "llama"
    for bad, key in ((dict(hidden_act="gelu"), "hidden_act"), (dict(attention_bias=True), "attention_bias"), (dict(mlp_bias=True), "mlp_bias"),
                     (dict(rope_scaling={"rope_type": "llama3", "factor": 8.0}), "rope_scaling"),
                     (dict(rope_scaling={"type": "linear", "factor": 2.0}), "rope_scaling"),
                     (dict(head_dim=64), "head_dim"), (dict(hidden_size=8192, num_attention_heads=64), "hidden_size")):
        with pytest.raises(NotImplementedError, match=key):
            SGPTConfig.from_hf_dict(dict(LLAMA_CFG, **bad))
    with pytest.raises(NotImplementedError):
        SGPTConfig.from_hf_dict(dict(LLAMA_CFG, model_type="roberta"))


def test_sliding_window_rule():
    """None or >= the maximum sequence length: no window; smaller: the window on every layer.  Llama ignores the key."""
    from sgpt_amd.model import SGPTConfig
    mistral = dict(LLAMA_CFG, model_type="mistral")
    for sw, want in ((None, 0), (4096, 0), (2048, 0), (2047, 2047), (16, 16)):
        c = SGPTConfig.from_hf_dict(dict(mistral, sliding_window=sw))
        assert c.model_type == "llama" and c.window_size == want, sw
        assert set(c.attention_layers) == ({"local"} if want else {"global"})
    assert SGPTConfig.from_hf_dict(dict(LLAMA_CFG, sliding_window=16)).window_size == 0
    # the longest sequence the library takes is 2048 tokens whatever the position table holds: Mistral-7B-v0.1 (window 4096 of 32768
    # positions) runs the no-window kernels; a config without the key carries HF MistralConfig's default of 4096
    long_ = dict(mistral, max_position_embeddings=32768)
    for sw, want in ((4096, 0), (2048, 0), (2047, 2047), (None, 0)):
        assert SGPTConfig.from_hf_dict(dict(long_, sliding_window=sw)).window_size == want, sw
    assert SGPTConfig.from_hf_dict(long_).window_size == 0
    assert SGPTConfig.from_hf_dict(dict(long_, max_position_embeddings=160)).window_size == 0          # default 4096 >= 160
    # the visibility rule of the existing window is HF's: key j visible to query i iff j <= i and j > i - window
    import attn_ref
    vis = attn_ref.visible(5, 2)
    assert vis.tolist() == [[j <= i and j > i - 2 for j in range(5)] for i in range(5)]


def test_llama_state_dict_mapping_prefix_fusion_and_lm_head():
    from sgpt_amd.model import SGPTConfig, llama_state_dict, synthetic_llama_weights
    cfg = SGPTConfig.from_hf_dict(dict(LLAMA_CFG, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                                       intermediate_size=384, vocab_size=50, max_position_embeddings=16))
    w = synthetic_llama_weights(cfg, seed=3)
    assert w["layers.0.self_attn.k_proj.weight"].shape == (64, 128) and w["layers.0.mlp.gate_proj.weight"].shape == (384, 128)
    plain = llama_state_dict(w)
    extra = {"lm_head.weight": np.zeros((50, 128), np.float32), "model.layers.0.self_attn.rotary_emb.inv_freq": np.zeros(32, np.float32)}
    prefixed = llama_state_dict({**{"model." + k: v for k, v in w.items()}, **extra})
    want = {"embed_tokens.weight", "norm.weight", "layers.0.input_layernorm.weight", "layers.0.post_attention_layernorm.weight",
            "layers.0.self_attn.qkv_proj.weight", "layers.0.self_attn.o_proj.weight", "layers.0.mlp.gate_up_proj.weight",
            "layers.0.mlp.down_proj.weight"}
    assert set(plain) == set(prefixed) == want
    p = "layers.0."
    for sd in (plain, prefixed):
        qkv = np.asarray(sd[p + "self_attn.qkv_proj.weight"])
        assert qkv.shape == (128 + 2 * 64, 128)
        assert np.array_equal(qkv, np.concatenate([w[p + f"self_attn.{n}_proj.weight"] for n in "qkv"]))        # q rows, k rows, v rows
        gu = np.asarray(sd[p + "mlp.gate_up_proj.weight"])
        assert np.array_equal(gu[:384], w[p + "mlp.gate_proj.weight"]) and np.array_equal(gu[384:], w[p + "mlp.up_proj.weight"])
        assert np.array_equal(np.asarray(sd["embed_tokens.weight"]), w["embed_tokens.weight"])
    with pytest.raises(NotImplementedError, match="bias"):
        llama_state_dict({**w, p + "self_attn.q_proj.bias": np.zeros(128, np.float32)})


@pytest.mark.parametrize("dh,theta", [(64, 10000.0), (128, 500000.0)])
def test_rotary_tables_against_hf_inv_freq(dh, theta):
    """inv_freq is HF's own (LlamaRotaryEmbedding, default rope) bit for bit; the tables are sin / cos of position * inv_freq in fp32."""
    import torch
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    from sgpt_amd.model import rotary_tables_half
    conf = LlamaConfig(hidden_size=2 * dh, num_attention_heads=2, num_hidden_layers=1, intermediate_size=128, vocab_size=10,
                       max_position_embeddings=160, rope_theta=theta)
    rot = LlamaRotaryEmbedding(conf)
    x = torch.zeros((1, 160, 2 * dh))
    cos, sin = rot(x, torch.arange(160)[None])
    s, c = rotary_tables_half(160, dh, theta)
    assert s.shape == c.shape == (160, dh // 2) and s.dtype == np.float32
    assert np.array_equal(c, cos[0, :, :dh // 2].numpy()) and np.array_equal(s, sin[0, :, :dh // 2].numpy())
    assert np.array_equal(cos[0, :, dh // 2:].numpy(), c)                                     # HF carries the half twice
    ref = np.arange(160)[:, None] * R.inv_freq(dh, theta)[None, :]
    assert np.abs(s - np.sin(ref)).max() < 160 * 2.0 ** -23 and np.abs(c - np.cos(ref)).max() < 160 * 2.0 ** -23   # fp32 angle: pos * 2^-24 relative


class _Tok:
    """Stub tokenizer: one id per whitespace word ('w7' -> 7 + 3)."""
    is_fast = False
    bos_token_id, eos_token_id = 1, 2

    def __init__(self, add_bos=True, add_eos=False):
        self.add_bos_token, self.add_eos_token = add_bos, add_eos

    def tokenize(self, txt):
        return txt.split()

    def convert_tokens_to_ids(self, toks):
        return [int(t[1:]) + 3 for t in toks]


def test_text_pipeline_frames_llama_inputs_after_truncation():
    from sgpt_amd.tokenization import TextPipeline
    short, long_ = "w0 w1 w2", " ".join(f"w{i}" for i in range(12))
    pipe = TextPipeline(_Tok(), 8, family="llama")                     # HF default: BOS, no EOS
    assert pipe.max_token_len == 7
    assert pipe.ids(short, True) == [1, 3, 4, 5] and pipe.batch([long_], False) == [[1] + list(range(3, 10))]
    assert pipe.docs_truncated == 1 and pipe.toks_truncated == 5
    both = TextPipeline(_Tok(add_eos=True), 8, family="llama")
    assert both.max_token_len == 6 and both.ids(long_, True) == [1] + list(range(3, 9)) + [2] and len(both.ids(long_, True)) == 8
    none = TextPipeline(_Tok(add_bos=False), 8, family="llama")
    assert none.max_token_len == 8 and none.ids(short, True) == [3, 4, 5]
    assert TextPipeline(_Tok(), 8).ids(short, True) == [3, 4, 5]                              # not a Llama model: untouched
    for kw in (dict(specb=True), dict(speca=True)):
        with pytest.raises(ValueError, match="Llama"):
            TextPipeline(_Tok(), 8, family="llama", **kw)
    t = _Tok()
    t.bos_token_id = None
    with pytest.raises(ValueError, match="bos_token_id"):
        TextPipeline(t, 8, family="llama")


def test_abi_constants_and_st_folder_round_trip(tmp_path):
    from sgpt_amd import _lib
    from sgpt_amd.formats import read_st_folder, write_st_folder
    assert _lib.SGPT_ARCH_LLAMA == 4 and _lib.ModelDesc._fields_[-1][0] == "n_kv_heads"
    for name in ("sgpt_rmsnorm", "sgpt_swiglu", "sgpt_rope_half", "sgpt_attention_gqa", "sgpt_lnf_pool_ex"):
        assert name in _lib.SIGNATURES
    p = str(tmp_path / "st")
    small = dict(LLAMA_CFG, model_type="mistral", hidden_size=128, num_attention_heads=2, num_key_value_heads=1, sliding_window=16)
    for mode in MODES:
        write_st_folder(p, small, {"embed_tokens.weight": np.zeros((4, 128), np.float32)}, pooling_mode=mode, max_seq_length=75)
        spec = read_st_folder(p)
        assert spec.pooling_mode == mode and spec.max_seq_length == 75
