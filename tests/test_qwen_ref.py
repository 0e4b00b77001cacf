"""CPU: the host side of the Qwen2 / Qwen3 members of the Llama family -- the float64 reference of tests/qwen_ref.py against HF
Qwen2Model / Qwen3Model's recorded values (tests/golden/tiny_qwen*.npz, recipe make_golden_qwen.py), config parsing with the head dim
that travels in `rotary_dim`, the state-dict mapping (fused QKV bias, head-norm gains), the refusals, the explicit `frame` of
TextPipeline, and the CPU emulation that shows the 16-bit bars of tests/test_gpu_qwen.py to be attainable.

Tolerance of the reference check: the one tests/test_llama_ref.py derives for its own float64 forward, (9 L + 2) * 32 u * max|hidden|.
(The head norm is a tenth fp32 stage per block in two of the three models; the bound is kept as it is -- the smaller one.)"""
import hashlib
import json
import os

import numpy as np
import pytest

import qwen_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
TAGS = ["tiny_qwen2", "tiny_qwen3", "tiny_qwen3_dh64"]
MODES = ("mean", "weightedmean", "lasttoken")
TOL_F16 = 1e-3                         # the bars of tests/test_gpu_qwen.py (= tests/test_gpu_llama.py): f16 1e-3, bf16 8 x that
BAR16 = {"f16": TOL_F16, "bf16": 8 * TOL_F16}


def load_qwen_case(tag):
    from sgpt_amd.model import SGPTConfig, synthetic_qwen_weights
    fx = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    hf = json.loads(str(fx["cfg"]))
    cfg = SGPTConfig.from_hf_dict(hf)
    w = synthetic_qwen_weights(cfg, seed=int(fx["seed"]), qkv_bias=bool(fx["qkv_bias"]), qk_norm=bool(fx["qk_norm"]))
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(fx["weights_sha256"]), "synthetic_qwen_weights no longer produces the fixture's weights"
    lens = fx["seq_lens"].tolist()
    cuts = np.cumsum([0] + lens)
    seqs = [fx["ids"][a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    return fx, hf, cfg, w, seqs, cuts


_ref_cache = {}


def ref_forward(tag, fmt=None):
    """The float64 hidden states of a fixture's sequences (fmt 'bf16' | 'f16': with the 16-bit forward's store points rounded), computed
    once per session and shared (read-only)."""
    from sgpt_amd.families import head_dim
    if (tag, fmt) not in _ref_cache:
        fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
        _ref_cache[(tag, fmt)] = Q.forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta,
                                           cfg.window_size, head_dim=head_dim(cfg), rnd=Q.round16(fmt) if fmt else None)
    return _ref_cache[(tag, fmt)]


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


@pytest.mark.parametrize("tag", TAGS)
def test_qwen_ref_reproduces_hf(tag):
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    L = cfg.num_layers
    assert [len(s) for s in seqs] == [1, 7, 64, 70, 130] and hf["max_position_embeddings"] == 160 and hf["vocab_size"] == 200 and L == 2
    hs = ref_forward(tag)
    want = fx["hidden"].astype(np.float64)                       # [L + 1, rows, d]
    assert want.shape[0] == L + 1
    bound = (9 * L + 2) * 32 * U32 * float(np.abs(want).max())
    worst = 0.0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        worst = max(worst, float(np.abs(hs[i] - want[:, a:b]).max()))
        for mode in MODES:
            worst = max(worst, float(np.abs(Q.pool(hs[i][-1], mode) - fx[f"emb_{mode}"][i]).max()))
    print(f"{tag}: max|qwen_ref - HF| = {worst:.3e} (bound {bound:.3e})")
    assert worst < bound


@pytest.mark.parametrize("tag", TAGS)
def test_the_fixture_needs_what_its_model_adds(tag):
    """Without the bias, or without the head norm, the reference leaves the recorded values by far more than rounding."""
    from sgpt_amd.families import head_dim
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    drop = ("_proj.bias",) if tag == "tiny_qwen2" else ("q_norm.weight", "k_norm.weight")
    less = {k: v for k, v in w.items() if not k.endswith(drop)}
    assert len(less) < len(w)
    got = Q.forward(less, seqs[1:2], cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, 0,
                    head_dim=head_dim(cfg))[0]
    assert np.abs(got - fx["hidden"].astype(np.float64)[:, cuts[1]:cuts[2]]).max() > 1e-2


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_cpu_emulation_of_the_16bit_forward_fits_half_the_gpu_bar(tag, fmt):
    """tests/qwen_ref.py with every value the 16-bit forward stores rounded to the format (and the matmul weights, which it holds in the
    format), under the metric of test_gpu_qwen.py's 16-bit test: max abs of the L2-normalised pooled embeddings and of their cosine
    matrix against the HF recording.  At most half the bar: the bars are attainable with the fixtures' norm-gain spread (0.1) and bias
    std (0.1) as the recipe has them."""
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    hs = ref_forward(tag, fmt)
    for mode in MODES:
        got = np.stack([Q.pool(h[-1], mode) for h in hs])
        ref = fx[f"emb_{mode}"]
        err = float(np.abs(_norm(got) - _norm(ref)).max())
        dcos = float(np.abs(_norm(got) @ _norm(got).T - _norm(ref) @ _norm(ref).T).max())
        print(f"{tag} {fmt} {mode} (emulated): max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dcos:.3e}, bar {BAR16[fmt]:.0e}")
        assert err <= BAR16[fmt] / 2 and dcos <= BAR16[fmt] / 2, (tag, fmt, mode)


# ---- config parsing, the head dim in rotary_dim ------------------------------------------------------------------------------

QWEN3_CFG = dict(model_type="qwen3", vocab_size=151669, hidden_size=1024, num_hidden_layers=28, num_attention_heads=16,
                 num_key_value_heads=8, head_dim=128, intermediate_size=3072, max_position_embeddings=32768, rms_norm_eps=1e-6,
                 rope_theta=1000000, hidden_act="silu", attention_bias=False, use_sliding_window=False, sliding_window=None,
                 rope_scaling=None, tie_word_embeddings=True)                                    # Qwen3-Embedding-0.6B
QWEN2_CFG = dict(model_type="qwen2", vocab_size=151646, hidden_size=1536, num_hidden_layers=28, num_attention_heads=12,
                 num_key_value_heads=2, intermediate_size=8960, max_position_embeddings=131072, rope_theta=1000000.0,
                 hidden_act="silu", use_sliding_window=False, sliding_window=131072, max_window_layers=21)   # gte-Qwen2-1.5B-instruct


def test_config_parses_qwen_and_the_head_dim_travels_in_rotary_dim():
    from sgpt_amd import _lib
    from sgpt_amd.families import head_dim
    from sgpt_amd.model import SGPTConfig, model_desc
    c = SGPTConfig.from_hf_dict(QWEN3_CFG)
    assert (c.model_type, c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.intermediate_size, c.vocab_size) == \
        ("llama", 1024, 28, 16, 8, 3072, 151669)
    assert c.rotary_dim == 128 and head_dim(c) == 128 and c.num_heads * head_dim(c) == 2048 != c.hidden_size
    assert c.layer_norm_epsilon == 1e-6 and c.rope_theta == 1e6 and c.window_size == 0 and set(c.attention_layers) == {"global"}
    desc, _local = model_desc(c, "f16", False, "plain")
    assert desc.arch == _lib.SGPT_ARCH_LLAMA and desc.rotary_dim == 128 and desc.n_kv_heads == 8 and desc.d_model == 1024
    assert desc.attn_scale == np.float32(1.0) / np.sqrt(np.float32(128))
    # without the field: 0 in the config, d / H in the descriptor -- what every Llama model has always sent
    c2 = SGPTConfig.from_hf_dict(QWEN2_CFG)
    assert c2.rotary_dim == 0 and head_dim(c2) == 128 and c2.layer_norm_epsilon == 1e-6 and c2.num_kv_heads == 2
    desc2, _local = model_desc(c2, "bf16", False, "plain")
    assert desc2.rotary_dim == 128 and desc2.n_kv_heads == 2
    # a head_dim that is d / H anyway is carried all the same ("only when the config gives one")
    c3 = SGPTConfig.from_hf_dict(dict(QWEN3_CFG, hidden_size=2048))
    assert c3.rotary_dim == 128 and head_dim(c3) == 128
    assert SGPTConfig.from_hf_dict(dict(QWEN3_CFG, rope_scaling={"rope_type": "default"})).rotary_dim == 128
    # Llama / Mistral keep 0
    from test_llama_ref import LLAMA_CFG
    assert SGPTConfig.from_hf_dict(dict(LLAMA_CFG, head_dim=128)).rotary_dim == 0


def test_refusals_by_type_and_text():
    from sgpt_amd.model import SGPTConfig
    from test_llama_ref import LLAMA_CFG
    cases = [
        (dict(QWEN3_CFG, use_sliding_window=True), "qwen3: use_sliding_window = true (the per-layer window of the Qwen models is not built)"),
        (dict(QWEN2_CFG, use_sliding_window=True), "qwen2: use_sliding_window = true (the per-layer window of the Qwen models is not built)"),
        (dict(QWEN3_CFG, attention_bias=True), "qwen3: attention_bias = true (the biased variants are not built)"),
        (dict(QWEN3_CFG, rope_scaling={"rope_type": "yarn", "factor": 4.0}),
         "qwen3: rope_scaling {'rope_type': 'yarn', 'factor': 4.0} (only the default rotary frequencies are built)"),
        (dict(QWEN2_CFG, hidden_act="gelu"), "qwen2: hidden_act 'gelu' (only 'silu', the SwiGLU MLP, is built)"),
        (dict(QWEN3_CFG, hidden_size=5120), "qwen3: hidden_size 5120 > 4096 (the row kernels hold one row of at most 4096 columns per wave)"),
        (dict(QWEN3_CFG, head_dim=96), "qwen3: head_dim 96 (the attention and the head norm of this family are built for 64 and 128)"),
        (dict(QWEN2_CFG, hidden_size=1280, num_attention_heads=16),
         "qwen2: head_dim 80 (the attention and the head norm of this family are built for 64 and 128)"),
        # pinned Llama behaviour: a biased Llama is still refused, and so is a head_dim of its own
        (dict(LLAMA_CFG, attention_bias=True), "llama: attention_bias = true (the biased variants are not built)"),
        (dict(LLAMA_CFG, model_type="mistral", attention_bias=True), "mistral: attention_bias = true (the biased variants are not built)"),
        (dict(LLAMA_CFG, head_dim=64), "llama: head_dim 64 with head_dim * num_attention_heads != hidden_size 4096"),
    ]
    for hf, text in cases:
        with pytest.raises(NotImplementedError) as e:
            SGPTConfig.from_hf_dict(hf)
        assert str(e.value) == text
    with pytest.raises(NotImplementedError) as e:
        SGPTConfig.from_hf_dict(dict(QWEN3_CFG, model_type="qwen3_moe"))
    assert str(e.value) == "model_type 'qwen3_moe': GPT-Neo, GPT-J, BLOOM, BERT and Llama / Mistral are the families built here"


# ---- state dict -> tensor list ----------------------------------------------------------------------------------------------

def _tensor_list(tag):
    from sgpt_amd.model import load_tensors
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    return [(n, tuple(t.shape)) for n, t in load_tensors(cfg, w)], w


def _layer(i, d, dq, dkv, ffn, dh, bias, norm):
    p = f"layers.{i}."
    out = [(p + "input_layernorm.weight", (d,)), (p + "self_attn.qkv_proj.weight", (dq + 2 * dkv, d))]
    if bias:
        out.append((p + "self_attn.qkv_proj.bias", (dq + 2 * dkv,)))
    if norm:
        out += [(p + "self_attn.q_norm.weight", (dh,)), (p + "self_attn.k_norm.weight", (dh,))]
    return out + [(p + "self_attn.o_proj.weight", (d, dq)), (p + "post_attention_layernorm.weight", (d,)),
                  (p + "mlp.gate_up_proj.weight", (2 * ffn, d)), (p + "mlp.down_proj.weight", (d, ffn))]


@pytest.mark.parametrize("tag,d,dq,dkv,ffn,dh,bias,norm", [("tiny_qwen2", 128, 128, 64, 256, 64, True, False),
                                                           ("tiny_qwen3", 128, 256, 128, 256, 128, False, True),
                                                           ("tiny_qwen3_dh64", 256, 128, 128, 384, 64, False, True)])
def test_ordered_tensor_list(tag, d, dq, dkv, ffn, dh, bias, norm):
    got, w = _tensor_list(tag)
    want = [("embed_tokens.weight", (200, d))] + _layer(0, d, dq, dkv, ffn, dh, bias, norm) + _layer(1, d, dq, dkv, ffn, dh, bias, norm) + \
        [("norm.weight", (d,)), ("rotary.sin", (160, dh // 2)), ("rotary.cos", (160, dh // 2))]
    assert got == want


def test_state_dict_fuses_the_qkv_bias_and_refuses_the_other_biases():
    from sgpt_amd.model import llama_state_dict
    fx, hf, cfg, w, seqs, cuts = load_qwen_case("tiny_qwen2")
    p = "layers.1.self_attn."
    plain = llama_state_dict(w)
    prefixed = llama_state_dict({**{"model." + k: v for k, v in w.items()}, "lm_head.weight": np.zeros((200, 128), np.float32)})
    assert list(plain) == list(prefixed)
    for sd in (plain, prefixed):
        assert np.array_equal(np.asarray(sd[p + "qkv_proj.bias"]), np.concatenate([w[p + f"{n}_proj.bias"] for n in "qkv"]))
        assert np.array_equal(np.asarray(sd[p + "qkv_proj.weight"]), np.concatenate([w[p + f"{n}_proj.weight"] for n in "qkv"]))
        assert not any(k.endswith((".q_proj.bias", ".k_proj.bias", ".v_proj.bias")) for k in sd)
    zero = np.zeros(128, np.float32)
    for name in ("layers.0.self_attn.o_proj.bias", "layers.0.mlp.gate_proj.bias", "layers.0.mlp.up_proj.bias", "layers.0.mlp.down_proj.bias"):
        with pytest.raises(NotImplementedError) as e:
            llama_state_dict({**w, name: zero})
        assert str(e.value) == f"llama: {name} (the biased variants are not built)"
    with pytest.raises(NotImplementedError) as e:
        llama_state_dict({k: v for k, v in w.items() if k != "layers.0.self_attn.v_proj.bias"})
    assert str(e.value) == "llama: layers.0.self_attn.q_proj.bias without the other two of q_proj / k_proj / v_proj .bias (a QKV bias is all three)"
    # the head-norm gains pass through under their own names
    fx, hf, cfg, w3, seqs, cuts = load_qwen_case("tiny_qwen3")
    sd = llama_state_dict(w3)
    assert sd["layers.0.self_attn.q_norm.weight"] is w3["layers.0.self_attn.q_norm.weight"]
    assert sd["layers.1.self_attn.k_norm.weight"].shape == (128,)


def test_synthetic_qwen_weights_have_a_stream_of_their_own():
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights, synthetic_qwen_weights
    cfg = SGPTConfig.from_hf_dict(dict(QWEN2_CFG, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                                       intermediate_size=256, vocab_size=50, max_position_embeddings=16))
    a, b = synthetic_qwen_weights(cfg, seed=5, qkv_bias=True), synthetic_qwen_weights(cfg, seed=5, qkv_bias=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert 0.05 < float(np.std(np.concatenate([a[f"layers.0.self_attn.{n}_proj.bias"] for n in "qkv"]))) < 0.2     # std 0.1: a dropped bias shows
    n = synthetic_qwen_weights(cfg, seed=5, qk_norm=True)
    gains = n["layers.0.self_attn.q_norm.weight"]
    assert gains.shape == (64,) and 0.03 < float(np.std(gains)) < 0.2 and abs(float(np.mean(gains)) - 1) < 0.1
    assert not np.array_equal(n["layers.0.self_attn.q_norm.weight"], n["layers.0.self_attn.k_norm.weight"])
    plain = synthetic_qwen_weights(cfg, seed=5)
    assert set(plain) == set(synthetic_llama_weights(cfg, seed=5))


# ---- TextPipeline(frame=...) ------------------------------------------------------------------------------------------------

class _QwenTok:
    """A tokenizer shaped as the Qwen ones: no add_bos_token attribute, no bos_token_id, an eos_token_id."""
    is_fast = False
    eos_token_id = 2

    def tokenize(self, txt):
        return txt.split()

    def convert_tokens_to_ids(self, toks):
        return [int(t[1:]) + 3 for t in toks]


def test_text_pipeline_takes_an_explicit_frame():
    from sgpt_amd.tokenization import TextPipeline
    tok = _QwenTok()
    short, long_ = "w0 w1 w2", " ".join(f"w{i}" for i in range(12))
    pipe = TextPipeline(tok, 8, family="llama", frame=([], [tok.eos_token_id]))           # the Qwen3-Embedding setting
    assert pipe.frame == ([], [2]) and pipe.max_token_len == 7
    assert pipe.ids(short, True) == [3, 4, 5, 2] and pipe.batch([long_, short], False) == [list(range(3, 10)) + [2], [3, 4, 5, 2]]
    assert pipe.docs_truncated == 1 and pipe.toks_truncated == 5
    both = TextPipeline(tok, 8, family="llama", frame=([7, 8], (9,)))
    assert both.frame == ([7, 8], [9]) and both.max_token_len == 5 and both.ids(long_, True) == [7, 8, 3, 4, 5, 6, 7, 9]
    assert TextPipeline(tok, 8, frame=([], [2])).ids(short, True) == [3, 4, 5, 2]         # any family: the frame as given
    empty = TextPipeline(tok, 8, family="llama", frame=([], []))
    assert empty.max_token_len == 8 and empty.ids(short, True) == [3, 4, 5]
    for kw in (dict(specb=True), dict(speca=True)):
        with pytest.raises(ValueError) as e:
            TextPipeline(tok, 8, frame=([], [2]), **kw)
        assert str(e.value) == "frame replaces the family's framing of the content: it does not go together with specb / speca brackets"
    # without `frame` nothing changes: this tokenizer is refused with the pinned text
    with pytest.raises(ValueError) as e:
        TextPipeline(tok, 8, family="llama")
    assert str(e.value) == "add_bos_token is set but the tokenizer has no bos_token_id"


def test_abi_v16_names():
    from sgpt_amd import _lib
    assert _lib.SGPT_ABI_VERSION >= 16 and "sgpt_qknorm_rope_half" in _lib.SIGNATURES
    assert _lib.ModelDesc._fields_[-1][0] == "n_kv_heads"                                # no new descriptor field
    assert [f.hf_model_types for f in __import__("sgpt_amd.families", fromlist=["FAMILIES"]).FAMILIES][-1] == ("llama", "mistral", "qwen2", "qwen3")
