"""The family table of the Python package (sgpt_amd/families.py) changes nothing that a caller can see.

Pinned here, without a GPU: every refusal by exception type and full message, as literals taken from the sources as they stood before
the table (SGPTModel with if-chains over model_type, TextPipeline(bert=, llama=)); the descriptor and the ordered tensor list that
reach sgpt_model_load, and the parsed configs, against tests/golden/family_descriptors.json -- recorded from that earlier
SGPTModel.__init__ (a capturing stub in place of sgpt_model_load) on HF_CASES / VARIANTS / case_weights() below; and the rule
that no other file of the package compares model_type with a literal."""
import dataclasses
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import sgpt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "family_descriptors.json")

# one tiny HF config.json per accepted HF model_type
HF_CASES = {
    "gpt_neo": dict(model_type="gpt_neo", vocab_size=64, max_position_embeddings=32, hidden_size=32, num_layers=4, num_heads=2,
                    attention_types=[[["global", "local"], 2]], window_size=8),
    "gptj": dict(model_type="gptj", vocab_size=64, n_positions=32, n_embd=32, n_layer=2, n_head=2, rotary_dim=8),
    "bloom": dict(model_type="bloom", vocab_size=64, hidden_size=48, n_layer=2, n_head=3),
    "bert": dict(model_type="bert", vocab_size=64, max_position_embeddings=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2,
                 intermediate_size=64, type_vocab_size=2, layer_norm_eps=1e-12),
    "llama": dict(model_type="llama", vocab_size=64, max_position_embeddings=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=4,
                  num_key_value_heads=2, intermediate_size=48, rms_norm_eps=1e-5, rope_theta=500000.0),
    "mistral": dict(model_type="mistral", vocab_size=64, max_position_embeddings=32, hidden_size=32, num_hidden_layers=2,
                    num_attention_heads=4, num_key_value_heads=1, intermediate_size=48, sliding_window=8),
}
# (dtype, precise_qk, precision) per case: the defaults, and for the decoders every descriptor field the three arguments move
VARIANTS = {"gpt_neo": [("f16", None, None), ("bf16", "attn", "plain"), ("f16", True, "plain"), ("f16", "act+logits", "x3"),
                        ("fp32", None, None), ("fp8", None, None), ("fp8mfma", None, None)],
            "gptj": [("f16", None, None), ("bf16", "full", "auto-class"), ("fp8", None, None)],
            "bloom": [("f16", None, None), ("bf16", "qkv+logits", "plain")],
            "bert": [("f16", None, None), ("bf16", None, None), ("fp32", None, None)],
            "llama": [("f16", None, None), ("bf16", None, None), ("fp32", None, None)],
            "mistral": [("f16", None, None), ("fp32", None, None)]}


def case_weights(tag, cfg):
    """Seeded weights of a case under its HF names, plus what the name filter has to deal with: a `transformer.` prefix, HF's mask
    buffers, a learntmean table, an LM head, and a torch tensor among the numpy arrays."""
    from sgpt_amd.model import synthetic_bert_weights, synthetic_llama_weights, synthetic_weights
    hf = {k: v for k, v in HF_CASES[tag].items() if k != "model_type"}
    if tag == "gpt_neo":
        w = synthetic_weights(cfg, seed=5)
    elif tag == "gptj":
        w = O.synth_weights_gptj(O.GPTJConfig(**hf), seed=5)
    elif tag == "bloom":
        w = O.synth_weights_bloom(O.BloomConfig(**hf), seed=5)
    elif tag == "bert":
        w = {"bert." + k: v for k, v in synthetic_bert_weights(cfg, seed=5).items()}
        w["cls.predictions.bias"] = np.zeros(4, np.float32)
        w["bert.embeddings.position_ids"] = np.arange(4, dtype=np.int64)
    else:
        w = {"model." + k: v for k, v in synthetic_llama_weights(cfg, seed=5).items()}
        w["model.layers.0.self_attn.rotary_emb.inv_freq"] = np.ones(4, np.float32)
    keys = list(w)
    if tag in ("gpt_neo", "gptj"):                      # HF *ForCausalLM checkpoints: every name prefixed (GPT-J here), or only some
        w = {("transformer." + k if tag == "gptj" or k == keys[0] else k): v for k, v in w.items()}
        keys = list(w)
    w[keys[1]] = torch.from_numpy(w[keys[1]]).to(torch.float64)
    rng = np.random.default_rng(9)
    w["transformer.h.0.attn.attention.bias"] = np.ones((4, 4), np.float32)
    w["h.0.attn.masked_bias"] = np.float32(-1e9).reshape(1)
    w["position_weights"] = rng.standard_normal(32).astype(np.float32)
    w["lm_head.weight"] = rng.standard_normal((cfg.vocab_size, cfg.hidden_size)).astype(np.float32)
    w["lm_head.bias"] = rng.standard_normal(cfg.vocab_size).astype(np.float32)
    return w


def desc_record(desc, local):
    rec = {name: getattr(desc, name) for name, _ in type(desc)._fields_ if name != "layer_is_local"}
    rec["layer_is_local"] = list(local)
    return rec


def tensor_record(name, t):
    data = t.detach().to("cpu", torch.float32).contiguous().numpy()
    return [name, list(data.shape), hashlib.sha256(data.tobytes()).hexdigest()]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- config parser, descriptor, tensor list ----------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", sorted(HF_CASES))
def test_from_hf_dict_equals_the_recording(golden, tag):
    from sgpt_amd.model import SGPTConfig
    assert dataclasses.asdict(SGPTConfig.from_hf_dict(HF_CASES[tag])) == golden[tag]["config"]


@pytest.mark.parametrize("tag", sorted(HF_CASES))
def test_model_desc_equals_the_recording(golden, tag):
    from sgpt_amd.model import SGPTConfig, check_args, model_desc
    cfg = SGPTConfig.from_hf_dict(HF_CASES[tag])
    assert len(golden[tag]["descriptors"]) == len(VARIANTS[tag])
    for (dtype, precise_qk, precision), want in zip(VARIANTS[tag], golden[tag]["descriptors"]):
        desc, local = model_desc(cfg, *check_args(cfg, dtype, precise_qk, precision))
        got = desc_record(desc, local)
        assert [desc.layer_is_local[i] for i in range(cfg.num_layers)] == got["layer_is_local"]
        # (float fields went through a C float on both sides: equal bits, so equal doubles)
        assert got == want, (dtype, precise_qk, precision)


@pytest.mark.parametrize("tag", sorted(HF_CASES))
def test_load_tensors_equals_the_recording(golden, tag):
    from sgpt_amd.model import SGPTConfig, load_tensors
    cfg = SGPTConfig.from_hf_dict(HF_CASES[tag])
    got = [tensor_record(name, t) for name, t in load_tensors(cfg, case_weights(tag, cfg))]
    assert [g[0] for g in got] == [w[0] for w in golden[tag]["tensors"]]
    assert got == golden[tag]["tensors"]
    kept = any(name.startswith("lm_head") for name, _, _ in got)
    assert kept == (tag == "gptj")                      # the other decoders tie the head to the embedding; BERT / Llama load none


# ---- refusals: type and full text, as they read before the table ----------------------------------------------------------------

E_PRECISION = "precision must be 'plain', 'x3', 'auto' or 'auto-class'"
E_PRECISION_DTYPE = "precision applies to dtype 'f16' / 'bf16'"
E_PQK = ("precise_qk must be None, False, True or one of ['act+logits', 'attn', 'full', 'full+logits', 'logits', 'qkv+logits']")
E_PQK_DTYPE = "precise_qk applies to dtype 'f16' / 'bf16'"
E_FP8 = {"bert": "dtype %r is not available for BERT models: use 'f16', 'bf16' or 'fp32'",
         "llama": "dtype %r is not available for Llama / Mistral models: use 'bf16', 'f16' or 'fp32'"}
E_SPLIT = {"bert": "split-precision operands (precision='x3' / 'auto' / 'auto-class', precise_qk) are not available for BERT models",
           "llama": "split-precision operands (precision='x3' / 'auto' / 'auto-class', precise_qk) are not available for "
                    "Llama / Mistral models"}
E_KV = "num_heads must be a multiple of num_kv_heads"
E_DTYPE = ("dtype must be 'f16' (IEEE-half MFMA operands, range-guarded: the 1e-3-parity mode), "
           "'bf16' (bf16 MFMA operands), 'fp32' (exact fp32 MFMA), "
           "'fp8' (e4m3fn weight storage, bf16 arithmetic) or 'fp8mfma' (fp8 storage + fp8 MFMA on the MLP)")
E_LEARNT = "method 'learntmean' (trained position weights of the SGPT checkpoints) is not available for BERT / Llama models"
E_LEARNT_NONE = "method 'learntmean' needs trained position weights (1_WeightedMeanPooling)"
E_LM = {"bert": "lm_logprobs: a BERT model carries no causal LM head",
        "llama": "lm_logprobs is not built for Llama / Mistral models (their LM head is not loaded)"}
E_ATT = "precise_qk='logits' needs head_dim 64 / 128 and no rotary embedding"
E_BRACKETS = {"bert": "specb / speca brackets belong to the GPT models; a BERT model is framed [CLS] ... [SEP]",
              "llama": "specb / speca brackets belong to the GPT models; a Llama / Mistral model takes its tokenizer's BOS / EOS"}
E_CLS = "a BERT model needs a tokenizer with cls_token_id and sep_token_id"
E_BOS = "add_bos_token is set but the tokenizer has no bos_token_id"
E_EOS = "add_eos_token is set but the tokenizer has no eos_token_id"
E_BOTH = "speca and specb are mutually exclusive"

DECODERS = ("gpt_neo", "gptj", "bloom")
EVERY = DECODERS + ("bert", "llama")


class _ContextReached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """SGPTModel(...) that is not refused gets as far as opening the device context, and stops there -- on any machine."""
    import sgpt_amd.model as M

    def stop(device=None):
        raise _ContextReached
    monkeypatch.setattr(M, "get_context", stop)


def refusal(cfg, **kw):
    from sgpt_amd.model import SGPTModel
    with pytest.raises(Exception) as e:
        SGPTModel(cfg, {}, **kw)
    return type(e.value), str(e.value)


def config(model_type, **kw):
    from sgpt_amd.model import SGPTConfig
    return SGPTConfig(model_type=model_type, **kw)


@pytest.mark.parametrize("mt", EVERY)
def test_argument_refusals_of_every_family(no_device, mt):
    cfg = config(mt)
    assert refusal(cfg, precision="x4") == (ValueError, E_PRECISION)
    assert refusal(cfg, dtype="fp32", precision="x3") == (ValueError, E_PRECISION_DTYPE)
    assert refusal(cfg, dtype="nope", precision="x3") == (ValueError, E_PRECISION_DTYPE)
    assert refusal(cfg, precise_qk="yes") == (ValueError, E_PQK)
    assert refusal(cfg, dtype="fp32", precise_qk="logits") == (ValueError, E_PQK_DTYPE)
    assert refusal(cfg, dtype="fp8", precise_qk=True) == (ValueError, E_PQK_DTYPE)
    assert refusal(cfg, dtype="nope") == (ValueError, E_DTYPE)           # not the family's refusal, on any row
    assert refusal(cfg, dtype="nope", precision="plain", precise_qk=False) == (ValueError, E_DTYPE)


@pytest.mark.parametrize("mt", ["bert", "llama"])
def test_family_refusals_of_bert_and_llama(no_device, mt):
    cfg = config(mt)
    for dtype in ("fp8", "fp8mfma"):
        assert refusal(cfg, dtype=dtype) == (ValueError, E_FP8[mt] % dtype)
    for kw in (dict(precision="x3"), dict(precision="auto"), dict(precision="auto-class"), dict(precise_qk=True),
               dict(precise_qk="logits", dtype="bf16"), dict(precision="x3", precise_qk="attn")):
        assert refusal(cfg, **kw) == (ValueError, E_SPLIT[mt])
    for kw in (dict(), dict(dtype="f16"), dict(dtype="fp16"), dict(dtype="bf16"), dict(dtype="fp32"), dict(precision="plain", precise_qk=False)):
        assert refusal(cfg, **kw) == (_ContextReached, "")               # f16 defaults to precision 'plain' here: nothing to probe for


def test_grouped_heads_refusal_is_llamas_and_comes_after_its_other_two(no_device):
    odd = config("llama", num_heads=12, num_kv_heads=5)
    assert refusal(odd) == (ValueError, E_KV)
    assert refusal(odd, dtype="fp8") == (ValueError, E_FP8["llama"] % "fp8")
    assert refusal(odd, precision="x3") == (ValueError, E_SPLIT["llama"])
    assert refusal(odd, dtype="nope") == (ValueError, E_KV)
    for mt in DECODERS + ("bert",):                                      # num_kv_heads is read for no other family
        assert refusal(config(mt, num_heads=12, num_kv_heads=5)) == (_ContextReached, "")


@pytest.mark.parametrize("mt", DECODERS)
def test_decoders_are_not_refused(no_device, mt):
    cfg = config(mt)
    for kw in (dict(), dict(dtype="fp8"), dict(dtype="fp8mfma"), dict(dtype="fp32"), dict(precision="x3"), dict(precision="auto"),
               dict(precision="auto-class", dtype="bf16"), dict(precise_qk=True), dict(precise_qk="attn", precision="x3")):
        assert refusal(cfg, **kw) == (_ContextReached, "")


def test_without_a_device_the_context_is_what_stops_a_model(monkeypatch):
    from sgpt_amd._lib import SgptHipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    kind, text = refusal(config("gpt_neo"), dtype="fp8")
    assert kind is SgptHipError and text.startswith("no HIP device visible")


def bare_model(mt, **attrs):
    from sgpt_amd.model import SGPTModel
    m = SGPTModel.__new__(SGPTModel)
    m.cfg = config(mt)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_default_precision_and_structural_precise_qk():
    from sgpt_amd.model import check_args, default_precise_qk
    for mt in EVERY:
        assert check_args(config(mt), "half", None, None)[2] == ("auto" if mt in DECODERS else "plain")
        assert check_args(config(mt), "bf16", None, None) == ("bf16", False, "plain")
        wide = config(mt, hidden_size=2048, num_heads=16)
        assert default_precise_qk(wide, "f16") == ("act+logits" if mt == "gpt_neo" else False)
        assert default_precise_qk(wide, "bf16") is False
    assert default_precise_qk(config("gpt_neo", hidden_size=2560, num_heads=20), "f16") == "qkv+logits"
    assert default_precise_qk(config("gpt_neo", hidden_size=2048, num_heads=8), "f16") == "full"


@pytest.mark.parametrize("mt", EVERY)
def test_learntmean_and_lm_head_refusals(mt):
    m = bare_model(mt, position_weights=None)
    m._check_learnt("weightedmean", None)
    with pytest.raises(ValueError) as e:
        m._check_learnt("learntmean", None)
    assert str(e.value) == (E_LEARNT_NONE if mt in DECODERS else E_LEARNT)
    with pytest.raises(Exception) as e:
        m.lm_logprobs(None, [0], [0])
    if mt in DECODERS:                                                  # past the family's refusal: the argument check answers
        assert (type(e.value), str(e.value)) == (ValueError, "lm_logprobs: hidden must be an fp32 tensor [T_pad, d_model]")
    else:
        assert (type(e.value), str(e.value)) == (ValueError, E_LM[mt])


def test_split_attention_refusal_of_the_structural_plan():
    with pytest.raises(ValueError) as e:
        bare_model("gptj", precise_qk="logits", _att_ok=False)._base_plan()
    assert str(e.value) == E_ATT
    plan = bare_model("gpt_neo", precise_qk="logits", _att_ok=True)._base_plan()
    assert plan.shape == (12, 5) and (plan[:, 1] == 1).all() and not plan[:, [0, 2, 3, 4]].any()


class _Tok:
    def __init__(self, **ids):
        self.__dict__.update(ids)

    def tokenize(self, text):
        return text.split()

    def convert_tokens_to_ids(self, tokens):
        return [len(t) for t in tokens]

    def encode(self, text, add_special_tokens=False):
        return self.convert_tokens_to_ids(self.tokenize(text))


def test_text_pipeline_refusals_and_frames():
    from sgpt_amd.families import family, family_of
    from sgpt_amd.tokenization import TextPipeline

    def said(*a, **kw):
        with pytest.raises(ValueError) as e:
            TextPipeline(*a, **kw)
        return str(e.value)
    full = _Tok(cls_token_id=101, sep_token_id=102, bos_token_id=1, eos_token_id=2)
    for fam in (None, "gpt_neo", "bert", "llama", family("bloom")):
        assert said(full, 8, specb=True, speca=True, family=fam) == E_BOTH
    for mt in ("bert", "llama"):
        for kw in (dict(specb=True), dict(speca=True)):
            assert said(full, 8, family=mt, **kw) == E_BRACKETS[mt]
            assert said(_Tok(), 8, family=family(mt), **kw) == E_BRACKETS[mt]      # before the tokenizer is looked at
    assert said(_Tok(cls_token_id=101), 8, family="bert") == E_CLS
    assert said(_Tok(sep_token_id=102), 8, family="bert") == E_CLS
    assert said(_Tok(eos_token_id=2), 8, family="llama") == E_BOS
    assert said(_Tok(bos_token_id=1, add_eos_token=True), 8, family="llama") == E_EOS
    # the frames, resolved once: a row, its model_type, and a model object's row all mean the same
    for fam in ("bert", family("bert"), family_of(bare_model("bert"))):
        p = TextPipeline(full, 8, family=fam)
        assert p.frame == ([101], [102]) and p.max_token_len == 6 and p.ids("aa bbb", True) == [101, 2, 3, 102]
    p = TextPipeline(full, 8, family="llama")
    assert p.frame == ([1], []) and p.max_token_len == 7 and p.ids("aa bbb", False) == [1, 2, 3]
    both = TextPipeline(_Tok(bos_token_id=1, eos_token_id=2, add_eos_token=True), 8, family="llama")
    assert both.frame == ([1], [2]) and both.max_token_len == 6
    none = TextPipeline(_Tok(add_bos_token=False), 8, family="llama")
    assert none.frame == ([], []) and none.max_token_len == 8 and none.ids("aa bbb", True) == [2, 3]
    for fam in (None, "gpt_neo", "gptj", "bloom", family_of(object())):
        p = TextPipeline(full, 8, specb=True, family=fam)
        assert p.frame is None and p.max_token_len == 6 and p.ids("aa bbb", True) == [1, 2, 3, 1]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def test_only_the_table_compares_model_type():
    seen = 0
    for dirpath, _, files in os.walk(os.path.join(ROOT, "sgpt_amd")):
        for f in files:
            if f.endswith(".py") and f != "families.py":
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"model_type\s*(==|!=|in\b|not\s+in\b)", src), f
                seen += 1
    assert seen > 5
    import sgpt_amd.families as F
    import sgpt_amd.tokenization as T
    assert not hasattr(T, "is_bert") and not hasattr(T, "is_llama") and not hasattr(F, "SGPTModel")
    assert not re.search(r"^\s*(from|import)\s+(\.model|oracle|sgpt_amd\.model)", open(F.__file__).read(), re.M)
    assert [f.model_type for f in F.FAMILIES] == list(EVERY) and [f.arch for f in F.FAMILIES] == [0, 1, 2, 3, 4]


def test_unknown_model_type_is_refused_by_name(no_device):
    """Before the table an unknown SGPTConfig.model_type passed as GPT-Neo, silently; now it is refused wherever a row is looked up."""
    from sgpt_amd.families import family, family_of
    from sgpt_amd.tokenization import TextPipeline
    text = "model_type 'roberta': SGPTConfig.model_type is one of ['gpt_neo', 'gptj', 'bloom', 'bert', 'llama']"
    for call in (lambda: family("roberta"), lambda: family_of(bare_model("roberta")), lambda: TextPipeline(_Tok(), 8, family="roberta")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert refusal(config("roberta")) == (ValueError, text)
    assert refusal(config("roberta"), dtype="bf16") == (ValueError, text)


class _NoLibrary:
    """Stands in for the context: every library call succeeds and is recorded by name."""
    handle = None
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []
        self.lib = self

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


@pytest.mark.parametrize("tag", sorted(HF_CASES))
def test_position_weights_are_taken_from_the_callers_dict(monkeypatch, tag):
    """A `position_weights` entry rides along with the weights: dropped from the tensor list, installed as the learntmean table.  It is
    looked up under that very name in the dict the caller passed (a `bert.` / `model.` prefixed spelling, which no checkpoint carries,
    is neither loaded nor installed)."""
    from sgpt_amd.model import SGPTConfig, SGPTModel, load_tensors
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    cfg = SGPTConfig.from_hf_dict(HF_CASES[tag])
    w = case_weights(tag, cfg)
    m = SGPTModel(cfg, w, ctx=_NoLibrary(), dtype="fp32")
    assert m.ctx.calls == ["sgpt_model_load", "sgpt_model_set_pool_weights"]
    assert torch.equal(m.position_weights, torch.from_numpy(w["position_weights"]))
    table = w.pop("position_weights")
    for prefix in ("bert.", "model."):
        w2 = dict(w, **{prefix + "position_weights": table})
        m = SGPTModel(cfg, w2, ctx=_NoLibrary(), dtype="fp32")
        assert m.ctx.calls == ["sgpt_model_load"] and m.position_weights is None
        strips = (tag, prefix) in (("bert", "bert."), ("llama", "model."), ("mistral", "model."))     # the family's mapping strips its own prefix
        names = [n for n, _ in load_tensors(cfg, w2)]
        assert ("position_weights" not in names) and ((prefix + "position_weights" in names) != strips)
