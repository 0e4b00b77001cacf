"""CPU: the host side of the bidirectional Llama / Mistral / Qwen embedders (ABI v24) -- the float64 reference of
tests/llama_bidir_ref.py against HF LlamaModel / Qwen2Model run without their causal mask (tests/golden/tiny_*_bidir.npz, recipe
make_golden_bidir.py), its ranged pooling against the recorded `pool_from = 3` vectors, and the Python surface: the attention mode and
its refusals, `pack(pool_from=)`, the prompt arithmetic of TextPipeline, the folder field `include_prompt`, the ABI table.

Tolerance of the reference check: the one tests/test_llama_ref.py derives for the causal fixtures, (9 L + 2) * 32 u * max|hidden| --
the stages of a block are the same nine, the softmax only sums over more keys."""
import ctypes as C
import dataclasses
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import llama_bidir_ref as B
import llama_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
TAGS = ["tiny_llama_bidir", "tiny_llama_g4_bidir", "tiny_llama_dh128_bidir", "tiny_qwen2_bidir"]
SHAPES = {"tiny_llama_bidir": (128, 2, 1), "tiny_llama_g4_bidir": (256, 4, 1), "tiny_llama_dh128_bidir": (256, 2, 2),
          "tiny_qwen2_bidir": (128, 2, 1)}                 # d, heads, kv heads
MODES = ("mean", "weightedmean", "lasttoken")


def load_bidir_case(tag):
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights, synthetic_qwen_weights
    fx = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    hf = json.loads(str(fx["cfg"]))
    cfg = SGPTConfig.from_hf_dict(hf)
    w = synthetic_qwen_weights(cfg, seed=int(fx["seed"]), qkv_bias=True) if bool(fx["qkv_bias"]) else synthetic_llama_weights(cfg, seed=int(fx["seed"]))
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(fx["weights_sha256"]), "the synthetic weight generator no longer produces the fixture's weights"
    lens = fx["seq_lens"].tolist()
    cuts = np.cumsum([0] + lens)
    seqs = [fx["ids"][a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    return fx, hf, cfg, w, seqs, cuts


_ref_cache = {}


def ref_forward(tag):
    """The float64 bidirectional hidden states of a fixture's sequences, computed once per session and shared (read-only)."""
    if tag not in _ref_cache:
        fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
        _ref_cache[tag] = B.forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta)
    return _ref_cache[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_bidir_ref_reproduces_hf_and_its_ranged_pooling_the_recorded_vectors(tag):
    fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
    L = cfg.num_layers
    assert [len(s) for s in seqs] == [1, 7, 64, 70, 130] and hf["max_position_embeddings"] == 160 and L == 2
    assert (cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads) == SHAPES[tag] and hf["is_causal"] is False and int(fx["pool_from"]) == 3
    assert any(k.endswith("q_proj.bias") for k in w) == (tag == "tiny_qwen2_bidir")
    hs = ref_forward(tag)
    want = fx["hidden"].astype(np.float64)                       # [L + 1, rows, d]
    assert want.shape[0] == L + 1
    bound = (9 * L + 2) * 32 * U32 * float(np.abs(want).max())
    worst = worst_from = 0.0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        worst = max(worst, float(np.abs(hs[i] - want[:, a:b]).max()))
        for mode in MODES:
            assert np.array_equal(B.pool_range(hs[i][-1], mode, 0), R.pool(hs[i][-1], mode))
            worst = max(worst, float(np.abs(B.pool_range(hs[i][-1], mode) - fx[f"emb_{mode}"][i]).max()))
            worst_from = max(worst_from, float(np.abs(B.pool_range(hs[i][-1], mode, 3) - fx[f"emb_{mode}_from"][i]).max()))
    print(f"{tag}: max|llama_bidir_ref - HF| = {worst:.3e}, pooled from token 3 {worst_from:.3e} (bound {bound:.3e})")
    assert worst < bound and worst_from < bound
    # the 1-token sequence: the empty range is a zero row, lasttoken its only row
    assert not fx["emb_mean_from"][0].any() and not fx["emb_weightedmean_from"][0].any()
    assert np.array_equal(fx["emb_lasttoken_from"], fx["emb_lasttoken"])


@pytest.mark.parametrize("tag", TAGS)
def test_the_fixture_is_not_a_causal_one(tag):
    """The causal reference leaves the recorded values by far more than rounding on every row but the last of the first block, and the
    pooling from token 3 differs from the pooling of everything."""
    fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
    import qwen_ref as Q
    causal = Q.forward(w, seqs[1:2], cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, 0)[0]
    want = fx["hidden"].astype(np.float64)[:, cuts[1]:cuts[2]]
    assert np.abs(causal[1, 0] - want[1, 0]).max() > 1e-3          # row 0 sees the later tokens
    assert np.abs(causal[1, -1] - want[1, -1]).max() < 1e-5        # the last row sees every key either way in the first block
    assert np.abs(causal[2] - want[2]).max() > 1e-3
    for mode in ("mean", "weightedmean"):
        assert np.abs(fx[f"emb_{mode}_from"][1:] - fx[f"emb_{mode}"][1:]).max() > 1e-3


def test_ranged_pooling_rules():
    rng = np.random.default_rng(0)
    h = rng.standard_normal((7, 8))
    for lo, rows in ((0, range(7)), (1, range(1, 7)), (6, [6]), (-2, range(7))):
        rows = list(rows)
        assert np.allclose(B.pool_range(h, "mean", lo), h[rows].mean(0))
        wgt = np.asarray(rows, np.float64) + 5 + 1                 # the padded position index: it does not restart behind the prompt
        assert np.allclose(B.pool_range(h, "weightedmean", lo, pad_left=5), (h[rows] * wgt[:, None]).sum(0) / wgt.sum())
        assert np.array_equal(B.pool_range(h, "lasttoken", lo), h[6])
    for lo in (7, 12):                                             # the empty range: zeros, not NaN
        assert not B.pool_range(h, "mean", lo).any() and not B.pool_range(h, "weightedmean", lo).any()
        assert np.array_equal(B.pool_range(h, "lasttoken", lo), h[6])


# ---- the attention mode: not a descriptor field, not a config field -----------------------------------------------------------------

class _Capture:
    """Stands in for the context: every library call succeeds and is recorded by name; sgpt_model_load's descriptor is kept."""
    handle = None
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.descs, self.lib = [], [], self

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + (tuple(args[1:]) if name == "sgpt_model_set_attention" else ()))
            if name == "sgpt_model_load":
                d = args[1]._obj
                self.descs.append({n: (getattr(d, n) if n != "layer_is_local" else [d.layer_is_local[i] for i in range(d.n_layers)])
                                   for n, _ in type(d)._fields_})
            return 0
        return call


@pytest.fixture
def no_sync(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)


@pytest.mark.parametrize("dtype", ["fp32", "f16", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_descriptor_and_config_do_not_know_the_attention_mode(no_sync, tag, dtype):
    from sgpt_amd.model import SGPTConfig, SGPTModel, check_args, model_desc
    fx, hf, cfg, w, seqs, cuts = load_bidir_case(tag)
    plain = SGPTConfig.from_hf_dict({k: v for k, v in hf.items() if k != "is_causal"})
    assert dataclasses.asdict(cfg) == dataclasses.asdict(plain)
    with open(os.path.join(ROOT, "tests", "golden", "family_descriptors.json")) as f:
        golden = json.load(f)
    assert set(dataclasses.asdict(cfg)) == set(golden["llama"]["config"])                # no new SGPTConfig field
    before = dataclasses.asdict(cfg)
    causal, bidir = SGPTModel(cfg, w, ctx=_Capture(), dtype=dtype), SGPTModel(cfg, w, ctx=_Capture(), dtype=dtype, attention="bidirectional")
    assert causal.attention == "causal" and bidir.attention == "bidirectional"
    assert [c[0] for c in causal.ctx.calls] == ["sgpt_model_load"]
    assert bidir.ctx.calls == [("sgpt_model_load",), ("sgpt_model_set_attention", 0)]
    assert causal.ctx.descs == bidir.ctx.descs and len(bidir.ctx.descs) == 1
    desc, local = model_desc(cfg, *check_args(cfg, dtype, None, None))
    want = {n: getattr(desc, n) for n, _ in type(desc)._fields_ if n != "layer_is_local"}
    want["layer_is_local"] = list(local)
    assert bidir.ctx.descs[0] == want and set(want) == set(golden["llama"]["descriptors"][0])   # no new descriptor field
    assert dataclasses.asdict(cfg) == before
    bidir.set_attention("causal")
    assert bidir.attention == "causal" and bidir.ctx.calls[-1] == ("sgpt_model_set_attention", 1)


def test_mode_resolution_from_the_raw_config(no_sync, tmp_path):
    from sgpt_amd.families import attention_from_hf_dict
    from sgpt_amd.formats import write_st_folder
    from sgpt_amd.model import SGPTModel
    assert attention_from_hf_dict({"is_causal": False}) == "bidirectional"
    assert attention_from_hf_dict({"is_causal": False}, "causal") == "causal"             # an explicit argument wins
    assert attention_from_hf_dict({"is_causal": True}) == "causal" and attention_from_hf_dict({}) == "causal"
    assert attention_from_hf_dict({"is_causal": None}) == "causal" and attention_from_hf_dict({}, "bidirectional") == "bidirectional"
    fx, hf, cfg, w, seqs, cuts = load_bidir_case("tiny_llama_bidir")
    p = str(tmp_path / "st")
    write_st_folder(p, hf, {"model." + k: v for k, v in w.items()}, pooling_mode="mean", max_seq_length=64)
    m = SGPTModel.from_pretrained(p, ctx=_Capture(), dtype="fp32")
    assert m.attention == "bidirectional" and ("sgpt_model_set_attention", 0) in m.ctx.calls
    assert not hasattr(m.cfg, "is_causal")
    m = SGPTModel.from_pretrained(p, ctx=_Capture(), dtype="fp32", attention="causal")
    assert m.attention == "causal" and [c[0] for c in m.ctx.calls] == ["sgpt_model_load"]
    p2 = str(tmp_path / "st2")
    write_st_folder(p2, {k: v for k, v in hf.items() if k != "is_causal"}, {"model." + k: v for k, v in w.items()}, pooling_mode="mean")
    assert SGPTModel.from_pretrained(p2, ctx=_Capture(), dtype="fp32").attention == "causal"
    assert SGPTModel.from_pretrained(p2, ctx=_Capture(), dtype="fp32", attention="bidirectional").attention == "bidirectional"


E_FAMILY = "attention='bidirectional' is a mode of the Llama / Mistral / Qwen family: a %s model %s"
E_WINDOW = ("attention='bidirectional' over an applied sliding window (window_size 16) is not built: only a window the config parser "
            "folded away (at least min(max_position_embeddings, 2048) tokens) runs bidirectionally")


def test_refusals_of_the_other_families_and_of_an_unfolded_window(no_sync):
    from sgpt_amd.model import SGPTConfig, SGPTModel
    cases = {"gpt_neo": ("GPT-Neo", "stays causal"), "gptj": ("GPT-J", "stays causal"), "bloom": ("BLOOM", "stays causal"),
             "bert": ("BERT", "is bidirectional by architecture")}
    for mt, (name, why) in cases.items():
        cfg = SGPTConfig(model_type=mt, hidden_size=128, num_layers=2, num_heads=2, vocab_size=50, max_position_embeddings=32)
        with pytest.raises(ValueError) as e:
            SGPTModel(cfg, {}, ctx=_Capture(), dtype="fp32", attention="bidirectional")
        assert str(e.value) == E_FAMILY % (name, why)
    mistral = dict(model_type="mistral", vocab_size=50, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                   intermediate_size=256, max_position_embeddings=160)
    windowed = SGPTConfig.from_hf_dict(dict(mistral, sliding_window=16))
    with pytest.raises(ValueError) as e:
        SGPTModel(windowed, {}, ctx=_Capture(), dtype="fp32", attention="bidirectional")
    assert str(e.value) == E_WINDOW
    # a window the parser folded away is not in the config: fine in either direction
    folded = SGPTConfig.from_hf_dict(dict(mistral, sliding_window=4096, max_position_embeddings=8192))
    assert folded.window_size == 0 and folded.max_position_embeddings == 4096
    from sgpt_amd.families import check_attention
    assert check_attention(folded, "bidirectional") == "bidirectional" and check_attention(windowed, "causal") == "causal"
    with pytest.raises(ValueError, match="attention must be 'causal' or 'bidirectional', not 'full'"):
        check_attention(folded, "full")
    # the BERT family runs its own mode whatever the default says, and reports it
    bert = SGPTConfig(model_type="bert", hidden_size=128, num_layers=1, num_heads=2, vocab_size=50, max_position_embeddings=32,
                      attention_layers=["global"], window_size=0)
    from sgpt_amd.model import synthetic_bert_weights
    m = SGPTModel(bert, synthetic_bert_weights(bert, seed=1), ctx=_Capture(), dtype="fp32")
    assert m.attention == "bidirectional" and [c[0] for c in m.ctx.calls] == ["sgpt_model_load"]


def test_encode_graph_refuses_both_features():
    from sgpt_amd.model import EncodeGraph, SGPTConfig
    cfg = SGPTConfig(model_type="llama", hidden_size=128, num_layers=1, num_heads=2, vocab_size=50, max_position_embeddings=32,
                     window_size=0, attention_layers=["global"])
    with pytest.raises(ValueError, match="EncodeGraph: a model with attention='bidirectional' is not captured"):
        EncodeGraph(types.SimpleNamespace(cfg=cfg, attention="bidirectional"), [[1, 2]])
    with pytest.raises(ValueError, match="EncodeGraph: pool_from is not captured"):
        EncodeGraph(types.SimpleNamespace(cfg=cfg, attention="causal"), [[1, 2]], pool_from=1)


# ---- pack(pool_from=) ---------------------------------------------------------------------------------------------------------------

def test_pack_pool_from_arena_layout_broadcast_and_refusals():
    from sgpt_amd.model import PackedBatch, SGPTModel, arena_ints, fill_arena, pack_host, pack_layout
    seqs = [[5, 6, 7], [8], [9, 10, 11, 12, 13, 14]]
    plain = pack_host(seqs)
    assert plain["pool_lo"] is None and len(plain["arena"]) == 2 * plain["T_pad"] + 3 * 3 + 1        # the layout of every earlier ABI
    one = pack_host(seqs, pool_from=2)
    B_, T = one["B"], one["T_pad"]
    assert len(one["arena"]) == 2 * T + 4 * B_ + 1 == len(plain["arena"]) + B_
    assert np.array_equal(one["arena"][: len(plain["arena"])], plain["arena"])                       # the new array sits BEHIND the others
    assert one["pool_lo"].dtype == np.int32 and one["pool_lo"].tolist() == [2, 1, 2]                 # one int for all, clamped to the length
    assert one["pool_lo"].base is one["arena"] or np.shares_memory(one["pool_lo"], one["arena"])
    assert one["arena"][2 * T + 3 * B_ + 1:].tolist() == [2, 1, 2]
    each = pack_host(seqs, pool_from=[0, 1, 5])
    assert each["pool_lo"].tolist() == [0, 1, 5]
    assert pack_host(seqs, pool_from=np.int64(0))["pool_lo"].tolist() == [0, 0, 0]
    # a bucket's filler sequences pool everything
    lay = pack_layout(seqs, None, (5, 32, 8), pool_from=[1, 0, 3])
    assert lay["pool_lo"].tolist() == [1, 0, 3, 0, 0] and arena_ints(lay) == 2 * 32 + 4 * 5 + 1
    arena = np.full(arena_ints(lay), -7, dtype=np.int32)
    fill_arena(seqs, lay, arena)
    assert arena[-5:].tolist() == [1, 0, 3, 0, 0] and (arena != -7).all()
    for bad, msg in (([1, 2], "one int, or one int per sequence"), (-1, "cannot be negative"), ([0, -3, 1], "cannot be negative"),
                     (1.5, "one int, or one int per sequence"), ([[1, 2, 3]], "one int, or one int per sequence")):
        with pytest.raises(ValueError, match=msg):
            pack_host(seqs, pool_from=bad)
    # the encode calls refuse it with cls and learntmean, before the library is reached
    z = torch.zeros(3, dtype=torch.int32)
    pb = PackedBatch(z, z, z, z, z, 3, 32, 6, 10, pool_lo=z)
    for mode in ("cls", "learntmean"):
        with pytest.raises(ValueError, match=f"pool_from .* serves 'mean', 'weightedmean' and 'lasttoken', not '{mode}'"):
            SGPTModel._check_pool_from(mode, pb)
    for mode in MODES:
        SGPTModel._check_pool_from(mode, pb)
    SGPTModel._check_pool_from("cls", PackedBatch(z, z, z, z, z, 3, 32, 6, 10))


# ---- prompts ------------------------------------------------------------------------------------------------------------------------

class _Tok:
    """Stub tokenizer: one id per whitespace word ('w7' -> 10), a word glued to a colon is ONE other token."""
    is_fast = False
    bos_token_id, eos_token_id, cls_token_id, sep_token_id = 1, 2, 101, 102
    add_bos_token, add_eos_token = True, True

    def tokenize(self, txt):
        return txt.split()

    def convert_tokens_to_ids(self, toks):
        return [int(re.sub(r"\D", "", t)) + 3 + (100 if ":" in t else 0) for t in toks]


def test_prompt_length_with_a_front_and_a_back_frame():
    from sgpt_amd.tokenization import TextPipeline
    prompt, text = "w1 w2 w3: ", "w7 w8"
    pipe = TextPipeline(_Tok(), 16, family="llama", prompt=prompt, include_prompt=False)          # BOS in front, EOS behind
    ids = pipe.ids(text, True)
    assert ids == [1, 4, 5, 106, 10, 11, 2]                                                        # prompt + text tokenised as ONE string
    assert pipe.pool_from() == 4 == 1 + 3                                                          # front frame + the prompt alone; no back frame
    assert ids[pipe.pool_from():] == [10, 11, 2]
    assert pipe.batch([text, text], False) == [ids, ids]
    assert TextPipeline(_Tok(), 16, family="llama", prompt=prompt).pool_from() is None             # include_prompt=True: everything is pooled
    assert TextPipeline(_Tok(), 16, family="llama", include_prompt=False).pool_from() is None      # no prompt: nothing to leave out
    assert pipe.pool_from("w9: ") == 2 and pipe.ids(text, True, prompt="w9: ") == [1, 112, 10, 11, 2]   # a call's own prompt
    # a prompt that ends INSIDE a token of the joined string: counted on the prompt alone, as sentence-transformers counts it
    glued = TextPipeline(_Tok(), 16, family="llama", prompt="w1 w2:", include_prompt=False)
    assert glued.ids("w7 w8", True) == [1, 4, 27 + 103, 11, 2] and glued.pool_from() == 3        # 'w2:w7' is one token of the joined string
    bert = TextPipeline(_Tok(), 16, family="bert", prompt=prompt, include_prompt=False)            # [CLS] ... [SEP]
    assert bert.ids(text, True) == [101, 4, 5, 106, 10, 11, 102] and bert.pool_from() == 4
    bare = TextPipeline(_Tok(), 16, frame=([], [2]), prompt=prompt, include_prompt=False)          # Qwen: no BOS, EOS behind
    assert bare.ids(text, True) == [4, 5, 106, 10, 11, 2] and bare.pool_from() == 3
    # truncation cuts the joined content; the frame survives
    short = TextPipeline(_Tok(), 6, family="llama", prompt=prompt, include_prompt=False)
    assert short.ids("w7 w8 w9", True) == [1, 4, 5, 106, 10, 2] and short.pool_from() == 4
    for kw in (dict(specb=True), dict(speca=True)):
        with pytest.raises(ValueError, match="prompt / include_prompt do not go together with specb / speca"):
            TextPipeline(_Tok(), 16, prompt=prompt, **kw)
        with pytest.raises(ValueError, match="prompt / include_prompt do not go together with specb / speca"):
            TextPipeline(_Tok(), 16, include_prompt=False, **kw)


class _Model:
    """Records what the adapters hand to encode_ids."""

    def __init__(self, cfg):
        self.cfg, self.device, self.calls = cfg, "cpu", []

    def encode_ids(self, seqs, mode="weightedmean", normalize=False, layer_idx=-1, **kw):
        self.calls.append(dict(seqs=seqs, mode=mode, **kw))
        return torch.zeros((len(seqs), self.cfg.hidden_size))


def test_adapters_pass_the_prompt_length_as_pool_from(tmp_path):
    from sgpt_amd.beir import CustomEmbedder
    from sgpt_amd.formats import read_st_folder, write_st_folder
    from sgpt_amd.model import SGPTConfig
    from sgpt_amd.st import SentenceTransformerSGPT, resolve_include_prompt
    cfg = SGPTConfig(model_type="llama", hidden_size=128, num_layers=1, num_heads=2, vocab_size=500, max_position_embeddings=64,
                     window_size=0, attention_layers=["global"])
    m = _Model(cfg)
    st = SentenceTransformerSGPT(m, _Tok(), max_seq_length=32, pooling_mode="mean", prompt="w1 w2: ", include_prompt=False)
    st.encode(["w7 w8", "w9"])
    assert m.calls[-1] == dict(seqs=[[1, 4, 105, 10, 11, 2], [1, 4, 105, 12, 2]], mode="mean", pool_from=3)
    st.encode(["w7"], prompt="w5: ")                                                               # the call's prompt, the module's include_prompt
    assert m.calls[-1] == dict(seqs=[[1, 108, 10, 2]], mode="mean", pool_from=2)
    st.encode(["w7"], include_prompt=True)
    assert m.calls[-1] == dict(seqs=[[1, 4, 105, 10, 2]], mode="mean")                             # everything pooled: the old call
    plain = SentenceTransformerSGPT(m, _Tok(), max_seq_length=32, pooling_mode="lasttoken")
    plain.encode(["w7"])
    assert m.calls[-1] == dict(seqs=[[1, 10, 2]], mode="lasttoken")
    plain.encode(["w7"], prompt="w1: ", include_prompt=False)
    assert m.calls[-1] == dict(seqs=[[1, 104, 10, 2]], mode="lasttoken", pool_from=2) and plain.pipe.include_prompt is True
    emb = CustomEmbedder(model=m, tokenizer=_Tok(), method="weightedmean", maxseqlen=32, prompt="w1 w2: ", include_prompt=False)
    emb.embed_device(["w7 w8"], True)
    assert m.calls[-1] == dict(seqs=[[1, 4, 105, 10, 11, 2]], mode="weightedmean", pool_from=3)
    # the folder's 1_Pooling field, and who wins
    p = str(tmp_path / "st")
    write_st_folder(p, dict(model_type="llama", hidden_size=128), {"embed_tokens.weight": np.zeros((4, 128), np.float32)}, pooling_mode="mean")
    assert read_st_folder(p).include_prompt is None
    pc = os.path.join(p, "1_Pooling", "config.json")
    for value in (False, True):
        with open(pc) as f:
            c = json.load(f)
        c["include_prompt"] = value
        with open(pc, "w") as f:
            json.dump(c, f)
        assert read_st_folder(p).include_prompt is value and read_st_folder(p).pooling_mode == "mean"
    assert [resolve_include_prompt(e, f) for e, f in ((None, None), (None, False), (None, True), (True, False), (False, True), (False, None))] == \
        [True, False, True, True, False, False]


def test_abi_v24():
    from sgpt_amd import _lib
    with open(os.path.join(ROOT, "include", "sgpt_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define SGPT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.SGPT_ABI_VERSION >= 24
    for name in ("sgpt_model_set_attention", "sgpt_attention_gqa_ex", "sgpt_encode_pool_from", "sgpt_encode_layers_pool_from",
                 "sgpt_lnf_pool_range"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr), name
    gqa, gqa_ex = _lib.SIGNATURES["sgpt_attention_gqa"][1], _lib.SIGNATURES["sgpt_attention_gqa_ex"][1]
    assert gqa_ex == gqa[:-1] + [C.c_int32, C.c_void_p] + gqa[-1:]                                 # the trailing causal, seq_len of sgpt_attention_ex
    host, frm = _lib.SIGNATURES["sgpt_encode_host_layout"][1], _lib.SIGNATURES["sgpt_encode_pool_from"][1]
    assert frm == host[:-1] + [C.c_void_p] + host[-1:]
    lay, lfrm = _lib.SIGNATURES["sgpt_encode_layers"][1], _lib.SIGNATURES["sgpt_encode_layers_pool_from"][1]
    assert lfrm == lay[:-1] + [C.c_void_p] + lay[-1:]
    ex, rng = _lib.SIGNATURES["sgpt_lnf_pool_ex"][1], _lib.SIGNATURES["sgpt_lnf_pool_range"][1]
    assert rng == ex[:-1] + [C.c_void_p] + ex[-1:]
    assert [n for n, _ in _lib.ModelDesc._fields_][-1] == "n_kv_heads"                             # the descriptor did not grow
