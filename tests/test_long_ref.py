"""CPU: sequences of more than 2048 tokens, host side -- the long fixtures (tests/golden/tiny_*_long*.npz, recipe make_golden_long.py)
against the float64 references of tests/llama_ref.py / qwen_ref.py, the one limit constant, the descriptor / rotary table rows,
Mistral's fold-and-cap rule, the max_seq_length clamp of the adapters and plan_batches with a sequence larger than a call.

The reference check carries the bound formula of tests/test_llama_ref.py::test_llama_ref_reproduces_hf unchanged: (9 L + 2) * 32 u *
max|hidden| -- a softmax over 4100 keys is still ONE fp32 stage whose output is a convex combination of V rows, so the count of
stages, not the length, sets it."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import llama_ref as R
import qwen_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
LLAMA_TAGS = ["tiny_llama_long", "tiny_llama_long_dh128", "tiny_mistral_long_window"]
TAGS = LLAMA_TAGS + ["tiny_qwen3_long"]
MODES = ("mean", "weightedmean", "lasttoken")
HF_WINDOW = {"tiny_mistral_long_window": 100}          # HF's own window, passed to the reference explicitly (not the parser's reading)


def load_long_case(tag):
    """(fixture, HF config dict, SGPTConfig, weights, sequences, cuts, hidden_rows) of a long fixture; the weights' sha is checked."""
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights, synthetic_qwen_weights
    fx = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    hf = json.loads(str(fx["cfg"]))
    cfg = SGPTConfig.from_hf_dict(hf)
    if hf["model_type"] == "qwen3":
        w = synthetic_qwen_weights(cfg, seed=int(fx["seed"]), qkv_bias=bool(fx["qkv_bias"]), qk_norm=bool(fx["qk_norm"]))
    else:
        w = synthetic_llama_weights(cfg, seed=int(fx["seed"]))
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(fx["weights_sha256"]), "the synthetic weights no longer produce the fixture's weights"
    lens = fx["seq_lens"].tolist()
    cuts = np.cumsum([0] + lens)
    seqs = [fx["ids"][a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    return fx, hf, cfg, w, seqs, cuts, fx["hidden_rows"].tolist()


def ref64(tag, w, seqs, cfg, window):
    from sgpt_amd.families import head_dim
    if tag == "tiny_qwen3_long":
        return Q.forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, window,
                         head_dim=head_dim(cfg))
    return R.forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, window)


_ref_cache = {}


def ref_forward(tag):
    """The float64 hidden states of a long fixture's sequences, computed once per session and shared (read-only)."""
    if tag not in _ref_cache:
        fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
        _ref_cache[tag] = ref64(tag, w, seqs, cfg, HF_WINDOW.get(tag, 0))
    return _ref_cache[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_long_fixtures_reproduce_the_float64_reference(tag):
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
    L = cfg.num_layers
    want_lens = [2049, 7] if tag == "tiny_qwen3_long" else [2049, 4100, 7]
    assert [len(s) for s in seqs] == want_lens and hf["max_position_embeddings"] == 4352 and cfg.max_position_embeddings == 4352
    assert cfg.window_size == HF_WINDOW.get(tag, 0)
    hs = ref_forward(tag)
    want = fx["hidden"].astype(np.float64)                       # [L + 1, recorded rows, d]
    # rows {0, 2047, 2048, last} of each long sequence (row 2048 IS the last of the 2049-token one)
    assert want.shape[:2] == (L + 1, len(rows)) and len(rows) == sum(len({0, 2047, 2048, n - 1}) for n in want_lens if n > 2048)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", tag + ".npz")) < 1 << 20
    bound = (9 * L + 2) * 32 * U32 * float(np.abs(want).max())
    worst_h = worst_p = 0.0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        for col, r in enumerate(rows):
            if a <= r < b:
                worst_h = max(worst_h, float(np.abs(hs[i][:, r - a] - want[:, col]).max()))
        for mode in MODES:
            worst_p = max(worst_p, float(np.abs(R.pool(hs[i][-1], mode) - fx[f"emb_{mode}"][i]).max()))
    print(f"{tag}: max|ref64 - HF| hidden {worst_h:.3e} pooled {worst_p:.3e} (bound {bound:.3e})")
    assert max(worst_h, worst_p) < bound


def test_the_long_fixture_needs_its_far_keys():
    """The 4100-token sequence cut to its last 2048 tokens -- what a library that stops at 2048 could offer -- moves the last token's
    final hidden row by far more than any tolerance here."""
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case("tiny_llama_long")
    full = ref_forward("tiny_llama_long")[1][-1, -1]
    cut = ref64("tiny_llama_long", w, [seqs[1][-2048:]], cfg, 0)[0][-1, -1]
    moved = float(np.abs(full - cut).max())
    print(f"truncation to the last 2048 of 4100 tokens moves the last row by {moved:.3f}")
    assert moved > 1e-2


def test_one_limit_constant():
    from sgpt_amd import _lib, families
    with open(os.path.join(ROOT, "include", "sgpt_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"#define SGPT_MAX_SEQ_LEN (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.SGPT_MAX_SEQ_LEN == families.MAX_SEQ_LEN == 32768
    assert int(re.search(r"#define SGPT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.SGPT_ABI_VERSION >= 23


QWEN_BIG = dict(model_type="qwen2", vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                intermediate_size=256, max_position_embeddings=131072, rope_theta=1000000.0, hidden_act="silu")


@pytest.mark.parametrize("max_pos, rows", [(160, 160), (4352, 4352), (32768, 32768), (131072, 32768)])
def test_descriptor_and_rotary_rows_stop_at_the_limit(max_pos, rows):
    """max_pos of the descriptor and the host rotary tables: min(max_position_embeddings, SGPT_MAX_SEQ_LEN) rows, angles still HF's
    fp32 position x fp32 inv_freq (the rows of the short table are the first rows of the full one)."""
    from sgpt_amd.families import family, rotary_tables_half, table_rows
    from sgpt_amd.model import SGPTConfig, model_desc
    cfg = SGPTConfig.from_hf_dict(dict(QWEN_BIG, max_position_embeddings=max_pos))
    assert cfg.max_position_embeddings == max_pos and table_rows(cfg) == rows
    desc, _local = model_desc(cfg, "fp32", False, "plain")
    assert desc.max_pos == rows
    t = family("llama").prepare_weights(cfg, {})
    assert t["rotary.sin"].shape == t["rotary.cos"].shape == (rows, 32) and t["rotary.sin"].dtype == np.float32
    if max_pos == 131072:
        sin, cos = rotary_tables_half(33000, 64, 1000000.0)
        assert np.array_equal(sin[:rows], t["rotary.sin"]) and np.array_equal(cos[:rows], t["rotary.cos"])


def test_mistral_fold_and_cap():
    """A window folded away caps the positions at it; a real window and `null` leave them alone."""
    from sgpt_amd.model import SGPTConfig
    base = dict(QWEN_BIG, model_type="mistral", max_position_embeddings=32768)
    for sw, window, pos in ((4096, 0, 4096), (None, 0, 32768), (100, 100, 32768), (2048, 0, 2048), (2047, 2047, 32768), (40000, 0, 32768)):
        c = SGPTConfig.from_hf_dict(dict(base, sliding_window=sw))
        assert (c.window_size, c.max_position_embeddings) == (window, pos), sw
    c = SGPTConfig.from_hf_dict(base)                               # no key: HF MistralConfig's default of 4096
    assert (c.window_size, c.max_position_embeddings) == (0, 4096)
    c = SGPTConfig.from_hf_dict(dict(base, max_position_embeddings=4352, sliding_window=2100))
    assert (c.window_size, c.max_position_embeddings) == (0, 2100)
    c = SGPTConfig.from_hf_dict(dict(base, model_type="llama", sliding_window=16))      # Llama ignores the key
    assert (c.window_size, c.max_position_embeddings) == (0, 32768)


class _Stand:
    """A model stand-in: a cfg, nothing on a device."""
    def __init__(self, cfg):
        self.cfg = cfg


def test_max_seq_length_defaults_clamp_and_refuse():
    from sgpt_amd.families import max_seq_len_of
    from sgpt_amd.model import SGPTConfig, SGPTModel
    from sgpt_amd.st import SentenceTransformerSGPT
    from sgpt_amd.tokenization import SyntheticTokenizer
    from sgpt_amd.useb import CustomEmbedder
    big = SGPTConfig(vocab_size=64, max_position_embeddings=131072)      # 131 072 positions: the library's limit binds
    small = SGPTConfig(vocab_size=64, max_position_embeddings=96)
    assert max_seq_len_of(_Stand(big)) == 32768 and max_seq_len_of(_Stand(small)) == 96 and max_seq_len_of(object()) is None
    m = SGPTModel.__new__(SGPTModel)
    m.cfg = big
    assert m.max_seq_len == 32768
    tok = SyntheticTokenizer(64)
    assert SentenceTransformerSGPT(_Stand(big), tok).max_seq_length == 300
    assert SentenceTransformerSGPT(_Stand(small), tok).max_seq_length == 96
    assert SentenceTransformerSGPT(_Stand(big), tok, max_seq_length=32768).max_seq_length == 32768
    with pytest.raises(ValueError, match="max_seq_length 32769 exceeds the 32768 tokens"):
        SentenceTransformerSGPT(_Stand(big), tok, max_seq_length=32769)
    with pytest.raises(ValueError, match="max_seq_length 97 exceeds the 96 tokens"):
        SentenceTransformerSGPT(_Stand(small), tok, max_seq_length=97)
    # over-long text is truncated by the tokeniser to the clamped length
    st = SentenceTransformerSGPT(_Stand(small), tok)
    assert max(len(s) for s in st.pipe.batch(["w%d " % i * 400 for i in range(3)], True)) <= 96
    assert CustomEmbedder(_Stand(big), tok).pipe.batch(["a b c " * 20000], True)[0].__len__() <= 32768


def test_plan_batches_gives_an_oversize_sequence_a_call_of_its_own():
    """A sequence whose allocation exceeds max_tokens_per_call: its own call -- no error, no endless loop, everything covered once."""
    from sgpt_amd.model import SGPTConfig, SGPTModel
    m = object.__new__(SGPTModel)
    m.cfg, m.max_tokens_per_call, m.device, m._num_cus = SGPTConfig(), 4096, "cpu", lambda: 256
    for lens in ([32768], [5000, 7, 130, 4100], [9000, 9000, 3, 3], [7, 32768, 4096, 4097]):
        lens = np.asarray(lens, dtype=np.int64)
        plan = m.plan_batches(lens)
        assert sorted(np.concatenate(plan).tolist()) == list(range(len(lens)))
        for sel in plan:
            rows = int(((lens[sel] + 1) // 2 * 2).sum())
            assert rows <= 4096 or len(sel) == 1, (lens, plan)
        assert all(len(sel) == 1 for sel in plan if lens[sel].max() > 4096)


def test_a_learned_position_table_is_loaded_up_to_the_limit():
    """GPT-Neo with a table beyond the limit: the descriptor names 32 768 positions and exactly those rows are handed to the library;
    a table inside the limit passes through whole."""
    from sgpt_amd.model import SGPTConfig, load_tensors, model_desc
    for rows, want in ((40000, 32768), (4352, 4352)):
        cfg = SGPTConfig(vocab_size=8, max_position_embeddings=rows, hidden_size=8, num_layers=1, num_heads=1)
        wpe = np.arange(rows, dtype=np.float32)[:, None].repeat(8, axis=1)
        t = dict(load_tensors(cfg, {"wte.weight": np.zeros((8, 8), np.float32), "wpe.weight": wpe}))
        assert model_desc(cfg, "fp32", False, "plain")[0].max_pos == want
        assert tuple(t["wpe.weight"].shape) == (want, 8) and float(t["wpe.weight"][-1, 0]) == want - 1
