"""CPU: the BERT family's host side -- the float64 reference of tests/bert_ref.py against HF BertModel's recorded values
(tests/golden/tiny_bert*.npz, recipe make_golden_bert.py), config parsing, state-dict mapping, [CLS] / [SEP] framing and the
sentence-transformers `cls` pooling flag.

Tolerance of the reference check.  The fixture is HF's fp32 forward, the reference float64, so the difference is fp32 rounding
alone (u = 2^-24).  tests/test_rowops_ref.py holds one fp32 row operation (LayerNorm + pooling) to 2e-6 |ref| ~ 32 u |ref| against
float64; a BERT layer chains six such stages on every element (Q | K | V projection, softmax . V, out-projection + LayerNorm, fc1 +
GELU, fc2 + LayerNorm -- the two LayerNorms re-normalise, they do not shrink an absolute error below their input's), the embedding
LayerNorm and the pooling are two more: (6 L + 2) * 32 u * max|hidden|."""
import hashlib
import json
import os

import numpy as np
import pytest

import bert_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def load_bert_case(tag):
    from sgpt_amd.model import SGPTConfig, synthetic_bert_weights
    fx = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    hf = json.loads(str(fx["cfg"]))
    cfg = SGPTConfig.from_hf_dict(hf)
    w = synthetic_bert_weights(cfg, seed=int(fx["seed"]))
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(fx["weights_sha256"]), "synthetic_bert_weights no longer produces the fixture's weights"
    lens = fx["seq_lens"].tolist()
    cuts = np.cumsum([0] + lens)
    seqs = [fx["ids"][a:b].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    return fx, hf, cfg, w, seqs, cuts


@pytest.mark.parametrize("tag", ["tiny_bert", "tiny_bert_dh128"])
def test_bert_ref_reproduces_hf_bertmodel(tag):
    fx, hf, cfg, w, seqs, cuts = load_bert_case(tag)
    L = cfg.num_layers
    hs = B.forward(w, seqs, L, cfg.num_heads, cfg.layer_norm_epsilon)
    want = fx["hidden"].astype(np.float64)                       # [L + 1, rows, d]
    assert want.shape[0] == L + 1
    bound = (6 * L + 2) * 32 * U32 * float(np.abs(want).max())
    worst = 0.0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        assert seqs[i][0] == 1 and (len(seqs[i]) < 2 or seqs[i][-1] == 2)       # [CLS] ... [SEP]
        worst = max(worst, float(np.abs(hs[i] - want[:, a:b]).max()))
        for mode in ("mean", "cls"):
            worst = max(worst, float(np.abs(B.pool(hs[i][-1], mode) - fx[f"emb_{mode}"][i]).max()))
    print(f"{tag}: max|bert_ref - HF| = {worst:.3e} (bound {bound:.3e})")
    assert worst < bound


def test_bidirectional_attention_reference_properties():
    """Every key of the own sequence is seen (a future key moves the output), none of a neighbour's; length 1 == causal."""
    import attn_ref
    rng = np.random.default_rng(0)
    lens = [1, 5, 4]
    off, alloc, T, _ = attn_ref.layout(lens)
    q, k, v = (rng.standard_normal((T, 2 * 8)) for _ in range(3))
    base = B.packed_attention_bidir(q, k, v, off, lens, 2, 0.3)
    causal = attn_ref.packed_attention(q, k, v, off, lens, 2, 0, 0.3)
    assert np.array_equal(base[off[0]], causal[off[0]])                          # one token: the two masks agree
    assert np.abs(base[off[1]] - causal[off[1]]).max() > 1e-3                    # query 0 of a longer sequence sees its future
    assert attn_ref.visible(3).tolist() == [[True, False, False], [True, True, False], [True, True, True]]   # restored
    v2 = v.copy()
    v2[off[1] + 4] += 1.0                                                        # last key of sequence 1
    moved = B.packed_attention_bidir(q, k, v2, off, lens, 2, 0.3)
    assert np.abs(moved[off[1]] - base[off[1]]).max() > 1e-3
    assert np.array_equal(moved[off[2]:off[2] + 4], base[off[2]:off[2] + 4]) and np.array_equal(moved[off[0]], base[off[0]])
    # uniform keys: the context is the plain mean of v over the whole sequence
    out = B.packed_attention_bidir(np.ones((4, 8)), np.ones((4, 8)), np.arange(32.0).reshape(4, 8), [0], [4], 1, 1.0)
    assert np.allclose(out, np.arange(32.0).reshape(4, 8).mean(0)[None, :], atol=1e-12)


BERT_CFG = dict(model_type="bert", vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                intermediate_size=3072, max_position_embeddings=512, layer_norm_eps=1e-12, type_vocab_size=2, hidden_act="gelu",
                position_embedding_type="absolute")


def test_config_accepts_bert_and_rejects_what_is_not_built():
    from sgpt_amd.model import SGPTConfig
    c = SGPTConfig.from_hf_dict(BERT_CFG)
    assert (c.model_type, c.hidden_size, c.num_layers, c.num_heads, c.intermediate_size, c.max_position_embeddings, c.vocab_size) == \
        ("bert", 768, 12, 12, 3072, 512, 30522)
    assert c.layer_norm_epsilon == 1e-12 and c.window_size == 0 and set(c.attention_layers) == {"global"}
    with pytest.raises(NotImplementedError, match="hidden_act"):
        SGPTConfig.from_hf_dict(dict(BERT_CFG, hidden_act="relu"))
    with pytest.raises(NotImplementedError, match="position_embedding_type"):
        SGPTConfig.from_hf_dict(dict(BERT_CFG, position_embedding_type="relative_key"))
    with pytest.raises(NotImplementedError):
        SGPTConfig.from_hf_dict(dict(BERT_CFG, model_type="roberta"))


def test_bert_state_dict_mapping_prefix_pooler_and_token_types():
    from sgpt_amd.model import SGPTConfig, bert_state_dict, synthetic_bert_weights
    cfg = SGPTConfig.from_hf_dict(dict(BERT_CFG, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                                       vocab_size=50, max_position_embeddings=16))
    w = synthetic_bert_weights(cfg, seed=3)
    extra = {"pooler.dense.weight": np.zeros((128, 128), np.float32), "pooler.dense.bias": np.zeros(128, np.float32),
             "embeddings.position_ids": np.arange(16)[None]}
    plain = bert_state_dict({**w, **extra})
    prefixed = bert_state_dict({**{"bert." + k: v for k, v in {**w, **extra}.items()}, "cls.predictions.bias": np.zeros(50, np.float32)})
    assert set(plain) == set(prefixed) == set(w) - {"embeddings.token_type_embeddings.weight"}
    assert not any(k.startswith(("pooler", "cls", "bert.")) or k.endswith("position_ids") for k in plain)
    want = w["embeddings.position_embeddings.weight"] + w["embeddings.token_type_embeddings.weight"][0][None, :]
    for sd in (plain, prefixed):
        assert np.array_equal(np.asarray(sd["embeddings.position_embeddings.weight"]), want)     # token type 0 folded in, fp32
        assert np.array_equal(np.asarray(sd["encoder.layer.0.attention.self.query.weight"]), w["encoder.layer.0.attention.self.query.weight"])


def _bert_tokenizer(words):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    vocab = {w: i for i, w in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(words))}
    tk = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    return PreTrainedTokenizerFast(tokenizer_object=tk, unk_token="[UNK]", pad_token="[PAD]", cls_token="[CLS]", sep_token="[SEP]")


def test_text_pipeline_frames_bert_inputs_and_truncates_first():
    """beir_dense_retriever.py:128-136: the content is cut to max_len - 2, THEN [CLS] ... [SEP] go around it."""
    from sgpt_amd.tokenization import TextPipeline
    words = [f"w{i}" for i in range(20)]
    tok = _bert_tokenizer(words)
    assert tok.cls_token_id == 2 and tok.sep_token_id == 3 and tok.is_fast
    pipe = TextPipeline(tok, 8, family="bert")
    assert pipe.max_token_len == 6
    short, long_ = "w0 w1 w2", " ".join(words[:12])
    for got in (pipe.batch([short, long_], True), [pipe.ids(short, False), pipe.ids(long_, False)]):   # batched and per-text paths
        assert got[0] == [2, 4, 5, 6, 3]
        assert got[1] == [2] + list(range(4, 10)) + [3] and len(got[1]) == 8
    assert pipe.docs_truncated == 2 and pipe.toks_truncated == 12
    plain = TextPipeline(tok, 8)                                   # not a BERT model: no framing, as before
    assert plain.ids(short, True) == [4, 5, 6]
    for kw in (dict(specb=True), dict(speca=True)):
        with pytest.raises(ValueError, match="BERT"):
            TextPipeline(tok, 8, family="bert", **kw)
    from sgpt_amd.tokenization import SyntheticTokenizer
    with pytest.raises(ValueError, match="cls_token_id"):
        TextPipeline(SyntheticTokenizer(100), 8, family="bert")


def test_st_folder_cls_flag_round_trip(tmp_path):
    from sgpt_amd import _lib
    from sgpt_amd.formats import pooling_mode_from_config, read_st_folder, write_st_folder
    assert _lib.POOL_MODES["cls"] == 4 and _lib.SGPT_ARCH_BERT == 3
    p = str(tmp_path / "sbert")
    write_st_folder(p, dict(BERT_CFG, hidden_size=128), {"embeddings.word_embeddings.weight": np.zeros((4, 128), np.float32)},
                    pooling_mode="cls", max_seq_length=75, normalize=True)
    spec = read_st_folder(p)
    assert spec.pooling_mode == "cls" and spec.max_seq_length == 75 and spec.normalize
    pc = json.load(open(os.path.join(p, "1_Pooling", "config.json")))
    assert pc["pooling_mode_cls_token"] is True and sum(bool(v) for k, v in pc.items() if k.startswith("pooling_mode")) == 1
    with pytest.raises(NotImplementedError):
        pooling_mode_from_config(dict(pc, pooling_mode_mean_tokens=True))          # two flags at once
    for flag in ("pooling_mode_max_tokens", "pooling_mode_mean_sqrt_len_tokens"):
        with pytest.raises(NotImplementedError):
            pooling_mode_from_config({flag: True})
