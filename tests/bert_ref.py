"""Test infrastructure: the BERT forward of include/sgpt_hip.h (SGPT_ARCH_BERT) restated in float64 numpy, and the bidirectional
option of the packed attention reference.  Pinned against HF BertModel by tests/test_bert_ref.py (fixture tests/golden/tiny_bert.npz).

    x = LN_emb(wte[id] + wpe[pos] + wtt[0])
    per layer:  q | k | v = x W^T + b ; ctx = softmax(q.k^T / sqrt(dh)) v over ALL keys of the sequence
                x = LN_att(x + ctx Wo^T + bo) ; x = LN_out(x + gelu_erf(x W1^T + b1) W2^T + b2)
    hidden_states = [x after the embedding LayerNorm, x after every layer]   (L + 1 entries, as HF numbers them; no final LayerNorm)

The attention arithmetic is tests/attn_ref.py's, with every key of the sequence visible."""
import math

import numpy as np

import attn_ref


def packed_attention_bidir(q, k, v, off, lens, H: int, scale: float = 1.0) -> np.ndarray:
    """attn_ref.packed_attention with the mask of a bidirectional encoder: key j of a sequence is visible to every query of it."""
    saved = attn_ref.visible
    attn_ref.visible = lambda n, window=0: np.ones((n, n), dtype=bool)
    try:
        return attn_ref.packed_attention(q, k, v, off, lens, H, 0, scale, None)
    finally:
        attn_ref.visible = saved


def layer_norm(x, g, b, eps):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu_erf(u):
    u = np.asarray(u, np.float64)
    return 0.5 * u * (1.0 + _erf(u / math.sqrt(2.0)))


def forward(w, seqs, n_layers: int, n_heads: int, eps: float):
    """w: HF BertModel state dict (numpy, no prefix); seqs: ragged id lists.  Returns a list (one entry per sequence) of float64
    [L + 1, len, d] hidden states."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids = np.concatenate([np.asarray(s, np.int64) for s in seqs])
    pos = np.concatenate([np.arange(n) for n in lens])
    x = W["embeddings.word_embeddings.weight"][ids] + W["embeddings.token_type_embeddings.weight"][0] + \
        W["embeddings.position_embeddings.weight"][pos]
    x = layer_norm(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps)
    d = x.shape[1]
    hs = [x]
    for i in range(n_layers):
        p = f"encoder.layer.{i}."
        lin = lambda a, name: a @ W[p + name + ".weight"].T + W[p + name + ".bias"]  # noqa: E731
        q, k, v = lin(x, "attention.self.query"), lin(x, "attention.self.key"), lin(x, "attention.self.value")
        ctx = packed_attention_bidir(q, k, v, off, lens, n_heads, 1.0 / math.sqrt(d // n_heads))
        x = layer_norm(x + lin(ctx, "attention.output.dense"), W[p + "attention.output.LayerNorm.weight"],
                       W[p + "attention.output.LayerNorm.bias"], eps)
        h = gelu_erf(lin(x, "intermediate.dense"))
        x = layer_norm(x + lin(h, "output.dense"), W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        hs.append(x)
    hs = np.stack(hs)                                   # [L + 1, rows, d]
    return [hs[:, o:o + n] for o, n in zip(off.tolist(), lens)]


def pool(h, mode: str):
    """h float64 [len, d] -> [d]: 'mean' over the tokens (Pooling.py:117-125, all real) or 'cls' (row 0, :103-105)."""
    return h.mean(0) if mode == "mean" else h[0]
