"""Test infrastructure: the BIDIRECTIONAL forward of a Llama-family model (SGPT_ARCH_LLAMA after sgpt_model_set_attention(0),
include/sgpt_hip.h ABI v24) restated in float64 numpy on the pieces of tests/llama_ref.py, and the pooling over the rows behind a
prompt.  Pinned against HF LlamaModel / Qwen2Model run with an all-zero 4-D mask by tests/test_llama_bidir_ref.py (fixtures
tests/golden/tiny_*_bidir.npz, recipe make_golden_bidir.py).

    x = wte[id]
    per layer:  a = RMS1(x) ; q | k | v = a W^T (+ b where the state dict has the three biases: Qwen2) ; rotate_half rotary on q and k ;
                x += softmax(q.k^T / sqrt(dh) over ALL keys of the sequence) v Wo^T, query head h reading key / value head h // (H / H_kv) ;
                a = RMS2(x) ; x += (silu(a Wgate^T) * (a Wup^T)) Wdown^T
    hidden_states = [x before every layer ..., RMS_f(x after the last)]

Everything but the mask is llama_ref.forward's block: the positions, the rotary and the norms do not know the attention mode."""
import math

import numpy as np

from bert_ref import packed_attention_bidir
from llama_ref import repeat_kv, rms_norm, rope_half, silu


def forward(w, seqs, n_layers: int, n_heads: int, n_kv: int, eps: float, theta: float = 10000.0):
    """w: HF LlamaModel / Qwen2Model state dict (numpy, no prefix); seqs: ragged id lists.  Returns a list (one entry per sequence) of
    float64 [L + 1, len, d] hidden states."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids = np.concatenate([np.asarray(s, np.int64) for s in seqs])
    pos = np.concatenate([np.arange(n) for n in lens])
    x = W["embed_tokens.weight"][ids]
    dh = x.shape[1] // n_heads
    g = n_heads // n_kv
    hs = []
    for i in range(n_layers):
        hs.append(x)
        p = f"layers.{i}."
        a = rms_norm(x, W[p + "input_layernorm.weight"], eps)
        q, k, v = (a @ W[p + f"self_attn.{n}_proj.weight"].T + W.get(p + f"self_attn.{n}_proj.bias", 0.0) for n in "qkv")
        q, k = rope_half(q, pos, n_heads, dh, theta), rope_half(k, pos, n_kv, dh, theta)
        ctx = packed_attention_bidir(q, repeat_kv(k, n_kv, g, dh), repeat_kv(v, n_kv, g, dh), off, lens, n_heads, 1.0 / math.sqrt(dh))
        x = x + ctx @ W[p + "self_attn.o_proj.weight"].T
        a = rms_norm(x, W[p + "post_attention_layernorm.weight"], eps)
        x = x + (silu(a @ W[p + "mlp.gate_proj.weight"].T) * (a @ W[p + "mlp.up_proj.weight"].T)) @ W[p + "mlp.down_proj.weight"].T
    hs.append(rms_norm(x, W["norm.weight"], eps))
    hs = np.stack(hs)
    return [hs[:, o:o + n] for o, n in zip(off.tolist(), lens)]


def pool_range(h, mode: str, lo: int = 0, pad_left: int = 0):
    """h float64 [len, d] -> [d], pooled over the rows [min(max(lo, 0), len), len) (include/sgpt_hip.h::sgpt_encode_pool_from):
    'mean' over that range; 'weightedmean' with the weight of row t still pad_left + t + 1, the padded position index -- it does not
    restart behind the prompt; both over a denominator clamped at 1e-9, so an empty range is a zero row; 'lasttoken' is row len - 1
    whatever lo is."""
    h = np.asarray(h, np.float64)
    n = h.shape[0]
    if mode == "lasttoken":
        return h[-1]
    lo = min(max(int(lo), 0), n)
    wgt = (np.arange(n, dtype=np.float64) + pad_left + 1.0 if mode == "weightedmean" else np.ones(n))[lo:]
    return (h[lo:] * wgt[:, None]).sum(0) / max(float(wgt.sum()), 1e-9)
