"""Test infrastructure: the Llama / Mistral forward of include/sgpt_hip.h (SGPT_ARCH_LLAMA) restated in float64 numpy.  Pinned against
HF LlamaModel / MistralModel by tests/test_llama_ref.py (fixtures tests/golden/tiny_llama*.npz, tiny_mistral_window.npz).

    x = wte[id]
    per layer:  a = RMS1(x) ; q | k | v = a W^T (H query heads, H_kv key / value heads) ; rotate_half rotary on q and k ;
                x += softmax(q.k^T / sqrt(dh), causal, window) v Wo^T with query head h reading key / value head h // (H / H_kv) ;
                a = RMS2(x) ; x += (silu(a Wgate^T) * (a Wup^T)) Wdown^T
    hidden_states = [x before every layer ..., RMS_f(x after the last)]     (L + 1 entries, as HF numbers them)

The attention arithmetic is tests/attn_ref.py's, fed K / V heads repeated with np.repeat."""
import math

import numpy as np

import attn_ref


def rms_norm(x, g, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * np.asarray(g, np.float64)


def silu(u):
    u = np.asarray(u, np.float64)
    return u / (1.0 + np.exp(-u))


def swiglu(gu):
    """gu float [T, 2 ffn] = gate | up columns -> silu(gate) * up, float64 [T, ffn]."""
    gu = np.asarray(gu, np.float64)
    ffn = gu.shape[1] // 2
    return silu(gu[:, :ffn]) * gu[:, ffn:]


def inv_freq(head_dim: int, theta: float = 10000.0):
    return theta ** (-np.arange(0, head_dim, 2, dtype=np.float64) / head_dim)


def rope_half(x, pos, n_heads: int, head_dim: int, theta: float = 10000.0, sin=None, cos=None):
    """HF rotate_half on x [T, n_heads * head_dim] (float64): x[i] pairs with x[i + head_dim / 2].  sin / cos [max_pos, head_dim / 2]
    tables may be given (the kernel's own tables, positions clamped into them); else exact float64 angles."""
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    half = head_dim // 2
    if sin is None:
        ang = np.asarray(pos, np.float64)[:, None] * inv_freq(head_dim, theta)[None, :]
        s, c = np.sin(ang), np.cos(ang)
    else:
        p = np.clip(np.asarray(pos, np.int64), 0, sin.shape[0] - 1)
        s, c = np.asarray(sin, np.float64)[p], np.asarray(cos, np.float64)[p]
    xh = x.reshape(T, n_heads, head_dim)
    lo, hi = xh[..., :half], xh[..., half:]
    out = np.concatenate([lo * c[:, None, :] - hi * s[:, None, :], hi * c[:, None, :] + lo * s[:, None, :]], axis=-1)
    return out.reshape(T, n_heads * head_dim)


def repeat_kv(k, n_kv: int, group: int, head_dim: int):
    """[T, n_kv * head_dim] -> [T, n_kv * group * head_dim]: every key / value head `group` times in a row (HF repeat_kv)."""
    T = k.shape[0]
    return np.repeat(np.asarray(k).reshape(T, n_kv, head_dim), group, axis=1).reshape(T, n_kv * group * head_dim)


def forward(w, seqs, n_layers: int, n_heads: int, n_kv: int, eps: float, theta: float = 10000.0, window: int = 0):
    """w: HF LlamaModel state dict (numpy, no prefix); seqs: ragged id lists.  Returns a list (one entry per sequence) of float64
    [L + 1, len, d] hidden states."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids = np.concatenate([np.asarray(s, np.int64) for s in seqs])
    pos = np.concatenate([np.arange(n) for n in lens])
    x = W["embed_tokens.weight"][ids]
    d = x.shape[1]
    dh = d // n_heads
    hs = []
    for i in range(n_layers):
        hs.append(x)
        p = f"layers.{i}."
        a = rms_norm(x, W[p + "input_layernorm.weight"], eps)
        q = rope_half(a @ W[p + "self_attn.q_proj.weight"].T, pos, n_heads, dh, theta)
        k = rope_half(a @ W[p + "self_attn.k_proj.weight"].T, pos, n_kv, dh, theta)
        v = a @ W[p + "self_attn.v_proj.weight"].T
        g = n_heads // n_kv
        ctx = attn_ref.packed_attention(q, repeat_kv(k, n_kv, g, dh), repeat_kv(v, n_kv, g, dh), off, lens, n_heads, window,
                                        1.0 / math.sqrt(dh))
        x = x + ctx @ W[p + "self_attn.o_proj.weight"].T
        a = rms_norm(x, W[p + "post_attention_layernorm.weight"], eps)
        h = silu(a @ W[p + "mlp.gate_proj.weight"].T) * (a @ W[p + "mlp.up_proj.weight"].T)
        x = x + h @ W[p + "mlp.down_proj.weight"].T
    hs.append(rms_norm(x, W["norm.weight"], eps))
    hs = np.stack(hs)                                   # [L + 1, rows, d]
    return [hs[:, o:o + n] for o, n in zip(off.tolist(), lens)]


def pool(h, mode: str):
    """h float64 [len, d] -> [d]: 'mean', 'weightedmean' (weights 1 .. len, Pooling.py:99-125) or 'lasttoken'."""
    if mode == "mean":
        return h.mean(0)
    if mode == "lasttoken":
        return h[-1]
    wgt = np.arange(1, len(h) + 1, dtype=np.float64)
    return (h * wgt[:, None]).sum(0) / wgt.sum()
