"""Test infrastructure: the Qwen2 / Qwen3 members of the Llama family (SGPT_ARCH_LLAMA, include/sgpt_hip.h ABI v16) restated in float64
numpy on top of tests/llama_ref.py.  Pinned against HF Qwen2Model / Qwen3Model by tests/test_qwen_ref.py (fixtures
tests/golden/tiny_qwen*.npz).

What they add to llama_ref.forward:
    q | k | v = a W^T + b          where the state dict has q_proj / k_proj / v_proj .bias (Qwen2)
    q, k = RMS_head(q), RMS_head(k)  per head over head_dim, gains q_norm.weight / k_norm.weight [head_dim] shared by the heads, before
                                     the rotary (Qwen3)
    head_dim of its own            n_heads * head_dim columns of q (and rows of o_proj's input) need not be d (Qwen3)

`rnd` (optional) rounds a value wherever the 16-bit forward of the library stores one -- the matmul weights, the RMSNorm outputs, q | k
behind the projection and behind the rotary, V, the attention context, gate | up and h -- so that the same code emulates the bf16 / f16
forwards on the CPU (test_qwen_ref.py holds the emulated error to half the GPU test's bar)."""
import math

import numpy as np

import attn_ref
from llama_ref import pool, repeat_kv, rms_norm, rope_half, silu  # noqa: F401


def head_rms_norm(x, g, n_heads: int, head_dim: int, eps: float):
    """x [T, n_heads * head_dim] -> every head normalised over head_dim with the gain g [head_dim]."""
    T = x.shape[0]
    return rms_norm(np.asarray(x, np.float64).reshape(T, n_heads, head_dim), g, eps).reshape(T, n_heads * head_dim)


def qknorm_rope_half(x, g, pos, n_heads: int, head_dim: int, eps: float, sin=None, cos=None, theta: float = 10000.0):
    """The fused kernel's arithmetic on one block of heads: the head norm, then llama_ref.rope_half."""
    return rope_half(head_rms_norm(x, g, n_heads, head_dim, eps), pos, n_heads, head_dim, theta, sin=sin, cos=cos)


def round16(fmt: str):
    """x -> x rounded (RNE) to 'bf16' | 'f16', as float64."""
    import torch
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    return lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dt).to(torch.float64).numpy()


def forward(w, seqs, n_layers: int, n_heads: int, n_kv: int, eps: float, theta: float = 10000.0, window: int = 0, head_dim=None,
            rnd=None):
    """w: HF Qwen2Model / Qwen3Model (or LlamaModel) state dict (numpy, no prefix); seqs: ragged id lists.  Returns a list (one entry
    per sequence) of float64 [L + 1, len, d] hidden states."""
    r = rnd if rnd is not None else (lambda x: x)
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ids = np.concatenate([np.asarray(s, np.int64) for s in seqs])
    pos = np.concatenate([np.arange(n) for n in lens])
    x = W["embed_tokens.weight"][ids]
    d = x.shape[1]
    dh = head_dim or d // n_heads
    g = n_heads // n_kv
    hs = []
    for i in range(n_layers):
        hs.append(x)
        p = f"layers.{i}.self_attn."
        a = r(rms_norm(x, W[f"layers.{i}.input_layernorm.weight"], eps))
        q, k, v = (a @ r(W[p + n + "_proj.weight"]).T + W.get(p + n + "_proj.bias", 0.0) for n in "qkv")
        if p + "q_norm.weight" in W:
            q = qknorm_rope_half(r(q), W[p + "q_norm.weight"], pos, n_heads, dh, eps, theta=theta)
            k = qknorm_rope_half(r(k), W[p + "k_norm.weight"], pos, n_kv, dh, eps, theta=theta)
        else:
            q, k = rope_half(r(q), pos, n_heads, dh, theta), rope_half(r(k), pos, n_kv, dh, theta)
        ctx = attn_ref.packed_attention(r(q), repeat_kv(r(k), n_kv, g, dh), repeat_kv(r(v), n_kv, g, dh), off, lens, n_heads, window,
                                        1.0 / math.sqrt(dh))
        x = x + r(ctx) @ r(W[p + "o_proj.weight"]).T
        m = f"layers.{i}.mlp."
        a = r(rms_norm(x, W[f"layers.{i}.post_attention_layernorm.weight"], eps))
        gate, up = r(a @ r(W[m + "gate_proj.weight"]).T), r(a @ r(W[m + "up_proj.weight"]).T)
        x = x + r(silu(gate) * up) @ r(W[m + "down_proj.weight"]).T
    hs.append(rms_norm(x, W["norm.weight"], eps))
    hs = np.stack(hs)                                   # [L + 1, rows, d]
    return [hs[:, o:o + n] for o, n in zip(off.tolist(), lens)]
