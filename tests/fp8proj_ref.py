"""Test infrastructure: the forward of a Llama-family model with fp8 projections (sgpt_model_set_projections(1), include/sgpt_hip.h ABI
v25) restated in float64 numpy on the pieces of tests/llama_ref.py / qwen_ref.py and the oracle's e4m3fn tables.

    weights     rounded to bf16 (what the loaded model holds); q | k | v, gate | up and down then quantised per output row:
                scale = the smallest 2^k with max|row| / 2^k <= 448, code = RNE e4m3fn(w / scale); o_proj stays bf16
    per layer   a8 = Q(RMS1(x)) ; q | k | v = bf16(a8 W8^T (+ b)) ; [head norm,] rotary -> bf16 ; ctx = bf16(attention) ;
                x += ctx Wo^T ; a8 = Q(RMS2(x)) ; gate | up = bf16(a8 W8^T) ; h8 = Q(silu(gate) * up) ; x += h8 Wdown8^T
    Q(v)        per token row: one power-of-two scale by the same rule, RNE e4m3fn codes; the value carried on is code * scale

fp8=False is the float64 forward itself (qwen_ref.forward with the bidirectional mask as an option): the reference both the emulation
and the device are measured against.  The residual stream, the norms, the softmax and every k-sum are float64 here and fp32 on the
device: at these widths one flipped e4m3 code moves a K = 256 sum by 0.4 %, so device and emulation agree statistically, not bit for bit
(tests/test_gpu_fp8proj_model.py bounds the device by twice the emulation's own deviation)."""
import math
import os
import sys

import numpy as np

import attn_ref
from bert_ref import packed_attention_bidir
from llama_ref import pool, repeat_kv, rms_norm, rope_half, silu  # noqa: F401
from qwen_ref import qknorm_rope_half, round16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import sgpt_oracle as O  # noqa: E402


def pow2_scale(amax):
    """The row-scale rule on a float64 (or fp32) row maximum: the smallest 2^k, k in [-126, 127], with amax / 2^k <= 448; 1 for 0."""
    amax = np.asarray(amax, np.float64)
    m, e = np.frexp(amax)                                   # amax = m 2^e, 0.5 <= m < 1;  448 = 0.875 * 2^9
    k = np.clip(np.where(m <= 0.875, e - 9, e - 8), -126, 127)
    return np.where(amax > 0, np.ldexp(1.0, k), 1.0)


def switch_margin(amax):
    """Relative distance of a row maximum from the nearest point where the scale rule switches (1.75 x 2^e): a reference maximum
    closer to one than the error bound of the arithmetic that produced it may legitimately land on either scale."""
    amax = np.asarray(amax, np.float64)
    m, _ = np.frexp(np.where(amax > 0, amax, 1.0))
    return np.minimum(np.abs(m - 0.875) / 0.875, np.minimum(np.abs(m - 0.4375) / 0.4375, np.abs(m - 1.75) / 1.75))   # this binade's, the neighbours'


def quantize_rows(v):
    """float64 [rows, cols] -> (codes uint8, scale float64 [rows]): the values are cast to fp32 first (the device holds fp32 rows), the
    division by a power of two is exact."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    s = pow2_scale(np.abs(v32).max(axis=1))
    return O.fp8_e4m3fn_encode((v32.astype(np.float64) / s[:, None]).astype(np.float32)), s


def dequantize_rows(codes, scale):
    return O.fp8_e4m3fn_decode(codes).astype(np.float64) * np.asarray(scale, np.float64)[:, None]


def qdq(v):
    """Q(v): the values a quantised operand carries into its k-sum."""
    return dequantize_rows(*quantize_rows(v))


def forward(w, seqs, n_layers: int, n_heads: int, n_kv: int, eps: float, theta: float = 10000.0, head_dim=None, bidir: bool = False,
            fp8: bool = False):
    """w: HF LlamaModel / Qwen2Model / Qwen3Model state dict (numpy, no prefix); seqs: ragged id lists.  Returns a list (one entry per
    sequence) of float64 [L + 1, len, d] hidden states."""
    r = round16("bf16") if fp8 else (lambda x: x)           # where the device stores bf16
    q8 = qdq if fp8 else (lambda x: x)                      # where it stores e4m3 codes + a row scale
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
        a = q8(rms_norm(x, W[f"layers.{i}.input_layernorm.weight"], eps))
        q, k, v = (r(a @ q8(r(W[p + n + "_proj.weight"])).T + W.get(p + n + "_proj.bias", 0.0)) for n in "qkv")
        if p + "q_norm.weight" in W:
            q = qknorm_rope_half(q, W[p + "q_norm.weight"], pos, n_heads, dh, eps, theta=theta)
            k = qknorm_rope_half(k, W[p + "k_norm.weight"], pos, n_kv, dh, eps, theta=theta)
        else:
            q, k = rope_half(q, pos, n_heads, dh, theta), rope_half(k, pos, n_kv, dh, theta)
        kk, vv = repeat_kv(r(k), n_kv, g, dh), repeat_kv(v, n_kv, g, dh)
        if bidir:
            ctx = packed_attention_bidir(r(q), kk, vv, off, lens, n_heads, 1.0 / math.sqrt(dh))
        else:
            ctx = attn_ref.packed_attention(r(q), kk, vv, off, lens, n_heads, 0, 1.0 / math.sqrt(dh))
        x = x + r(ctx) @ r(W[p + "o_proj.weight"]).T
        m = f"layers.{i}.mlp."
        a = q8(rms_norm(x, W[f"layers.{i}.post_attention_layernorm.weight"], eps))
        gate, up = r(a @ q8(r(W[m + "gate_proj.weight"])).T), r(a @ q8(r(W[m + "up_proj.weight"])).T)
        x = x + q8(silu(gate) * up) @ q8(r(W[m + "down_proj.weight"])).T
    hs.append(rms_norm(x, W["norm.weight"], eps))
    hs = np.stack(hs)                                       # [L + 1, rows, d]
    return [hs[:, o:o + n] for o, n in zip(off.tolist(), lens)]


# ---- the test models of tests/test_fp8proj_ref.py and tests/test_gpu_fp8proj_model.py: weights from seeds, no fixture files ----
VOCAB, MAX_POS, EPS = 300, 128, 1e-6
LENS = [1, 9, 17, 26, 35, 44, 53, 64]                       # eight sequences of 1 ... 64 tokens
MODES = ("mean", "weightedmean", "lasttoken")
#          hidden, heads, kv heads, explicit head dim, ffn, layers, qkv bias, head norm, weight std, seed
MODELS = {
    "llama": (256, 4, 4, 0, 512, 2, False, False, 0.05, 11),
    "gqa": (512, 8, 4, 0, 1024, 2, False, False, 0.03, 12),
    "qwen3": (256, 8, 4, 64, 768, 2, False, True, 0.05, 13),    # query width 512 != hidden 256, key / value width 256
    "qwen2": (256, 4, 4, 0, 512, 2, True, False, 0.02, 14),
}


def make_model(tag: str, n_layers=None):
    """-> (SGPTConfig, HF-named numpy state dict, token lists)."""
    from sgpt_amd.families import SGPTConfig, synthetic_qwen_weights
    d, H, kv, dh, ffn, L, bias, norm, std, seed = MODELS[tag]
    cfg = SGPTConfig(model_type="llama", vocab_size=VOCAB, max_position_embeddings=MAX_POS, hidden_size=d, num_layers=n_layers or L, num_heads=H,
                     num_kv_heads=kv, intermediate_size=ffn, window_size=0, rotary_dim=dh, layer_norm_epsilon=EPS)
    w = synthetic_qwen_weights(cfg, seed=seed, qkv_bias=bias, qk_norm=norm, std=std)
    rng = np.random.default_rng(1000 + seed)
    seqs = [rng.integers(0, VOCAB, size=n).tolist() for n in LENS]
    return cfg, w, seqs


def ref_forward(tag: str, fp8: bool, bidir: bool = False):
    from sgpt_amd.families import head_dim
    cfg, w, seqs = make_model(tag)
    return forward(w, seqs, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, theta=cfg.rope_theta,
                   head_dim=head_dim(cfg), bidir=bidir, fp8=fp8)


def unit(e):
    e = np.asarray(e, np.float64)
    return e / np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-12)


def embeddings(hidden, mode: str, pool_from=None):
    """Hidden states of forward() -> unit embeddings float64 [n, d] of the last hidden state (pool_from: rows behind that token)."""
    from llama_bidir_ref import pool_range
    return unit(np.stack([pool(h[-1], mode) if pool_from is None else pool_range(h[-1], mode, pool_from) for h in hidden]))


def deviation(e, ref):
    """(max |e - ref|, max |cos(e) - cos(ref)|) of two sets of unit embeddings."""
    return float(np.abs(e - ref).max()), float(np.abs(e @ e.T - ref @ ref.T).max())


if __name__ == "__main__":      # the E lines of profiles/llama_fp8_projections.txt
    for tag in MODELS:
        ref, emu = ref_forward(tag, fp8=False), ref_forward(tag, fp8=True)
        for mode in MODES:
            de, dcos = deviation(embeddings(emu, mode), embeddings(ref, mode))
            print(f"E {tag:6s} {mode:12s} max|de| = {de:.3e}  max|dcos| = {dcos:.3e}")
