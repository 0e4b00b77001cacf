"""-m gpu: fp8 projections of the Llama family end to end (SGPTModel(projections='fp8'), sgpt_model_set_projections, ABI v25) on the
seeded models of tests/fp8proj_ref.py -- a tiny Llama, a grouped-K/V one, a Qwen3-style one (head norm, query width 512 over hidden 256)
and a Qwen2-style one (QKV bias); eight sequences of 1 ... 64 tokens.

Conversion   bytes_freed is the 16-bit bytes of w_qkv, w_fc and w_proj minus codes and scales; one-way; the C refusals by message.
Composition  hidden_out of a converted 1-layer model is bit-identical to the block run from the stand-alone entries in the forward's
             order (sgpt_embed, sgpt_rmsnorm_fp8, sgpt_linear_fp8, sgpt_rope_half / sgpt_qknorm_rope_half, sgpt_attention_gqa,
             sgpt_linear, sgpt_swiglu_fp8) on weights from sgpt_fp8_quantize_rows of the bf16-rounded tensors: a wrong scale pointer,
             row offset or weight rule is a bit difference.
End to end   max |e - e_float64| <= 2 E on unit embeddings, E = the float64 emulation's own deviation for that model and pooling mode,
             computed here.  The emulation and the device agree statistically only -- perturbing the emulation's activations by 1e-6
             relative moves the embeddings by 1e-3 ... 7e-3, one flipped e4m3 code being 0.4 % of a K = 256 sum -- so 2 E covers that
             noise, and a wiring error is O(1).  Measured on the MI355X, max |e - e_float64| / E: llama 0.97 - 1.00, gqa 1.01 - 1.08,
             qwen3 1.01 - 1.10, qwen2 0.92 - 0.99, bidirectional with pool_from 0.85 - 0.86 (profiles/llama_fp8_projections.txt)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fp8proj_ref as F
from test_fp8proj_ref import emulated_deviation

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


_models = {}


def model(tag, projections="fp8", n_layers=None, attention="causal"):
    from sgpt_amd import SGPTModel
    key = (tag, projections, n_layers, attention)
    if key not in _models:
        cfg, w, seqs = F.make_model(tag, n_layers)
        _models[key] = SGPTModel(cfg, w, device="cuda:0", dtype="bf16", projections=projections, attention=attention)
    return _models[key]


def last_error(ctx):
    return (ctx.lib.sgpt_last_error(ctx.handle) or b"").decode()


def expected_bytes_freed(cfg):
    from sgpt_amd.families import head_dim
    d, ffn, dh = cfg.hidden_size, cfg.intermediate_size, head_dim(cfg)
    rows_cols = [(cfg.num_heads * dh + 2 * cfg.num_kv_heads * dh, d), (2 * ffn, d), (d, ffn)]
    return cfg.num_layers * sum(r * c * 2 - (r * c + r * 4) for r, c in rows_cols)


# ---- conversion -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["llama", "qwen3"])
def test_conversion_frees_the_16bit_bytes_and_is_one_way(ctx, tag):
    from sgpt_amd import SGPTModel
    cfg, w, seqs = F.make_model(tag)
    m = SGPTModel(cfg, w, device="cuda:0", dtype="bf16")
    lib = ctx.lib
    kind, freed = C.c_int32(-5), C.c_int64(-1)
    try:
        assert m.projections is None and m.row_tile is None
        assert lib.sgpt_model_get_projections(m.handle, C.byref(kind)) == 0 and kind.value == 0
        assert lib.sgpt_model_set_projections(m.handle, 0, C.byref(freed)) == 0 and freed.value == 0      # 16-bit on a 16-bit model: nothing
        for bad in (2, -1):
            assert lib.sgpt_model_set_projections(m.handle, bad, C.byref(freed)) == -1
            assert last_error(ctx) == "sgpt_model_set_projections: kind 0 (16-bit) | 1 (fp8)"
        assert lib.sgpt_model_get_projections(m.handle, C.byref(kind)) == 0 and kind.value == 0
        assert lib.sgpt_model_set_projections(m.handle, 1, C.byref(freed)) == 0
        assert freed.value == expected_bytes_freed(cfg) > 0
        assert lib.sgpt_model_get_projections(m.handle, C.byref(kind)) == 0 and kind.value == 1
        assert lib.sgpt_model_set_projections(m.handle, 1, C.byref(freed)) == -1 and freed.value == 0
        assert last_error(ctx) == "sgpt_model_set_projections: the model is converted already"
        assert lib.sgpt_model_set_projections(m.handle, 0, None) == -1
        assert last_error(ctx) == "sgpt_model_set_projections: the conversion is one-way: the 16-bit weights are gone (load the model again)"
    finally:
        m.close()
    mq = model(tag)
    assert mq.projections == "fp8" and mq.projection_bytes_freed == expected_bytes_freed(cfg) and mq.row_tile == 256


def test_c_refusals_by_message(ctx):
    from sgpt_amd import SGPTConfig, SGPTModel, synthetic_weights
    from sgpt_amd.families import synthetic_qwen_weights
    lib = ctx.lib
    freed = C.c_int64(0)
    assert lib.sgpt_model_set_projections(None, 1, C.byref(freed)) == -1
    neo = SGPTConfig(vocab_size=64, max_position_embeddings=64, hidden_size=256, num_layers=1, num_heads=4, window_size=8)
    cases = [(SGPTModel(neo, synthetic_weights(neo, seed=1), device="cuda:0", dtype="bf16"),
              "fp8 projections belong to SGPT_ARCH_LLAMA models (SGPT_ARCH_GPTNEO has its fp8 compute dtypes or none)")]
    cfg, w, _ = F.make_model("llama", 1)
    cases.append((SGPTModel(cfg, w, device="cuda:0", dtype="f16"), "the model must be loaded with SGPT_BF16"))
    cases.append((SGPTModel(cfg, w, device="cuda:0", dtype="fp32"), "the model must be loaded with SGPT_BF16"))
    kw = dict(model_type="llama", vocab_size=64, max_position_embeddings=64, num_layers=1, window_size=0)
    for over, text in ((dict(hidden_size=128, num_heads=2, intermediate_size=256), "d_model = 128"),
                       (dict(hidden_size=256, num_heads=4, num_kv_heads=1, intermediate_size=256), "d_q + d_kv = 320"),
                       (dict(hidden_size=256, num_heads=2, rotary_dim=64, num_kv_heads=2, intermediate_size=256), "d_kv = 128"),
                       (dict(hidden_size=256, num_heads=4, intermediate_size=384), "d_ffn = 384")):
        c = SGPTConfig(**kw, **over)
        cases.append((SGPTModel(c, synthetic_qwen_weights(c, seed=2), device="cuda:0", dtype="bf16"),
                      text + " is not a multiple of 256 (the fp8 MFMA kernel's tile)"))
    try:
        for m, text in cases:
            for kind in (1, 0, 9):                                        # (these refusals come before the kind is looked at)
                assert lib.sgpt_model_set_projections(m.handle, kind, C.byref(freed)) == -1 and freed.value == 0
                assert last_error(ctx) == "sgpt_model_set_projections: " + text
    finally:
        for m, _ in cases:
            m.close()


# ---- composition from the stand-alone entries ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["llama", "qwen3", "qwen2"])
def test_one_layer_forward_is_the_standalone_entries_bit_for_bit(ctx, tag):
    from sgpt_amd.families import head_dim, rotary_tables_half, table_rows
    cfg, w, seqs = F.make_model(tag, 1)
    m = model(tag, n_layers=1)
    d, ffn, H, kv, dh, eps = cfg.hidden_size, cfg.intermediate_size, cfg.num_heads, cfg.num_kv_heads, head_dim(cfg), cfg.layer_norm_epsilon
    dq, dkv = H * dh, kv * dh

    def f32(name):
        return torch.from_numpy(np.ascontiguousarray(w[name])).to("cuda:0", torch.float32)

    def bf16_values(*names):                                              # what the loaded bf16 model holds, widened back to fp32
        return torch.cat([f32(n) for n in names], dim=0).to(BF).to(torch.float32).contiguous()
    p = "layers.0."
    wqkv8, sqkv = ctx.fp8_quantize_rows(bf16_values(*(p + f"self_attn.{n}_proj.weight" for n in "qkv")))
    wgu8, sgu = ctx.fp8_quantize_rows(bf16_values(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"))
    wd8, sd = ctx.fp8_quantize_rows(bf16_values(p + "mlp.down_proj.weight"))
    wo = f32(p + "self_attn.o_proj.weight").to(BF).contiguous()
    bias = torch.cat([f32(p + f"self_attn.{n}_proj.bias") for n in "qkv"]).contiguous() if p + "self_attn.q_proj.bias" in w else None
    sin, cos = (torch.from_numpy(t).to("cuda:0") for t in rotary_tables_half(table_rows(cfg), dh, cfg.rope_theta))
    zeros = torch.zeros(max(d, ffn), device="cuda:0")

    pb = m.pack(seqs)
    T = pb.T_pad
    assert T % 256 == 0
    got = m.encode_packed(pb, mode="mean", return_hidden=True)[1]

    x = ctx.embed(pb.ids, None, f32("embed_tokens.weight").contiguous())
    a8, sa = ctx.rmsnorm_fp8(x, f32(p + "input_layernorm.weight"), eps)
    nqk = dq + dkv
    qk = torch.zeros((T + 256, nqk), dtype=BF, device="cuda:0")            # the attention's over-read rows: finite
    qk[:T] = ctx.linear_fp8(a8, wqkv8[:nqk], sqkv[:nqk], None if bias is None else bias[:nqk], "store", a_scale=sa, out_dtype=BF)
    vt = torch.zeros((dkv, T + 256), dtype=BF, device="cuda:0")
    vt[:, :T] = ctx.linear_fp8(a8, wqkv8[nqk:], sqkv[nqk:], None if bias is None else bias[nqk:], "vt", a_scale=sa, out_dtype=BF)
    if p + "self_attn.q_norm.weight" in w:
        ctx.qknorm_rope_half(qk, pb.pos, sin, cos, f32(p + "self_attn.q_norm.weight"), f32(p + "self_attn.k_norm.weight"), H, kv, dh, dq,
                             eps=eps, T=T)
    else:
        ctx.rope_half(qk, pb.pos, sin, cos, H, kv, dh, dq, T=T)
    att = torch.zeros((T, dq), dtype=BF, device="cuda:0")                  # rows of no sequence stay zero, as in the forward
    ctx.attention(qk[:T, :dq], qk[:T, dq:], vt, att, pb.seq_off, H, dh, pb.max_alloc, scale=float(1.0 / np.sqrt(np.float32(dh))),
                  n_kv_heads=kv)
    x = ctx.linear(att, wo, bias=zeros[:d], epi="resid", resid=x)
    a8, sa = ctx.rmsnorm_fp8(x, f32(p + "post_attention_layernorm.weight"), eps)
    gu = ctx.linear_fp8(a8, wgu8, sgu, None, "store", a_scale=sa, out_dtype=BF)
    h8, sh = ctx.swiglu_fp8(gu)
    x = ctx.linear_fp8(h8, wd8, sd, zeros[:d], "resid", a_scale=sh, resid=x)
    want = ctx.rmsnorm(x, f32("norm.weight"), eps)
    torch.cuda.synchronize()
    off, lens = pb.off_host, [len(s) for s in seqs]
    real = torch.zeros(T, dtype=torch.bool)
    for o, n in zip(off[:-1].tolist(), lens):
        real[o:o + n] = True
    real = real.to("cuda:0")
    assert int(real.sum()) == sum(lens)
    same = torch.equal(got[real].view(torch.int32), want[real].view(torch.int32))
    assert same, f"{tag}: hidden_out differs from the stand-alone entries, max |d| = {float((got[real] - want[real]).abs().max()):.3e}"


# ---- end to end -------------------------------------------------------------------------------------------------------------------

_ref = {}


def measured(tag, mode, e, bidir=False, pool_from=None):
    """(max |de|, max |dcos|) of device embeddings against the float64 forward's (computed once per model and attention mode)."""
    if (tag, bidir) not in _ref:
        _ref[(tag, bidir)] = F.ref_forward(tag, fp8=False, bidir=bidir)
    return F.deviation(F.unit(e), F.embeddings(_ref[(tag, bidir)], mode, pool_from))


@pytest.mark.parametrize("tag", list(F.MODELS))
def test_embeddings_within_twice_the_emulations_deviation(tag):
    cfg, w, seqs = F.make_model(tag)
    m = model(tag)
    for mode in F.MODES:
        E, Ecos = emulated_deviation(tag, mode)
        e = m.encode_ids(seqs, mode=mode, normalize=True).to(torch.float64).cpu().numpy()
        de, dcos = measured(tag, mode, e)
        print(f"GPU {tag:6s} {mode:12s} max|de| = {de:.3e}  max|dcos| = {dcos:.3e}   E = {E:.3e}  ratio {de / E:.2f}")
        assert np.isfinite(e).all() and de <= 2.0 * E, (tag, mode, de, E)


def test_bidirectional_attention_and_pool_from_compose():
    tag, lo = "qwen2", 3
    cfg, w, seqs = F.make_model(tag)
    m = model(tag, attention="bidirectional")
    assert m.attention == "bidirectional" and m.projections == "fp8"
    causal = model(tag).encode_ids(seqs, mode="mean", normalize=True)
    for mode in ("mean", "weightedmean"):
        E, _ = emulated_deviation(tag, mode, bidir=True, pool_from=lo)
        e = m.encode_ids(seqs, mode=mode, normalize=True, pool_from=lo)
        if mode == "mean":
            assert float((e - causal).abs().max()) > 0.05                  # the mask and the range are live
        de, dcos = measured(tag, mode, e.to(torch.float64).cpu().numpy(), bidir=True, pool_from=lo)
        print(f"GPU {tag:6s} bidirectional, pool_from={lo}, {mode:12s} max|de| = {de:.3e}  max|dcos| = {dcos:.3e}   E = {E:.3e}  ratio {de / E:.2f}")
        assert de <= 2.0 * E, (mode, de, E)


# ---- other checks -----------------------------------------------------------------------------------------------------------------

def test_a_layout_of_224_rows_is_refused_through_the_raw_abi(ctx):
    m = model("llama")
    T, n = 224, 8
    i32 = dict(dtype=torch.int32, device="cuda:0")
    ids, pos = torch.zeros(T, **i32), torch.zeros(T, **i32)
    pos[:n] = torch.arange(n, **i32)
    seq_off, seq_len = torch.tensor([0, n], **i32), torch.tensor([n], **i32)
    out = torch.full((1, m.cfg.hidden_size), 7.0, device="cuda:0")
    st = ctx.lib.sgpt_encode(m.handle, ids.data_ptr(), pos.data_ptr(), seq_off.data_ptr(), seq_len.data_ptr(), None, 1, T, n, 1,
                             m.cfg.num_layers, 1, 0, out.data_ptr(), None, None)
    assert st == -1
    assert last_error(ctx) == "sgpt_encode: a model with fp8 projections takes layouts of T_pad % 256 == 0 token rows (T_pad = 224)"
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # the same layout on 256 rows is served
    ids, pos = torch.zeros(256, **i32), torch.zeros(256, **i32)
    pos[:n] = torch.arange(n, **i32)
    st = ctx.lib.sgpt_encode(m.handle, ids.data_ptr(), pos.data_ptr(), seq_off.data_ptr(), seq_len.data_ptr(), None, 1, 256, n, 1,
                             m.cfg.num_layers, 1, 0, out.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert st == 0 and torch.isfinite(out).all() and not (out == 7.0).any()


def test_encode_graph_refuses_a_converted_model():
    from sgpt_amd import EncodeGraph
    m = model("llama")
    with pytest.raises(ValueError, match="EncodeGraph: a model with projections='fp8' is not captured"):
        EncodeGraph(m, F.make_model("llama")[2])
    assert math.isfinite(float(m.encode_ids([[1, 2, 3]]).sum()))          # the model is untouched by the refusal
