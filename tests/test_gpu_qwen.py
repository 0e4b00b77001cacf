"""-m gpu: the Qwen2 / Qwen3 members of the Llama family on the device -- the fused per-head RMSNorm + half-split rotary kernel
(sgpt_qknorm_rope_half) against float64 and against the two kernels it fuses, and the forward (QKV bias, q / k norm, a query width
n_heads * head_dim != d_model) against HF Qwen2Model / Qwen3Model's recorded values (tests/golden/tiny_qwen*.npz).

Bars.
sgpt_qknorm_rope_half: per element  8 B + 2 u32 (|n_i| + |n_j|)  (+ ulp16(ref) / 2 for a 16-bit buffer), derived and not measured:
  B is the RMSNorm unit of tests/test_gpu_llama.py (rowops_ref.layernorm_unit with mean 0) on the [T * heads, head_dim] view, n the
  normed pair values of the reference, u32 = 2^-23.  The norm is held to 4 B per element as sgpt_rmsnorm is, both elements of a pair
  enter one output with |s|, |c| <= 1 (8 B), and the rotation's own term is the one test_rope_half_vs_float64 asserts.
Fused against two-step (sgpt_rmsnorm on the head view, then sgpt_rope_half; fp32): the sum of the two sides' bars, each side being
  within 8 B + 2 u32 (|n_i| + |n_j|) of the float64 reference.
Forward: TOL_FP32 = 1e-3 on every hidden state and the three pooled embeddings; f16 1e-3 and bf16 8e-3 on the L2-normalised pooled
  embeddings and on their cosine matrix -- the bars of tests/test_gpu_llama.py; tests/test_qwen_ref.py shows on the CPU that the 16-bit
  ones are attainable on these fixtures (emulated error at most half the bar)."""
import ctypes as C

import numpy as np
import pytest
import torch

import qwen_ref as Q
import rowops_ref as RO
from helpers import maxabs
from test_qwen_ref import MODES, TAGS, load_qwen_case

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3
TOL_F16 = 1e-3
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
TDT = {"fp32": torch.float32, **HALF}
U32 = 2.0 ** -23
EPS = 1e-6
INVALID, MISSING = -1, -3


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def host64(t) -> np.ndarray:
    return t.detach().to("cpu", torch.float64).numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def range_flag(ctx) -> int:
    v = C.c_int32(0)
    assert ctx.lib.sgpt_range_check(ctx.handle, C.byref(v), 1, None) == 0
    return v.value


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


_models = {}


def qwen_model(tag, dtype):
    from sgpt_amd import SGPTModel
    if (tag, dtype) not in _models:
        fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
        _models[(tag, dtype)] = SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    return _models[(tag, dtype)]


# ---- the fused kernel --------------------------------------------------------------------------------------------------------

H, T, MAX_POS = 4, 32, 40
_kcache = {}


def kernel_case(Hkv, dh, dt):
    """Input buffer (values exact in dt), positions, tables, gains and the float64 reference with its bound -- computed once and shared.
    Layout of test_rope_half_vs_float64: the q block (4 heads) at column 0, 8 sentinel columns, the k block (Hkv heads) at k_off, 8 more
    sentinel columns, one sentinel row after T; positions repeated, out of order and out of range; row scales as rms_setup's."""
    from sgpt_amd.model import rotary_tables_half
    if (Hkv, dh, dt) not in _kcache:
        k_off = H * dh + 8
        ld = k_off + Hkv * dh + 8
        sin, cos = rotary_tables_half(MAX_POS, dh, 10000.0)
        rng = np.random.default_rng(1000 * Hkv + dh)
        pos = rng.integers(0, MAX_POS, size=T).astype(np.int32)
        pos[:6] = [0, 39, 39, -5, 40, 1000]
        x32 = (rng.standard_normal((T + 1, ld)) * rng.uniform(0.5, 30, size=(T + 1, 1))).astype(np.float32)
        x = host64(torch.from_numpy(x32).to(TDT[dt]))            # what the buffer holds, exactly
        gq = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
        gk = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
        assert not np.array_equal(gq, gk)
        half = dh // 2
        ref, bound = x.copy(), np.zeros_like(x)
        touched = np.zeros(x.shape, dtype=bool)
        for c0, nh, g in ((0, H, gq), (k_off, Hkv, gk)):
            blk = x[:T, c0:c0 + nh * dh]
            n = Q.head_rms_norm(blk, g, nh, dh, EPS)                                              # [T, nh * dh]
            ref[:T, c0:c0 + nh * dh] = Q.rope_half(n, pos, nh, dh, sin=sin, cos=cos)
            rows = blk.reshape(T * nh, dh)
            rstd = 1.0 / np.sqrt((rows ** 2).mean(-1) + EPS)
            B = RO.layernorm_unit(rows, g, n.reshape(T * nh, dh), np.zeros(T * nh), rstd).reshape(T, nh, 1)
            nn = np.abs(n).reshape(T, nh, dh)
            pair = nn[..., :half] + nn[..., half:]
            bnd = 8 * B + 2 * U32 * np.concatenate([pair, pair], axis=-1)
            bound[:T, c0:c0 + nh * dh] = bnd.reshape(T, nh * dh)
            touched[:T, c0:c0 + nh * dh] = True
        if dt != "fp32":
            bound = bound + 0.5 * RO.ulp16(ref, dt)
        _kcache[(Hkv, dh, dt)] = dict(k_off=k_off, ld=ld, sin=sin, cos=cos, pos=pos, x=x, gq=gq, gk=gk, ref=ref, bound=bound, touched=touched)
    return _kcache[(Hkv, dh, dt)]


@pytest.mark.parametrize("dt", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("Hkv", [1, 2, 4])
def test_qknorm_rope_half_vs_float64(ctx, Hkv, dh, dt):
    c = kernel_case(Hkv, dh, dt)
    buf = dev(c["x"], TDT[dt])
    before = buf.clone()
    range_flag(ctx)
    ctx.qknorm_rope_half(buf, dev(c["pos"]), dev(c["sin"]), dev(c["cos"]), dev(c["gq"]), dev(c["gk"]), H, Hkv, dh, k_off=c["k_off"], eps=EPS, T=T)
    same = (bits(buf) == bits(before)).cpu().numpy()
    assert same[~c["touched"]].all(), "a sentinel column, a key head past H_kv or the row after T was written"
    err = np.abs(host64(buf) - c["ref"])
    ratio = float((err[c["touched"]] / c["bound"][c["touched"]]).max())
    print(f"qknorm_rope_half {dt} Hkv={Hkv} dh={dh}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert np.abs(host64(buf) - c["x"])[c["touched"]].max() > 1.0                   # something happened
    assert range_flag(ctx) == 0
    # gains of 1 at position 0: the per-head RMSNorm alone, held to the norm's own bar 4 B (+ the one rounding)
    ones = torch.ones(dh, device="cuda:0")
    buf1 = before.clone()
    ctx.qknorm_rope_half(buf1, torch.zeros(T, dtype=torch.int32, device="cuda:0"), dev(c["sin"]), dev(c["cos"]), ones, ones, H, Hkv, dh,
                         k_off=c["k_off"], eps=EPS, T=T)
    for c0, nh in ((0, H), (c["k_off"], Hkv)):
        blk = c["x"][:T, c0:c0 + nh * dh]
        n = Q.head_rms_norm(blk, np.ones(dh), nh, dh, EPS)
        rows = blk.reshape(T * nh, dh)
        rstd = 1.0 / np.sqrt((rows ** 2).mean(-1) + EPS)
        B = RO.layernorm_unit(rows, np.ones(dh), n.reshape(T * nh, dh), np.zeros(T * nh), rstd)
        bnd = np.repeat(4 * B.reshape(T, nh), dh, axis=1) + (0.0 if dt == "fp32" else 0.5 * RO.ulp16(n, dt))
        assert (np.abs(host64(buf1[:T, c0:c0 + nh * dh]) - n) <= bnd).all(), (c0, nh)


def test_qknorm_rope_half_records_f16_overflow_and_refuses_bad_arguments(ctx):
    from sgpt_amd.model import rotary_tables_half
    sin, cos = (dev(t) for t in rotary_tables_half(8, 64))
    pos = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    big, one = torch.full((64,), 40000.0, device="cuda:0"), torch.ones(64, device="cuda:0")
    x = torch.randn((4, 256), device="cuda:0")
    range_flag(ctx)
    ctx.qknorm_rope_half(x.to(torch.bfloat16), pos, sin, cos, big, one, 2, 1, 64, k_off=128)
    assert range_flag(ctx) == 0
    ctx.qknorm_rope_half(x.to(torch.float16), pos, sin, cos, one, big, 2, 1, 64, k_off=128)         # the key gain alone
    assert range_flag(ctx) & 1
    ctx.qknorm_rope_half(x.to(torch.float16), pos, sin, cos, one, one, 2, 1, 64, k_off=128)
    assert range_flag(ctx) == 0
    buf = torch.zeros((4, 256), device="cuda:0")
    lib, h = ctx.lib, ctx.handle

    def call(dtype=0, ld=256, k_off=128, dh=64, gq=one.data_ptr(), gk=one.data_ptr(), eps=1e-6, Hq=2, Hkv=1, sin_p=sin.data_ptr()):
        return lib.sgpt_qknorm_rope_half(h, buf.data_ptr(), dtype, ld, k_off, pos.data_ptr(), sin_p, cos.data_ptr(), 4, Hq, Hkv, dh, 8, gq, gk,
                                         eps, None)
    assert call() == 0
    assert call(k_off=120) == INVALID                              # what sgpt_rope_half refuses: the k block inside the q block,
    assert call(k_off=200) == INVALID                              # past the row,
    assert call(ld=254) == INVALID                                 # ld % 4,
    assert call(Hkv=0) == INVALID and call(sin_p=None) == INVALID  # no key head, no table
    for dh in (32, 96, 256):                                       # head_dim other than 64 | 128
        assert call(dh=dh, Hq=1, Hkv=1) == INVALID, dh
    assert call(gq=None) == INVALID and call(gk=None) == INVALID   # a null gain
    assert call(dtype=2) == INVALID and call(dtype=4) == INVALID   # fp8
    assert call(eps=-1.0) == INVALID
    torch.cuda.synchronize()
    assert (buf == 0).all()                                        # (RMSNorm of a zero row is zero; nothing else was launched)


@pytest.mark.parametrize("dh", [64, 128])
def test_qknorm_rope_half_against_rmsnorm_then_rope_half(ctx, dh):
    """fp32, the q and k blocks adjacent (contiguous head views for sgpt_rmsnorm): the fused kernel against the two tested kernels."""
    Hkv = 2
    c = kernel_case(Hkv, dh, "fp32")
    k_off = H * dh
    x = np.concatenate([c["x"][:T, :H * dh], c["x"][:T, c["k_off"]:c["k_off"] + Hkv * dh]], axis=1).astype(np.float32)
    pos, sin, cos = dev(c["pos"]), dev(c["sin"]), dev(c["cos"])
    fused = dev(x)
    ctx.qknorm_rope_half(fused, pos, sin, cos, dev(c["gq"]), dev(c["gk"]), H, Hkv, dh, k_off=k_off, eps=EPS)
    q = ctx.rmsnorm(dev(x[:, :k_off]).reshape(T * H, dh), dev(c["gq"]), EPS)
    k = ctx.rmsnorm(dev(x[:, k_off:]).reshape(T * Hkv, dh), dev(c["gk"]), EPS)
    two = torch.cat([q.reshape(T, H * dh), k.reshape(T, Hkv * dh)], dim=1).contiguous()
    ctx.rope_half(two, pos, sin, cos, H, Hkv, dh, k_off=k_off)
    bound = np.concatenate([c["bound"][:T, :H * dh], c["bound"][:T, c["k_off"]:c["k_off"] + Hkv * dh]], axis=1)
    ratio = float((np.abs(host64(fused) - host64(two)) / (2 * bound)).max())
    print(f"qknorm_rope_half vs rmsnorm + rope_half dh={dh}: worst difference / (sum of the bars) = {ratio:.3f}")
    assert ratio <= 1.0


# ---- forward -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_qwen_forward_fp32_vs_hf_golden(tag):
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    m = qwen_model(tag, "fp32")
    L = cfg.num_layers
    for mode in MODES:
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        err = maxabs(got, fx[f"emb_{mode}"])
        print(f"{tag} fp32 {mode}: max|emb - ref| = {err:.3e}")
        assert err < TOL_FP32, (tag, mode)
    want = fx["hidden"]
    worst = 0.0
    for li in range(L + 1):                                      # hidden_states[li] per token, as HF numbers them
        hid = m.token_embeddings(seqs, layer_idx=li)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            e = maxabs(hid[i].cpu().numpy(), want[li, a:b])
            worst = max(worst, e)
            assert e < TOL_FP32, (tag, li, i)
    print(f"{tag} fp32 hidden states: max|h - ref| = {worst:.3e}")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_qwen_forward_16bit_vs_hf_golden(tag, dtype):
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    m = qwen_model(tag, dtype)
    for mode in MODES:
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        ref = fx[f"emb_{mode}"]
        assert np.isfinite(got).all()
        err = maxabs(_norm(got), _norm(ref))
        dev_ = maxabs(_norm(got) @ _norm(got).T, _norm(ref) @ _norm(ref).T)
        print(f"{tag} {dtype} {mode}: max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dev_:.3e}")
        bar = TOL_F16 if dtype == "f16" else 8 * TOL_F16
        assert err < bar and dev_ < bar, (tag, mode)
        gn = m.encode_ids(seqs, mode=mode, normalize=True).cpu().numpy()
        assert maxabs(gn, _norm(got)) < 1e-6
    assert m.range_flags(reset=False) == 0


# ---- invariants where the query width is not d_model -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f16", "fp32"])
def test_qwen3_batch_and_layout_invariance(dtype):
    """tiny_qwen3 (query width 256, d 128): a batch and its sentences alone agree bit for bit; so do a 32-row layout and the same sequence
    inside a layout of more than 32 rows and inside one of exactly 256 rows (test_llama_256_row_layout's)."""
    fx, hf, cfg, w, seqs, cuts = load_qwen_case("tiny_qwen3")
    from sgpt_amd.families import head_dim
    assert cfg.num_heads * head_dim(cfg) == 256 != cfg.hidden_size
    m = qwen_model("tiny_qwen3", dtype)
    batch = m.encode_ids(seqs, mode="weightedmean")
    for i, s in enumerate(seqs):
        assert torch.equal(m.encode_ids([s], mode="weightedmean")[0], batch[i]), (dtype, i)
    one = (seqs[1] * 3)[:18]
    pb = m.pack([one])
    assert pb.T_pad == 32
    alone = m.encode_packed(pb, mode="mean")
    pb2 = m.pack([one] + seqs[2:])
    assert pb2.T_pad > 32, pb2.T_pad
    assert torch.equal(alone[0], m.encode_packed(pb2, mode="mean")[0]), dtype
    fill = [seqs[2], seqs[3], seqs[2], seqs[1] + seqs[1] + seqs[1][:4]]     # 18 + 64 + 70 + 64 + 18 allocated rows = 234 -> 256
    pb3 = m.pack([one] + fill)
    assert pb3.T_pad == 256, pb3.T_pad
    assert torch.equal(alone[0], m.encode_packed(pb3, mode="mean")[0]), dtype


@pytest.mark.parametrize("dtype", ["f16", "fp32"])
def test_qwen3_every_hidden_state_through_encode_layers(dtype):
    fx, hf, cfg, w, seqs, cuts = load_qwen_case("tiny_qwen3")
    m = qwen_model("tiny_qwen3", dtype)
    want = fx["hidden"].astype(np.float64)
    for mode in MODES:
        ref = np.stack([[Q.pool(want[li, a:b], mode) for a, b in zip(cuts[:-1], cuts[1:])] for li in range(cfg.num_layers + 1)])
        layers, mean = m.encode_packed_layers(m.pack(seqs), mode=mode, per_layer=True)
        layers, mean = layers.cpu().numpy(), mean.cpu().numpy()
        assert layers.shape == (cfg.num_layers + 1, len(seqs), cfg.hidden_size)
        if dtype == "fp32":
            assert maxabs(layers, ref) < TOL_FP32 and maxabs(mean, ref.mean(0)) < TOL_FP32
        else:
            for li in range(cfg.num_layers + 1):
                assert maxabs(_norm(layers[li]), _norm(ref[li])) < TOL_F16, (mode, li)


def test_qwen2_bias_is_live():
    """tiny_qwen2 reloaded with its three bias tensors zeroed moves the fp32 embeddings by more than 10 x TOL_FP32."""
    from sgpt_amd import SGPTModel
    fx, hf, cfg, w, seqs, cuts = load_qwen_case("tiny_qwen2")
    zeroed = {k: (np.zeros_like(v) if k.endswith("_proj.bias") else v) for k, v in w.items()}
    assert sum(k.endswith("_proj.bias") for k in w) == 3 * cfg.num_layers
    m0 = SGPTModel(cfg, zeroed, device="cuda:0", dtype="fp32")
    try:
        for mode in MODES:
            moved = maxabs(m0.encode_ids(seqs, mode=mode).cpu().numpy(), fx[f"emb_{mode}"])
            print(f"tiny_qwen2 without its bias, {mode}: max|emb - ref| = {moved:.3e}")
            assert moved > 10 * TOL_FP32, mode
    finally:
        m0.close()


# ---- a checkpoint folder -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["tiny_qwen2", "tiny_qwen3"])
def test_qwen_loads_from_a_checkpoint_folder(tmp_path, tag):
    """A sentence-transformers folder as HF saves a *ForCausalLM checkpoint -- `model.`-prefixed names, an `lm_head`, separate q / k / v
    biases, the head-norm gains -- through SGPTModel.from_pretrained and SentenceTransformerSGPT.from_pretrained with the Qwen3-Embedding
    frame ([], [eos]): the embeddings of the model built from the plain dict."""
    from test_qwen_ref import _QwenTok
    from sgpt_amd import SGPTModel
    from sgpt_amd.families import head_dim
    from sgpt_amd.formats import write_st_folder
    from sgpt_amd.st import SentenceTransformerSGPT
    fx, hf, cfg, w, seqs, cuts = load_qwen_case(tag)
    sd = {"model." + k: v for k, v in w.items()}
    sd["lm_head.weight"] = np.ones_like(w["embed_tokens.weight"])
    p = str(tmp_path / "st")
    write_st_folder(p, hf, sd, pooling_mode="lasttoken", max_seq_length=64, normalize=True)
    ref_model = qwen_model(tag, "f16")
    want = ref_model.encode_ids(seqs, mode="lasttoken")
    m = SGPTModel.from_pretrained(p, device="cuda:0", dtype="f16")
    assert m.cfg.model_type == "llama" and m.cfg.rotary_dim == cfg.rotary_dim and head_dim(m.cfg) == head_dim(cfg)
    assert torch.equal(m.encode_ids(seqs, mode="lasttoken"), want)
    m.close()
    tok = _QwenTok()
    with pytest.raises(ValueError, match="bos_token_id"):                            # the Qwen tokenizers need the explicit frame
        SentenceTransformerSGPT.from_pretrained(p, tokenizer=tok, device="cuda:0", dtype="f16")
    st = SentenceTransformerSGPT.from_pretrained(p, tokenizer=tok, device="cuda:0", dtype="f16", frame=([], [tok.eos_token_id]))
    assert st.pooling_mode == "lasttoken" and st.normalize and st.pipe.frame == ([], [2])
    texts = ["w5 w9 w120 w33", "w7", " ".join(f"w{i}" for i in range(80))]            # the last one is cut to 63 tokens + EOS
    ids = [[int(t[1:]) + 3 for t in x.split()][:63] + [2] for x in texts]
    ref = ref_model.encode_ids(ids, mode="lasttoken", normalize=True).cpu().numpy()
    assert maxabs(st.encode(texts), ref) < 1e-6
    st.model.close()


# ---- the descriptor and the optional tensors through the C ABI -------------------------------------------------------------------------

def test_descriptor_and_tensor_refusals_through_the_c_abi(ctx):
    from sgpt_amd import _lib
    from sgpt_amd import model as M
    lib, h = ctx.lib, ctx.handle
    V, P, D, Hh, FFN = 40, 64, 128, 2, 128
    cfg = M.SGPTConfig(model_type="llama", vocab_size=V, max_position_embeddings=P, hidden_size=D, num_layers=2, num_heads=Hh,
                       intermediate_size=FFN, window_size=0)
    w = M.llama_state_dict(M.synthetic_qwen_weights(cfg, seed=3, qk_norm=True))
    w["rotary.sin"], w["rotary.cos"] = M.rotary_tables_half(P, D // Hh)
    tensors = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to("cuda:0", torch.float32).contiguous()
               for k, v in w.items()}

    def load(drop=(), **over):
        t = {k: v for k, v in tensors.items() if k not in drop}
        views = (_lib.TensorView * len(t))(*[_lib.TensorView(k.encode(), v.data_ptr(), v.numel()) for k, v in t.items()])
        d = dict(arch=_lib.SGPT_ARCH_LLAMA, n_layers=2, d_model=D, n_heads=Hh, d_ffn=FFN, vocab=V, max_pos=P, window=0, ln_eps=1e-6,
                 attn_scale=0.125, compute_dtype=_lib.SGPT_F32, rotary_dim=0, qk_split=0, split_weights=0, n_kv_heads=0)
        d.update(over)
        hh = C.c_void_p()
        torch.cuda.synchronize()
        st = lib.sgpt_model_load(h, C.byref(_lib.ModelDesc(**d)), views, len(t), C.byref(hh))
        assert (st == 0) == bool(hh.value)
        if hh.value:
            lib.sgpt_model_free(hh)
        return st, (lib.sgpt_last_error(h) or b"").decode()

    assert load()[0] == 0                                          # rotary_dim = 0 still loads: head_dim = d_model / n_heads
    assert load(rotary_dim=64)[0] == 0                             # ... and so does the same head dim said out loud
    assert load(rotary_dim=96) == (INVALID, "SGPT_ARCH_LLAMA: head_dim 64 or 128")
    assert load(rotary_dim=96, compute_dtype=_lib.SGPT_F16) == (INVALID, "16-bit attention supports head_dim 64, 128 or 256")
    assert load(d_model=384, n_heads=3, rotary_dim=64) == \
        (INVALID, "SGPT_ARCH_LLAMA: n_heads * rotary_dim (the query width) must be a multiple of 128")
    assert load(d_model=4096, n_heads=64, rotary_dim=128) == \
        (INVALID, "SGPT_ARCH_LLAMA: n_heads * rotary_dim (the query width) > 4096 not supported")
    # one gain without the other; a layer that disagrees with layer 0 -- by name
    assert load(drop=("layers.0.self_attn.k_norm.weight",)) == (MISSING, "missing weight tensor: layers.0.self_attn.k_norm.weight")
    assert load(drop=("layers.0.self_attn.q_norm.weight",)) == (MISSING, "missing weight tensor: layers.0.self_attn.q_norm.weight")
    assert load(drop=("layers.1.self_attn.q_norm.weight",)) == (MISSING, "missing weight tensor: layers.1.self_attn.q_norm.weight")
    assert load(drop=("layers.0.self_attn.q_norm.weight", "layers.0.self_attn.k_norm.weight")) == \
        (MISSING, "missing weight tensor: layers.0.self_attn.q_norm.weight")
    # a head dim of its own changes the fused weight's shape: these tensors are d / H = 64 ones
    assert load(rotary_dim=128) == (INVALID, "wrong numel for rotary.cos")                                  # (the last failure answers)
