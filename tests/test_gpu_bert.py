"""-m gpu: the BERT family (SGPT_ARCH_BERT) on the device -- its new kernels one by one against float64, and the forward against
HF BertModel's recorded values (tests/golden/tiny_bert*.npz).

Bars.  Forward, fp32: TOL_FP32 = 1e-3 on raw embeddings / hidden states, the bar tests/test_gpu_encode.py holds the fp32 GPT-Neo tiny
fixtures to.  Forward, f16: the project's 1e-3 bar on L2-normalised pooled embeddings (max abs) and on cosine scores.
erf-GELU epilogue: u = acc + bias is an fp32 sum of K = 128 exact products, at most K roundings of partial sums of magnitude <= ~30
(sum |a||w|), random walk sqrt(K) 2^-24 30 ~ 2e-5; gelu is 1-Lipschitz-ish (|gelu'| <= 1.13), erff is good to 4 ulp (2.4e-7), and a 16-bit
output is rounded once: |out - ref| <= 1.13 |u - u64| + 4e-7 |u| + u16 |ref|, asserted as 2e-5 + 2 u16 |ref| (fp32: 2e-5 + 1e-6 |ref|).
Write-back LayerNorm: the fp32 rows against float64 at the tolerance tests/test_gpu_rowops.py uses for the same RowLN arithmetic
(2e-6 x the row's bound); the 16-bit copy must be the fp32 output rounded ONCE: bit-equal to torch's RNE cast of it."""
import math

import numpy as np
import pytest
import torch

import bert_ref as B
from helpers import maxabs
from test_bert_ref import load_bert_case

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3
TOL_F16 = 1e-3
HALF = {"bf16": torch.bfloat16, "f16": torch.float16}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


_models = {}


def bert_model(tag, dtype):
    from sgpt_amd import SGPTModel
    if (tag, dtype) not in _models:
        fx, hf, cfg, w, seqs, cuts = load_bert_case(tag)
        _models[(tag, dtype)] = SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    return _models[(tag, dtype)]


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


# ---- kernels ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [32, 256])
@pytest.mark.parametrize("fmt", ["f16", "bf16", "fp32"])
def test_gelu_erf_epilogue_vs_float64(ctx, M, fmt):
    """sgpt_linear epi 9 at a query-sized (32 rows: the small-tile kernel) and a bulk (256 rows, N = 512, tile policy 1: the
    256x256 kernel) shape.  BERT layouts of every size run these bulk kernels; sgpt_linear_query keeps refusing the epilogue."""
    N, K = 512, 128
    rng = np.random.default_rng(M)
    dt = torch.float32 if fmt == "fp32" else HALF[fmt]
    a = torch.from_numpy(rng.uniform(-2, 2, size=(M, K)).astype(np.float32)).to(dt).cuda()
    w = torch.from_numpy(rng.uniform(-0.4, 0.4, size=(N, K)).astype(np.float32)).to(dt).cuda()
    bias = torch.from_numpy(rng.uniform(-1, 1, size=N).astype(np.float32)).cuda()
    u64 = a.double().cpu().numpy() @ w.double().cpu().numpy().T + bias.double().cpu().numpy()
    ref = B.gelu_erf(u64)
    assert np.abs(u64).max() > 6                                 # the whole range the erf matters on, and its saturated tails
    worst = 0.0
    for policy in ((0, 1) if (M == 256 and fmt != "fp32") else (0,)):
        old = ctx.lib.sgpt_ctx_set_tile_policy(ctx.handle, policy)
        try:
            got = ctx.linear(a, w, bias, epi="gelu_erf").double().cpu().numpy()
            tanh = ctx.linear(a, w, bias, epi="gelu").double().cpu().numpy()
        finally:
            ctx.lib.sgpt_ctx_set_tile_policy(ctx.handle, old)
        tol = 2e-5 + (1e-6 if fmt == "fp32" else 2 * U16[fmt]) * np.abs(ref)
        err = np.abs(got - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), f"policy {policy}: {float((err / tol).max()):.2f} x the bound"
        assert np.abs(tanh - got).max() > 1e-4 or fmt == "bf16"          # the two GELUs are different functions (4.7e-4 apart at most)
    print(f"gelu_erf M={M} {fmt}: worst error / bound = {worst:.3f}")
    if fmt != "fp32":                                            # not a query-kernel epilogue: refused by the C entry itself
        out = torch.empty((M, N), dtype=dt, device="cuda")
        assert ctx.lib.sgpt_linear_query(ctx.handle, 3 if fmt == "f16" else 1, 9, a.data_ptr(), None, None, None, 0.0, w.data_ptr(),
                                         bias.data_ptr(), None, out.data_ptr(), None, 0, M, N, K, None) == -1


def test_gelu_erf_leaves_the_tanh_gelu_alone(ctx):
    """EPI_BIAS_GELU after the change: still HF gelu_new, to the bound of tests/test_gpu_linear.py's own check (f16, 2 u16 |ref|)."""
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.uniform(-2, 2, size=(64, 128)).astype(np.float32)).half().cuda()
    w = torch.from_numpy(rng.uniform(-0.4, 0.4, size=(256, 128)).astype(np.float32)).half().cuda()
    bias = torch.from_numpy(rng.uniform(-1, 1, size=256).astype(np.float32)).cuda()
    u = a.double().cpu().numpy() @ w.double().cpu().numpy().T + bias.double().cpu().numpy()
    ref = 0.5 * u * (1 + np.tanh(math.sqrt(2 / math.pi) * (u + 0.044715 * u ** 3)))
    got = ctx.linear(a, w, bias, epi="gelu").double().cpu().numpy()
    assert (np.abs(got - ref) <= 2e-5 + 2 * U16["f16"] * np.abs(ref)).all()


@pytest.mark.parametrize("d", [128, 768, 1024])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_layernorm_writeback(ctx, d, fmt):
    T = 37                                                       # not a multiple of the 4 rows of a workgroup
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((T, d)) * rng.uniform(0.5, 30, size=(T, 1)) + rng.uniform(-1, 1, size=(T, 1))).astype(np.float32)
    g = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32)
    b = (0.2 * rng.standard_normal(d)).astype(np.float32)
    ref = B.layer_norm(x, g, b, 1e-12)
    big = torch.full((T + 3, d), 7.0, dtype=torch.float32, device="cuda")
    big[:T] = torch.from_numpy(x)
    xd = big[:T]
    separate = ctx.layernorm(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), eps=1e-12)
    a16 = ctx.layernorm_writeback(xd, torch.from_numpy(g).cuda(), torch.from_numpy(b).cuda(), eps=1e-12, out_dtype=HALF[fmt])
    torch.cuda.synchronize()
    assert (big[T:] == 7.0).all(), "rows past T were written"
    assert torch.equal(xd, separate), "in place: the bits of the stand-alone LayerNorm kernel"
    bound = 2e-6 * (np.abs(g)[None, :] * math.sqrt(d) + np.abs(b)[None, :])       # |x_hat| <= sqrt(d)
    assert (np.abs(xd.double().cpu().numpy() - ref) <= bound).all()
    assert torch.equal(a16, xd.to(HALF[fmt])), "the 16-bit copy is the fp32 output rounded once (RNE)"


def test_layernorm_writeback_records_f16_overflow(ctx):
    """gamma 40000: every output leaves the guard band of the f16 format -> bit 0 of the ctx range word; bf16: nothing to record."""
    d = 128
    x = torch.randn((8, d), device="cuda")
    g = torch.full((d,), 40000.0, device="cuda")
    b = torch.zeros(d, device="cuda")
    import ctypes as C

    def flag():
        v = C.c_int32(0)
        assert ctx.lib.sgpt_range_check(ctx.handle, C.byref(v), 1, None) == 0
        return v.value
    flag()
    ctx.layernorm_writeback(x.clone(), g, b, out_dtype=torch.bfloat16)
    assert flag() == 0
    ctx.layernorm_writeback(x.clone(), g, b, out_dtype=torch.float16)
    assert flag() & 1
    ctx.layernorm_writeback(x.clone(), g / 40000.0, b, out_dtype=torch.float16)
    assert flag() == 0


def test_cls_pooling_stand_alone(ctx):
    rng = np.random.default_rng(2)
    h = rng.standard_normal((5, 9, 132)).astype(np.float32)
    mask = (rng.uniform(size=(5, 9)) < 0.6).astype(np.int32)
    mask[:, 0] = [1, 1, 0, 1, 1]                                 # row 0 is taken whatever the mask says (Pooling.py:103-105)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        hd = torch.from_numpy(h).to(dt).cuda()
        got = ctx.pool(hd, torch.from_numpy(mask), "cls")
        assert torch.equal(got.cpu(), hd[:, 0].float().cpu())
    with pytest.raises(ValueError):
        ctx.lnf_pool(torch.zeros((32, 64), device="cuda"), torch.tensor([0, 32], dtype=torch.int32, device="cuda"),
                     torch.tensor([5], dtype=torch.int32, device="cuda"), mode="cls")     # the stand-alone fused entry keeps modes 0..3


# ---- forward ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["tiny_bert", "tiny_bert_dh128"])
def test_bert_forward_fp32_vs_hf_golden(tag):
    fx, hf, cfg, w, seqs, cuts = load_bert_case(tag)
    m = bert_model(tag, "fp32")
    L = cfg.num_layers
    for mode in ("mean", "cls"):
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        err = maxabs(got, fx[f"emb_{mode}"])
        print(f"{tag} fp32 {mode}: max|emb - ref| = {err:.3e}")
        assert err < TOL_FP32, (tag, mode)
    want = fx["hidden"]
    for li in range(L + 1):                                      # hidden_states[li] per token, as HF numbers them
        hid = m.token_embeddings(seqs, layer_idx=li)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            assert maxabs(hid[i].cpu().numpy(), want[li, a:b]) < TOL_FP32, (tag, li, i)
    # weightedmean / lasttoken work for this family as for the others
    last = [want[L, a:b].astype(np.float64) for a, b in zip(cuts[:-1], cuts[1:])]
    wm = np.stack([(h * np.arange(1, len(h) + 1)[:, None]).sum(0) / np.arange(1, len(h) + 1).sum() for h in last])
    assert maxabs(m.encode_ids(seqs, mode="weightedmean").cpu().numpy(), wm) < TOL_FP32
    assert maxabs(m.encode_ids(seqs, mode="lasttoken").cpu().numpy(), np.stack([h[-1] for h in last])) < TOL_FP32
    assert maxabs(m.encode_ids(seqs, mode="cls", layer_idx=1).cpu().numpy(), np.stack([want[1, a] for a in cuts[:-1]])) < TOL_FP32


@pytest.mark.parametrize("tag", ["tiny_bert", "tiny_bert_dh128"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_bert_forward_16bit_vs_hf_golden(tag, dtype):
    fx, hf, cfg, w, seqs, cuts = load_bert_case(tag)
    m = bert_model(tag, dtype)
    for mode in ("mean", "cls"):
        got = m.encode_ids(seqs, mode=mode).cpu().numpy()
        ref = fx[f"emb_{mode}"]
        assert np.isfinite(got).all()
        err = maxabs(_norm(got), _norm(ref))
        dev = maxabs(_norm(got) @ _norm(got).T, _norm(ref) @ _norm(ref).T)
        print(f"{tag} {dtype} {mode}: max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dev:.3e}")
        if dtype == "f16":
            assert err < TOL_F16 and dev < TOL_F16, (tag, mode)
        else:                                                    # bf16 falls out of the same kernels: 8x the f16 rounding unit
            assert err < 8 * TOL_F16 and dev < 8 * TOL_F16, (tag, mode)
        gn = m.encode_ids(seqs, mode=mode, normalize=True).cpu().numpy()
        assert maxabs(gn, _norm(got)) < 1e-6
    assert m.range_flags(reset=False) == 0


@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_bert_every_hidden_state_through_encode_layers(dtype):
    fx, hf, cfg, w, seqs, cuts = load_bert_case("tiny_bert")
    m = bert_model("tiny_bert", dtype)
    want = fx["hidden"].astype(np.float64)
    for mode in ("mean", "cls"):
        ref = np.stack([[B.pool(want[li, a:b], mode) for a, b in zip(cuts[:-1], cuts[1:])] for li in range(cfg.num_layers + 1)])
        layers, mean = m.encode_packed_layers(m.pack(seqs), mode=mode, per_layer=True)
        layers, mean = layers.cpu().numpy(), mean.cpu().numpy()
        if dtype == "fp32":
            assert maxabs(layers, ref) < TOL_FP32 and maxabs(mean, ref.mean(0)) < TOL_FP32
        else:
            for li in range(cfg.num_layers + 1):
                assert maxabs(_norm(layers[li]), _norm(ref[li])) < TOL_F16, (mode, li)
            assert maxabs(_norm(mean), _norm(ref.mean(0))) < TOL_F16
        assert maxabs(m.encode_ids_all_layers(seqs, mode=mode).cpu().numpy(), mean) < 1e-6     # `meanmean`


def test_bert_query_layout_and_bulk_layout_agree():
    """One sequence of 18 tokens alone (a 32-row layout) and inside a 256-row layout: the same embedding within the f16 bar."""
    fx, hf, cfg, w, seqs, cuts = load_bert_case("tiny_bert")
    m = bert_model("tiny_bert", "f16")
    one = [1] + list(range(3, 19)) + [2]
    assert len(one) == 18
    pb = m.pack([one])
    assert pb.T_pad == 32
    alone = m.encode_packed(pb, mode="mean", normalize=True).cpu().numpy()
    others = [s for s in seqs if len(s) in (33, 63, 64, 65)]
    pb2 = m.pack([one] + others)
    assert pb2.T_pad == 256, pb2.T_pad
    bulk = m.encode_packed(pb2, mode="mean", normalize=True).cpu().numpy()[:1]
    err = maxabs(alone, bulk)
    print(f"18 tokens, 32-row layout vs 256-row layout: {err:.3e}")
    assert err < TOL_F16
    hs = B.forward(w, [one], cfg.num_layers, cfg.num_heads, cfg.layer_norm_epsilon)[0][-1]
    assert maxabs(alone, _norm(B.pool(hs, "mean")[None])) < TOL_F16


def test_bert_adapters_run_end_to_end():
    """CustomEmbedder, SentenceTransformerSGPT.encode, DenseRetrievalExactSearch.search and useb.make_semb_fn on a BERT model with a
    synthetic [CLS] / [SEP] tokenizer, `mean` and `cls`: the embeddings are those of the framed ids through encode_ids."""
    from test_bert_ref import _bert_tokenizer
    from sgpt_amd.beir import CustomEmbedder, DenseRetrievalExactSearch
    from sgpt_amd.st import SentenceTransformerSGPT
    from sgpt_amd import useb
    m = bert_model("tiny_bert", "f16")
    words = [f"w{i}" for i in range(150)]
    tok = _bert_tokenizer(words)
    rng = np.random.default_rng(4)
    texts = [" ".join(rng.choice(words, size=n)) for n in (3, 9, 17, 40)]
    framed = [[tok.cls_token_id] + tok.convert_tokens_to_ids(t.split()) + [tok.sep_token_id] for t in texts]
    for mode in ("mean", "cls"):
        want = m.encode_ids(framed, mode=mode).cpu().numpy()
        emb = CustomEmbedder(model=m, tokenizer=tok, method=mode, maxseqlen=64)
        assert maxabs(emb.embed_device(texts, True).cpu().numpy(), want) < 1e-6
        st = SentenceTransformerSGPT(m, tok, max_seq_length=64, pooling_mode=mode)
        assert maxabs(st.encode(texts), want) < 1e-6
    with pytest.raises(ValueError, match="BERT"):
        CustomEmbedder(model=m, tokenizer=tok, method="mean", specb=True)
    emb = CustomEmbedder(model=m, tokenizer=tok, method="mean", maxseqlen=64)
    corpus = {f"d{i}": {"title": "", "text": t} for i, t in enumerate(texts)}
    res = DenseRetrievalExactSearch(emb, corpus_chunk_size=3).search(corpus, {"q0": texts[1], "q1": texts[3]}, 2, "cos_sim")
    assert max(res["q0"], key=res["q0"].get) == "d1" and max(res["q1"], key=res["q1"].get) == "d3"
    for mode in ("mean", "cls", "meanmean"):
        fn = useb.make_semb_fn(useb.CustomEmbedder(m, tok, method=mode, maxseqlen=64))
        want = m.encode_ids_all_layers(framed, mode="mean") if mode == "meanmean" else m.encode_ids(framed, mode=mode)
        out = fn(texts).numpy()
        assert out.shape == (4, m.cfg.hidden_size) and maxabs(out, want.cpu().numpy()) < 1e-6


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_bert_refuses_what_it_does_not_build():
    from sgpt_amd import SGPTModel
    fx, hf, cfg, w, seqs, cuts = load_bert_case("tiny_bert")
    for dtype in ("fp8", "fp8mfma"):
        with pytest.raises(ValueError, match="BERT"):
            SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    for kw in (dict(precision="x3"), dict(precision="auto-class"), dict(precise_qk="full")):
        with pytest.raises(ValueError, match="BERT"):
            SGPTModel(cfg, w, device="cuda:0", dtype="f16", **kw)
    m = bert_model("tiny_bert", "f16")
    with pytest.raises(ValueError, match="learntmean"):
        m.encode_ids(seqs[:3], mode="learntmean")
    with pytest.raises(ValueError, match="LM head"):
        m.lm_logprobs(torch.zeros((32, cfg.hidden_size), device="cuda"), [0], [1])
    # the C ABI refuses on its own, whatever the Python host checked first
    import ctypes as C
    lib, h = m.ctx.lib, m.handle
    plan = np.ones(cfg.num_layers * 5, dtype=np.int32)
    assert lib.sgpt_model_set_precision(h, plan.ctypes.data_as(C.c_void_p), plan.size) == -1
    n = C.c_int32(0)
    assert lib.sgpt_model_range_adapt(h, C.byref(n), None) == -1
    sh = np.zeros(cfg.num_layers * 4, dtype=np.int32)
    assert lib.sgpt_model_set_range_shifts(h, sh.ctypes.data_as(C.c_void_p), sh.size) == -1
    assert lib.sgpt_model_precision_probe_begin(h) == -1
    out = torch.zeros(1, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.sgpt_lm_logprobs(h, torch.zeros((32, cfg.hidden_size), device="cuda").data_ptr(), idx.data_ptr(), idx.data_ptr(), 1,
                                out.data_ptr(), None, None) == -1
    pb = m.pack(seqs[:2])
    o = torch.zeros((2, cfg.hidden_size), device="cuda")
    assert lib.sgpt_encode(h, pb.ids.data_ptr(), pb.pos.data_ptr(), pb.seq_off.data_ptr(), pb.seq_len.data_ptr(), pb.pad_left.data_ptr(),
                           pb.B, pb.T_pad, pb.max_alloc, 3, cfg.num_layers, 0, 0, o.data_ptr(), None, None) == -1
    assert "learntmean" in lib.sgpt_last_error(m.ctx.handle).decode()
