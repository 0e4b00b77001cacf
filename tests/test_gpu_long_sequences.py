"""-m gpu: sequences of more than 2048 tokens on the device (the limit is SGPT_MAX_SEQ_LEN = 32 768, include/sgpt_hip.h).

1. The attention kernels stand-alone against tests/attn_ref.py in float64, through Context.attention(causal=True) / (n_kv_heads=) --
   the entries that take the long layouts.  Inputs, needles and sentinels are tests/test_gpu_attention.py's (make_inputs); the packed
   layout is three sequences [L, 7, 130].
   16-bit: the bound of that file, 3 u16 max|v| -- the context is a convex combination of V rows, p is rounded once and the context
   once, whatever the number of keys (f16: e_j below 2^-14 land on the subnormal grid, absolute 2^-25 each; 4100 of them are
   < 0.25 u16 max|v|, inside the 0.87 u16 the bound leaves).
   fp32 (attn_f32_long_kernel for a call with an allocation above 2048 rows), bound derived from operation counts, u = 2^-24, n the
   most keys a row sees, C = ceil(n / 2048) chunks, Lmax = scale * max_ij sum_c |q_ic k_jc| (computed from the inputs):
     logit: an fma chain over head_dim products and the scale multiply: |ds| <= (dh + 1) u Lmax; the subtraction s - m rounds once on
       |s - m| <= 2 Lmax: 2 u Lmax; expf is good to 1 ulp = 2 u.  A weight e_j so carries a relative error eps = u ((dh + 3) Lmax + 2)
       (an error of m is common to all weights and cancels), and relative errors eps on the weights move a convex combination of V
       rows by at most 2 eps max|v|;
     numerator: ONE serial fma chain over the row's n products: n u sum|e_j v_j| <= n u max|v| l;
     denominator: lane-strided partial sums of n / 64 terms and a 6-step butterfly: (n / 64 + 6) u l;
     every chunk after the first rescales l and the numerator by exp(m_old - m_new): expf, one product, and the add of l: 4 u each;
     the final 1 / l and the product: 2 u.
   |ctx - ref| <= u max|v| [n + n / 64 + 6 + 4 C + 2 + 2 ((dh + 3) Lmax + 2)]: 5.3e-4 max|v| at n = 4100, head_dim 128, Lmax 18 -- it must
   stay below 1e-3 max|v| (asserted); a dropped chunk costs ~0.5 max|v|.
   Rows that see at most 2048 keys (the 7- and 130-token sequences, the first 2048 rows of the long one) equal bit for bit the same
   rows in a call with max_alloc_len <= 2048, i.e. attn_f32_kernel: the batch-invariance rule.
2. The forward against HF's recorded values (tests/golden/tiny_*_long*.npz): fp32 < 1e-3 on pooled vectors and the recorded hidden
   rows; f16 < 1e-3 and bf16 < 8e-3 on normalised embeddings and their cosines (tests/test_gpu_llama.py's bars); the 2049-token
   sequence alone (at most 4096 rows) and all sequences together (more than 4096 rows).
3. Each sequence encoded alone equals its row of the batch bit for bit, fp32 and f16.
4. Refusals: the library's limit, the model's position range, a folded Mistral window; the context works afterwards.
5. One sequence of exactly 32 768 tokens, f16, against a float64 reference of its `lasttoken` vector."""
import math
import re

import numpy as np
import pytest
import torch

import llama_ref as R
import test_gpu_attention as A
from attn_ref import packed_attention
from bert_ref import packed_attention_bidir
from helpers import maxabs
from test_long_ref import MODES, TAGS, load_long_case

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3
TOL_F16 = 1e-3
U32 = 2.0 ** -24
SHORT = [7, 130]


@pytest.fixture(scope="module")
def ctx():
    from sgpt_amd import get_context
    return get_context("cuda:0")


# ---- 1. attention ------------------------------------------------------------------------------------------------------------

_inputs = {}


def inputs(dh, L, window, H, scale):
    """make_inputs of one case and its float64 reference, built once and shared (read-only)."""
    key = (dh, L, window, H, scale)
    if key not in _inputs:
        while len(_inputs) > 1:                                  # (a case is ~150 MB of float64: the last two are kept)
            _inputs.pop(next(iter(_inputs)))
        inp = A.make_inputs([L] + SHORT, H, dh, window, scale, seed=7000 * L + dh + window)
        _inputs[key] = (inp, packed_attention(inp["q"], inp["k"], inp["v"], inp["off"], inp["lens"], H, window, scale))
    return _inputs[key]


def _sub_layout(inp, first):
    """seq_off of the call's sequences from `first` on, in the same buffers: the short sequences as a call of their own."""
    off, alloc = inp["off"][first:], inp["alloc"][first:]
    return torch.tensor(np.concatenate([off, [off[-1] + alloc[-1]]]), dtype=torch.int32, device="cuda"), int(alloc.max())


# (head_dim, L, window, n_kv_heads or None, the branch of launch_attn_bf16 the longest allocation selects)
CASES16 = [(64, 2049, 0, None, "8w-dh64"), (64, 2049, 100, None, "8w-dh64"), (64, 2200, 0, None, "w16"), (64, 2200, 100, None, "w16"),
           (64, 2300, 0, None, "zz8"), (64, 2300, 100, None, "zz8"), (128, 2049, 0, None, "8w-dh128"), (128, 2049, 100, None, "8w-dh128"),
           (64, 2300, 0, 12, "zz8")]


@pytest.mark.parametrize("dh,L,window,n_kv,variant", CASES16)
def test_attention16_beyond_2048_rows_vs_float64(ctx, dh, L, window, n_kv, variant):
    H = n_kv or (12 if dh == 64 else 8)
    scale = 1.0 if dh == 64 else 128 ** -0.5
    inp, ref = inputs(dh, L, window, H, scale)
    assert A.attn_variant(dh, inp["max_alloc"]) == variant and inp["max_alloc"] > 2048
    T, d = inp["T"], H * dh
    so = A._seq_off(inp)
    for fmt in ("bf16", "f16"):
        qk, vt = A._buffers16(inp, fmt)
        outs = []
        for _ in range(2):
            if n_kv is None:
                out = torch.full((T, d + 8), A.OUT_FILL, dtype=A.HALF[fmt], device="cuda")
                ctx.attention(qk[0, :T, :d], qk[0, :T, d:], vt[0], out, so, H, dh, inp["max_alloc"], window=window, scale=scale, causal=True)
            else:
                # grouped 2 : 1 -- query heads 2 g and 2 g + 1 read key / value head g; head 2 g + 1's queries are halved (exact), so the
                # two heads of a group differ: reference = plain attention on the replicated K / V
                # (q2 [rows, 2 d] has the leading dimension of the q | k buffer: k stays where it is)
                qh = qk[0, :, :d].reshape(-1, H, dh)
                q2 = torch.stack([qh, qh * 0.5], dim=2).reshape(-1, 2 * d).contiguous()
                out = torch.full((T, 2 * d + 8), A.OUT_FILL, dtype=A.HALF[fmt], device="cuda")
                ctx.attention(q2[:T], qk[0, :T, d:], vt[0], out, so, 2 * H, dh, inp["max_alloc"], window=window, scale=scale, n_kv_heads=H)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), "two runs of one call differ"
        out = outs[0].cpu()
        in_alloc = np.zeros(T, bool)
        for s0, a in zip(inp["off"].tolist(), inp["alloc"].tolist()):
            in_alloc[s0:s0 + a] = True
        assert (out[torch.from_numpy(~in_alloc)].double() == A.OUT_FILL).all(), "a row outside every allocation was written"
        if n_kv is None:
            assert (out[:, d:].double() == A.OUT_FILL).all()
            A.check16(f"dh{dh} L={L} w={window} [{variant}]", out, ref, inp, fmt)
        else:
            assert (out[:, 2 * d:].double() == A.OUT_FILL).all()
            ref2 = _grouped_ref(inp, H, dh, window, scale)
            rows = A._real_rows(inp)
            err = float(np.abs(out[:, :2 * d].double().numpy()[rows] - ref2[rows]).max())
            bound = A.BOUND16 * A.U16[fmt] * A._vmax(inp)
            print(f"dh{dh} L={L} grouped 2:1 [{variant}] {fmt}: max|ctx - ref| = {err:.3e}  (bound {bound:.3e}, {err / bound:.2f})")
            assert err <= bound


_grouped = {}


def _grouped_ref(inp, H, dh, window, scale):
    key = (id(inp), window)
    if key not in _grouped:
        _grouped.clear()
        R_ = inp["q"].shape[0]
        q2 = np.stack([inp["q"].reshape(R_, H, dh), inp["q"].reshape(R_, H, dh) * 0.5], axis=2).reshape(R_, 2 * H * dh)
        _grouped[key] = packed_attention(q2, R.repeat_kv(inp["k"], H, 2, dh), R.repeat_kv(inp["v"], H, 2, dh), inp["off"], inp["lens"], 2 * H,
                                         window, scale)
    return _grouped[key]


def f32_bound(inp, n_keys, dh, scale):
    """The fp32 bound of the module docstring, as a multiple of max|v|, from the inputs of the case."""
    H, L = inp["H"], int(inp["lens"][0])
    q = np.abs(inp["q"][:L]).astype(np.float32).reshape(L, H, dh)
    k = np.abs(inp["k"][:L]).astype(np.float32).reshape(L, H, dh)
    lmax = scale * max(float((q[:, h] @ k[:, h].T).max()) for h in range(H))
    chunks = -(-n_keys // 2048)
    return U32 * (n_keys + n_keys / 64 + 6 + 4 * chunks + 2 + 2 * ((dh + 3) * lmax + 2)), lmax


# (head_dim, L, window, mode): mode "causal" | "gqa" (grouped 2 : 1) | "bidir" (seq_len = the real lengths)
CASES32 = [(64, 2049, 0, "causal"), (64, 4100, 0, "causal"), (64, 4100, 100, "causal"), (128, 2049, 100, "causal"), (128, 4100, 0, "causal"),
           (128, 4100, 0, "gqa"), (128, 4100, 0, "bidir")]


@pytest.mark.parametrize("dh,L,window,mode", CASES32)
def test_attention_fp32_beyond_2048_keys_vs_float64(ctx, dh, L, window, mode):
    H = 12 if dh == 64 else 8
    scale = 1.0 if dh == 64 else 128 ** -0.5
    inp, ref = inputs(dh, L, window, H, scale)
    T, d = inp["T"], H * dh
    Hq = 2 * H if mode == "gqa" else H
    dq = Hq * dh
    if mode == "gqa":
        ref = _grouped_ref(inp, H, dh, window, scale)
    elif mode == "bidir":
        ref = packed_attention_bidir(inp["q"], inp["k"], inp["v"], inp["off"], inp["lens"], H, scale)
    qkv = torch.zeros((T + A.SLACK_ROWS, dq + 2 * d), dtype=torch.float32)
    q = torch.from_numpy(inp["q"]).float()
    qkv[:, :dq] = q if mode != "gqa" else torch.stack([q.view(-1, H, dh), q.view(-1, H, dh) * 0.5], dim=2).reshape(-1, dq)
    qkv[:, dq:dq + d] = torch.from_numpy(inp["k"])
    qkv[:, dq + d:] = torch.from_numpy(inp["v"])
    qkv = qkv.cuda()
    lens_dev = torch.tensor(inp["lens"], dtype=torch.int32, device="cuda")

    def run(so, max_alloc, first=0):
        out = torch.full((T, dq), A.OUT_FILL, dtype=torch.float32, device="cuda")
        kw = dict(window=window, scale=scale)
        if mode == "gqa":
            kw["n_kv_heads"] = H
        elif mode == "bidir":
            kw.update(causal=False, seq_len=lens_dev[first:])
        else:
            kw["causal"] = True
        ctx.attention(qkv[:T, :dq], qkv[:T, dq:dq + d], qkv[:T, dq + d:], out, so, Hq, dh, max_alloc, **kw)
        return out

    outs = [run(A._seq_off(inp), inp["max_alloc"]) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and inp["max_alloc"] > 2048
    rows = A._real_rows(inp)
    got = outs[0].cpu().double().numpy()
    n_keys = min(L, window) if window else L
    mult, lmax = f32_bound(inp, n_keys, dh, scale)
    vmax = A._vmax(inp)
    err = float(np.abs(got[rows] - ref[rows]).max())
    print(f"fp32 dh{dh} L={L} w={window} {mode}: Lmax {lmax:.1f}, max|ctx - ref| = {err:.3e}  (bound {mult * vmax:.3e}, measured / bound {err / (mult * vmax):.3f})")
    assert mult < 1e-3, "the derived bound must stay below 1e-3 max|v| (a dropped chunk costs ~0.5 max|v|)"
    assert err <= mult * vmax
    in_alloc = np.zeros(T, bool)
    for s0, a in zip(inp["off"].tolist(), inp["alloc"].tolist()):
        in_alloc[s0:s0 + a] = True
    assert (got[~in_alloc] == A.OUT_FILL).all(), "a row outside every allocation was written"
    # rows of at most 2048 keys: the bits of a call the one-chunk kernel serves -- the short sequences as a call of their own ...
    so_short, ma_short = _sub_layout(inp, 1)
    short = run(so_short, ma_short, first=1)
    lo = int(inp["off"][1])
    assert ma_short <= 2048 and torch.equal(short[lo:], outs[0][lo:]), "a short sequence beside a long one lost its bits"
    # ... and (causal) the head of the long sequence: its first 2048 rows as a sequence of 2048 tokens
    if mode != "bidir":
        head = run(torch.tensor([0, 2048], dtype=torch.int32, device="cuda"), 2048)
        assert torch.equal(head[:2048], outs[0][:2048]), "a row of at most 2048 keys differs from the one-chunk kernel's"


# ---- 2. forward against the fixtures --------------------------------------------------------------------------------------------

_models = {}


def long_model(tag, dtype):
    from sgpt_amd import SGPTModel
    if (tag, dtype) not in _models:
        fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
        _models[(tag, dtype)] = SGPTModel(cfg, w, device="cuda:0", dtype=dtype)
    return _models[(tag, dtype)]


def _norm(a):
    a = np.asarray(a, np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)


def _paths(seqs):
    """(which fixture sequences, the rows the call packs): the 2049-token sequence alone, and all of them."""
    return [([0], "query path"), (list(range(len(seqs))), "bulk path" if sum(len(s) for s in seqs) > 4096 else "query path")]


@pytest.mark.parametrize("tag", TAGS)
def test_long_forward_fp32_vs_hf_golden(tag):
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
    m = long_model(tag, "fp32")
    assert m.max_seq_len == 4352
    for sel, path in _paths(seqs):
        sub = [seqs[i] for i in sel]
        pb = m.pack(sub)
        assert pb.max_alloc > 2048 and (pb.T_pad <= 4096) == (path == "query path")
        for mode in MODES:
            got = m.encode_ids(sub, mode=mode).cpu().numpy()
            err = maxabs(got, fx[f"emb_{mode}"][sel])
            print(f"{tag} fp32 {path} {mode}: max|emb - ref| = {err:.3e}")
            assert err < TOL_FP32, (tag, path, mode)
        worst = 0.0
        for li in range(cfg.num_layers + 1):
            hid = m.token_embeddings(sub, layer_idx=li)
            for col, r in enumerate(rows):
                i = int(np.searchsorted(cuts, r, side="right")) - 1
                if i in sel:
                    worst = max(worst, maxabs(hid[sel.index(i)][r - cuts[i]].cpu().numpy(), fx["hidden"][li, col]))
        print(f"{tag} fp32 {path} recorded hidden rows: max|h - ref| = {worst:.3e}")
        assert worst < TOL_FP32
    assert m.range_flags(reset=False) == 0


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_long_forward_16bit_vs_hf_golden(tag, dtype):
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
    m = long_model(tag, dtype)
    bar = TOL_F16 if dtype == "f16" else 8 * TOL_F16
    for sel, path in _paths(seqs):
        sub = [seqs[i] for i in sel]
        for mode in MODES:
            got = m.encode_ids(sub, mode=mode).cpu().numpy()
            ref = fx[f"emb_{mode}"][sel]
            assert np.isfinite(got).all()
            err = maxabs(_norm(got), _norm(ref))
            dcos = maxabs(_norm(got) @ _norm(got).T, _norm(ref) @ _norm(ref).T)
            print(f"{tag} {dtype} {path} {mode}: max|normalised emb - ref| = {err:.3e}, max|cos - cos_ref| = {dcos:.3e}")
            assert err < bar and dcos < bar, (tag, path, mode)
    assert m.range_flags(reset=False) == 0


# ---- 3. invariance ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_long_batch_invariance(tag, dtype):
    """Each sequence encoded alone equals its row of the batch, bit for bit: the 7-token one changes attention kernel (fp32) and
    projection path (a 32-row layout against the bulk one) on the way."""
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case(tag)
    m = long_model(tag, dtype)
    batch = m.encode_ids(seqs, mode="weightedmean")
    for i, s in enumerate(seqs):
        alone = m.encode_ids([s], mode="weightedmean")
        assert torch.equal(alone[0], batch[i]), (tag, dtype, i, float((alone[0] - batch[i]).abs().max()))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(ctx, tmp_path):
    from sgpt_amd import SGPTModel
    from sgpt_amd._lib import SGPT_MAX_SEQ_LEN
    from sgpt_amd.model import SGPTConfig, synthetic_llama_weights
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case("tiny_llama_long")
    m = long_model("tiny_llama_long", "f16")
    before = m.encode_ids(seqs[2:], mode="mean")
    with pytest.raises(ValueError, match="sequence longer than 32768 tokens"):
        m.encode_ids([[5] * 32770])
    with pytest.raises(ValueError, match="sequence longer than max_position_embeddings"):
        m.encode_ids([[5] * 4353])
    m.encode_ids([[5] * 4352])                                      # the last position of the table is in range
    # the C entry's own refusal, behind pack()'s: a layout that claims an allocation above the limit (nothing is launched)
    import dataclasses
    with pytest.raises(ValueError, match=re.escape("sgpt_encode: sequence longer than 32768 tokens (SGPT_MAX_SEQ_LEN)")):
        m.encode_packed(dataclasses.replace(m.pack(seqs[2:]), max_alloc=SGPT_MAX_SEQ_LEN + 2), mode="mean")
    folded = SGPTConfig.from_hf_dict(dict(hf, model_type="mistral", sliding_window=2100))
    assert (folded.window_size, folded.max_position_embeddings) == (0, 2100)
    mm = SGPTModel(folded, synthetic_llama_weights(folded, seed=5), device="cuda:0", dtype="f16")
    assert mm.max_seq_len == 2100
    with pytest.raises(ValueError, match="sequence longer than max_position_embeddings"):
        mm.encode_ids([seqs[1]])                                    # 4100 tokens against a window of 2100 folded away
    assert torch.isfinite(mm.encode_ids([seqs[1][:2100]])).all()
    mm.close()
    # the stand-alone entries: SGPT_MAX_SEQ_LEN + 2 rows through the causal entry, and the plain entry's own bound of 2048
    z = torch.zeros((64, 64), dtype=torch.float16, device="cuda")
    so = torch.tensor([0, 32], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=re.escape(f"sgpt_attention_ex: max_alloc_len even, in [2, {SGPT_MAX_SEQ_LEN}]")):
        ctx.attention(z[:32], z[:32], z, z[:32].clone(), so, 1, 64, SGPT_MAX_SEQ_LEN + 2, causal=True)
    with pytest.raises(ValueError, match=re.escape(f"sgpt_attention_gqa: max_alloc_len even, in [2, {SGPT_MAX_SEQ_LEN}]")):
        ctx.attention(z[:32], z[:32], z, z[:32].clone(), so, 1, 64, SGPT_MAX_SEQ_LEN + 2, n_kv_heads=1)
    with pytest.raises(ValueError, match=re.escape("sgpt_attention: max_alloc_len even, in [2, 2048]")):
        ctx.attention(z[:32], z[:32], z, z[:32].clone(), so, 1, 64, 2050)
    assert torch.equal(m.encode_ids(seqs[2:], mode="mean"), before)
    # an adapter over the model: the default max_seq_length is the model's longest sequence, over-long text is truncated, not refused
    from sgpt_amd.formats import write_st_folder
    from sgpt_amd.st import SentenceTransformerSGPT
    from sgpt_amd.tokenization import SyntheticTokenizer
    p = str(tmp_path / "st")
    write_st_folder(p, hf, {k: torch.from_numpy(v) for k, v in w.items()}, pooling_mode="lasttoken", max_seq_length=100000)
    st = SentenceTransformerSGPT.from_pretrained(p, tokenizer=SyntheticTokenizer(hf["vocab_size"]), device="cuda:0", dtype="f16", frame=([1], [2]))
    assert st.max_seq_length == 4352
    emb = st.encode(["tok%d " % (i % 50) * 1 for i in range(1)] + [" ".join("w%d" % (i % 90) for i in range(6000))])
    assert emb.shape == (2, cfg.hidden_size) and np.isfinite(emb).all()
    st.model.close()


# ---- 5. one call at the limit ---------------------------------------------------------------------------------------------------

def _lasttoken_ref64(w, ids, cfg):
    """float64 `lasttoken` vector of ONE sequence: llama_ref.forward's arithmetic with the causal attention taken in blocks of 1024
    queries (a [n, n] score matrix of 32 768 tokens is 8.6 GB) and the last block reduced to the one row that is pooled."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    n, H, n_kv, L = len(ids), cfg.num_heads, cfg.num_kv_heads, cfg.num_layers
    x = W["embed_tokens.weight"][np.asarray(ids, np.int64)]
    dh = x.shape[1] // H
    pos = np.arange(n)
    scale = 1.0 / math.sqrt(dh)
    for i in range(L):
        p = f"layers.{i}."
        a = R.rms_norm(x, W[p + "input_layernorm.weight"], cfg.layer_norm_epsilon)
        k = R.rope_half(a @ W[p + "self_attn.k_proj.weight"].T, pos, n_kv, dh, cfg.rope_theta)
        v = a @ W[p + "self_attn.v_proj.weight"].T
        first = n - 1 if i == L - 1 else 0                      # the last block: only the pooled row goes on
        q = R.rope_half(a[first:] @ W[p + "self_attn.q_proj.weight"].T, pos[first:], H, dh, cfg.rope_theta)
        ctx_ = np.empty((n - first, H * dh))
        for h in range(H):
            kh, vh = k[:, (h // (H // n_kv)) * dh:][:, :dh], v[:, (h // (H // n_kv)) * dh:][:, :dh]
            for b0 in range(first, n, 1024):
                b1 = min(b0 + 1024, n)
                s = scale * (q[b0 - first:b1 - first, h * dh:(h + 1) * dh] @ kh[:b1].T)
                s[:, b0:][np.triu_indices(b1 - b0, 1)] = -np.inf          # the diagonal block's future keys
                s -= s.max(axis=-1, keepdims=True)
                np.exp(s, out=s)
                ctx_[b0 - first:b1 - first, h * dh:(h + 1) * dh] = (s @ vh[:b1]) / s.sum(axis=-1, keepdims=True)
        x = x[first:] + ctx_ @ W[p + "self_attn.o_proj.weight"].T
        a = R.rms_norm(x, W[p + "post_attention_layernorm.weight"], cfg.layer_norm_epsilon)
        x = x + (R.silu(a @ W[p + "mlp.gate_proj.weight"].T) * (a @ W[p + "mlp.up_proj.weight"].T)) @ W[p + "mlp.down_proj.weight"].T
    return R.rms_norm(x, W["norm.weight"], cfg.layer_norm_epsilon)[-1]


def test_blockwise_reference_is_llama_ref():
    """The block-wise reference of the limit test IS llama_ref.forward where that one can run (the 2049-token fixture sequence)."""
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case("tiny_llama_long")
    want = R.forward(w, seqs[:1], cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.layer_norm_epsilon, cfg.rope_theta, 0)[0][-1, -1]
    assert np.abs(_lasttoken_ref64(w, seqs[0], cfg) - want).max() < 1e-12


def test_one_sequence_at_the_limit(ctx):
    """32 768 tokens, f16, one bulk call: grid sizing and 32-bit offsets at the cap; the `lasttoken` vector against float64."""
    from sgpt_amd import SGPTModel
    from sgpt_amd._lib import SGPT_MAX_SEQ_LEN
    from sgpt_amd.model import SGPTConfig
    fx, hf, cfg, w, seqs, cuts, rows = load_long_case("tiny_llama_long")
    cfg = SGPTConfig.from_hf_dict(dict(hf, max_position_embeddings=SGPT_MAX_SEQ_LEN))
    ids = np.random.default_rng(99).integers(3, hf["vocab_size"], size=SGPT_MAX_SEQ_LEN).tolist()
    m = SGPTModel(cfg, w, device="cuda:0", dtype="f16")
    assert m.max_seq_len == SGPT_MAX_SEQ_LEN and len(m.plan_batches(np.asarray([len(ids)]))) == 1
    pb = m.pack([ids])
    assert (pb.T_pad, pb.max_alloc) == (SGPT_MAX_SEQ_LEN, SGPT_MAX_SEQ_LEN)
    got = m.encode_packed(pb, mode="lasttoken").cpu().numpy()
    assert got.shape == (1, cfg.hidden_size) and np.isfinite(got).all() and m.range_flags() == 0
    m.close()
    ref = _lasttoken_ref64(w, ids, cfg)[None, :]
    err = maxabs(_norm(got), _norm(ref))
    print(f"32 768 tokens f16 lasttoken: max|normalised emb - ref64| = {err:.3e}")
    assert err < TOL_F16
