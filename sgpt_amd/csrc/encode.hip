// C ABI (include/sgpt_hip.h): the forward -- one block function per arithmetic (16-bit, fp32, fp8 MFMA) under encode_impl -- and the LM head.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
#include "host.h"
#include "encode_split.h"

namespace {

// What the block functions of one forward share: the call's token layout, the operand format, the launch path and the workspace.
struct Fwd {
    sgpt_model* m; sgpt_ctx* c; hipStream_t s;
    const Family* F;      // the model's family row (host.h)
    const int32_t *pos, *seq_off, *seq_len;
    int B, T, max_alloc;
    // query width n_heads * head_dim and key / value width n_kv_heads * head_dim: both d_model unless the family carries its own head
    // dim (d_q) or groups K / V (d_kv)
    int d_q, d_kv;
    int dt;               // operand format of the projections: SGPT_F32 | SGPT_BF16 | SGPT_F16
    int* range_flag;      // the model's range words (SGPT_F16 stores, e4m3 codes of the fp8-MFMA block) or null
    // can_split: the format takes a precision plan (prec[]); any_*: a block of this call splits that class; split: any of them.
    // fp8: fp8 weight codes, mlp8: with the fp8-MFMA block (block_fp8) rather than weights de-quantised per block.
    // qpath: query-sized kernels (qgemm.hip), qln: with the LayerNorms of a block inside their prologues.
    bool can_split, any_ln, any_att, any_ctx, any_h, split, fp8, mlp8, qpath, qln;
    float* x;             // residual stream fp32
    // LayerNorm output; attention context [T][d_q]; 16-bit: [T][d_q + d_kv] q | k + V^T [d_kv][T] (x3 attention: the lo halves att_lo
    // elements behind), fp32: [T][d_q + 2 d_kv]; MLP hidden
    void *a, *ctx, *qkv, *vt, *h;
    void* gu;             // SGPT_ARCH_LLAMA: fc1 output [T][2 ffn] = gate | up columns, the input of the SwiGLU row kernel
    void* a8; float* sa;  // fp8-MFMA block: LayerNorm output as e4m3 codes + one scale per row
    // q8: a converted SGPT_ARCH_LLAMA model (sgpt_model_set_projections: block_llama_q8) -- a8 / sa hold the RMSNorm output, h the SwiGLU
    // output as e4m3 codes [T][ffn] with sh, one scale per row
    bool q8; float* sh;
    long att_lo;
    long ldvt;            // row length of V^T: the token rows of the CALL
    // One of the two chains of a call (chain_of): the chain owns rows [row0, row0 + T) = sequences [b0, b0 + B) of the call's buffers.
    // pos / seq_off / seq_len / x / a / ctx / qkv / h start at its first row or sequence, vt at its first column; seq_off[] keeps
    // counting from the call's first row.  0, 0: the whole call.
    long row0; int b0;
    hipEvent_t half_ev;   // block_16 records it behind the out-projection when set (the other chain's start, half a block behind)
};

// Descriptor of one projection, out[T][N] = (resid +) A[T][K] . W[N][K]^T (+ bias), from the per-call base.  Built for one launch: the
// caller adds what that launch has more (shifts, split-precision fields, fp8 scales) and lets it go out of scope.
GemmArgs proj(const Fwd& f, const void* A, long lda, const void* W, int N, int K, void* out, long ldo, const float* bias,
              const float* resid = nullptr) {
    GemmArgs g{};
    g.M = f.T; g.m_valid = f.T; g.range_flag = f.range_flag;
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.N = N; g.K = K; g.out = out; g.ldo = ldo; g.bias = bias; g.resid = resid;
    return g;
}

// A split-precision A operand ([hi | lo | hi] rows of 3 k) contracts as ONE K' = 3 k against the [W_hi | W_hi | W_lo] rows of W3:
// a_hi.W_hi + a_lo.W_hi + a_hi.W_lo  (nblk = 2: the activation alone is split -- the first TWO blocks of both layouts)
void split_w(GemmArgs& g, const void* W3, int k, int nblk = 3) { g.W = W3; g.K = nblk * k; g.ldw = 3 * k; g.k_algo = k; }

// The Q | K and V projections of a 16-bit block as two launches over the fused weight (and bias) rows: q | k -> out[T][n_qk] row-major from
// rows [0, n_qk), then V^T[n_v][T] from the n_v rows behind them.  `g` carries what both share (A, K, bias base, shifts).  Split-precision
// operands, by the block's plan for the LayerNorm-1 class p_ln1 (block_16): 0 plain | 1, 2: Q | K contract over all three blocks of W3's
// [W_hi | W_hi | W_lo] rows | 3: over the first two (the activation alone is split); 2: V too, over the rows behind them.
void proj_qk_vt(const Fwd& f, const GemmArgs& g, int n_qk, int n_v, const void* W3 = nullptr, int p_ln1 = 0) {
    GemmArgs qk = g, v = g;
    if (p_ln1) split_w(qk, W3, g.K, p_ln1 == 3 ? 2 : 3);
    qk.N = n_qk;
    gemm(f.c, f.dt, EPI_STORE, f.dt, qk, f.s);
    if (p_ln1 == 2) split_w(v, (const bf16_t*)W3 + (size_t)n_qk * 3 * g.K, g.K);
    else v.W = (const bf16_t*)g.W + (size_t)n_qk * g.K;
    v.N = n_v; v.out = f.vt; v.ldo = f.ldvt; v.bias = g.bias ? g.bias + n_qk : nullptr;
    gemm(f.c, f.dt, EPI_VT, f.dt, v, f.s);
}

// q | k | v of every family: q rows of d_q columns, k and v of d_kv (both d unless the family says otherwise: kv_group query heads share
// one key / value head); the context has q's width
AttnArgs attn_base(const Fwd& f, const LayerW& l, int k_qkv) {
    const sgpt_model_desc& d = f.m->d;
    const int dq = f.d_q;
    AttnArgs at{};
    at.dtype = f.dt;
    at.seq_off = f.seq_off; at.B = f.B; at.H = d.n_heads; at.dh = dq / d.n_heads; at.window = l.is_local ? d.window : 0;
    at.scale = d.attn_scale * pow2f(2 * k_qkv);      // q and k are both stored down-shifted
    at.max_alloc_len = f.max_alloc; at.ctx = f.ctx; at.ldo = dq; at.alibi = f.m->alibi;
    at.q = f.qkv; at.kv_group = d.n_heads / d.n_kv_heads;
    if (f.vt) { at.k = (bf16_t*)f.qkv + dq; at.v = f.vt; at.ldq = dq + f.d_kv; at.ldvt = f.ldvt; }
    else { at.k = (float*)f.qkv + dq; at.v = (float*)f.qkv + dq + f.d_kv; at.ldq = dq + 2 * f.d_kv; }
    if (f.row0) {        // a chain (16-bit, ctx rows of d_q elements): the kernel indexes rows by seq_off[], from the call's first row
        at.ctx = (bf16_t*)f.ctx - f.row0 * dq; at.q = (bf16_t*)f.qkv - f.row0 * at.ldq; at.k = (const bf16_t*)at.q + dq;
        at.v = (bf16_t*)f.vt - f.row0;
    }
    return at;
}

// ---- the BERT family (SGPT_ARCH_BERT; HF:bert/modeling_bert.py BertLayer): post-LayerNorm blocks, bidirectional attention ----
//   q|k|v = x W_qkv^T + b ; ctx = attention(non-causal) ; x = LN_att(x + ctx Wo^T + bo) ; x = LN_out(x + gelu_erf(x W1^T + b1) W2^T + b2)
// Every block ends in a LayerNorm whose output IS the residual stream.  No range shifts (every f16 store is tracked), no precision
// plan, bulk kernels at every layout (the LayerNorm prologues of the query-sized projections assume pre-LN).
AttnArgs attn_bidir(const Fwd& f, const LayerW& l) {
    AttnArgs at = attn_base(f, l, 0);
    at.noncausal = 1; at.seq_len = f.seq_len;        // (window and alibi are 0 already: no local layer, no slopes in this family)
    return at;
}

// the attention of a Llama-family block: causal with the model's window, or -- sgpt_model_set_attention(0) -- that of attn_bidir with
// kv_group query heads per key / value head (no window on any layer then: the setter refuses it)
AttnArgs attn_llama(const Fwd& f, const LayerW& l) { return f.m->bidir ? attn_bidir(f, l) : attn_base(f, l, 0); }

// fp32: the projections read the residual stream itself
sgpt_status block_bert_f32(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T;
    gemm(f.c, SGPT_F32, EPI_STORE, SGPT_F32, proj(f, f.x, dm, l.w_qkv, 3 * dm, dm, f.qkv, 3 * dm, l.b_qkv), f.s);
    launch_attn_f32(attn_bidir(f, l), f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dm, l.w_o, dm, dm, f.x, dm, l.b_o, f.x), f.s);
    launch_layernorm(f.x, l.ln1_g, l.ln1_b, f.x, SGPT_F32, T, dm, d.ln_eps, f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_GELU_ERF, SGPT_F32, proj(f, f.x, dm, l.w_fc, ffn, dm, f.h, ffn, l.b_fc), f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.s);
    launch_layernorm(f.x, l.ln2_g, l.ln2_b, f.x, SGPT_F32, T, dm, d.ln_eps, f.s);
    return SGPT_OK;
}

// 16-bit: `a` holds the 16-bit copy of x the previous write-back LayerNorm (or the embedding LayerNorm) left; the context shares
// its buffer (a is consumed by the Q | K | V projection before the attention writes)
sgpt_status block_bert16(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T, dt = f.dt;
    GemmArgs q = proj(f, f.a, dm, l.w_qkv, 3 * dm, dm, f.qkv, 2 * dm, l.b_qkv);
    if (gemm_qkv_one_launch(T, 2 * dm, f.c->force256 != 0)) {        // query-sized batch: q | k and V^T from one launch
        q.n_split = 2 * dm; q.out2 = f.vt; q.ldo2 = f.ldvt;
        gemm(f.c, dt, EPI_QKV, dt, q, f.s);
    } else proj_qk_vt(f, q, 2 * dm, dm);
    launch_attn_bf16(attn_bidir(f, l), f.s);
    gemm(f.c, dt, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dm, l.w_o, dm, dm, f.x, dm, l.b_o, f.x), f.s);
    launch_layernorm_writeback(f.x, l.ln1_g, l.ln1_b, f.a, dt, T, dm, d.ln_eps, f.range_flag, f.s);
    gemm(f.c, dt, EPI_BIAS_GELU_ERF, dt, proj(f, f.a, dm, l.w_fc, ffn, dm, f.h, ffn, l.b_fc), f.s);
    gemm(f.c, dt, EPI_BIAS_RESID, SGPT_F32, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.s);
    launch_layernorm_writeback(f.x, l.ln2_g, l.ln2_b, f.a, dt, T, dm, d.ln_eps, f.range_flag, f.s);
    return SGPT_OK;
}

// ---- the Llama / Mistral family (SGPT_ARCH_LLAMA; HF:llama/modeling_llama.py LlamaDecoderLayer): pre-RMSNorm, grouped K / V, half-split
// rotary, SwiGLU, no bias -- but the Q | K | V bias of a Qwen2 model (l.b_qkv) and the per-head q / k norm of a Qwen3 model (l.qn_g) ----
//   a = RMS1(x) ; q | k | v = a W^T (+ b) (d_q + 2 d_kv columns) ; [q, k = RMS_head(q, k)] rope_half(q, k) ; x += attention(kv_group) Wo^T ;
//   a = RMS2(x) ; gu = a [Wgate | Wup]^T ; h = silu(gate) * up ; x += h Wdown^T
// No range shifts (every f16 store is tracked), no precision plan, bulk kernels at every layout.  l.b_o / l.b_proj are the model's
// zero vector (the residual epilogue reads a bias).

// the rotary on q (column 0) and k (column d_q) of the projection buffer, behind the head norm where the layer has its gains
void rope_llama(const Fwd& f, const LayerW& l, int dt, long ld, int dh) {
    const sgpt_model_desc& d = f.m->d;
    if (l.qn_g)
        launch_qknorm_rope_half(f.qkv, dt, ld, f.d_q, f.pos, f.m->rot_sin, f.m->rot_cos, l.qn_g, l.kn_g, d.ln_eps, f.T, d.n_heads, d.n_kv_heads,
                                dh, d.max_pos, f.range_flag, f.s);
    else launch_rope_half(f.qkv, dt, ld, f.d_q, f.pos, f.m->rot_sin, f.m->rot_cos, f.T, d.n_heads, d.n_kv_heads, dh, d.max_pos, f.s);
}
sgpt_status block_llama_f32(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T, dq = f.d_q, dh = dq / d.n_heads, dkv = f.d_kv;
    launch_rmsnorm(f.x, l.ln1_g, f.a, SGPT_F32, T, dm, d.ln_eps, nullptr, f.s);
    gemm(f.c, SGPT_F32, EPI_STORE, SGPT_F32, proj(f, f.a, dm, l.w_qkv, dq + 2 * dkv, dm, f.qkv, dq + 2 * dkv, l.b_qkv), f.s);
    rope_llama(f, l, SGPT_F32, dq + 2 * dkv, dh);
    launch_attn_f32(attn_llama(f, l), f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dq, l.w_o, dm, dq, f.x, dm, l.b_o, f.x), f.s);
    launch_rmsnorm(f.x, l.ln2_g, f.a, SGPT_F32, T, dm, d.ln_eps, nullptr, f.s);
    gemm(f.c, SGPT_F32, EPI_STORE, SGPT_F32, proj(f, f.a, dm, l.w_fc, 2 * ffn, dm, f.gu, 2 * ffn, nullptr), f.s);
    launch_swiglu(f.gu, f.h, SGPT_F32, T, ffn, nullptr, f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.s);
    return SGPT_OK;
}

// 16-bit: the context shares a's buffer (a is consumed by the Q | K and V projections before the attention writes)
sgpt_status block_llama16(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T, dt = f.dt, dq = f.d_q, dh = dq / d.n_heads, dkv = f.d_kv;
    launch_rmsnorm(f.x, l.ln1_g, f.a, dt, T, dm, d.ln_eps, f.range_flag, f.s);
    proj_qk_vt(f, proj(f, f.a, dm, l.w_qkv, dq + dkv, dm, f.qkv, dq + dkv, l.b_qkv), dq + dkv, dkv);
    rope_llama(f, l, dt, dq + dkv, dh);
    launch_attn_bf16(attn_llama(f, l), f.s);
    gemm(f.c, dt, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dq, l.w_o, dm, dq, f.x, dm, l.b_o, f.x), f.s);
    launch_rmsnorm(f.x, l.ln2_g, f.a, dt, T, dm, d.ln_eps, f.range_flag, f.s);
    gemm(f.c, dt, EPI_STORE, dt, proj(f, f.a, dm, l.w_fc, 2 * ffn, dm, f.gu, 2 * ffn, nullptr), f.s);
    launch_swiglu(f.gu, f.h, dt, T, ffn, f.range_flag, f.s);
    gemm(f.c, dt, EPI_BIAS_RESID, SGPT_F32, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.s);
    return SGPT_OK;
}

// fp8 projections (sgpt_model_set_projections(1); SGPT_BF16 models, T % 256 == 0): no calibration -- every A operand carries one dynamic
// power-of-two scale per token row, written by the row kernel in front of the projection, every weight one per output channel:
//   a8, sa = e4m3(RMS1(x)) ; q | k = bf16((a8 . Wqk8^T) sa s_w (+ b)) ; V^T alike ; rope, attention, out-projection + residual as block_llama16
//   (w_o is 16-bit: the context has no row scale) ; a8, sa = e4m3(RMS2(x)) ; gu = bf16((a8 . Wgu8^T) sa s_w) ; h8, sh = e4m3(silu(gate) * up) ;
//   x += (h8 . Wdown8^T) sh s_w
// `a` is written by no norm on this path: it holds the context alone (zero_overread).
sgpt_status block_llama_q8(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T, dt = f.dt, dq = f.d_q, dh = dq / d.n_heads, dkv = f.d_kv;
    auto launch = [&](int epi, int out_dtype, GemmArgs q, const float* a_scale, const float* w_scale) {
        Prof pr(f.c, f.s, 2.0 * T * (double)q.N * q.K);
        q.a_scale = a_scale; q.a_scalar = 1.0f; q.w_scale = w_scale;
        q.cu_cap = f.c->cu_cap;                        // per-ctx workgroup cap, as gemm() sets it for the 16-bit launches
        launch_gemm_fp8(epi, out_dtype, q, f.s);
    };
    launch_rmsnorm_q8(f.x, l.ln1_g, f.a8, f.sa, T, dm, d.ln_eps, f.s);
    launch(EPI_STORE, dt, proj(f, f.a8, dm, l.w_qkv, dq + dkv, dm, f.qkv, dq + dkv, l.b_qkv), f.sa, l.s_qkv);
    launch(EPI_VT, dt, proj(f, f.a8, dm, (const uint8_t*)l.w_qkv + (size_t)(dq + dkv) * dm, dkv, dm, f.vt, f.ldvt, l.b_qkv ? l.b_qkv + dq + dkv : nullptr),
           f.sa, l.s_qkv + dq + dkv);
    rope_llama(f, l, dt, dq + dkv, dh);
    launch_attn_bf16(attn_llama(f, l), f.s);
    gemm(f.c, dt, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dq, l.w_o, dm, dq, f.x, dm, l.b_o, f.x), f.s);
    launch_rmsnorm_q8(f.x, l.ln2_g, f.a8, f.sa, T, dm, d.ln_eps, f.s);
    launch(EPI_STORE, dt, proj(f, f.a8, dm, l.w_fc, 2 * ffn, dm, f.gu, 2 * ffn, nullptr), f.sa, l.s_fc);
    launch_swiglu_q8(f.gu, dt, f.h, f.sh, T, ffn, f.s);
    launch(EPI_BIAS_RESID, 0, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.sh, l.s_proj);
    return SGPT_OK;
}

// ---- fp32 block (SGPT_F32): plain operands, q | k | v rows in one buffer ----
sgpt_status block_f32(const Fwd& f, const LayerW& l, int) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T;
    const bool gptj = d.arch == SGPT_ARCH_GPTJ;
    launch_layernorm(f.x, l.ln1_g, l.ln1_b, f.a, SGPT_F32, T, dm, d.ln_eps, f.s);
    gemm(f.c, SGPT_F32, EPI_STORE, SGPT_F32, proj(f, f.a, dm, l.w_qkv, 3 * dm, dm, f.qkv, 3 * dm, l.b_qkv), f.s);
    if (gptj) launch_rope(f.qkv, SGPT_F32, 3 * dm, dm, f.pos, f.m->rot_sin, f.m->rot_cos, T, d.n_heads, dm / d.n_heads, d.rotary_dim, d.max_pos, f.s);
    launch_attn_f32(attn_base(f, l, 0), f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.ctx, dm, l.w_o, dm, dm, f.x, dm, l.b_o, f.x), f.s);   // x += ctx . Wo^T (+ bo)
    // GPT-Neo: x += MLP(LN2(x));  GPT-J (parallel block, HF:gptj:400-411): x += MLP(LN1(x_old)), `a` still holds it
    if (!gptj) launch_layernorm(f.x, l.ln2_g, l.ln2_b, f.a, SGPT_F32, T, dm, d.ln_eps, f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_GELU, SGPT_F32, proj(f, f.a, dm, l.w_fc, ffn, dm, f.h, ffn, l.b_fc), f.s);
    gemm(f.c, SGPT_F32, EPI_BIAS_RESID, SGPT_F32, proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x), f.s);
    return SGPT_OK;
}

// ---- fp8-MFMA block (SGPT_FP8M with calibrated activation scales): the e4m3 weight codes feed the MFMA directly ----
sgpt_status block_fp8(const Fwd& f, const LayerW& l, int li) {
    const sgpt_model_desc& d = f.m->d;
    const int dm = d.d_model, ffn = d.d_ffn, T = f.T;
    const bool gptj = d.arch == SGPT_ARCH_GPTJ;
    const float s_h = f.m->act_scale[li], s_c = f.m->act_scale[d.n_layers + li];     // scales of the GELU output's / the context's codes
    auto launch = [&](int epi, int out_dtype, GemmArgs q) {
        Prof pr(f.c, f.s, 2.0 * T * (double)q.N * q.K);
        q.cu_cap = f.c->cu_cap;                        // per-ctx workgroup cap (sgpt_ctx_set_gemm_cu_cap), as gemm() sets it for the 16-bit launches
        launch_gemm_fp8(epi, out_dtype, q, f.s);
    };
    // attention projections: a8 = e4m3(LN1(x) / sa[row]) feeds Q, K (row-major 16-bit) and V^T
    launch_layernorm_q8(f.x, l.ln1_g, l.ln1_b, f.a8, f.sa, T, dm, d.ln_eps, f.s);
    GemmArgs qk = proj(f, f.a8, dm, l.w_qkv, 2 * dm, dm, f.qkv, 2 * dm, l.b_qkv);
    qk.a_scale = f.sa; qk.a_scalar = 1.0f; qk.w_scale = l.s_qkv;
    launch(EPI_STORE, f.dt, qk);
    GemmArgs v = proj(f, f.a8, dm, (const uint8_t*)l.w_qkv + (size_t)2 * dm * dm, dm, dm, f.vt, T, l.b_qkv ? l.b_qkv + 2 * dm : nullptr);
    v.a_scale = f.sa; v.a_scalar = 1.0f; v.w_scale = l.s_qkv + 2 * dm;
    launch(EPI_VT, f.dt, v);
    if (gptj) launch_rope(f.qkv, f.dt, 2 * dm, dm, f.pos, f.m->rot_sin, f.m->rot_cos, T, d.n_heads, dm / d.n_heads, d.rotary_dim, d.max_pos, f.s);
    AttnArgs at = attn_base(f, l, 0);
    at.out_fp8 = 1; at.out_scale = s_c; at.range_flag = f.range_flag;
    launch_attn_bf16(at, f.s);                         // context as e4m3 codes of ctx / s_c, [T][dm] bytes
    GemmArgs o = proj(f, f.ctx, dm, l.w_o, dm, dm, f.x, dm, l.b_o, f.x);
    o.a_scalar = s_c; o.w_scale = l.s_o;
    launch(EPI_BIAS_RESID, 0, o);
    // a8 = e4m3(LN(x) / sa[row]);  h8 = e4m3(gelu(a8 . W1_8^T * sa * s1 + b1) / s_h);  x += h8 . W2_8^T * s_h * s2 + b2
    // (GPT-J, parallel block: a8 still holds LN1(x_old))
    if (!gptj) launch_layernorm_q8(f.x, l.ln2_g, l.ln2_b, f.a8, f.sa, T, dm, d.ln_eps, f.s);
    GemmArgs fc = proj(f, f.a8, dm, l.w_fc, ffn, dm, f.h, ffn, l.b_fc);
    fc.a_scale = f.sa; fc.a_scalar = 1.0f; fc.w_scale = l.s_fc; fc.out_scale = s_h;
    launch(EPI_BIAS_GELU, 0, fc);
    GemmArgs p = proj(f, f.h, ffn, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x);
    p.a_scalar = s_h; p.w_scale = l.s_proj;
    launch(EPI_BIAS_RESID, 0, p);
    return SGPT_OK;
}

// A LayerNorm of the residual stream in front of the projection `q` that reads it: inside that projection's prologue (qln), or
// one launch into `a` -- [hi | lo | hi] rows of 3 d when the plan splits this class -- with the crest probe behind it.
void block_ln(const Fwd& f, QGemmArgs& q, const float* g, const float* b, int k, bool split, unsigned* crest) {
    const int dm = f.m->d.d_model;
    const float eps = f.m->d.ln_eps;
    q.eps = eps;
    if (f.qln) { q.x = f.x; q.ln_g = g; q.ln_b = b; q.ln_mul = pow2f(-k); return; }
    if (split) launch_layernorm_split(f.x, g, b, f.a, f.dt, f.T, dm, eps, f.s, pow2f(-k));
    else launch_layernorm(f.x, g, b, f.a, f.dt, f.T, dm, eps, f.s, pow2f(-k));
    if (crest) launch_crest16(f.a, f.T, dm, q.g.lda, f.dt, crest, f.s);
}

// One projection of a 16-bit block: the query-sized kernels on the query path, the bulk launchers otherwise.
sgpt_status launch16(const Fwd& f, int epi, int out_dtype, const QGemmArgs& q, const char* what) {
    if (!f.qpath) gemm(f.c, f.dt, epi, out_dtype, q.g, f.s);
    else if (!qgemm(f.c, f.dt, epi, out_dtype, q, f.s)) return fail(f.c, SGPT_ERR_INVALID, std::string("query path: ") + what + " not served");
    return SGPT_OK;
}

// ---- 16-bit block (bf16 / f16 operands; FP8W and un-calibrated FP8M with l's weights de-quantised to bf16) ----
// [LN1 +] QKV -> (rope) -> attention -> out-proj + residual -> [LN2 +] fc1 + GELU -> fc2 + residual
sgpt_status block_16(const Fwd& f, const LayerW& l, int li) {
    sgpt_model* m = f.m; sgpt_ctx* c = f.c; hipStream_t s = f.s;
    const int dm = m->d.d_model, ffn = m->d.d_ffn, T = f.T, dt = f.dt;
    const bool gptj = m->d.arch == SGPT_ARCH_GPTJ;
    // SGPT_F16 range shifts of this block (all 0 unless the checkpoint needed them): class stored as value * 2^-k
    const bool f16m = dt == SGPT_F16;
    const int* sh = &m->shift[(size_t)li * RS_N];
    const int k_ln1 = f16m ? sh[RS_LN1] : 0, k_qkv = f16m ? sh[RS_QKV] : 0, k_h = f16m ? sh[RS_H] : 0;
    const int k_ln2 = f16m ? (gptj ? sh[RS_LN1] : sh[RS_LN2]) : 0;     // GPT-J: ln_1's output feeds the MLP too
    unsigned* slots = m->range_dev + 1 + (size_t)li * RS_N;
    // this block's precision plan
    const int* pc = &m->prec[(size_t)li * PC_N];
    const int p_ln1 = f.can_split ? pc[PC_LN1] : 0;                  // 0 | 1 (q, k split) | 2 (q, k, v split) | 3 (q, k: activation split only)
    const bool p_att = f.can_split && pc[PC_ATT] != 0, p_ctx = f.can_split && pc[PC_CTX] != 0, p_h = f.can_split && pc[PC_H] != 0;
    const bool p_ln2 = f.can_split && pc[PC_LN2] != 0 && (!gptj || p_ln1 != 0);   // GPT-J: fc1 reads ln_1's output (its [hi | lo | hi] rows)
    unsigned* crest = (m->probing && m->crest_dev) ? m->crest_dev + (size_t)li * RS_N : nullptr;
    // row strides of this block's LayerNorm-1 output, of fc1's input (GPT-J: ln_1's output again), of the context and the GELU output
    const long lda1 = p_ln1 ? 3 * dm : dm, lda2 = gptj ? lda1 : (p_ln2 ? 3 * dm : dm), ldc = p_ctx ? 3 * dm : dm, ldh = p_h ? 3 * ffn : ffn;
    sgpt_status st;
    {   // Q,K -> qk[T][2d] row-major ; V -> V^T[d][T]   (p_att: each also as a lo half, att_lo elements behind)
        QGemmArgs q{};
        q.g = proj(f, f.a, lda1, l.w_qkv, 3 * dm, dm, f.qkv, 2 * dm, l.b_qkv);                           // bias: BLOOM only
        q.g.in_mul = pow2f(k_ln1); q.g.out_mul = q.g.out_mul2 = pow2f(-k_qkv); q.g.range_amax = f16m ? slots + RS_QKV : nullptr;
        q.g.lo_delta = q.g.lo_delta2 = p_att ? f.att_lo : 0;
        block_ln(f, q, l.ln1_g, l.ln1_b, k_ln1, p_ln1 != 0, crest ? crest + RS_LN1 : nullptr);
        // ONE EPI_QKV launch: the query path always; a query-sized batch on the bulk path (a launch costs ~8 us there); a bulk batch
        // with plain operands and no bias (GPT-Neo / GPT-J) on the 256x256 kernel -- the V column tiles run with swapped operand
        // roles and leave through the same whole-row store epilogue (gemm.hip); the LayerNorm output panel is read once, one launch
        // boundary less per block.  Same sums: identical bits.
        if (f.qpath || ((p_ln1 == 0 || p_ln1 == 2) && gemm_qkv_one_launch(T, 2 * dm, c->force256 != 0)) ||
            (p_ln1 == 0 && !p_att && l.b_qkv == nullptr && gemm_qkv_bulk(T, 3 * dm, dm, 2 * dm, c->force256 != 0))) {
            if (p_ln1 == 2) split_w(q.g, l.w_qkv3, dm);
            q.g.n_split = 2 * dm; q.g.out2 = f.vt; q.g.ldo2 = f.ldvt;
            if ((st = launch16(f, EPI_QKV, dt, q, "QKV projection")) != SGPT_OK) return st;
        } else {
            // Q | K (split: K' = 3d, or 2d for p_ln1 == 3), then V from the hi block alone unless the plan splits it too (p_ln1 == 2)
            proj_qk_vt(f, q.g, 2 * dm, dm, l.w_qkv3, p_ln1);
        }
    }
    if (gptj) launch_rope(f.qkv, dt, 2 * dm, dm, f.pos, m->rot_sin, m->rot_cos, T, m->d.n_heads, dm / m->d.n_heads, m->d.rotary_dim, m->d.max_pos, s);
    AttnArgs at = attn_base(f, l, k_qkv);
    at.x3 = p_att ? 1 : 0; at.qk_lo_delta = f.att_lo; at.v_lo_delta = f.att_lo;
    at.ldo = ldc; at.ctx_lo_delta = p_ctx ? dm : 0; at.ctx_hi2_delta = p_ctx ? 2 * dm : 0;
    launch_attn_bf16(at, s);
    if (crest) launch_crest16(f.ctx, T, dm, ldc, dt, crest + RS_QKV, s);
    if (m->calibrating)   // FP8M calibration: range of this block's attention context
        launch_absmax16(f.ctx, (long)T * dm, dt, m->h_amax + m->d.n_layers + li, s);
    {   // x += ctx . Wo^T (+ bo)      (the context carries v's shift; split context: K' = 3d against [Wo_hi | Wo_hi | Wo_lo])
        QGemmArgs q{};
        q.g = proj(f, f.ctx, ldc, l.w_o, dm, dm, f.x, dm, l.b_o, f.x);
        if (p_ctx) split_w(q.g, l.w_o3, dm);
        q.g.in_mul = pow2f(k_qkv);
        if ((st = launch16(f, EPI_BIAS_RESID, SGPT_F32, q, "out-projection")) != SGPT_OK) return st;
    }
    if (f.half_ev) HIPC(c, hipEventRecord(f.half_ev, s));
    {   // GPT-Neo: x += MLP(LN2(x));  GPT-J (parallel block, HF:gptj:400-411): x += MLP(LN1(x_old)), `a` still holds it
        QGemmArgs q{};
        q.g = proj(f, f.a, lda2, l.w_fc, ffn, dm, f.h, ldh, l.b_fc);
        if (p_ln2) split_w(q.g, l.w_fc3, dm);
        if (p_h) { q.g.lo_delta = ffn; q.g.hi2_delta = 2 * ffn; }       // the GELU output as a [hi | lo | hi] row for fc2
        q.g.in_mul = pow2f(k_ln2); q.g.out_mul = pow2f(-k_h); q.g.range_amax = f16m ? slots + RS_H : nullptr;
        if (!gptj) block_ln(f, q, l.ln2_g, l.ln2_b, k_ln2, p_ln2, crest ? crest + RS_LN2 : nullptr);
        if ((st = launch16(f, EPI_BIAS_GELU, dt, q, "fc1")) != SGPT_OK) return st;
    }
    if (crest) launch_crest16(f.h, T, ffn, ldh, dt, crest + RS_H, s);
    if (m->calibrating) launch_absmax16(f.h, (long)T * ffn, dt, m->h_amax + li, s);   // FP8M calibration: range of this block's GELU output
    QGemmArgs q{};
    q.g = proj(f, f.h, ldh, l.w_proj, dm, ffn, f.x, dm, l.b_proj, f.x);
    if (p_h) split_w(q.g, l.w_proj3, ffn);
    q.g.in_mul = pow2f(k_h);
    return launch16(f, EPI_BIAS_RESID, SGPT_F32, q, "fc2");
}

using BlockFn = sgpt_status (*)(const Fwd&, const LayerW&, int);
// the block function of this forward: per family, then per arithmetic
BlockFn pick_block(const Fwd& f) {
    const bool bf = f.dt != SGPT_F32;
    if (f.m->d.arch == SGPT_ARCH_BERT) return bf ? block_bert16 : block_bert_f32;
    if (f.m->d.arch == SGPT_ARCH_LLAMA) return f.q8 ? block_llama_q8 : (bf ? block_llama16 : block_llama_f32);
    return f.mlp8 ? block_fp8 : (bf ? block_16 : block_f32);
}

// The argument and pooling refusals of a forward.  layout: ids, pos, seq_off, seq_len; pooled: the outputs that go through the pool
// (out, layer_out, layer_mean).
sgpt_status check_call(sgpt_model* m, const int32_t* const (&layout)[4], const int32_t* pad_left, const int32_t* pool_lo, int B, int T, int max_alloc,
                       int pool_mode, int n_layers_run, bool pooled, const float* hidden_out) {
    sgpt_ctx* c = m->ctx;
    const Family& F = family(m->d.arch);
    if (!layout[0] || !layout[1] || !layout[2] || !layout[3] || B <= 0 || T <= 0 || T % 32 != 0 || max_alloc <= 0 || max_alloc % 2 != 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_encode: bad token layout (T_pad % 32, max_alloc_len % 2)");
    if (n_layers_run < 0 || n_layers_run > m->d.n_layers) return fail(c, SGPT_ERR_INVALID, "sgpt_encode: n_layers_run out of range");
    if (pool_mode < 0 || pool_mode > SGPT_POOL_CLS) return fail(c, SGPT_ERR_INVALID, "sgpt_encode: bad pool_mode");
    if (pool_mode == SGPT_POOL_LEARNTMEAN && !F.learntmean)
        return fail(c, SGPT_ERR_INVALID, std::string("sgpt_encode: learntmean pooling (trained position weights of the SGPT checkpoints) is not available for ") + F.name);
    if (pool_mode == SGPT_POOL_CLS && !F.cls) return fail(c, SGPT_ERR_INVALID, "sgpt_encode: cls pooling belongs to SGPT_ARCH_BERT");
    if (pool_lo && (pool_mode == SGPT_POOL_CLS || pool_mode == SGPT_POOL_LEARNTMEAN))
        return fail(c, SGPT_ERR_INVALID, "sgpt_encode: pool_lo (pooling from a row on) serves weightedmean, mean and lasttoken, not cls or learntmean");
    if (pool_mode == SGPT_POOL_LEARNTMEAN && pooled) {
        if (!m->pool_w) return fail(c, SGPT_ERR_MISSING, "sgpt_encode: learntmean needs sgpt_model_set_pool_weights first");
        // with pad_left on the device the longest padded position is not known here: the kernel clamps the table index,
        // and the Python host checks max(pad_left + len) before the call (model.py::_check_learnt)
        // (allocations are 8-row aligned: the longest sequence has at least max_alloc - 7 tokens)
        if (!pad_left && max_alloc - 7 > m->pool_w_n)
            return fail(c, SGPT_ERR_INVALID, "sgpt_encode: fewer learnt position weights than the longest sequence");
    }
    if (max_alloc > SGPT_MAX_SEQ_LEN)
        return fail(c, SGPT_ERR_INVALID, "sgpt_encode: sequence longer than " + std::to_string(SGPT_MAX_SEQ_LEN) + " tokens (SGPT_MAX_SEQ_LEN)");
    if (!pooled && !hidden_out) return fail(c, SGPT_ERR_INVALID, "sgpt_encode: no output requested");
    return SGPT_OK;
}

constexpr size_t SLACK = 64;  // rows of zeroed slack behind buffers the attention key tiles may over-read

// Fills what the blocks of this call share (the caller has set m, c, s, F, the token layout): the precision-plan scan, the launch path
// (mlp8 / qpath / qln), the workspace carve and the pointers into it.  lp: receives scratch for the per-layer pooled vectors, or null.
sgpt_status plan(Fwd& f, int n_layers_run, float** lp) {
    sgpt_model* m = f.m; sgpt_ctx* c = f.c;
    const int T = f.T, dm = m->d.d_model, ffn = m->d.d_ffn;
    const bool gptj = m->d.arch == SGPT_ARCH_GPTJ, fp8m = m->d.compute_dtype == SGPT_FP8M;
    const bool bf = m->d.compute_dtype != SGPT_F32;                 // 16-bit MFMA operands (bf16 or f16)
    const size_t esz = bf ? 2 : 4;
    f.fp8 = m->d.compute_dtype == SGPT_FP8W || fp8m;
    f.dt = !bf ? SGPT_F32 : (m->d.compute_dtype == SGPT_F16 ? SGPT_F16 : SGPT_BF16);
    f.d_q = m->d.n_heads * head_dim(m->d); f.d_kv = m->d.n_kv_heads * head_dim(m->d);
    const size_t dq = f.d_q, dkv = f.d_kv;
    // Precision plan (prec[]): a split class is stored as [hi | lo | hi] rows of 3 x its width (the consuming GEMM contracts over
    // all three blocks against [W_hi | W_hi | W_lo]; a consumer that is not split reads the first block alone).  Any split at
    // all: the attention context gets its own buffer (the LayerNorm buffer has 3 d rows then).
    f.can_split = bf && !f.fp8;
    for (int li = 0; f.can_split && li < n_layers_run; ++li) {
        const int* pc = &m->prec[(size_t)li * PC_N];
        f.any_ln |= pc[PC_LN1] != 0 || pc[PC_LN2] != 0; f.any_att |= pc[PC_ATT] != 0; f.any_ctx |= pc[PC_CTX] != 0; f.any_h |= pc[PC_H] != 0;
    }
    f.split = f.any_ln || f.any_att || f.any_ctx || f.any_h;
    // FP8M: fp8 MFMA on all four projections when the shapes fit the 256x256x128 kernel and the activation scales are
    // calibrated; otherwise (and while calibrating) the block runs the SGPT_FP8W arithmetic (weights de-quantised to bf16)
    const bool shapes8 = gemm_fp8_shape_ok(T, ffn, dm) && gemm_fp8_shape_ok(T, dm, ffn) && gemm_fp8_shape_ok(T, 2 * dm, dm);
    f.mlp8 = fp8m && !m->calibrating && shapes8;
    if (f.mlp8)
        for (int li = 0; li < n_layers_run; ++li)
            if (!(m->act_scale[li] > 0.f) || !(m->act_scale[m->d.n_layers + li] > 0.f))
                return fail(c, SGPT_ERR_INVALID, "SGPT_FP8M: activation scales are not set (sgpt_model_calibrate_begin / _end, or sgpt_model_set_act_scales)");
    // fp8 projections of a converted Llama-family model: the 16-bit weights are gone, so a layout the fp8 MFMA kernel does not take is
    // refused, not served another way
    if (m->proj8 < 0) return fail(c, SGPT_ERR_INVALID, "sgpt_encode: sgpt_model_set_projections failed part of the way on this model; load it again");
    f.q8 = m->proj8 == 1;
    if (f.q8 && T % 256 != 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_encode: a model with fp8 projections takes layouts of T_pad % 256 == 0 token rows (T_pad = " + std::to_string(T) + ")");
    // Query-sized batches (round 6; qgemm.hip): at most QGEMM_MAX_ROWS token rows, plain 16-bit operands, no probe / calibration
    // pass riding on the forward.  Every projection takes the register-staged deep-prefetch kernel; at d = 512 / 768 / 1024 the two
    // LayerNorms of a sequential block (GPT-Neo, BLOOM) run inside the prologues of the projections they feed: five launches per block
    // instead of seven.  Same arithmetic per element as the bulk path (identical bits); sgpt_ctx_set_tile_policy(1 | 2) keeps the bulk kernels.
    f.qpath = bf && !f.fp8 && !f.split && f.F->qpath && !(m->probing && m->crest_dev) && !m->calibrating && !c->force256 && !c->no_qpath && T <= QGEMM_MAX_ROWS &&
              qgemm_shape_ok(T, 3 * dm, dm, EPI_QKV, 2 * dm) && qgemm_shape_ok(T, dm, dm, EPI_BIAS_RESID, 0) &&
              qgemm_shape_ok(T, ffn, dm, EPI_BIAS_GELU, 0) && qgemm_shape_ok(T, dm, ffn, EPI_BIAS_RESID, 0);
    f.qln = f.qpath && !gptj && qgemm_ln_ok(T, 3 * dm, dm, EPI_QKV, 2 * dm) && qgemm_ln_ok(T, ffn, dm, EPI_BIAS_GELU, 0);
    // workspace carve (all offsets 256-B aligned)
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_x = carve((size_t)T * dm * 4);                        // residual stream fp32
    // LN output [T][d]; where the attention context [T][d_q] shares the buffer it holds the wider of the two
    const size_t o_a = carve((size_t)T * (dq > (size_t)dm ? dq : (size_t)dm) * esz * (f.any_ln ? 3 : 1));
    const size_t o_c = (gptj || f.split) ? carve((size_t)T * dm * esz * (f.any_ctx ? 3 : 1)) : o_a;   // GPT-J: ctx separate (ln_1 output feeds the MLP too)
    // q | k rows of d_q + d_kv columns with V^T (d_kv rows) behind them, or q | k | v rows: (T + SLACK) rows of d_q + 2 d_kv columns.
    // 16-bit: the attention loads query fragments up to 255 rows past the last sequence -- never used, but inside this carve
    size_t qkv_elems = ((size_t)T + SLACK) * (dq + 2 * dkv);
    if (bf && ((size_t)T + 256) * (dq + dkv) > qkv_elems) qkv_elems = ((size_t)T + 256) * (dq + dkv);
    const size_t qkv_bytes = qkv_elems * esz;
    const size_t o_qkv = carve(qkv_bytes * (f.any_att ? 2 : 1));         // 16-bit: q | k rows + V^T (x3 attention: the lo halves behind); fp32: q | k | v rows
    // MLP hidden (FP8M: e4m3 codes in the same region; fp8 projections: codes alone, the 16-bit h is never written)
    const size_t o_h = carve(f.q8 ? (size_t)T * ffn : (size_t)T * ffn * esz * (f.any_h ? 3 : 1));
    const size_t o_gu = f.F->swiglu ? carve((size_t)T * 2 * ffn * esz) : 0;                     // SGPT_ARCH_LLAMA: fc1 output, gate | up columns
    const size_t o_a8 = (f.mlp8 || f.q8) ? carve((size_t)T * dm) : 0;    // FP8M / fp8 projections: norm output as e4m3 codes
    const size_t o_sa = (f.mlp8 || f.q8) ? carve((size_t)T * 4) : 0;     //       + one scale per row
    const size_t o_sh = f.q8 ? carve((size_t)T * 4) : 0;                 // fp8 projections: one scale per row of the SwiGLU codes
    const size_t o_lp = lp ? carve((size_t)(m->d.n_layers + 1) * f.B * dm * 4) : 0;
    sgpt_status st = ensure(c, &c->ws, &c->ws_bytes, off);
    if (st != SGPT_OK) return st;
    char* base = (char*)c->ws;
    f.range_flag = (f.mlp8 || f.dt == SGPT_F16) ? (int*)m->range_dev : nullptr;
    f.x = (float*)(base + o_x); f.a = base + o_a; f.ctx = base + o_c; f.qkv = base + o_qkv; f.h = base + o_h;
    if (f.F->swiglu) f.gu = base + o_gu;
    f.vt = bf ? (void*)((bf16_t*)f.qkv + ((size_t)T + SLACK) * (dq + dkv)) : nullptr;
    if (f.mlp8 || f.q8) { f.a8 = base + o_a8; f.sa = (float*)(base + o_sa); }
    if (f.q8) f.sh = (float*)(base + o_sh);
    if (lp) *lp = (float*)(base + o_lp);
    f.att_lo = (long)(qkv_bytes / 2);      // element distance of the lo halves of q | k and of V^T (x3 attention)
    f.ldvt = T;
    return SGPT_OK;
}

// Rows that are over-read by the attention key tiles but never written in this call must be finite
// (a masked key contributes p = 0, and 0 * NaN = NaN): the slack behind the q/k/v buffers, and -- when
// the attention context has its own buffer (GPT-J) -- the filler rows past the last sequence.  The
// workspace is reused across calls / dtypes, so stale bytes there can decode to NaN.
sgpt_status zero_overread(const Fwd& f) {
    sgpt_ctx* c = f.c; const size_t T = f.T, dm = f.m->d.d_model, dq = f.d_q, dkv = f.d_kv, esz = f.vt ? 2 : 4;
    if (f.vt)            // q | k rows of d_q + d_kv columns, V^T of d_kv rows; x3 attention: their lo halves too
        for (long lo = 0; lo <= (f.any_att ? f.att_lo : 0); lo += f.att_lo) {
            HIPC(c, hipMemsetAsync((bf16_t*)f.qkv + lo + T * (dq + dkv), 0, SLACK * (dq + dkv) * esz, f.s));
            HIPC(c, hipMemsetAsync((bf16_t*)f.vt + lo + T * dkv, 0, SLACK * dkv * esz, f.s));
        }
    else if (f.F->slack_f32) HIPC(c, hipMemsetAsync((float*)f.qkv + T * (dq + 2 * dkv), 0, SLACK * (dq + 2 * dkv) * esz, f.s));
    // (query path with the LayerNorm inside the projections: no LayerNorm launch fills the buffer the context shares with it)
    // (post-LN family in fp32: no LayerNorm ever writes the buffer the context lives in)
    if (f.m->d.arch == SGPT_ARCH_GPTJ || f.mlp8 || f.split || f.qln || (f.F->post_ln && !f.vt))
        HIPC(c, hipMemsetAsync(f.ctx, 0, T * dm * esz * (f.any_ctx ? 3 : 1), f.s));   // (fp8: stale bytes would decode to NaN codes)
    // (fp8 projections: the norms write a8, so nothing fills the buffer the context [T][d_q] lives in -- its filler rows feed the out-projection)
    else if (f.q8) HIPC(c, hipMemsetAsync(f.ctx, 0, T * dq * esz, f.s));
    // (a context wider than the norm output it shares the buffer with: the norm fills T * d elements, and the filler rows of the rest
    // feed the out-projection -- stale bytes there would raise the f16 range word from rows that belong to no sequence)
    else if (dq > dm) HIPC(c, hipMemsetAsync(f.ctx, 0, T * dq * esz, f.s));
    return SGPT_OK;
}

// ---- a bulk call as two chains of whole sequences (include/sgpt_hip.h: sgpt_ctx_set_encode_chains) ----
// Chain A = rows [0, r) on the caller's stream, chain B = [r, T) on the context's stream.  Same buffers, same weights: each launch of a
// chain covers its row range (row kernels, projections: M = its rows) or its sequences (attention, pool).  Every kernel computes a
// row / a sequence from that row / sequence alone, and the projections stay on the 256x256 kernel: identical bits.

// what sgpt_ctx_set_encode_chains(n = 0) means: 1 = one chain | 2 = two (measured; -DSGPT_CHAINS_DEFAULT=1 / 2: same-box A/B builds)
#ifndef SGPT_CHAINS_DEFAULT
#define SGPT_CHAINS_DEFAULT 2
#endif
constexpr int CHAINS_DEFAULT = SGPT_CHAINS_DEFAULT;
constexpr int CHAINS_AUTO_ROWS = 131072;      // row threshold unless the caller gave one: the measured call (1024 x 128 tokens)
// How far chain B starts behind chain A, in half blocks: 0 = together | 1 = behind A's first out-projection | 2 = behind A's first
// block.  Out of phase, one chain's LayerNorm / attention / epilogue-heavy launches meet the other's k-loops instead of their twins.
// Measured: profiles/encode_two_chains_ab.txt.
#ifndef SGPT_CHAIN_PHASE
#define SGPT_CHAIN_PHASE 1
#endif
constexpr int CHAIN_PHASE = SGPT_CHAIN_PHASE;

// Where this call is cut, or row == 0: the conditions of the header, cheapest first.  f: after plan().
EncodeSplit chain_cut(const Fwd& f, BlockFn block, const int32_t* seq_off_host, bool pooled_only) {
    sgpt_model* m = f.m; sgpt_ctx* c = f.c;
    const EncodeSplit none{0, 0};
    const int mode = c->chains ? c->chains : CHAINS_DEFAULT;
    const int dm = m->d.d_model, ffn = m->d.d_ffn;
    if (mode != 2 || !seq_off_host || !pooled_only || block != block_16) return none;
    if (f.qpath || f.fp8 || f.mlp8 || f.split || m->calibrating || m->probing) return none;
    if (f.T < (c->chain_min_rows > 0 ? c->chain_min_rows : CHAINS_AUTO_ROWS) || f.T % ENCODE_SPLIT_TILE != 0) return none;
    const EncodeSplit cut = encode_split_point(seq_off_host, f.B, f.T);
    if (cut.row == 0) return none;
    const bool f256 = c->force256 != 0;
    for (int rows : {cut.row, f.T - cut.row})
        if (!gemm_bulk_256(rows, 2 * dm, dm, EPI_STORE, f256) || !gemm_bulk_256(rows, dm, dm, EPI_VT, f256) ||
            !gemm_bulk_256(rows, dm, dm, EPI_BIAS_RESID, f256) || !gemm_bulk_256(rows, ffn, dm, EPI_BIAS_GELU, f256) ||
            !gemm_bulk_256(rows, dm, ffn, EPI_BIAS_RESID, f256))
            return none;
    // a capturing stream records the call as one chain: a captured graph never gets parallel branches (a failed query counts as capturing)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(f.s, &cap) != hipSuccess) { (void)hipGetLastError(); return none; }
    return cap == hipStreamCaptureStatusNone ? cut : none;
}

// the context's stream and events, on the first call that is cut
sgpt_status chain_init(sgpt_ctx* c) {
    if (!c->chain_stream) HIPC(c, hipStreamCreateWithFlags(&c->chain_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->chain_ev)
        if (!e) HIPC(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return SGPT_OK;
}

// The chain of call `f` that owns rows [row0, row0 + rows) = sequences [b0, b0 + nb), on stream s (16-bit block_16 families: the
// LayerNorm output, the context and q, k, v all have d_model columns)
Fwd chain_of(const Fwd& f, int row0, int rows, int b0, int nb, hipStream_t s) {
    const size_t dm = f.m->d.d_model, ffn = f.m->d.d_ffn, r = row0;
    Fwd h = f;
    h.s = s; h.row0 = row0; h.b0 = b0; h.T = rows; h.B = nb;
    h.pos += r; h.seq_off += b0; h.seq_len += b0;
    h.x += r * dm;
    h.a = (bf16_t*)f.a + r * dm; h.ctx = (bf16_t*)f.ctx + r * dm; h.qkv = (bf16_t*)f.qkv + r * 2 * dm; h.vt = (bf16_t*)f.vt + r;
    h.h = (bf16_t*)f.h + r * ffn;
    return h;
}

// Before the chains part: chain A's last sequences load keys (up to 63 rows) and query fragments (up to 255 rows) past their end, in
// chain B's rows -- masked, but 0 * NaN = NaN, and in the first block chain B may not have written them yet in this call.
sgpt_status zero_cut_overread(const Fwd& f, int r) {
    const size_t dm = f.m->d.d_model;
    HIPC(f.c, hipMemsetAsync((bf16_t*)f.qkv + (size_t)r * 2 * dm, 0, (size_t)256 * 2 * dm * 2, f.s));
    HIPC(f.c, hipMemset2DAsync((bf16_t*)f.vt + r, (size_t)f.ldvt * 2, 0, SLACK * 2, dm, f.s));
    return SGPT_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// One forward over the packed token axis.  `layer_out` (fp32 [n_layers+1, B, d]) additionally receives the pooled
// vector of every hidden state on the way (sgpt_encode_layers).
static sgpt_status encode_impl(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                               const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                               int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln, int32_t normalize,
                               float* out, float* hidden_out, float* layer_out, float* layer_mean, void* stream,
                               const int32_t* seq_off_host = nullptr, const int32_t* pool_lo = nullptr) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    const Family& F = family(m->d.arch);
    sgpt_status st = check_call(m, {ids, pos, seq_off, seq_len}, pad_left, pool_lo, B, T, max_alloc, pool_mode, n_layers_run, out || layer_out || layer_mean, hidden_out);
    if (st != SGPT_OK) return st;
    if (!F.lnf) apply_final_ln = 0;    // no final norm in this family: the last block's LayerNorm output is hidden_states[-1]
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    Fwd f{};
    f.m = m; f.c = c; f.s = s; f.F = &F; f.pos = pos; f.seq_off = seq_off; f.seq_len = seq_len; f.B = B; f.T = T; f.max_alloc = max_alloc;
    if ((st = plan(f, n_layers_run, layer_mean && !layer_out ? &layer_out : nullptr)) != SGPT_OK) return st;   // (their mean alone: scratch)
    if ((st = zero_overread(f)) != SGPT_OK) return st;
    const int dm = m->d.d_model, ffn = m->d.d_ffn, dt = f.dt; float* x = f.x;
    auto pool = [&](int final_ln, float* dst, int* range_flag) {
        launch_lnf_pool(x, m->lnf_g, m->lnf_b, seq_off, seq_len, pad_left, B, dm, m->d.ln_eps, final_ln, pool_mode, normalize, m->pool_w,
                        m->pool_w_n, dst, s, range_flag, F.norm_kind, pool_lo);
    };
    // the embedding (and its LayerNorm) of the rows of g: the call, or one of its chains
    auto embed = [&](const Fwd& g) {
        launch_embed(ids + g.row0, g.pos, m->wte, m->wpe, g.x, g.T, dm, m->d.vocab, m->d.max_pos, g.s);
        if (F.post_ln && g.vt) launch_layernorm_writeback(g.x, m->emb_ln_g, m->emb_ln_b, g.a, dt, g.T, dm, m->d.ln_eps, g.range_flag, g.s);   // x and its 16-bit copy
        else if (m->emb_ln_g) launch_layernorm(g.x, m->emb_ln_g, m->emb_ln_b, g.x, SGPT_F32, g.T, dm, m->d.ln_eps, g.s);   // BLOOM :499
    };
    const BlockFn block = pick_block(f);
    const EncodeSplit cut = chain_cut(f, block, seq_off_host, out && !hidden_out && !layer_out && !layer_mean);
    if (cut.row) {
        // Two chains.  Fork: chain B's stream waits for what the caller's stream holds so far; each chain pools its own sequences;
        // join: the caller's stream waits for chain B.  No host or device-wide wait.
        if ((st = chain_init(c)) != SGPT_OK || (st = zero_cut_overread(f, cut.row)) != SGPT_OK) return st;
        hipStream_t sb = c->chain_stream;
        const Fwd fa = chain_of(f, 0, cut.row, 0, cut.seq, s), fb = chain_of(f, cut.row, T - cut.row, cut.seq, B - cut.seq, sb);
        HIPC(c, hipEventRecord(c->chain_ev[0], s));
        HIPC(c, hipStreamWaitEvent(sb, c->chain_ev[0], 0));
        embed(fa);
        if (CHAIN_PHASE == 0 || n_layers_run == 0) embed(fb);
        for (int li = 0; li < n_layers_run; ++li) {
            Fwd a = fa;
            if (li == 0 && CHAIN_PHASE == 1) a.half_ev = c->chain_ev[1];
            if ((st = block(a, m->L[li], li)) != SGPT_OK) return st;
            if (li == 0 && CHAIN_PHASE != 0) {
                if (CHAIN_PHASE == 2) HIPC(c, hipEventRecord(c->chain_ev[1], s));
                HIPC(c, hipStreamWaitEvent(sb, c->chain_ev[1], 0));
                embed(fb);
            }
            if ((st = block(fb, m->L[li], li)) != SGPT_OK) return st;
        }
        int* rf = m->d.compute_dtype == SGPT_F16 ? (int*)m->range_dev : nullptr;
        for (const Fwd* g : {&fa, &fb})
            launch_lnf_pool(x, m->lnf_g, m->lnf_b, g->seq_off, g->seq_len, pad_left ? pad_left + g->b0 : nullptr, g->B, dm, m->d.ln_eps,
                            apply_final_ln, pool_mode, normalize, m->pool_w, m->pool_w_n, out + (size_t)g->b0 * dm, g->s, rf, F.norm_kind,
                            pool_lo ? pool_lo + g->b0 : nullptr);
        HIPC(c, hipEventRecord(c->chain_ev[2], sb));
        HIPC(c, hipStreamWaitEvent(s, c->chain_ev[2], 0));
        c->chain_calls++;
        HIPC(c, hipGetLastError());
        return SGPT_OK;
    }
    embed(f);
    for (int li = 0; li < n_layers_run; ++li) {
        LayerW l = m->L[li];
        if (layer_out) pool(0, layer_out + (size_t)li * B * dm, nullptr);   // hidden_states[li] = input of block li (HF:gpt_neo:475-478)
        if (f.fp8 && !f.mlp8) {  // this block's weights: e4m3fn codes * 2^k -> bf16, exact; <1 % of the block's time at T >= 16k
            launch_fp8_dequant_rows(l.w_qkv, l.s_qkv, (long)3 * dm, dm, m->dq[0], SGPT_BF16, s);
            launch_fp8_dequant_rows(l.w_o, l.s_o, dm, dm, m->dq[1], SGPT_BF16, s);
            launch_fp8_dequant_rows(l.w_fc, l.s_fc, ffn, dm, m->dq[2], SGPT_BF16, s);
            launch_fp8_dequant_rows(l.w_proj, l.s_proj, dm, ffn, m->dq[3], SGPT_BF16, s);
            l.w_qkv = m->dq[0]; l.w_o = m->dq[1]; l.w_fc = m->dq[2]; l.w_proj = m->dq[3];
        }
        if ((st = block(f, l, li)) != SGPT_OK) return st;
    }
    if (hidden_out) {
        if (apply_final_ln && F.norm_kind == 1) launch_rmsnorm(x, m->lnf_g, hidden_out, SGPT_F32, T, dm, m->d.ln_eps, nullptr, s);
        else if (apply_final_ln) launch_layernorm(x, m->lnf_g, m->lnf_b, hidden_out, SGPT_F32, T, dm, m->d.ln_eps, s);
        else HIPC(c, hipMemcpyAsync(hidden_out, x, (size_t)T * dm * 4, hipMemcpyDeviceToDevice, s));
    }
    if (out) pool(apply_final_ln, out, m->d.compute_dtype == SGPT_F16 ? (int*)m->range_dev : nullptr);
    if (layer_out) pool(apply_final_ln, layer_out + (size_t)n_layers_run * B * dm, nullptr);
    if (layer_mean) launch_mean_over_axis0(layer_out, n_layers_run + 1, (long)B * dm, layer_mean, s);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

extern "C" {

sgpt_status sgpt_encode(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                        const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                        int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln, int32_t normalize,
                        float* out, float* hidden_out, void* stream) {
    return encode_impl(m, ids, pos, seq_off, seq_len, pad_left, B, T, max_alloc, pool_mode, n_layers_run,
                       apply_final_ln, normalize, out, hidden_out, nullptr, nullptr, stream);
}

sgpt_status sgpt_encode_host_layout(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                                    const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                                    int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln, int32_t normalize,
                                    float* out, float* hidden_out, const int32_t* seq_off_host, void* stream) {
    return encode_impl(m, ids, pos, seq_off, seq_len, pad_left, B, T, max_alloc, pool_mode, n_layers_run,
                       apply_final_ln, normalize, out, hidden_out, nullptr, nullptr, stream, seq_off_host);
}

sgpt_status sgpt_encode_pool_from(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                                  const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                                  int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln, int32_t normalize,
                                  float* out, float* hidden_out, const int32_t* seq_off_host, const int32_t* pool_lo, void* stream) {
    return encode_impl(m, ids, pos, seq_off, seq_len, pad_left, B, T, max_alloc, pool_mode, n_layers_run,
                       apply_final_ln, normalize, out, hidden_out, nullptr, nullptr, stream, seq_off_host, pool_lo);
}

sgpt_status sgpt_encode_layers_pool_from(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                                         const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                                         int32_t pool_mode, int32_t normalize, float* out_layers, float* out_mean, const int32_t* pool_lo,
                                         void* stream) {
    if (!m) return SGPT_ERR_INVALID;
    if (!out_layers && !out_mean) return fail(m->ctx, SGPT_ERR_INVALID, "sgpt_encode_layers: no output requested");
    return encode_impl(m, ids, pos, seq_off, seq_len, pad_left, B, T, max_alloc, pool_mode, m->d.n_layers, 1, normalize,
                       nullptr, nullptr, out_layers, out_mean, stream, nullptr, pool_lo);
}

sgpt_status sgpt_encode_layers(sgpt_model* m, const int32_t* ids, const int32_t* pos, const int32_t* seq_off,
                               const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t T, int32_t max_alloc,
                               int32_t pool_mode, int32_t normalize, float* out_layers, float* out_mean, void* stream) {
    if (!m) return SGPT_ERR_INVALID;
    if (!out_layers && !out_mean) return fail(m->ctx, SGPT_ERR_INVALID, "sgpt_encode_layers: no output requested");
    return encode_impl(m, ids, pos, seq_off, seq_len, pad_left, B, T, max_alloc, pool_mode, m->d.n_layers, 1, normalize,
                       nullptr, nullptr, out_layers, out_mean, stream);
}

sgpt_status sgpt_lm_logprobs(sgpt_model* m, const float* hidden, const int32_t* row_idx, const int32_t* targets,
                             int32_t n, float* out_logprob, int32_t* out_greedy, void* stream) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (!hidden || !row_idx || !targets || !out_logprob || n <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_lm_logprobs: bad arguments");
    if (family(m->d.arch).no_lm) return fail(c, SGPT_ERR_INVALID, std::string("sgpt_lm_logprobs: ") + family(m->d.arch).no_lm);
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int dm = m->d.d_model, V = m->d.vocab;
    const long ldv = (V + 3) / 4 * 4;
    const int R = n < 1024 ? n : 1024;                       // rows per chunk: logits chunk [R, V] fp32 (206 MB at V = 50 257)
    const size_t rows_bytes = align_up((size_t)R * dm * 4, 256), lg_bytes = align_up((size_t)R * ldv * 4, 256);
    sgpt_status st = ensure(c, &c->ws2, &c->ws2_bytes, rows_bytes + lg_bytes);
    if (st != SGPT_OK) return st;
    float* rows = (float*)c->ws2;
    float* logits = (float*)((char*)c->ws2 + rows_bytes);
    for (int r0 = 0; r0 < n; r0 += R) {
        const int nr = (n - r0) < R ? (n - r0) : R;
        launch_gather_rows(hidden, row_idx + r0, nr, dm, rows, s);
        GemmArgs g{};
        g.A = rows; g.lda = dm; g.W = m->lm_w; g.ldw = dm; g.M = nr; g.m_valid = nr; g.N = V; g.K = dm;
        g.out = logits; g.ldo = ldv; g.bias = m->lm_b;
        gemm(c, SGPT_F32, EPI_STORE, SGPT_F32, g, s);          // exact fp32 MFMA: scores are sums of ~30 log-probabilities
        launch_logprob_rows(logits, ldv, V, targets + r0, nr, out_logprob + r0, out_greedy ? out_greedy + r0 : nullptr, s);
    }
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

}  // extern "C"
