// C ABI (include/sgpt_hip.h): stand-alone entries of single kernels, for the tests, the studies and the bench.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
#include "host.h"

extern "C" {

sgpt_status sgpt_pool(sgpt_ctx* c, const void* hidden, int32_t dtype, const int32_t* mask, int32_t B, int32_t S,
                      int32_t d, int32_t mode, float* out, void* stream) {
    if (!c || !hidden || !mask || !out || B <= 0 || S <= 0 || d <= 0 || d % 4 || mode < 0 || (mode > 2 && mode != SGPT_POOL_CLS) ||
        (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_pool: bad arguments (d % 4 == 0 required; mode 0 | 1 | 2 | 4; hidden fp32, bf16 or f16)");
    HIPC(c, hipSetDevice(c->device));
    launch_pool(hidden, dtype, mask, B, S, d, mode, nullptr, out, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_pool_learnt(sgpt_ctx* c, const void* hidden, int32_t dtype, const int32_t* mask, int32_t B, int32_t S,
                             int32_t d, const float* pos_weights, float* out, void* stream) {
    if (!c || !hidden || !mask || !out || !pos_weights || B <= 0 || S <= 0 || d <= 0 || d % 4 ||
        (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_pool_learnt: bad arguments (d % 4 == 0 required; hidden fp32, bf16 or f16)");
    HIPC(c, hipSetDevice(c->device));
    launch_pool(hidden, dtype, mask, B, S, d, SGPT_POOL_LEARNTMEAN, pos_weights, out, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_fp8_quantize_rows(sgpt_ctx* c, const float* w, int64_t rows, int64_t cols, uint8_t* codes, float* scale,
                                   void* stream) {
    if (!c || !w || !codes || !scale || rows <= 0 || cols <= 0 || cols % 4)
        return fail(c, SGPT_ERR_INVALID, "sgpt_fp8_quantize_rows: bad arguments (cols % 4 == 0 required)");
    HIPC(c, hipSetDevice(c->device));
    launch_fp8_quant_rows(w, rows, cols, codes, scale, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_fp8_dequantize_rows(sgpt_ctx* c, const uint8_t* codes, const float* scale, int64_t rows, int64_t cols,
                                     void* out, int32_t out_dtype, void* stream) {
    if (!c || !codes || !scale || !out || rows <= 0 || cols <= 0 || cols % 4 || (out_dtype != SGPT_F32 && out_dtype != SGPT_BF16 && out_dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_fp8_dequantize_rows: bad arguments (cols % 4 == 0 required)");
    HIPC(c, hipSetDevice(c->device));
    launch_fp8_dequant_rows(codes, scale, rows, cols, out, out_dtype, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_u8_prepare_queries(sgpt_ctx* c, const float* q, const float* start, const float* step, int32_t nq, int32_t d, int32_t ld,
                                    void* qpad, float* qscale, float* qbias, void* stream) {
    if (!c || !q || !start || !step || !qpad || !qscale || !qbias || nq <= 0 || nq > 64 || d <= 0 || ld < 128 || ld % 128 || d > ld)
        return fail(c, SGPT_ERR_INVALID, "sgpt_u8_prepare_queries: bad arguments (1 <= nq <= 64, ld % 128 == 0, 0 < d <= ld)");
    HIPC(c, hipSetDevice(c->device));
    launch_u8_prepare_queries(q, start, step, nq, d, ld, qpad, qscale, qbias, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_f32_to_16(sgpt_ctx* c, const float* in, int64_t numel, void* out, int32_t out_dtype, void* stream) {
    if (!c || !in || !out || numel <= 0 || (out_dtype != SGPT_BF16 && out_dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_f32_to_16: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    launch_f32_to_16(in, numel, out, out_dtype, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_f32_to_bf16(sgpt_ctx* c, const float* in, int64_t numel, void* out, void* stream) {
    return sgpt_f32_to_16(c, in, numel, out, SGPT_BF16, stream);
}

sgpt_status sgpt_layernorm_fp8(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, int32_t T, int32_t d, float eps,
                               uint8_t* codes, float* row_scale, void* stream) {
    if (!c || !x || !gamma || !beta || !codes || !row_scale || T <= 0 || d <= 0 || d % 4 || d > 4096)
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm_fp8: bad arguments (d % 4 == 0, d <= 4096)");
    HIPC(c, hipSetDevice(c->device));
    launch_layernorm_q8(x, gamma, beta, codes, row_scale, T, d, eps, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_linear_fp8(sgpt_ctx* c, int32_t epi, int32_t out_dtype, const uint8_t* A, const float* a_scale, float a_scalar,
                            const uint8_t* W, const float* w_scale, const float* bias, const float* resid, void* out,
                            float out_scale, int32_t M, int32_t N, int32_t K, void* stream) {
    if (!c || !A || !W || !w_scale || !out || !(a_scalar > 0.f)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: bad arguments");
    if (!gemm_fp8_shape_ok(M, N, K)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: M, N, K must be multiples of 256");
    if (epi != EPI_BIAS_GELU && epi != EPI_BIAS_RESID && epi != EPI_STORE && epi != EPI_VT)
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: epi 0 (store 16-bit), 1 (bias+gelu -> fp8), 2 (bias+residual -> fp32) or 4 (transposed 16-bit)");
    if ((epi == EPI_STORE || epi == EPI_VT) && out_dtype != SGPT_BF16 && out_dtype != SGPT_F16)
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: store epilogues write bf16 or f16");
    if ((epi == EPI_BIAS_GELU || epi == EPI_BIAS_RESID) && !bias) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: bias required");
    if (epi == EPI_BIAS_RESID && !resid) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: residual required");
    if (epi == EPI_BIAS_GELU && !(out_scale > 0.f)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_fp8: out_scale required");
    HIPC(c, hipSetDevice(c->device));
    GemmArgs q{};
    q.A = A; q.lda = K; q.W = W; q.ldw = K; q.M = M; q.m_valid = M; q.N = N; q.K = K; q.out = out; q.ldo = epi == EPI_VT ? M : N;
    q.bias = bias; q.resid = resid; q.a_scale = a_scale; q.a_scalar = a_scalar; q.w_scale = w_scale; q.out_scale = out_scale;
    q.range_flag = c->range_flag; q.cu_cap = c->cu_cap;
    { Prof pr(c, (hipStream_t)stream, 2.0 * M * (double)N * K); launch_gemm_fp8(epi, out_dtype, q, (hipStream_t)stream); }
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_row_crest(sgpt_ctx* c, const void* x, int32_t dtype, int64_t n, int32_t d, int64_t ld, float* crest_out, void* stream) {
    if (!c || !x || !crest_out || n <= 0 || n > INT32_MAX || d <= 0 || d % 2 || ld < d || (dtype != SGPT_BF16 && dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_row_crest: bad arguments (16-bit rows, d % 2 == 0)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned* slot = (unsigned*)c->range_flag + 16;          // a scratch word of the ctx's 256-byte flag block
    HIPC(c, hipMemsetAsync(slot, 0, 4, s));
    launch_crest16(x, (int)n, d, ld, dtype, slot, s);
    unsigned h = 0;
    HIPC(c, hipMemcpyAsync(&h, slot, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    memcpy(crest_out, &h, 4);
    return SGPT_OK;
}

sgpt_status sgpt_split16(sgpt_ctx* c, const float* in, int64_t n, int32_t d, int32_t layout, void* out, int32_t out_dtype,
                         void* stream) {
    if (!c || !in || !out || n <= 0 || d <= 0 || d % 4 || (layout != 0 && layout != 1) || (out_dtype != SGPT_BF16 && out_dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_split16: bad arguments (d % 4 == 0, layout 0 | 1, 16-bit out_dtype)");
    HIPC(c, hipSetDevice(c->device));
    launch_split16_rows(in, n, d, layout, out, out_dtype, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_linear(sgpt_ctx* c, int32_t dtype, int32_t epi, int32_t out_dtype, const void* A, const void* W,
                        const float* bias, const float* resid, void* out, int32_t M, int32_t N, int32_t K, void* stream) {
    if (!c || !A || !W || !out || M <= 0 || N <= 0 || K <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: bad arguments");
    const bool in16 = dtype == SGPT_BF16 || dtype == SGPT_F16, o16 = out_dtype == SGPT_BF16 || out_dtype == SGPT_F16;
    if (!in16 && dtype != SGPT_F32) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: bad dtype");
    if (epi != EPI_STORE && !epi_is_gelu(epi) && epi != EPI_BIAS_RESID && epi != EPI_VT)
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear: epi must be 0 (store), 1 (bias+gelu), 2 (bias+residual), 4 (transposed store) or 9 (bias+erf gelu)");
    if ((epi_is_gelu(epi) || epi == EPI_BIAS_RESID) && !bias) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: bias required");
    if (epi == EPI_BIAS_RESID && (!resid || out_dtype != SGPT_F32)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: residual epilogue is fp32");
    if (epi == EPI_VT && (!in16 || out_dtype != dtype || M % 128)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: transposed store is 16-bit, M % 128 == 0");
    if (epi_is_gelu(epi) && out_dtype != dtype) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: gelu output has the operand dtype");
    if (in16 && (o16 ? out_dtype != dtype : false)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: 16-bit output must match the operand format");
    if (!in16 && o16) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: fp32 operands give fp32 output");
    if (K % (in16 ? 8 : 4) || (epi != EPI_STORE && N % 4)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear: K % 8 (16-bit) / 4 (fp32), N % 4");
    HIPC(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.m_valid = M; g.N = N; g.K = K; g.out = out;
    g.ldo = epi == EPI_VT ? M : N; g.bias = bias; g.resid = resid;
    g.range_flag = out_dtype == SGPT_F16 ? c->range_flag : nullptr;
    gemm(c, dtype, epi, out_dtype, g, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_linear_query(sgpt_ctx* c, int32_t dtype, int32_t epi, const void* A, const float* x, const float* ln_gamma,
                              const float* ln_beta, float ln_eps, const void* W, const float* bias, const float* resid, void* out,
                              void* out_vt, int32_t n_split, int32_t M, int32_t N, int32_t K, void* stream) {
    if (!c || !W || !out || M <= 0 || N <= 0 || K <= 0 || (!A && !x)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: bad arguments");
    if (dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: 16-bit operands (SGPT_BF16 | SGPT_F16)");
    if (epi != EPI_STORE && epi != EPI_BIAS_GELU && epi != EPI_BIAS_RESID && epi != EPI_QKV)
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: epi must be 0 (store), 1 (bias+gelu), 2 (bias+residual) or 7 (q | k | V^T)");
    if (x && (!ln_gamma || !ln_beta || (epi != EPI_QKV && epi != EPI_BIAS_GELU)))
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: the LayerNorm prologue feeds epi 7 (QKV) and 1 (fc1 + GELU) and needs gamma / beta");
    if ((epi == EPI_BIAS_GELU || epi == EPI_BIAS_RESID) && !bias) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: bias required");
    if (epi == EPI_BIAS_RESID && !resid) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: residual required");
    if (epi == EPI_QKV && (!out_vt || n_split <= 0 || n_split >= N)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: epi 7 needs out_vt and 0 < n_split < N");
    HIPC(c, hipSetDevice(c->device));
    QGemmArgs q{};
    q.g.A = A; q.g.lda = K; q.g.W = W; q.g.ldw = K; q.g.M = M; q.g.m_valid = M; q.g.N = N; q.g.K = K; q.g.out = out;
    q.g.ldo = epi == EPI_QKV ? n_split : N; q.g.out2 = out_vt; q.g.ldo2 = M; q.g.n_split = epi == EPI_QKV ? n_split : 0;
    q.g.bias = bias; q.g.resid = resid;
    const int out_dtype = epi == EPI_BIAS_RESID ? SGPT_F32 : dtype;
    q.g.range_flag = out_dtype == SGPT_F16 ? c->range_flag : nullptr;
    if (x) { q.x = x; q.ln_g = ln_gamma; q.ln_b = ln_beta; q.eps = ln_eps; q.g.A = nullptr; }
    q.tile = c->qtile;              // the test knob of this entry alone (sgpt_ctx_set_query_tile): sgpt_encode's launches never read it
    if (!qgemm(c, dtype, epi, out_dtype, q, (hipStream_t)stream))
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_query: shape not served by the query-sized kernels (M % 32, M <= 4096; K / 128 a multiple of 4 or 6; "
                                         "N % 16; LayerNorm prologue: K = 512 | 768 | 1024, N % 32)");
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_linear_split(sgpt_ctx* c, int32_t dtype, int32_t epi, const void* A, const void* W, const float* bias, void* out,
                              int64_t ldo, int64_t lo_delta, int64_t hi2_delta, int32_t M, int32_t N, int32_t K, void* stream) {
    if (!c || !A || !W || !out || M <= 0 || N <= 0 || K <= 0 || lo_delta == 0) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: bad arguments");
    if (dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: 16-bit operands");
    if (epi != EPI_STORE && epi != EPI_BIAS_GELU && epi != EPI_VT) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: epi 0 (store), 1 (bias+gelu) or 4 (transposed store)");
    if (epi == EPI_BIAS_GELU && !bias) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: bias required");
    if (epi == EPI_VT && (M % 128 || hi2_delta != 0)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: transposed store needs M % 128 == 0 and writes hi + lo only");
    if (K % 8 || N % 4 || ldo < (epi == EPI_VT ? M : N)) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_split: K % 8, N % 4, ldo >= row length");
    HIPC(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.m_valid = M; g.N = N; g.K = K; g.out = out; g.ldo = ldo; g.bias = bias;
    g.lo_delta = lo_delta; g.hi2_delta = hi2_delta;
    g.range_flag = dtype == SGPT_F16 ? c->range_flag : nullptr;
    gemm(c, dtype, epi, dtype, g, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_linear_qkv(sgpt_ctx* c, int32_t dtype, const void* A, const void* W, void* out, void* out_vt, int32_t n_split,
                            int32_t M, int32_t N, int32_t K, void* stream) {
    if (!c || !A || !W || !out || !out_vt || M <= 0 || N <= 0 || K <= 0 || n_split <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_qkv: bad arguments");
    if (dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_linear_qkv: 16-bit operands (SGPT_BF16 | SGPT_F16)");
    if (!gemm_qkv_bulk(M, N, K, n_split, c->force256 != 0))
        return fail(c, SGPT_ERR_INVALID, "sgpt_linear_qkv: not a bulk shape (M, N, n_split % 256; K % 64, K >= 128; 0 < n_split < N; more than "
                                         "half a wave of q | k tiles)");
    HIPC(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.m_valid = M; g.N = N; g.K = K;
    g.out = out; g.ldo = n_split; g.out2 = out_vt; g.ldo2 = M; g.n_split = n_split;
    g.range_flag = dtype == SGPT_F16 ? c->range_flag : nullptr;
    gemm(c, dtype, EPI_QKV, dtype, g, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

}  // extern "C"

// sgpt_attention / sgpt_attention_ex / sgpt_attention_gqa: one argument check, one descriptor.  kv_group = query heads per key / value head.
static sgpt_status attention_impl(sgpt_ctx* c, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                              void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t dh,
                              int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                              float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                              int64_t ctx_lo_delta, int64_t ctx_hi2_delta, int32_t causal, const int32_t* seq_len, int32_t kv_group, int32_t max_seq,
                              const char* who, void* stream) {
    // max_seq: the longest allocation the entry takes -- SGPT_MAX_SEQ_LEN, but 2048 (the bound and the message of ABI <= v22) for sgpt_attention
    const std::string w = std::string(who) + ": ";   // the entry the caller used: its name leads every refusal
    if (causal != 0 && causal != 1) return fail(c, SGPT_ERR_INVALID, w + "causal 0 | 1");
    if (causal && seq_len) return fail(c, SGPT_ERR_INVALID, w + "seq_len belongs to the bidirectional mode (causal = 0)");
    if (!causal) {
        if (window != 0 || alibi != nullptr) return fail(c, SGPT_ERR_INVALID, w + "bidirectional attention takes no window and no ALiBi");
        if (out_fp8 || x3 || ctx_lo_delta != 0 || ctx_hi2_delta != 0)
            return fail(c, SGPT_ERR_INVALID, w + "out_fp8 and the split-precision modes are causal only");
        if (dtype != SGPT_F32 && dh != 64 && dh != 128) return fail(c, SGPT_ERR_INVALID, w + "16-bit bidirectional attention serves head_dim 64 | 128");
    }
    // every combination launch_attn_bf16 would abort() on is refused here, before anything is launched
    auto mis = [](const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; };
    if (!c || !q || !k || !v || !out || !seq_off || B <= 0 || T <= 0 || H <= 0 || window < 0 || !std::isfinite(scale))
        return fail(c, SGPT_ERR_INVALID, w + "bad arguments");
    const bool in16 = dtype == SGPT_BF16 || dtype == SGPT_F16;
    if (!in16 && dtype != SGPT_F32) return fail(c, SGPT_ERR_INVALID, w + "dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    if (dh != 64 && dh != 128 && dh != 256) return fail(c, SGPT_ERR_INVALID, w + "head_dim 64, 128 or 256");
    if (T % 32) return fail(c, SGPT_ERR_INVALID, w + "T % 32 == 0");
    if (max_alloc_len <= 0 || max_alloc_len > max_seq || max_alloc_len % 2)
        return fail(c, SGPT_ERR_INVALID, w + "max_alloc_len even, in [2, " + std::to_string(max_seq) + "]");
    const long d = (long)H * dh;
    if (ldq < d || ldo < d) return fail(c, SGPT_ERR_INVALID, w + "ldq, ldo >= H * head_dim");
    const bool split_ctx = ctx_lo_delta != 0;
    if (!in16 && (out_fp8 || x3 || split_ctx || ctx_hi2_delta))
        return fail(c, SGPT_ERR_INVALID, w + "out_fp8 / x3 / split context are 16-bit modes");
    if (ctx_hi2_delta != 0 && !split_ctx) return fail(c, SGPT_ERR_INVALID, w + "ctx_hi2_delta needs ctx_lo_delta");
    if (out_fp8) {
        if (dtype != SGPT_BF16) return fail(c, SGPT_ERR_INVALID, w + "out_fp8 takes bf16 operands");
        if (x3 || split_ctx) return fail(c, SGPT_ERR_INVALID, w + "out_fp8 with a split-precision mode");
        if (!(out_scale > 0.f) || !std::isfinite(out_scale)) return fail(c, SGPT_ERR_INVALID, w + "out_scale > 0");
    }
    if (x3 && !attn_x3_supported(dh)) return fail(c, SGPT_ERR_INVALID, w + "x3 needs head_dim 64 | 128");
    if (x3 && (qk_lo_delta == 0 || v_lo_delta == 0)) return fail(c, SGPT_ERR_INVALID, w + "x3 needs non-zero lo deltas");
    if (in16) {
        if (mis(q, 16) || mis(k, 16) || mis(v, 4) || mis(out, 16))
            return fail(c, SGPT_ERR_INVALID, w + "16-byte aligned q / k / out, 4-byte aligned V^T");
        if (ldq % 8 || ldo % (out_fp8 ? 16 : 8) || qk_lo_delta % 8 || ctx_lo_delta % 8 || ctx_hi2_delta % 8 || ldvt % 2 || v_lo_delta % 2)
            return fail(c, SGPT_ERR_INVALID, w + "ldq, ldo, qk / ctx deltas % 8 (out_fp8: ldo % 16); ldvt, v_lo_delta even");
        if (ldvt < T) return fail(c, SGPT_ERR_INVALID, w + "ldvt >= T");
    } else if (mis(q, 16) || mis(k, 16) || mis(v, 16) || mis(out, 4) || ldq % 4) {
        return fail(c, SGPT_ERR_INVALID, w + "fp32 q / k / v 16-byte aligned, ldq % 4");
    }
    HIPC(c, hipSetDevice(c->device));
    AttnArgs at{};
    at.q = q; at.k = k; at.v = v; at.ctx = out; at.seq_off = seq_off;
    at.B = B; at.H = H; at.dh = dh; at.ldq = ldq; at.ldvt = ldvt; at.ldo = ldo;
    at.window = window; at.scale = scale; at.max_alloc_len = max_alloc_len; at.alibi = alibi;
    at.dtype = in16 ? dtype : SGPT_F32;
    at.out_fp8 = out_fp8 ? 1 : 0; at.out_scale = out_scale; at.range_flag = range_flag;
    at.x3 = x3 ? 1 : 0; at.qk_lo_delta = qk_lo_delta; at.v_lo_delta = v_lo_delta;
    at.ctx_lo_delta = ctx_lo_delta; at.ctx_hi2_delta = ctx_hi2_delta;
    at.noncausal = causal ? 0 : 1; at.seq_len = seq_len; at.kv_group = kv_group;
    if (in16) launch_attn_bf16(at, (hipStream_t)stream);
    else launch_attn_f32(at, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

extern "C" {

sgpt_status sgpt_attention_ex(sgpt_ctx* c, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                              void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t dh,
                              int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                              float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                              int64_t ctx_lo_delta, int64_t ctx_hi2_delta, int32_t causal, const int32_t* seq_len, void* stream) {
    return attention_impl(c, dtype, q, k, v, ldq, ldvt, out, ldo, seq_off, B, T, H, dh, window, scale, alibi, max_alloc_len, out_fp8,
                          out_scale, range_flag, x3, qk_lo_delta, v_lo_delta, ctx_lo_delta, ctx_hi2_delta, causal, seq_len, 1, SGPT_MAX_SEQ_LEN, "sgpt_attention_ex", stream);
}

sgpt_status sgpt_attention_gqa(sgpt_ctx* c, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                               void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t n_kv_heads,
                               int32_t dh, int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                               float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                               int64_t ctx_lo_delta, int64_t ctx_hi2_delta, void* stream) {
    if (H <= 0 || n_kv_heads <= 0 || H % n_kv_heads) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa: n_heads % n_kv_heads == 0, both > 0");
    if (alibi != nullptr) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa: no ALiBi with grouped K / V");
    if (out_fp8 || x3 || ctx_lo_delta != 0 || ctx_hi2_delta != 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa: out_fp8 and the split-precision modes are not available with grouped K / V");
    if (dtype != SGPT_F32 && dh != 64 && dh != 128) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa: 16-bit grouped attention serves head_dim 64 | 128");
    return attention_impl(c, dtype, q, k, v, ldq, ldvt, out, ldo, seq_off, B, T, H, dh, window, scale, nullptr, max_alloc_len, 0,
                          out_scale, range_flag, 0, qk_lo_delta, v_lo_delta, 0, 0, 1, nullptr, H / n_kv_heads, SGPT_MAX_SEQ_LEN, "sgpt_attention_gqa", stream);
}

sgpt_status sgpt_attention_gqa_ex(sgpt_ctx* c, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                                  void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t n_kv_heads,
                                  int32_t dh, int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                                  float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                                  int64_t ctx_lo_delta, int64_t ctx_hi2_delta, int32_t causal, const int32_t* seq_len, void* stream) {
    if (H <= 0 || n_kv_heads <= 0 || H % n_kv_heads) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa_ex: n_heads % n_kv_heads == 0, both > 0");
    if (alibi != nullptr) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa_ex: no ALiBi with grouped K / V");
    if (out_fp8 || x3 || ctx_lo_delta != 0 || ctx_hi2_delta != 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa_ex: out_fp8 and the split-precision modes are not available with grouped K / V");
    if (dtype != SGPT_F32 && dh != 64 && dh != 128) return fail(c, SGPT_ERR_INVALID, "sgpt_attention_gqa_ex: 16-bit grouped attention serves head_dim 64 | 128");
    // (causal = 0 with a window: refused by attention_impl, as for sgpt_attention_ex)
    return attention_impl(c, dtype, q, k, v, ldq, ldvt, out, ldo, seq_off, B, T, H, dh, window, scale, nullptr, max_alloc_len, 0,
                          out_scale, range_flag, 0, qk_lo_delta, v_lo_delta, 0, 0, causal, seq_len, H / n_kv_heads, SGPT_MAX_SEQ_LEN, "sgpt_attention_gqa_ex", stream);
}

sgpt_status sgpt_attention(sgpt_ctx* c, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                           void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t dh,
                           int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                           float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                           int64_t ctx_lo_delta, int64_t ctx_hi2_delta, void* stream) {
    return attention_impl(c, dtype, q, k, v, ldq, ldvt, out, ldo, seq_off, B, T, H, dh, window, scale, alibi, max_alloc_len, out_fp8,
                          out_scale, range_flag, x3, qk_lo_delta, v_lo_delta, ctx_lo_delta, ctx_hi2_delta, 1, nullptr, 1, 2048, "sgpt_attention", stream);
}

// ---- the encoder's row kernels stand-alone (elementwise.hip; tests/test_gpu_rowops.py): every argument a launch would index or
// dispatch on is checked here, nothing is launched on a refusal ----
static bool row_width_ok(int32_t d) { return d > 0 && d % 4 == 0 && d <= 4096; }   // RowLN: float4 per lane, NV <= 16
static bool mis(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }  // rows move as float4 / uint2 words

sgpt_status sgpt_embed(sgpt_ctx* c, const int32_t* ids, const int32_t* pos, const float* wte, const float* wpe, int32_t T,
                       int32_t d, int32_t vocab, int32_t max_pos, float* out, void* stream) {
    if (!c || !ids || !wte || !out || T <= 0 || d <= 0 || d % 4 || vocab <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_embed: bad arguments (d % 4 == 0 required)");
    if (wpe && (!pos || max_pos <= 0)) return fail(c, SGPT_ERR_INVALID, "sgpt_embed: a position table needs pos and max_pos > 0");
    if (mis(wte, 16) || mis(wpe, 16) || mis(out, 16)) return fail(c, SGPT_ERR_INVALID, "sgpt_embed: 16-byte aligned tables and output");
    HIPC(c, hipSetDevice(c->device));
    launch_embed(ids, pos, wte, wpe, out, T, d, vocab, max_pos, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_layernorm(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, int32_t T, int32_t d, float eps,
                           void* out, int32_t out_dtype, float out_mul, int32_t split, void* stream) {
    if (!c || !x || !gamma || !beta || !out || T <= 0 || !row_width_ok(d) || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: bad arguments (d % 4 == 0, d <= 4096)");
    const bool o16 = out_dtype == SGPT_BF16 || out_dtype == SGPT_F16;
    if (!o16 && out_dtype != SGPT_F32) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: out_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    int e = 0;
    if (!(out_mul > 0.f) || !std::isfinite(out_mul) || std::frexp(out_mul, &e) != 0.5f)
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: out_mul must be a positive power of two");
    if (out_mul != 1.0f && out_dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: out_mul != 1 is the range shift of an f16 output");
    if (split != 0 && split != 1) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: split 0 | 1");
    if (split && !o16) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: the [hi | lo | hi] split output is 16-bit");
    if ((const void*)out == (const void*)x && (o16 || split)) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: in place is fp32 only");
    if (mis(x, 16) || mis(gamma, 16) || mis(beta, 16) || mis(out, o16 ? 8 : 16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm: 16-byte aligned x / gamma / beta / fp32 out, 8-byte aligned 16-bit out");
    HIPC(c, hipSetDevice(c->device));
    if (split) launch_layernorm_split(x, gamma, beta, out, out_dtype, T, d, eps, (hipStream_t)stream, out_mul);
    else launch_layernorm(x, gamma, beta, out, out_dtype, T, d, eps, (hipStream_t)stream, out_mul);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_layernorm_writeback(sgpt_ctx* c, float* x, const float* gamma, const float* beta, int32_t T, int32_t d, float eps,
                                     void* out16, int32_t out_dtype, void* stream) {
    if (!c || !x || !gamma || !beta || !out16 || T <= 0 || !row_width_ok(d) || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm_writeback: bad arguments (d % 4 == 0, d <= 4096)");
    if (out_dtype != SGPT_BF16 && out_dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm_writeback: out_dtype SGPT_BF16 | SGPT_F16");
    if ((const void*)out16 == (const void*)x) return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm_writeback: out16 is a buffer of its own");
    if (mis(x, 16) || mis(gamma, 16) || mis(beta, 16) || mis(out16, 8))
        return fail(c, SGPT_ERR_INVALID, "sgpt_layernorm_writeback: 16-byte aligned x / gamma / beta, 8-byte aligned out16");
    HIPC(c, hipSetDevice(c->device));
    launch_layernorm_writeback(x, gamma, beta, out16, out_dtype, T, d, eps, out_dtype == SGPT_F16 ? c->range_flag : nullptr, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_rmsnorm(sgpt_ctx* c, const float* x, const float* gamma, int32_t T, int32_t d, float eps, void* out, int32_t out_dtype,
                         void* stream) {
    if (!c || !x || !gamma || !out || T <= 0 || !row_width_ok(d) || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm: bad arguments (d % 4 == 0, d <= 4096)");
    const bool o16 = out_dtype == SGPT_BF16 || out_dtype == SGPT_F16;
    if (!o16 && out_dtype != SGPT_F32) return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm: out_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    if ((const void*)out == (const void*)x && o16) return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm: in place is fp32 only");
    if (mis(x, 16) || mis(gamma, 16) || mis(out, o16 ? 8 : 16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm: 16-byte aligned x / gamma / fp32 out, 8-byte aligned 16-bit out");
    HIPC(c, hipSetDevice(c->device));
    launch_rmsnorm(x, gamma, out, out_dtype, T, d, eps, out_dtype == SGPT_F16 ? c->range_flag : nullptr, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_swiglu(sgpt_ctx* c, const void* gu, int32_t dtype, int32_t T, int32_t ffn, void* out, void* stream) {
    if (!c || !gu || !out || T <= 0 || ffn <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu: bad arguments");
    if (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu: dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    // a thread moves 16 bytes of a row: 4 fp32 / 8 16-bit columns, the up half ffn elements behind the gate half
    if (ffn % (dtype == SGPT_F32 ? 4 : 8) || mis(gu, 16) || mis(out, 16) || gu == (const void*)out)
        return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu: ffn % 8 (16-bit) / 4 (fp32); 16-byte aligned buffers; out is a buffer of its own");
    HIPC(c, hipSetDevice(c->device));
    launch_swiglu(gu, out, dtype, T, ffn, dtype == SGPT_F16 ? c->range_flag : nullptr, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_rmsnorm_fp8(sgpt_ctx* c, const float* x, const float* gamma, int32_t T, int32_t d, float eps, uint8_t* codes,
                             float* row_scale, void* stream) {
    if (!c || !x || !gamma || !codes || !row_scale || T <= 0 || !row_width_ok(d) || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm_fp8: bad arguments (d % 4 == 0, d <= 4096)");
    if (mis(x, 16) || mis(gamma, 16) || mis(codes, 4) || mis(row_scale, 4))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rmsnorm_fp8: 16-byte aligned x / gamma, 4-byte aligned codes / row_scale");
    HIPC(c, hipSetDevice(c->device));
    launch_rmsnorm_q8(x, gamma, codes, row_scale, T, d, eps, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_swiglu_fp8(sgpt_ctx* c, const void* gu, int32_t dtype, int32_t T, int32_t ffn, uint8_t* codes, float* row_scale,
                            void* stream) {
    if (!c || !gu || !codes || !row_scale || T <= 0 || ffn <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu_fp8: bad arguments");
    if (dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu_fp8: dtype SGPT_BF16 | SGPT_F16");
    // a thread moves 16 columns of a row per step: two 16-byte words of the gate half, two of the up half, one of codes
    if (ffn % 16 || mis(gu, 16) || mis(codes, 16) || mis(row_scale, 4) || gu == (const void*)codes)
        return fail(c, SGPT_ERR_INVALID, "sgpt_swiglu_fp8: ffn % 16; 16-byte aligned gu / codes; codes is a buffer of its own");
    HIPC(c, hipSetDevice(c->device));
    launch_swiglu_q8(gu, dtype, codes, row_scale, T, ffn, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

static sgpt_status lnf_pool_impl(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                                 const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                                 int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                                 int32_t* nonfinite_flag, int32_t norm_kind, const int32_t* pool_lo, void* stream);

sgpt_status sgpt_lnf_pool(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                          const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                          int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                          int32_t* nonfinite_flag, void* stream) {
    return lnf_pool_impl(c, x, gamma, beta, seq_off, seq_len, pad_left, B, d, eps, apply_ln, mode, normalize, pos_weights, n_weights, out,
                         nonfinite_flag, 0, nullptr, stream);
}

sgpt_status sgpt_lnf_pool_ex(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                             const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                             int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                             int32_t* nonfinite_flag, int32_t norm_kind, void* stream) {
    if (norm_kind != 0 && norm_kind != 1) return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool_ex: norm_kind 0 (LayerNorm) | 1 (RMSNorm)");
    return lnf_pool_impl(c, x, gamma, beta, seq_off, seq_len, pad_left, B, d, eps, apply_ln, mode, normalize, pos_weights, n_weights, out,
                         nonfinite_flag, norm_kind, nullptr, stream);
}

sgpt_status sgpt_lnf_pool_range(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                                const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                                int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                                int32_t* nonfinite_flag, int32_t norm_kind, const int32_t* pool_lo, void* stream) {
    if (norm_kind != 0 && norm_kind != 1) return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool_range: norm_kind 0 (LayerNorm) | 1 (RMSNorm)");
    if (pool_lo && (mode == SGPT_POOL_CLS || mode == SGPT_POOL_LEARNTMEAN))
        return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool_range: pool_lo serves weightedmean, mean and lasttoken, not cls or learntmean");
    return lnf_pool_impl(c, x, gamma, beta, seq_off, seq_len, pad_left, B, d, eps, apply_ln, mode, normalize, pos_weights, n_weights, out,
                         nonfinite_flag, norm_kind, pool_lo, stream);
}

static sgpt_status lnf_pool_impl(sgpt_ctx* c, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                                 const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                                 int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                                 int32_t* nonfinite_flag, int32_t norm_kind, const int32_t* pool_lo, void* stream) {
    if (!c || !x || !seq_off || !seq_len || !out || B <= 0 || !row_width_ok(d))
        return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool: bad arguments (d % 4 == 0, d <= 4096)");
    if (mode < SGPT_POOL_WEIGHTEDMEAN || mode > SGPT_POOL_LEARNTMEAN) return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool: mode 0 .. 3");
    if (apply_ln && (!gamma || (!beta && norm_kind == 0) || !(eps >= 0.f) || !std::isfinite(eps)))
        return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool: apply_ln needs gamma, beta (LayerNorm) and eps >= 0");
    if (mode == SGPT_POOL_LEARNTMEAN && (!pos_weights || n_weights <= 0))
        return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool: learntmean needs pos_weights and n_weights > 0");
    if (mis(x, 16) || mis(gamma, 16) || mis(beta, 16)) return fail(c, SGPT_ERR_INVALID, "sgpt_lnf_pool: 16-byte aligned x / gamma / beta");
    HIPC(c, hipSetDevice(c->device));
    launch_lnf_pool(x, gamma, beta, seq_off, seq_len, pad_left, B, d, eps, apply_ln ? 1 : 0, mode, normalize ? 1 : 0, pos_weights,
                    n_weights, out, (hipStream_t)stream, nonfinite_flag, norm_kind, pool_lo);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_rope(sgpt_ctx* c, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos, const float* sin_t,
                      const float* cos_t, int32_t T, int32_t H, int32_t head_dim, int32_t rotary_dim, int32_t max_pos, void* stream) {
    if (!c || !buf || !pos || !sin_t || !cos_t || T <= 0 || H <= 0 || head_dim <= 0 || max_pos <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_rope: bad arguments");
    if (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_rope: dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    if (rotary_dim <= 0 || rotary_dim % 2 || rotary_dim > head_dim)
        return fail(c, SGPT_ERR_INVALID, "sgpt_rope: rotary_dim even, in [2, head_dim]");
    // a thread moves one (x[2i], x[2i+1]) pair as one 8- / 4-byte word; q [0, H dh) and k [k_off, k_off + H dh) of one row must not overlap
    const int64_t dm = (int64_t)H * head_dim;
    if (head_dim % 2 || ld % 2 || k_off % 2 || k_off < dm || ld < k_off + dm || ((uintptr_t)buf & (dtype == SGPT_F32 ? 7u : 3u)))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rope: head_dim, ld, k_off even; k_off >= H * head_dim; ld >= k_off + H * head_dim; buf aligned to a pair");
    HIPC(c, hipSetDevice(c->device));
    launch_rope(buf, dtype, ld, k_off, pos, sin_t, cos_t, T, H, head_dim, rotary_dim, max_pos, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_rope_half(sgpt_ctx* c, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos, const float* sin_t,
                           const float* cos_t, int32_t T, int32_t H, int32_t H_kv, int32_t head_dim, int32_t max_pos, void* stream) {
    if (!c || !buf || !pos || !sin_t || !cos_t || T <= 0 || H <= 0 || H_kv <= 0 || head_dim <= 0 || max_pos <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_rope_half: bad arguments");
    if (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_rope_half: dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    // a thread moves four consecutive x[i] and their partners x[i + dh/2] as 16- / 8-byte words, with one float4 of each table
    const int64_t dq = (int64_t)H * head_dim, dk = (int64_t)H_kv * head_dim;
    if (head_dim % 8 || ld % 4 || k_off % 4 || k_off < dq || ld < k_off + dk || mis(buf, dtype == SGPT_F32 ? 16 : 8) || mis(sin_t, 16) || mis(cos_t, 16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_rope_half: head_dim % 8; ld, k_off % 4; k_off >= H * head_dim; ld >= k_off + H_kv * head_dim; "
                                         "buf aligned to four elements, tables to 16 bytes");
    HIPC(c, hipSetDevice(c->device));
    launch_rope_half(buf, dtype, ld, k_off, pos, sin_t, cos_t, T, H, H_kv, head_dim, max_pos, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_qknorm_rope_half(sgpt_ctx* c, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos, const float* sin_t,
                                  const float* cos_t, int32_t T, int32_t H, int32_t H_kv, int32_t head_dim, int32_t max_pos,
                                  const float* q_gamma, const float* k_gamma, float eps, void* stream) {
    if (!c || !buf || !pos || !sin_t || !cos_t || T <= 0 || H <= 0 || H_kv <= 0 || head_dim <= 0 || max_pos <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_qknorm_rope_half: bad arguments");
    if (!q_gamma || !k_gamma || !(eps >= 0.f) || !std::isfinite(eps))
        return fail(c, SGPT_ERR_INVALID, "sgpt_qknorm_rope_half: needs q_gamma, k_gamma and eps >= 0");
    if (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16)
        return fail(c, SGPT_ERR_INVALID, "sgpt_qknorm_rope_half: dtype SGPT_F32 | SGPT_BF16 | SGPT_F16");
    if (head_dim != 64 && head_dim != 128) return fail(c, SGPT_ERR_INVALID, "sgpt_qknorm_rope_half: head_dim 64 | 128");
    // sgpt_rope_half's words per thread; a head's square sum is a butterfly over its head_dim / 8 lanes
    const int64_t dq = (int64_t)H * head_dim, dk = (int64_t)H_kv * head_dim;
    if (ld % 4 || k_off % 4 || k_off < dq || ld < k_off + dk || mis(buf, dtype == SGPT_F32 ? 16 : 8) || mis(sin_t, 16) || mis(cos_t, 16) ||
        mis(q_gamma, 16) || mis(k_gamma, 16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_qknorm_rope_half: ld, k_off % 4; k_off >= H * head_dim; ld >= k_off + H_kv * head_dim; "
                                         "buf aligned to four elements, tables and gains to 16 bytes");
    HIPC(c, hipSetDevice(c->device));
    launch_qknorm_rope_half(buf, dtype, ld, k_off, pos, sin_t, cos_t, q_gamma, k_gamma, eps, T, H, H_kv, head_dim, max_pos,
                            dtype == SGPT_F16 ? c->range_flag : nullptr, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_logprob_rows(sgpt_ctx* c, const float* logits, int64_t ld, int32_t V, const int32_t* targets, int32_t n,
                              float* out_logprob, int32_t* out_greedy, void* stream) {
    if (!c || !logits || !targets || !out_logprob || n <= 0 || V <= 0 || ld < V)
        return fail(c, SGPT_ERR_INVALID, "sgpt_logprob_rows: bad arguments (ld >= V)");
    HIPC(c, hipSetDevice(c->device));
    launch_logprob_rows(logits, ld, V, targets, n, out_logprob, out_greedy, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_bench_gemm(sgpt_ctx* c, int32_t dtype, int32_t epi, int32_t out_dtype, int32_t M, int32_t N, int32_t K,
                            int32_t iters, float* ms_out) {
    if (!c || !ms_out || M <= 0 || N <= 0 || K <= 0 || iters <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_bench_gemm: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    if (dtype == SGPT_FP8M) {   // fp8 MFMA kernel: random fp32 operands quantised row-wise to e4m3 codes + power-of-two scales
        if (!gemm_fp8_shape_ok(M, N, K) || (epi != EPI_BIAS_GELU && epi != EPI_BIAS_RESID && epi != EPI_NONE))
            return fail(c, SGPT_ERR_INVALID, "sgpt_bench_gemm(fp8): shapes % 256, epi 1 | 2 | 5");
        float *Af = nullptr, *Wf = nullptr, *sa = nullptr, *sw = nullptr, *bias = nullptr; uint8_t *A8 = nullptr, *W8 = nullptr; void* O = nullptr;
        HIPC(c, hipMalloc((void**)&Af, (size_t)M * K * 4)); HIPC(c, hipMalloc((void**)&Wf, (size_t)N * K * 4));
        HIPC(c, hipMalloc((void**)&A8, (size_t)M * K)); HIPC(c, hipMalloc((void**)&W8, (size_t)N * K));
        HIPC(c, hipMalloc((void**)&sa, (size_t)M * 4)); HIPC(c, hipMalloc((void**)&sw, (size_t)N * 4));
        HIPC(c, hipMalloc((void**)&bias, (size_t)N * 4)); HIPC(c, hipMalloc(&O, (size_t)M * N * 4));
        launch_fill_rand(Af, (long)M * K, 0, 1u, 1.0f, 0); launch_fill_rand(Wf, (long)N * K, 0, 2u, 0.05f, 0);
        launch_fill_rand(bias, N, 0, 3u, 0.1f, 0); launch_fill_rand((float*)O, (long)M * N, 0, 4u, 1.0f, 0);
        launch_fp8_quant_rows(Af, M, K, A8, sa, 0); launch_fp8_quant_rows(Wf, N, K, W8, sw, 0);
        GemmArgs q{};
        q.A = A8; q.lda = K; q.W = W8; q.ldw = K; q.M = M; q.m_valid = M; q.N = N; q.K = K; q.out = O; q.ldo = N; q.bias = bias;
        q.resid = (const float*)O; q.a_scale = sa; q.a_scalar = 1.0f; q.w_scale = sw; q.out_scale = 0.0625f;
        hipEvent_t e0, e1;
        HIPC(c, hipEventCreate(&e0)); HIPC(c, hipEventCreate(&e1));
        for (int i = 0; i < 3; ++i) launch_gemm_fp8(epi, out_dtype, q, 0);
        HIPC(c, hipEventRecord(e0, 0));
        for (int i = 0; i < iters; ++i) launch_gemm_fp8(epi, out_dtype, q, 0);
        HIPC(c, hipEventRecord(e1, 0));
        HIPC(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms / iters;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        (void)hipFree(Af); (void)hipFree(Wf); (void)hipFree(A8); (void)hipFree(W8); (void)hipFree(sa); (void)hipFree(sw); (void)hipFree(bias); (void)hipFree(O);
        HIPC(c, hipGetLastError());
        return SGPT_OK;
    }
    const size_t esz = dtype == SGPT_F32 ? 4 : 2, osz = out_dtype == SGPT_F32 ? 4 : 2;
    void *A = nullptr, *W = nullptr, *O = nullptr; float* bias = nullptr;
    HIPC(c, hipMalloc(&A, (size_t)M * K * esz));
    HIPC(c, hipMalloc(&W, (size_t)N * K * esz));
    HIPC(c, hipMalloc(&O, (size_t)M * N * (epi == EPI_BIAS_RESID ? 4 : osz) + 4096));
    HIPC(c, hipMalloc((void**)&bias, (size_t)N * 4));
    launch_fill_rand(A, (long)M * K, dtype, 1u, 1.0f, 0);
    launch_fill_rand(W, (long)N * K, dtype, 2u, 0.05f, 0);
    launch_fill_rand(bias, N, 0, 3u, 0.1f, 0);
    launch_fill_rand(O, (long)M * N, epi == EPI_BIAS_RESID ? 0 : out_dtype, 4u, 1.0f, 0);
    GemmArgs g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.m_valid = M; g.N = N; g.K = K; g.out = O;
    g.ldo = epi == EPI_VT ? M : N; g.bias = bias; g.resid = epi == EPI_BIAS_RESID ? (const float*)O : nullptr;
    hipEvent_t e0, e1;
    HIPC(c, hipEventCreate(&e0)); HIPC(c, hipEventCreate(&e1));
    long long* dbg = nullptr;
    if (exp_env("SGPT_GEMM_DBG")) { HIPC(c, hipMalloc((void**)&dbg, 128 * 8)); HIPC(c, hipMemset(dbg, 0, 128 * 8)); g.dbg = dbg; }
    for (int i = 0; i < 3; ++i) launch_gemm(dtype, epi, out_dtype, g, 0);
    HIPC(c, hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) launch_gemm(dtype, epi, out_dtype, g, 0);
    HIPC(c, hipEventRecord(e1, 0));
    HIPC(c, hipEventSynchronize(e1));
    float ms = 0;
    HIPC(c, hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    if (dbg) {
        long long h[128];
        HIPC(c, hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
        for (int tl = 0; tl < 4; ++tl) {
            const long long* r = h + tl * 8;
            const long long* ks = h + 64 + tl * 16;
            fprintf(stderr, "tile %d: k-step starts (rel. to step 0):", tl);
            for (int q = 1; q < 12; ++q) fprintf(stderr, " %lld", ks[q] - ks[0]);
            fprintf(stderr, " | kloop_end %lld  dma_wait +%lld  barrier +%lld  epilogue +%lld | next tile step0 at %lld\n",
                    r[0] - ks[0], r[1] - r[0], r[2] - r[1], r[3] - r[2], h[64 + (tl + 1) * 16] - ks[0]);
        }
        (void)hipFree(dbg);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(A); (void)hipFree(W); (void)hipFree(O); (void)hipFree(bias);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

}  // extern "C"
