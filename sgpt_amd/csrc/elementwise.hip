// The HBM-bound kernels around the GEMMs and the attention, and their launchers:
//   row normalisation (one wave per row, rowln.h): LayerNorm to fp32 / 16 bit, with write-back, as [hi | lo | hi], as fp8 codes; RMSNorm, to 16 bit / fp32 and as fp8 codes;
//     the fused final norm + pooling + L2 normalise (one workgroup per sequence, LDS for its cross-wave combine only);
//   other row kernels: embedding gather-add, stand-alone pooling, L2 normalise, pairwise scores, row gather, log-prob of a logits row,
//     crest factor;
//   SwiGLU as fp8 codes under one scale per row (one workgroup per row);
//   element maps: SwiGLU, the three rotary embeddings (GPT-J pairs, half-split, half-split behind a per-head RMSNorm);
//   formats: fp8 row quantise (from fp32 and from bf16 rows) / de-quantise, split-precision rows and weights, sign bits, fp32 -> 16 bit, BLOOM's QKV re-ordering;
//   small tools: abs-max (fp32, 16 bit), mean over axis 0, fill, pseudo-random fill.
#include <type_traits>

#include "common.h"
#include "rowln.h"

namespace {

// an index from outside clamped into a table of n rows: a C-ABI caller's bad id / position / target reads a wrong row, never out of
// bounds (the Python host validates and raises before the call, model.py::SGPTModel.pack)
__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- wte[ids] + wpe[pos]  (HF:gpt_neo/modeling_gpt_neo.py:444,462-463) ----
__global__ __launch_bounds__(256) void embed_kernel(const int* __restrict__ ids, const int* __restrict__ pos,
                                                    const float* __restrict__ wte, const float* __restrict__ wpe,
                                                    float* __restrict__ x, int T, int d, int vocab, int max_pos) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int lane = threadIdx.x & 63;
    const float4* a = reinterpret_cast<const float4*>(wte + (long)clamp_index(ids[row], vocab) * d);
    float4* o = reinterpret_cast<float4*>(x + (long)row * d);
    if (wpe == nullptr) {  // GPT-J: no learned position embedding (HF:gptj:484)
        for (int c = lane; c < d / 4; c += 64) o[c] = a[c];
        return;
    }
    const float4* b = reinterpret_cast<const float4*>(wpe + (long)clamp_index(pos[row], max_pos) * d);
    for (int c = lane; c < d / 4; c += 64) {
        const float4 u = a[c], v = b[c];
        o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
}

// out_mul: power-of-two range shift of an f16 output (the consuming GEMMs multiply their accumulators by 1 / out_mul);
// 1 for every other format and for models without shifts (v * 1 == v: the default path keeps its bits)
template <typename OutT, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, OutT* __restrict__ out, int T,
                                                        int d, float eps, float out_mul) {
    rownorm_row<NV>(x, T, d, RowLayerNorm<>(g, b, eps), RowStore<OutT, true, false>{out, out_mul, nullptr});
}

// Post-LayerNorm blocks (SGPT_ARCH_BERT, HF:bert/modeling_bert.py BertSelfOutput / BertOutput: `LayerNorm(dense(h) + input)`): the
// normalised row IS the next residual stream, so it goes back to x in fp32, in place, and to the 16-bit operand buffer the next
// projection reads.  f16: every rounded value passes the range tracker (no load-time bound on gamma / beta is relied upon for this family).
template <typename OutT, int NV>
__global__ __launch_bounds__(256) void layernorm_writeback_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                                  const float* __restrict__ b, OutT* __restrict__ out16, int T,
                                                                  int d, float eps, int* __restrict__ range_flag) {
    rownorm_row<NV>(x, T, d, RowLayerNorm<>(g, b, eps), RowStoreWriteback<OutT>{x, out16, range_flag});
}

// RMSNorm of the Llama family (rowln.h: rms_normalize), rounded once to OutT (fp32: stored as it is, out may alias x).  f16: every
// rounded value passes the range tracker (no load-time bound on the gain is relied upon).
template <typename OutT, int NV>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ g, OutT* __restrict__ out,
                                                      int T, int d, float eps, int* __restrict__ range_flag) {
    rownorm_row<NV>(x, T, d, RowRMSNorm<>(g, nullptr, eps), RowStore<OutT, false, true>{out, 1.0f, range_flag});
}

// SwiGLU of the Llama family (HF:llama/modeling_llama.py LlamaMLP: down(silu(gate(x)) * up(x))): gu [T][2 ffn] holds the gate
// columns, then the up columns, of ONE fc1 launch; h[t][j] = silu(gu[t][j]) * gu[t][ffn + j] with silu(u) = u / (1 + exp(-u)) in
// fp32 (expf and the IEEE divide: the kernel moves 3 values per 4 flops + one exp, it waits on memory), rounded once to T.  One
// thread per 16 bytes of h: 8 (16-bit) or 4 (fp32) consecutive columns, two 16-byte loads.  f16: the product passes the range tracker.
__device__ __forceinline__ float silu_mul(float u, float v) { return u / (1.0f + expf(-u)) * v; }
template <typename T>
__global__ __launch_bounds__(256) void swiglu_kernel(const T* __restrict__ gu, T* __restrict__ h, long n_vec, int ffn,
                                                     int* __restrict__ range_flag) {
    constexpr int VW = 16 / sizeof(T);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    RangeTrack<T> range;
    if (idx < n_vec) {
        const int vpr = ffn / VW;                        // vectors per row
        const long t = idx / vpr;
        const int j = (int)(idx - t * vpr) * VW;
        const T* grow = gu + t * 2 * (long)ffn + j;
        const uint4 a = *reinterpret_cast<const uint4*>(grow), b = *reinterpret_cast<const uint4*>(grow + ffn);
        uint4 o;
        if constexpr (sizeof(T) == 4) {
            o.x = __float_as_uint(silu_mul(__uint_as_float(a.x), __uint_as_float(b.x)));
            o.y = __float_as_uint(silu_mul(__uint_as_float(a.y), __uint_as_float(b.y)));
            o.z = __float_as_uint(silu_mul(__uint_as_float(a.z), __uint_as_float(b.z)));
            o.w = __float_as_uint(silu_mul(__uint_as_float(a.w), __uint_as_float(b.w)));
        } else {
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
            uint32_t ow[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float p0 = silu_mul(Half<T>::lo(aw[w]), Half<T>::lo(bw[w])), p1 = silu_mul(Half<T>::hi(aw[w]), Half<T>::hi(bw[w]));
                range.note(p0, p1);
                ow[w] = Half<T>::pack2(p0, p1);
            }
            o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
        *reinterpret_cast<uint4*>(h + t * (long)ffn + j) = o;
    }
    if constexpr (sizeof(T) != 4) range.finish(range_flag);
}

// LayerNorm for the split-precision Q / K projection (sgpt_model_desc.qk_split): the normalised row a is written as
// [hi | lo | hi] with hi = round16(a), lo = round16(a - hi) -- three K blocks of a [T, 3d] operand.  Against weights packed as
// [W_hi | W_hi | W_lo] (pack_split_rows_kernel) one ordinary GEMM over K' = 3d computes a_hi.W_hi + a_lo.W_hi + a_hi.W_lo:
// the product of the two operands to ~2^-22 instead of 2^-11 each, on the 16-bit MFMA, with no kernel of its own.  The V
// projection (and GPT-J's MLP) read the first block alone (lda = 3d, K = d): the plain 16-bit LayerNorm output.
template <typename OutT, int NV>
__global__ __launch_bounds__(256) void layernorm_split_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                              const float* __restrict__ b, uint16_t* __restrict__ out, int T,
                                                              int d, float eps, float out_mul) {
    rownorm_row<NV>(x, T, d, RowLayerNorm<>(g, b, eps), RowStoreSplit<OutT>{out, out_mul});
}

// weights of the split-precision projection: src fp32 [rows, cols] -> dst 16-bit [rows, 3 * cols] = [W_hi | W_hi | W_lo]
template <typename H>
__global__ __launch_bounds__(256) void pack_split_rows_kernel(const float* __restrict__ src, long rows, long cols,
                                                              uint16_t* __restrict__ dst) {
    const long n = rows * cols, stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const long r = e / cols, c = e - r * cols;
        const float w = src[e];
        const uint32_t hi = Half<H>::pack2(w, 0.0f);
        const uint16_t lo = f32_to_h<H>(w - Half<H>::lo(hi));
        uint16_t* o = dst + r * 3 * cols + c;
        o[0] = (uint16_t)(hi & 0xffffu); o[cols] = (uint16_t)(hi & 0xffffu); o[2 * cols] = lo;
    }
}

// LayerNorm whose output feeds an fp8-MFMA GEMM (gemm256q.hip): the normalised row is quantised to OCP e4m3fn codes under
// ONE power-of-two scale per row (fp8_pow2_scale), which factors out of the GEMM's k-sum and is applied to its accumulators.
template <int NV>
__global__ __launch_bounds__(256) void layernorm_q8_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ b, uint8_t* __restrict__ q,
                                                           float* __restrict__ scale, int T, int d, float eps) {
    rownorm_row<NV>(x, T, d, RowLayerNorm<>(g, b, eps), RowStoreFp8{q, scale});
}

// RMSNorm whose output feeds an fp8-MFMA GEMM (fp8 projections of the Llama family): rmsnorm_kernel's arithmetic, layernorm_q8_kernel's sink
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_q8_kernel(const float* __restrict__ x, const float* __restrict__ g, uint8_t* __restrict__ q,
                                                         float* __restrict__ scale, int T, int d, float eps) {
    rownorm_row<NV>(x, T, d, RowRMSNorm<>(g, nullptr, eps), RowStoreFp8{q, scale});
}

// SwiGLU whose output feeds an fp8-MFMA GEMM (the down-projection of a converted Llama model): h = silu_mul(gate, up) in fp32 from the
// 16-bit gu [T][2 ffn] -- the expression of swiglu_kernel, NOT rounded to 16 bits -- then e4m3fn codes of h / scale under ONE scale per
// row, fp8_pow2_scale(max|h_row|), as RowStoreFp8 writes them.  A row is up to 28 672 columns (Qwen2.5-72B; 14 336 at Mistral-7B): more
// than a wave holds, so one 256-thread workgroup per row, 16 columns per thread and step (four 16-byte loads, one 16-byte store), the row
// maximum through the wave butterfly and four LDS words.
// NIT > 0: the row's h stays in registers between the two passes (NIT steps of 16 fp32 values per thread, ffn <= NIT * 4096).  Chosen
// over a second read of the row from the compiler's report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch and no spill
// in any variant, 38 / 58 / 80 / 143 VGPRs at NIT = 1 / 2 / 4 / 7 (14 336 columns run NIT = 4), and the second pass would compute
// expf and the IEEE divide of every element again -- the kernel moves 5 bytes per element and is near the VALU's rate already.
// NIT == 0 (ffn > 28 672): any width, the second pass reads the row again (at 4 bytes per column it sits in L2) and recomputes h.
template <typename T, int NIT>
__global__ __launch_bounds__(256) void swiglu_q8_kernel(const T* __restrict__ gu, uint8_t* __restrict__ q, float* __restrict__ scale,
                                                        int ffn) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const int t = threadIdx.x, nchunk = ffn / 16;
    const T* grow = gu + row * 2 * (long)ffn;
    uint8_t* qrow = q + row * (long)ffn;
    // h of columns 16 c .. 16 c + 15, and the largest |h| among them folded into amax
    auto chunk = [&](int c, float (&h)[16], float& amax) {
        const T* gp = grow + (long)c * 16;
        const uint4 a0 = *reinterpret_cast<const uint4*>(gp), a1 = *reinterpret_cast<const uint4*>(gp + 8);
        const uint4 b0 = *reinterpret_cast<const uint4*>(gp + ffn), b1 = *reinterpret_cast<const uint4*>(gp + ffn + 8);
        const uint32_t aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            h[2 * w] = silu_mul(Half<T>::lo(aw[w]), Half<T>::lo(bw[w]));
            h[2 * w + 1] = silu_mul(Half<T>::hi(aw[w]), Half<T>::hi(bw[w]));
            amax = fmaxf(amax, fmaxf(fabsf(h[2 * w]), fabsf(h[2 * w + 1])));
        }
    };
    auto store = [&](int c, const float (&h)[16], float inv) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int p = __builtin_amdgcn_cvt_pk_fp8_f32(h[4 * u] * inv, h[4 * u + 1] * inv, 0, false);
            p = __builtin_amdgcn_cvt_pk_fp8_f32(h[4 * u + 2] * inv, h[4 * u + 3] * inv, p, true);
            w[u] = (uint32_t)p;
        }
        *reinterpret_cast<uint4*>(qrow + (long)c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    };
    float amax = 0.f;
    float hr[NIT > 0 ? NIT : 1][16];
    if constexpr (NIT > 0) {
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (i * 256 + t < nchunk) chunk(i * 256 + t, hr[i], amax);
    } else {
        for (int c = t; c < nchunk; c += 256) chunk(c, hr[0], amax);
    }
    amax = wave_max(amax);
    if ((t & 63) == 0) red[t >> 6] = amax;
    __syncthreads();
    const float sc = fp8_pow2_scale(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
    if (t == 0) scale[row] = sc;
    const float inv = 1.0f / sc;                                      // exact: power of two
    if constexpr (NIT > 0) {
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (i * 256 + t < nchunk) store(i * 256 + t, hr[i], inv);
    } else {
        for (int c = t; c < nchunk; c += 256) { float unused = 0.f; chunk(c, hr[0], unused); store(c, hr[0], inv); }
    }
}

// ---- ln_f + pooling + optional L2 normalise, one workgroup (4 waves) per sequence ----
// weightedmean: sum_t (P+t+1) * h_t / clamp(sum_t (P+t+1), 1e-9), P = pad_left
//   (Pooling.py:99-125; beir_dense_retriever.py:258-270; weights follow the PADDED index)
// mean: Pooling.py:117-125 / beir_dense_retriever.py:238-242;  lasttoken: :271-282 (index len-1)
// learntmean (mode 3): w_t = position_weights[P+t], clamp 1e-9 (WeightedMeanPooling.py:21-39)
// Norm: RowLayerNorm<true>, or RowRMSNorm<true> for the final norm of the Llama family (g alone; b is not read).
// pool_lo (or null = zeros): the first pooled row of every sequence, clamped into [0, len] -- weightedmean / mean / learntmean run over
//   rows [lo, len) (the tokens behind an instruction prompt); the weight of row t stays P + t + 1, the PADDED position index, and does not
//   restart behind the prompt (GritLM, Pooling.py with include_prompt = false).  lasttoken is row len - 1 whatever lo is.  An empty range
//   leaves a zero numerator over the clamped denominator: a zero row.
template <int NV, typename Norm>
__global__ __launch_bounds__(256) void lnf_pool_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                       const float* __restrict__ b, const int* __restrict__ seq_off,
                                                       const int* __restrict__ seq_len,
                                                       const int* __restrict__ pad_left, const int* __restrict__ pool_lo, int d, float eps,
                                                       int apply_ln, int mode, int normalize,
                                                       const float* __restrict__ pw, int pw_n, float* __restrict__ out,
                                                       int* __restrict__ nonfinite_flag) {
    extern __shared__ __attribute__((aligned(16))) float sm[];  // [4][d] + 8
    const int sq = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s0 = seq_off[sq], len = seq_len[sq], P = pad_left ? pad_left[sq] : 0;
    const Norm norm(g, b, eps);

    float4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    float den = 0.f;
    int lo = pool_lo ? pool_lo[sq] : 0;
    lo = lo < 0 ? 0 : (lo > len ? len : lo);
    const int t_lo = mode == 2 ? (len > 0 ? len - 1 : 0) : lo;
    const int t_hi = mode == 4 ? (len > 0 ? 1 : 0) : len;        // cls (mode 4): the first row alone (Pooling.py:103-105)
    // A wave's rows t = t_lo + wave, t_lo + wave + 4, ... are accumulated in that order; their LOADS go out LPB rows at a time (round 6: one
    // sequence of 30 tokens is eight dependent load -> normalise -> accumulate round trips per wave otherwise -- 14 us of a
    // 0.43 ms single-query encode; a bulk call has thousands of workgroups to hide the latency behind).  Same sums, same bits.
    constexpr int LPB = NV <= 4 ? 4 : 2;
    for (int t = t_lo + wave; t < t_hi; t += 4 * LPB) {
        RowLN<NV> r[LPB];
#pragma unroll
        for (int u = 0; u < LPB; ++u)
            if (t + 4 * u < t_hi) r[u].load(x + (long)(s0 + t + 4 * u) * d, d, lane);
#pragma unroll
        for (int u = 0; u < LPB; ++u) {
            const int tt = t + 4 * u;
            if (tt >= t_hi) break;
            if (apply_ln) norm(r[u], d, lane);
            // mode 3 (learntmean): trained per-position weights, indexed like the padded position
            // (WeightedMeanPooling.py:21-39; useb_dense_retriever.py:253-270)
            const float w = mode == 0 ? (float)(P + tt + 1) : (mode == 3 ? pw[P + tt < pw_n ? P + tt : pw_n - 1] : 1.0f);   // index clamped: no OOB read
            den += w;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                acc[i].x += w * r[u].v[i].x; acc[i].y += w * r[u].v[i].y;
                acc[i].z += w * r[u].v[i].z; acc[i].w += w * r[u].v[i].w;
            }
        }
    }
    RowLN<NV>::for_cols(d, lane, [&](int i, int c) { *reinterpret_cast<float4*>(sm + wave * d + c) = acc[i]; });
    float* red = sm + 4 * d;
    if (lane == 0) red[wave] = den;
    __syncthreads();
    float dsum = (red[0] + red[1]) + (red[2] + red[3]);
    if (mode != 2 && mode != 4) dsum = fmaxf(dsum, 1e-9f);  // Pooling.py:122
    else dsum = 1.0f;
    float ss = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) {
        const float e = ((sm[c] + sm[d + c]) + (sm[2 * d + c] + sm[3 * d + c])) / dsum;
        sm[c] = e;
        ss += e * e;
    }
    // f16 models: a NaN / inf that reached the pooled embedding (an under-shifted LayerNorm output overflowing to inf gives
    // inf - inf in the next GEMM, and the per-launch range trackers' fmaxf drops NaN) raises the model's guard word: never silent
    if (nonfinite_flag != nullptr && !(ss < INFINITY)) atomicOr(nonfinite_flag, 1);
    if (normalize) {  // F.normalize(p=2, dim=1), SentenceTransformer.py:248-249
        ss = wave_sum(ss);
        __syncthreads();
        if (lane == 0) red[4 + wave] = ss;
        __syncthreads();
        const float nrm = fmaxf(sqrtf((red[4] + red[5]) + (red[6] + red[7])), 1e-12f);
        for (int c = threadIdx.x; c < d; c += 256) out[(long)sq * d + c] = sm[c] / nrm;
    } else {
        for (int c = threadIdx.x; c < d; c += 256) out[(long)sq * d + c] = sm[c];
    }
}

// ---- stand-alone pooling over [B,S,d] hidden states + {0,1} mask (any padding side) ----
template <typename T>
__device__ __forceinline__ float4 load4(const T* p);
template <> __device__ __forceinline__ float4 load4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 load4<bf16_t>(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}

template <> __device__ __forceinline__ float4 load4<f16_t>(const f16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(Half<f16_t>::lo(u.x), Half<f16_t>::hi(u.x), Half<f16_t>::lo(u.y), Half<f16_t>::hi(u.y));
}

template <typename T>
__global__ __launch_bounds__(256) void pool_kernel(const T* __restrict__ h, const int* __restrict__ mask, int S, int d,
                                                   int mode, const float* __restrict__ pw, float* __restrict__ out) {
    const int bq = blockIdx.x;
    const int c = (blockIdx.y * 256 + threadIdx.x) * 4;
    if (c >= d) return;
    const T* hb = h + (long)bq * S * d + c;
    const int* mb = mask + (long)bq * S;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 4) {            // cls: `token_embeddings[:, 0]`, whatever the mask says (Pooling.py:103-105)
        acc = load4<T>(hb);
    } else if (mode == 2) {
        int last = 0;
        for (int t = 0; t < S; ++t) if (mb[t] != 0) last = t;
        acc = load4<T>(hb + (long)last * d);
    } else {
        float den = 0.f;
#pragma unroll 4
        for (int t = 0; t < S; ++t) {
            const float w = mb[t] != 0 ? (mode == 0 ? (float)(t + 1) : (mode == 3 ? pw[t] : 1.0f)) : 0.0f;
            const float4 v = load4<T>(hb + (long)t * d);
            den += w;
            acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
        }
        den = fmaxf(den, 1e-9f);
        acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den;
    }
    *reinterpret_cast<float4*>(out + (long)bq * d + c) = acc;
}

// ---- x / max(||x||, 1e-12) per row; fp32 or bf16 output ----
template <typename OutT>
__global__ __launch_bounds__(256) void l2norm_kernel(const float* __restrict__ in, long n, int d,
                                                     OutT* __restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float* xr = in + row * d;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) { const float v = xr[c]; s += v * v; }
    const float nrm = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    for (int c = lane; c < d; c += 64) {
        const float v = xr[c] / nrm;
        if constexpr (sizeof(OutT) == 4) reinterpret_cast<float*>(out)[row * d + c] = v;
        else reinterpret_cast<uint16_t*>(out)[row * d + c] = f32_to_h<OutT>(v);
    }
}

// ---- row-wise scores of two equally shaped matrices: util.pairwise_dot_score / pairwise_cos_sim (util.py:66-91) ----
// out[i] = sum_j a[i][j] b[i][j]            (COS = false: `(a * b).sum(dim=-1)`)
//        = sum_j (a[i][j] / max(|a[i]|, 1e-12)) (b[i][j] / max(|b[i]|, 1e-12))   (COS = true: both sides through
//          normalize_embeddings first, then the same product sum -- the reference's order of operations, not dot / (|a| |b|)).
// One wave per row pair, scalar loads strided by the wave (any d), wavefront butterflies for the three sums.
template <bool COS>
__global__ __launch_bounds__(256) void pairwise_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, int d,
                                                       float* __restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float* ar = a + row * d;
    const float* br = b + row * d;
    float na = 1.f, nb = 1.f;
    if constexpr (COS) {
        float sa = 0.f, sb = 0.f;
        for (int c = lane; c < d; c += 64) { const float x = ar[c], y = br[c]; sa += x * x; sb += y * y; }
        na = fmaxf(sqrtf(wave_sum(sa)), 1e-12f);
        nb = fmaxf(sqrtf(wave_sum(sb)), 1e-12f);
    }
    float s = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float x = COS ? ar[c] / na : ar[c], y = COS ? br[c] / nb : br[c];
        s += x * y;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

// ---- GPT-J rotary position embedding (HF:gptj/modeling_gptj.py:57-67,190-210) ----
// For every token, head and pair i < rotary_dim/2 of the head's leading dims:
//   (x[2i], x[2i+1]) <- (x[2i] cos - x[2i+1] sin, x[2i+1] cos + x[2i] sin),  angle = pos * inv_freq[i]
// applied in place to q (column 0) and k (column k_off) of the projection buffer.  One thread per pair.
template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(T* __restrict__ buf, long ld, long k_off, const int* __restrict__ pos,
                                                   const float* __restrict__ sin_t, const float* __restrict__ cos_t,
                                                   int Tn, int H, int dh, int half, int max_pos) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_tok = (long)H * half;
    if (idx >= (long)Tn * per_tok) return;
    const int tkn = (int)(idx / per_tok);
    const int rem = (int)(idx - (long)tkn * per_tok);
    const int h = rem / half, i = rem - h * half;
    const int ps = clamp_index(pos[tkn], max_pos);
    const float sn = sin_t[(long)ps * half + i], cs = cos_t[(long)ps * half + i];
    T* q = buf + (long)tkn * ld + (long)h * dh + 2 * i;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        T* ptr = q + which * k_off;
        if constexpr (sizeof(T) == 4) {
            const float2 v = *reinterpret_cast<const float2*>(ptr);
            *reinterpret_cast<float2*>(ptr) = make_float2(v.x * cs - v.y * sn, v.y * cs + v.x * sn);
        } else {
            const uint32_t u = *reinterpret_cast<const uint32_t*>(ptr);
            const float x0 = Half<T>::lo(u), x1 = Half<T>::hi(u);   // f16: |rotated| <= sqrt(2) * RANGE_LIMIT < 65504
            *reinterpret_cast<uint32_t*>(ptr) = Half<T>::pack2(x0 * cs - x1 * sn, x1 * cs + x0 * sn);
        }
    }
}

// ---- half-split rotary position embedding of the Llama family (HF:llama/modeling_llama.py rotate_half / apply_rotary_pos_emb) ----
// For every token, head and i < dh/2:  (x[i], x[i + dh/2]) <- (x[i] cos - x[i + dh/2] sin, x[i + dh/2] cos + x[i] sin), angle =
// pos * inv_freq[i] -- the two halves of a head pair up, not GPT-J's neighbours.  In place on the H query heads at column 0 and the
// H_kv key heads at column k_off of [T][ld].  One thread per four consecutive i of one head: two 16- / 8-byte words of the row and
// one float4 of each table; fp32 arithmetic, one rounding.  f16: |rotated| <= sqrt(2) * RANGE_LIMIT < 65504, as rope_kernel.
// the thread's two groups of four consecutive T at lo / hi (one 16- / 8-byte word each) -> fp32, and back rounded once
template <typename T>
__device__ __forceinline__ void load_2x4(const T* lo, const T* hi, float (&a)[4], float (&b)[4]) {
    if constexpr (sizeof(T) == 4) {
        const float4 va = *reinterpret_cast<const float4*>(lo), vb = *reinterpret_cast<const float4*>(hi);
        a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w; b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
    } else {
        const uint2 ua = *reinterpret_cast<const uint2*>(lo), ub = *reinterpret_cast<const uint2*>(hi);
        a[0] = Half<T>::lo(ua.x); a[1] = Half<T>::hi(ua.x); a[2] = Half<T>::lo(ua.y); a[3] = Half<T>::hi(ua.y);
        b[0] = Half<T>::lo(ub.x); b[1] = Half<T>::hi(ub.x); b[2] = Half<T>::lo(ub.y); b[3] = Half<T>::hi(ub.y);
    }
}
template <typename T>
__device__ __forceinline__ void store_2x4(T* lo, T* hi, const float (&a)[4], const float (&b)[4]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(lo) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(hi) = make_float4(b[0], b[1], b[2], b[3]);
    } else {
        *reinterpret_cast<uint2*>(lo) = make_uint2(Half<T>::pack2(a[0], a[1]), Half<T>::pack2(a[2], a[3]));
        *reinterpret_cast<uint2*>(hi) = make_uint2(Half<T>::pack2(b[0], b[1]), Half<T>::pack2(b[2], b[3]));
    }
}
// (a, b) <- (a cos - b sin, b cos + a sin) by the table row of position ps (clamped into the tables), columns i .. i + 3 of `half`
__device__ __forceinline__ void rotate_half_2x4(float (&a)[4], float (&b)[4], const float* __restrict__ sin_t, const float* __restrict__ cos_t,
                                                int ps, int max_pos, int half, int i) {
    const long at = (long)clamp_index(ps, max_pos) * half + i;
    const float4 sn4 = *reinterpret_cast<const float4*>(sin_t + at), cs4 = *reinterpret_cast<const float4*>(cos_t + at);
    const float sn[4] = {sn4.x, sn4.y, sn4.z, sn4.w}, cs[4] = {cs4.x, cs4.y, cs4.z, cs4.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float ra = a[u] * cs[u] - b[u] * sn[u], rb = b[u] * cs[u] + a[u] * sn[u];
        a[u] = ra; b[u] = rb;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void rope_half_kernel(T* __restrict__ buf, long ld, long k_off, const int* __restrict__ pos,
                                                        const float* __restrict__ sin_t, const float* __restrict__ cos_t,
                                                        int Tn, int H, int H_kv, int dh, int max_pos) {
    const int half = dh / 2, qpt = half / 4;             // quads per head
    const long per_tok = (long)(H + H_kv) * qpt;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Tn * per_tok) return;
    const int tkn = (int)(idx / per_tok);
    const int rem = (int)(idx - (long)tkn * per_tok);
    const int h = rem / qpt, i = (rem - h * qpt) * 4;
    // heads [0, H): q at column h * dh; heads [H, H + H_kv): k at column k_off + (h - H) * dh
    T* lo = buf + (long)tkn * ld + (h < H ? (long)h * dh : k_off + (long)(h - H) * dh) + i;
    T* hi = lo + half;
    float a[4], b[4];
    load_2x4(lo, hi, a, b);
    rotate_half_2x4(a, b, sin_t, cos_t, pos[tkn], max_pos, half, i);
    store_2x4(lo, hi, a, b);
}

// ---- per-head RMSNorm of q and k fused with the half-split rotary (HF:qwen3/modeling_qwen3.py Qwen3Attention: q_norm / k_norm over
// head_dim, then apply_rotary_pos_emb) ----
// For every token and head: n = x * rsqrt(mean_over_head_dim(x^2) + eps) * g (g = q_g for the H query heads, k_g for the H_kv key heads,
// fp32 [DH] shared by the heads; HF's order: x * rstd first, then * g), then rope_half_kernel's rotation of n, rounded once.  The
// thread-to-element map is rope_half_kernel's -- four consecutive i and their partners i + DH/2 per thread, 16- / 8-byte words -- so a
// head is DH / 8 consecutive lanes (8 | 16: aligned inside a wave, 256 % (DH / 8) == 0) and its square sum a butterfly over those
// lanes.  Threads past the last head carry zeros through the butterfly and store nothing.  f16: the rounded values pass the range
// tracker (a gain is not bounded at load time).
template <typename T, int DH>
__global__ __launch_bounds__(256) void qknorm_rope_half_kernel(T* __restrict__ buf, long ld, long k_off, const int* __restrict__ pos,
                                                               const float* __restrict__ sin_t, const float* __restrict__ cos_t,
                                                               const float* __restrict__ q_g, const float* __restrict__ k_g, float eps,
                                                               int Tn, int H, int H_kv, int max_pos, int* __restrict__ range_flag) {
    constexpr int half = DH / 2, qpt = half / 4;        // quads (= lanes) per head
    const long per_tok = (long)(H + H_kv) * qpt;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < (long)Tn * per_tok;         // (whole heads: the count is a multiple of qpt)
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    T *lo = nullptr, *hi = nullptr;
    int tkn = 0, h = 0, i = 0;
    if (live) {
        tkn = (int)(idx / per_tok);
        const int rem = (int)(idx - (long)tkn * per_tok);
        h = rem / qpt; i = (rem - h * qpt) * 4;
        // heads [0, H): q at column h * DH; heads [H, H + H_kv): k at column k_off + (h - H) * DH
        lo = buf + (long)tkn * ld + (h < H ? (long)h * DH : k_off + (long)(h - H) * DH) + i;
        hi = lo + half;
        load_2x4(lo, hi, a, b);
    }
    float ss = (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]) + ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]));
#pragma unroll
    for (int o = qpt / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    RangeTrack<T> range;
    if (live) {
        const float rstd = 1.0f / sqrtf(ss / (float)DH + eps);
        const float* g = h < H ? q_g : k_g;
        const float4 ga = *reinterpret_cast<const float4*>(g + i), gb = *reinterpret_cast<const float4*>(g + half + i);
        const float gav[4] = {ga.x, ga.y, ga.z, ga.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = a[u] * rstd * gav[u]; b[u] = b[u] * rstd * gbv[u]; }
        rotate_half_2x4(a, b, sin_t, cos_t, pos[tkn], max_pos, half, i);
        if constexpr (sizeof(T) != 4) { range.note(a[0], a[1]); range.note(a[2], a[3]); range.note(b[0], b[1]); range.note(b[2], b[3]); }
        store_2x4(lo, hi, a, b);
    }
    if constexpr (sizeof(T) != 4) range.finish(range_flag);
}

// BLOOM stores the QKV projection fused and head-interleaved: row h*3*dh + which*dh + c (HF:bloom:214).
// Re-order to row which*d + h*dh + c so the Q/K and V projections are the same contiguous blocks as for GPT-Neo.
__global__ __launch_bounds__(256) void qkv_deinterleave_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               int H, int dh, long row_len) {
    const int drow = blockIdx.x;                       // destination row in [0, 3*H*dh)
    const int d = H * dh;
    const int which = drow / d, rem = drow - which * d, h = rem / dh, c = rem - h * dh;
    const long srow = (long)h * 3 * dh + (long)which * dh + c;
    for (long i = threadIdx.x; i < row_len; i += 256) dst[(long)drow * row_len + i] = src[srow * row_len + i];
}

// ---- fp8 (OCP e4m3fn) weight storage with one power-of-two fp32 scale per output channel (row) ----
// scale[r] = smallest 2^k with amax_r / 2^k <= 448; code = RNE(w / scale) in e4m3fn.  Dividing by a power of
// two is exact, and code * scale is exactly representable in bf16 (4 significant bits), so the bf16 MFMA path
// runs on precisely the de-quantised weights the oracle uses in fp32.  Software encode/decode: load-time and
// once-per-layer work, and independent of any hardware conversion / saturation mode.
__device__ __forceinline__ uint32_t e4m3fn_encode(float x) {
    const uint32_t sign = (__float_as_uint(x) >> 24) & 0x80u;
    const float a = fabsf(x);
    if (!(a < 464.f)) return sign | (a != a ? 0x7fu : 0x7eu);        // saturate to 448; NaN stays NaN
    if (a < 0.015625f) return sign | (uint32_t)rintf(a * 512.f);      // subnormals: multiples of 2^-9 (8 -> min normal)
    uint32_t u = __float_as_uint(a);
    u += 0x7ffffu + ((u >> 20) & 1u);                                 // RNE to 3 mantissa bits
    u >>= 20;
    const uint32_t code = u - (120u << 3);                            // re-bias 127 -> 7
    return sign | (code > 0x7eu ? 0x7eu : code);
}
__device__ __forceinline__ float e4m3fn_decode(uint32_t c) {
    const uint32_t e = (c >> 3) & 15u, m = c & 7u;
    const float a = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
    if ((c & 0x7fu) == 0x7fu) return __uint_as_float(0x7fc00000u);   // the NaN codes 0x7f / 0xff (the encoder emits them for NaN input only)
    return (c & 0x80u) ? -a : a;
}

// one wave per row: amax -> scale, then encode
__global__ __launch_bounds__(256) void fp8_quant_rows_kernel(const float* __restrict__ w, long rows, long cols,
                                                             uint8_t* __restrict__ q, float* __restrict__ scale) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* wr = w + row * cols;
    float amax = 0.f;
    for (long c = lane; c < cols; c += 64) amax = fmaxf(amax, fabsf(wr[c]));
    const float sc = fp8_pow2_scale(wave_max(amax));
    if (lane == 0) scale[row] = sc;
    const float inv = 1.0f / sc;                                      // exact: power of two
    for (long c = lane; c < cols; c += 64) q[row * cols + c] = (uint8_t)e4m3fn_encode(wr[c] * inv);
}

// the same from bf16 rows (sgpt_model_set_projections: the loader has dropped the fp32 source): same scale rule, same RNE codes -- the
// codes of fp8_quant_rows_kernel on the bf16 values widened to fp32.  cols % 2 == 0: two columns per lane and step.
__global__ __launch_bounds__(256) void fp8_quant_rows_bf16_kernel(const uint32_t* __restrict__ w2, long rows, long cols,
                                                                  uint8_t* __restrict__ q, float* __restrict__ scale) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long c2 = cols / 2;
    const uint32_t* wr = w2 + row * c2;
    float amax = 0.f;
    for (long c = lane; c < c2; c += 64) { const uint32_t u = wr[c]; amax = fmaxf(amax, fmaxf(fabsf(Half<bf16_t>::lo(u)), fabsf(Half<bf16_t>::hi(u)))); }
    const float sc = fp8_pow2_scale(wave_max(amax));
    if (lane == 0) scale[row] = sc;
    const float inv = 1.0f / sc;                                      // exact: power of two
    uint16_t* qr = reinterpret_cast<uint16_t*>(q + row * cols);
    for (long c = lane; c < c2; c += 64) {
        const uint32_t u = wr[c];
        qr[c] = (uint16_t)(e4m3fn_encode(Half<bf16_t>::lo(u) * inv) | (e4m3fn_encode(Half<bf16_t>::hi(u) * inv) << 8));
    }
}

// Sign bits of the rows x - center (center null: x), packed in the order of numpy.packbits: dimension i is bit 7 - i % 8 of byte i / 8,
// set exactly when the element is > 0 (NaN, +0, -0: clear); bits d .. 8 ldb - 1 are zero.  One thread per output byte.  The test is
// taken on the bit pattern (0 < bits <= +inf's), so a subnormal element counts as positive whatever the denormal mode of the compare.
__global__ __launch_bounds__(256) void pack_sign_bits_kernel(const float* __restrict__ x, long n, int d, const float* __restrict__ center,
                                                             uint8_t* __restrict__ bits, long ldb) {
    const long total = n * ldb, stride = (long)gridDim.x * 256;
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += stride) {
        const long r = o / ldb;
        const int i0 = (int)(o - r * ldb) * 8;
        const float* xr = x + r * d;
        uint32_t b = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j;
            if (i < d) {
                const float v = center ? xr[i] - center[i] : xr[i];
                const uint32_t u = __float_as_uint(v);
                b |= (u - 1u < 0x7f800000u ? 1u : 0u) << (7 - j);
            }
        }
        bits[o] = (uint8_t)b;
    }
}

template <typename OutT>
__global__ __launch_bounds__(256) void fp8_dequant_rows_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scale,
                                                               long rows, long cols, OutT* __restrict__ out) {
    // cols % 4 == 0: each thread decodes 4 codes of one row
    const long n4 = rows * cols / 4, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const uint32_t u = reinterpret_cast<const uint32_t*>(q)[i];
        const float sc = scale[i * 4 / cols];
        const float v0 = e4m3fn_decode(u & 0xffu) * sc, v1 = e4m3fn_decode((u >> 8) & 0xffu) * sc;
        const float v2 = e4m3fn_decode((u >> 16) & 0xffu) * sc, v3 = e4m3fn_decode(u >> 24) * sc;
        if constexpr (sizeof(OutT) == 4) reinterpret_cast<float4*>(out)[i] = make_float4(v0, v1, v2, v3);
        else reinterpret_cast<uint2*>(out)[i] = make_uint2(Half<OutT>::pack2(v0, v1), Half<OutT>::pack2(v2, v3));
    }
}

template <typename H>
__global__ __launch_bounds__(256) void cvt16_kernel(const float* __restrict__ in, long numel, uint16_t* __restrict__ out) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) out[i] = f32_to_h<H>(in[i]);
}

// max |x| of an fp32 array folded into *out_bits by atomicMax on the bit pattern (non-negative floats order like
// unsigned integers; NaN maps above +inf and is therefore caught by a `< limit` test on the result)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ in, long numel, unsigned* __restrict__ out_bits) {
    const long stride = (long)gridDim.x * 256;
    unsigned m = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
        const unsigned b = __float_as_uint(in[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out_bits, m);
}

__global__ __launch_bounds__(256) void mean_axis0_kernel(const float* __restrict__ in, int n0, long n,
                                                         float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int j = 0; j < n0; ++j) acc += in[(long)j * n + i];
    out[i] = acc / (float)n0;
}

// ---- cross-encoder scoring: rows of the last hidden state -> log P(target | prefix) (crossencoder/beir/sgptce.py:150-262) ----
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ row_idx, int n,
                                                          int d, float* __restrict__ dst) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    const float4* s4 = reinterpret_cast<const float4*>(src + (long)row_idx[r] * d);
    float4* d4 = reinterpret_cast<float4*>(dst + (long)r * d);
    for (int c = lane; c < d / 4; c += 64) d4[c] = s4[c];
}

// one workgroup per row of logits [n, ld]: log_softmax over the V entries, gathered at the target id
// (F.log_softmax + torch.gather, sgptce.py:233,255), and the greedy token (argmax, first maximum, :243)
__global__ __launch_bounds__(256) void logprob_rows_kernel(const float* __restrict__ logits, long ld, int V,
                                                           const int* __restrict__ targets, float* __restrict__ out_lp,
                                                           int* __restrict__ out_arg) {
    __shared__ float s_f[4];
    __shared__ int s_i[4];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* x = logits + (long)r * ld;
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int i = t; i < V; i += 256) {
        const float v = x[i];
        if (v > mx || (v == mx && i < am)) { mx = v; am = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (ov > mx || (ov == mx && oi < am)) { mx = ov; am = oi; }
    }
    if (lane == 0) { s_f[wave] = mx; s_i[wave] = am; }
    __syncthreads();
    mx = s_f[0]; am = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_f[w] > mx || (s_f[w] == mx && s_i[w] < am)) { mx = s_f[w]; am = s_i[w]; }
    __syncthreads();
    float sum = 0.f;
    for (int i = t; i < V; i += 256) sum += expf(x[i] - mx);
    sum = wave_sum(sum);
    if (lane == 0) s_f[wave] = sum;
    __syncthreads();
    if (t == 0) {
        const float tot = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
        out_lp[r] = (x[clamp_index(targets[r], V)] - mx) - logf(tot);   // a bad target scores a wrong token
        if (out_arg) out_arg[r] = am;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ p, long n, float v) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = v;
}

// deterministic pseudo-random fill in [-scale, scale) (micro-benchmarks: never time MFMA on zeros, DVFS)
template <typename T>
__global__ __launch_bounds__(256) void fill_rand_kernel(T* __restrict__ p, long n, unsigned seed, float scale) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        unsigned h = (unsigned)i * 2654435761u ^ seed;
        h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
        const float v = ((float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale;
        if constexpr (sizeof(T) == 4) p[i] = v; else reinterpret_cast<uint16_t*>(p)[i] = f32_to_h<T>(v);
    }
}

// max |x| of a 16-bit array (fp8 activation-scale calibration: the range of a block's GELU output)
template <typename H>
__global__ __launch_bounds__(256) void absmax16_kernel(const uint32_t* __restrict__ in, long n2, unsigned* __restrict__ out_bits) {
    const long stride = (long)gridDim.x * 256;
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += stride) {
        const uint32_t u = in[i];
        m = fmaxf(m, fmaxf(fabsf(Half<H>::lo(u)), fabsf(Half<H>::hi(u))));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out_bits, __float_as_uint(m));
}

// Precision probe (sgpt_model_precision_probe_begin / _end): the crest factor max|v| / rms(v) of every row of a 16-bit
// operand [T][cols] (leading dimension ld), its maximum over the rows folded into *out_bits (fp32 bits, atomicMax).  A row of
// 11-bit values whose energy sits in one or two entries (outlier channels / hidden units of real GPT-Neo checkpoints: crest
// ~ sqrt(cols / 2); a well-conditioned row: 4-9) puts the whole relative rounding error of those entries on the dot product.
// One wave per row.
template <typename H>
__global__ __launch_bounds__(256) void crest16_kernel(const uint16_t* __restrict__ in, int T, int cols, long ld,
                                                      unsigned* __restrict__ out_bits) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int lane = threadIdx.x & 63;
    const uint32_t* r = reinterpret_cast<const uint32_t*>(in + (long)row * ld);
    float mx = 0.f, ss = 0.f;
    for (int c = lane; c < cols / 2; c += 64) {
        const uint32_t u = r[c];
        const float a = Half<H>::lo(u), b = Half<H>::hi(u);
        mx = fmaxf(mx, fmaxf(fabsf(a), fabsf(b)));
        ss += a * a + b * b;
    }
    mx = wave_max(mx);
    ss = wave_sum(ss);
    if (lane == 0 && ss > 0.f && mx < INFINITY) {
        const float crest = mx / sqrtf(ss / (float)cols);
        atomicMax(out_bits, __float_as_uint(crest));
    }
}

// fp32 rows [n][d] -> split-precision 16-bit rows [n][3 d]: layout 0 = [hi | lo | hi] (the streamed operand: activations,
// documents), layout 1 = [hi | hi | lo] (the resident operand: weights, queries); hi = round16(v), lo = round16(v - hi).
// One contraction over 3 d of a layout-0 row with a layout-1 row is hi.hi + lo.hi + hi.lo: the product to ~2^-22.
template <typename H>
__global__ __launch_bounds__(256) void split16_rows_kernel(const float* __restrict__ in, long n, int d, int layout,
                                                           uint16_t* __restrict__ out) {
    const long total = n * (long)(d / 4), stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const long r = e / (d / 4);
        const int c = (int)(e - r * (d / 4)) * 4;
        const float4 v = *reinterpret_cast<const float4*>(in + r * d + c);
        const uint32_t h01 = Half<H>::pack2(v.x, v.y), h23 = Half<H>::pack2(v.z, v.w);
        const uint2 hi = make_uint2(h01, h23);
        const uint2 lo = make_uint2(Half<H>::pack2(v.x - Half<H>::lo(h01), v.y - Half<H>::hi(h01)),
                                    Half<H>::pack2(v.z - Half<H>::lo(h23), v.w - Half<H>::hi(h23)));
        uint16_t* o = out + r * 3 * d + c;
        *reinterpret_cast<uint2*>(o) = hi;
        *reinterpret_cast<uint2*>(o + d) = layout == 0 ? lo : hi;
        *reinterpret_cast<uint2*>(o + 2 * d) = layout == 0 ? hi : lo;
    }
}

inline int cap_grid(long blocks) { return (int)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks)); }
inline dim3 row_grid(long rows) { return dim3((unsigned)((rows + 3) / 4)); }   // one wave per row, four rows per workgroup

// f(std::integral_constant<int, NV>) with the rung NV >= ceil(d / 256) the one-wave-per-row kernels are instantiated for: NV float4
// column blocks per lane (d <= 4096)
template <typename F>
inline void for_row_width(int d, F&& f) {
    const int nv = (d + 255) / 256;
    if (nv <= 1) f(std::integral_constant<int, 1>{});
    else if (nv <= 2) f(std::integral_constant<int, 2>{});
    else if (nv <= 3) f(std::integral_constant<int, 3>{});
    else if (nv <= 4) f(std::integral_constant<int, 4>{});
    else if (nv <= 8) f(std::integral_constant<int, 8>{});
    else if (nv <= 10) f(std::integral_constant<int, 10>{});
    else f(std::integral_constant<int, 16>{});
}
// f(E{}) with E the element type of a dtype code: bf16, f16, anything else float -- or, 16-bit alone, f16, anything else bf16
template <typename F>
inline void for_dtype(int dtype, F&& f) {
    if (dtype == DT_BF16) f(bf16_t{});
    else if (dtype == DT_F16) f(f16_t{});
    else f(float{});
}
template <typename F>
inline void for_dtype16(int dtype, F&& f) {
    if (dtype == DT_F16) f(f16_t{});
    else f(bf16_t{});
}

}  // namespace

void launch_embed(const int* ids, const int* pos, const float* wte, const float* wpe, float* x, int T, int d, int vocab,
                  int max_pos, hipStream_t s) {
    hipLaunchKernelGGL(embed_kernel, row_grid(T), dim3(256), 0, s, ids, pos, wte, wpe, x, T, d, vocab, max_pos);
}

void launch_layernorm(const float* x, const float* g, const float* b, void* out, int out_dtype, int T, int d,
                      float eps, hipStream_t s, float out_mul) {
    const float mul = out_dtype == DT_F16 ? out_mul : 1.0f;
    for_row_width(d, [&](auto nv) {
        for_dtype(out_dtype, [&](auto e) {
            using E = decltype(e);
            hipLaunchKernelGGL((layernorm_kernel<E, decltype(nv)::value>), row_grid(T), dim3(256), 0, s, x, g, b, (E*)out, T, d, eps, mul);
        });
    });
}

void launch_layernorm_writeback(float* x, const float* g, const float* b, void* out16, int out_dtype, int T, int d, float eps,
                                int* range_flag, hipStream_t s) {
    for_row_width(d, [&](auto nv) {
        for_dtype16(out_dtype, [&](auto e) {
            using E = decltype(e);
            hipLaunchKernelGGL((layernorm_writeback_kernel<E, decltype(nv)::value>), row_grid(T), dim3(256), 0, s, x, g, b, (E*)out16, T, d,
                               eps, range_flag);
        });
    });
}

void launch_rmsnorm(const float* x, const float* g, void* out, int out_dtype, int T, int d, float eps, int* range_flag, hipStream_t s) {
    for_row_width(d, [&](auto nv) {
        for_dtype(out_dtype, [&](auto e) {
            using E = decltype(e);
            hipLaunchKernelGGL((rmsnorm_kernel<E, decltype(nv)::value>), row_grid(T), dim3(256), 0, s, x, g, (E*)out, T, d, eps, range_flag);
        });
    });
}

void launch_swiglu(const void* gu, void* h, int dtype, int T, int ffn, int* range_flag, hipStream_t s) {
    const long n_vec = (long)T * ffn / (dtype == DT_F32 ? 4 : 8);
    const unsigned grid = (unsigned)((n_vec + 255) / 256);
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(swiglu_kernel<E>, dim3(grid), dim3(256), 0, s, (const E*)gu, (E*)h, n_vec, ffn, range_flag);
    });
}

void launch_layernorm_split(const float* x, const float* g, const float* b, void* out, int out_dtype, int T, int d,
                            float eps, hipStream_t s, float out_mul) {
    const float mul = out_dtype == DT_F16 ? out_mul : 1.0f;
    for_row_width(d, [&](auto nv) {
        for_dtype16(out_dtype, [&](auto e) {
            hipLaunchKernelGGL((layernorm_split_kernel<decltype(e), decltype(nv)::value>), row_grid(T), dim3(256), 0, s, x, g, b,
                               (uint16_t*)out, T, d, eps, mul);
        });
    });
}

void launch_crest16(const void* in, int T, int cols, long ld, int dtype, unsigned* out_bits, hipStream_t s) {
    for_dtype16(dtype, [&](auto e) {
        hipLaunchKernelGGL(crest16_kernel<decltype(e)>, row_grid(T), dim3(256), 0, s, (const uint16_t*)in, T, cols, ld, out_bits);
    });
}

void launch_split16_rows(const float* in, long n, int d, int layout, void* out, int out_dtype, hipStream_t s) {
    const int grid = cap_grid((n * (d / 4) + 255) / 256);
    for_dtype16(out_dtype, [&](auto e) {
        hipLaunchKernelGGL(split16_rows_kernel<decltype(e)>, dim3(grid), dim3(256), 0, s, in, n, d, layout, (uint16_t*)out);
    });
}

void launch_pack_split_rows(const float* src, long rows, long cols, void* dst, int out_dtype, hipStream_t s) {
    const int grid = cap_grid((rows * cols + 255) / 256);
    for_dtype16(out_dtype, [&](auto e) {
        hipLaunchKernelGGL(pack_split_rows_kernel<decltype(e)>, dim3(grid), dim3(256), 0, s, src, rows, cols, (uint16_t*)dst);
    });
}

void launch_layernorm_q8(const float* x, const float* g, const float* b, void* q, float* scale, int T, int d, float eps, hipStream_t s) {
    for_row_width(d, [&](auto nv) {
        hipLaunchKernelGGL(layernorm_q8_kernel<decltype(nv)::value>, row_grid(T), dim3(256), 0, s, x, g, b, (uint8_t*)q, scale, T, d, eps);
    });
}

void launch_rmsnorm_q8(const float* x, const float* g, void* q, float* scale, int T, int d, float eps, hipStream_t s) {
    for_row_width(d, [&](auto nv) {
        hipLaunchKernelGGL(rmsnorm_q8_kernel<decltype(nv)::value>, row_grid(T), dim3(256), 0, s, x, g, (uint8_t*)q, scale, T, d, eps);
    });
}

// ffn % 16 == 0; the register steps of a row: 1, 2, 4 or 7 x 4096 columns, beyond that the re-reading variant
void launch_swiglu_q8(const void* gu, int dtype, void* q, float* scale, int T, int ffn, hipStream_t s) {
    for_dtype16(dtype, [&](auto e) {
        using E = decltype(e);
        const auto kernel = ffn <= 4096 ? swiglu_q8_kernel<E, 1> : ffn <= 8192 ? swiglu_q8_kernel<E, 2> : ffn <= 16384 ? swiglu_q8_kernel<E, 4>
                          : ffn <= 28672 ? swiglu_q8_kernel<E, 7> : swiglu_q8_kernel<E, 0>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)T), dim3(256), 0, s, (const E*)gu, (uint8_t*)q, scale, ffn);
    });
}

void launch_fp8_quant_rows_bf16(const void* w, long rows, long cols, void* q, float* scale, hipStream_t s) {
    hipLaunchKernelGGL(fp8_quant_rows_bf16_kernel, row_grid(rows), dim3(256), 0, s, (const uint32_t*)w, rows, cols, (uint8_t*)q, scale);
}

void launch_absmax16(const void* in, long numel, int dtype, unsigned* out_bits, hipStream_t s) {
    const int grid = cap_grid((numel / 2 + 255) / 256);
    for_dtype16(dtype, [&](auto e) {
        hipLaunchKernelGGL(absmax16_kernel<decltype(e)>, dim3(grid), dim3(256), 0, s, (const uint32_t*)in, numel / 2, out_bits);
    });
}

void launch_lnf_pool(const float* x, const float* g, const float* b, const int* seq_off, const int* seq_len,
                     const int* pad_left, int B, int d, float eps, int apply_ln, int mode, int normalize,
                     const float* pos_weights, int pos_weights_n, float* out, hipStream_t s, int* nonfinite_flag, int norm_kind,
                     const int* pool_lo) {
    const size_t sm = (size_t)(4 * d + 8) * sizeof(float);
    for_row_width(d, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        const auto kernel = norm_kind == 1 ? lnf_pool_kernel<NV, RowRMSNorm<true>> : lnf_pool_kernel<NV, RowLayerNorm<true>>;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(256), sm, s, x, g, b, seq_off, seq_len, pad_left, pool_lo, d, eps, apply_ln, mode, normalize,
                           pos_weights, pos_weights_n, out, nonfinite_flag);
    });
}

void launch_pool(const void* hidden, int dtype, const int* mask, int B, int S, int d, int mode,
                 const float* pos_weights, float* out, hipStream_t s) {
    dim3 grid(B, (d / 4 + 255) / 256);
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(pool_kernel<E>, grid, dim3(256), 0, s, (const E*)hidden, mask, S, d, mode, pos_weights, out);
    });
}

void launch_pack_sign_bits(const float* x, long n, int d, const float* center, uint8_t* bits, long ldb, hipStream_t s) {
    const long blocks = (n * ldb + 255) / 256;
    hipLaunchKernelGGL(pack_sign_bits_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks))), dim3(256), 0, s, x, n, d,
                       center, bits, ldb);
}

void launch_fp8_quant_rows(const float* w, long rows, long cols, void* q, float* scale, hipStream_t s) {
    hipLaunchKernelGGL(fp8_quant_rows_kernel, row_grid(rows), dim3(256), 0, s, w, rows, cols, (uint8_t*)q, scale);
}

// f16: exact as long as code * scale stays an f16 value (a quantised corpus of unit rows does)
void launch_fp8_dequant_rows(const void* q, const float* scale, long rows, long cols, void* out, int out_dtype,
                             hipStream_t s) {
    const int grid = cap_grid((rows * cols / 4 + 255) / 256);
    for_dtype(out_dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(fp8_dequant_rows_kernel<E>, dim3(grid), dim3(256), 0, s, (const uint8_t*)q, scale, rows, cols, (E*)out);
    });
}

void launch_gather_rows(const float* src, const int* row_idx, int n, int d, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, row_grid(n), dim3(256), 0, s, src, row_idx, n, d, dst);
}

void launch_logprob_rows(const float* logits, long ld, int V, const int* targets, int n, float* out_lp, int* out_arg,
                         hipStream_t s) {
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(n), dim3(256), 0, s, logits, ld, V, targets, out_lp, out_arg);
}

void launch_mean_over_axis0(const float* in, int n0, long n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mean_axis0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n0, n, out);
}

void launch_pairwise(const float* a, const float* b, long n, int d, bool cosine, float* out, hipStream_t s) {
    hipLaunchKernelGGL(cosine ? pairwise_kernel<true> : pairwise_kernel<false>, row_grid(n), dim3(256), 0, s, a, b, n, d, out);
}

void launch_l2norm(const float* in, long n, int d, void* out, int out_dtype, hipStream_t s) {
    for_dtype(out_dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(l2norm_kernel<E>, row_grid(n), dim3(256), 0, s, in, n, d, (E*)out);
    });
}

void launch_f32_to_16(const float* in, long numel, void* out, int out_dtype, hipStream_t s) {
    const int grid = cap_grid((numel + 255) / 256);
    for_dtype16(out_dtype, [&](auto e) {
        hipLaunchKernelGGL(cvt16_kernel<decltype(e)>, dim3(grid), dim3(256), 0, s, in, numel, (uint16_t*)out);
    });
}

void launch_absmax(const float* in, long numel, unsigned* out_bits, hipStream_t s) {
    hipLaunchKernelGGL(absmax_kernel, dim3(cap_grid((numel + 255) / 256)), dim3(256), 0, s, in, numel, out_bits);
}

void launch_fill_f32(float* p, long n, float v, hipStream_t s) {
    hipLaunchKernelGGL(fill_kernel, dim3(cap_grid((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

void launch_fill_rand(void* p, long n, int dtype, unsigned seed, float scale, hipStream_t s) {
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(fill_rand_kernel<E>, dim3(cap_grid((n + 255) / 256)), dim3(256), 0, s, (E*)p, n, seed, scale);
    });
}

void launch_rope(void* qk, int dtype, long ld, long k_off, const int* pos, const float* sin_t, const float* cos_t, int T,
                 int H, int dh, int rotary_dim, int max_pos, hipStream_t s) {
    const int half = rotary_dim / 2;
    const long n = (long)T * H * half;
    const int grid = (int)((n + 255) / 256);
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(rope_kernel<E>, dim3(grid), dim3(256), 0, s, (E*)qk, ld, k_off, pos, sin_t, cos_t, T, H, dh, half, max_pos);
    });
}

void launch_rope_half(void* qk, int dtype, long ld, long k_off, const int* pos, const float* sin_t, const float* cos_t, int T,
                      int H, int H_kv, int dh, int max_pos, hipStream_t s) {
    const long n = (long)T * (H + H_kv) * (dh / 8);
    const int grid = (int)((n + 255) / 256);
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL(rope_half_kernel<E>, dim3(grid), dim3(256), 0, s, (E*)qk, ld, k_off, pos, sin_t, cos_t, T, H, H_kv, dh, max_pos);
    });
}

void launch_qknorm_rope_half(void* qk, int dtype, long ld, long k_off, const int* pos, const float* sin_t, const float* cos_t,
                             const float* q_g, const float* k_g, float eps, int T, int H, int H_kv, int dh, int max_pos, int* range_flag,
                             hipStream_t s) {
    const long n = (long)T * (H + H_kv) * (dh / 8);
    const int grid = (int)((n + 255) / 256);
    if (dh != 64 && dh != 128) return;                  // (the callers refuse it: sgpt_qknorm_rope_half, check_desc)
    for_dtype(dtype, [&](auto e) {
        using E = decltype(e);
        hipLaunchKernelGGL((dh == 64 ? qknorm_rope_half_kernel<E, 64> : qknorm_rope_half_kernel<E, 128>), dim3(grid), dim3(256), 0, s,
                           (E*)qk, ld, k_off, pos, sin_t, cos_t, q_g, k_g, eps, T, H, H_kv, max_pos, range_flag);
    });
}

void launch_qkv_deinterleave(const float* src, float* dst, int H, int dh, long row_len, hipStream_t s) {
    hipLaunchKernelGGL(qkv_deinterleave_kernel, dim3(3 * H * dh), dim3(256), 0, s, src, dst, H, dh, row_len);
}
