// One-wave-per-row normalisation in registers, shared by the streaming kernels (elementwise.hip) and by the query-sized
// projections that normalise their own A rows (qgemm.hip): the SAME loads, reductions and arithmetic, so a LayerNorm that
// runs inside a projection's prologue produces the bits of the stand-alone kernel.  Here: the row in registers (RowLN), the two
// normalisers (LayerNorm, RMSNorm), the store loops of the stand-alone kernels (sinks) and the skeleton that joins them (rownorm_row).
#pragma once
#include "common.h"

#ifndef SGPT_LN_NT_LOAD
#define SGPT_LN_NT_LOAD 1   // LayerNorm / ln_f+pool read the residual stream with non-temporal loads: x is not needed again
                            // before the next residual epilogue, and leaving the caches to `a` (the next GEMM's operand) is
                            // +2.9 % end to end (36.07 k -> 37.11 k sentences/s, A/B on one box)
#endif

// row statistics + normalise in registers: nn.LayerNorm(eps) (HF:gpt_neo:317-319,385,492)
// NT = non-temporal row loads (the bulk kernels); the query-sized prologues re-read a row once per column tile: cached loads
template <int NV, bool NT = (SGPT_LN_NT_LOAD != 0)>
struct RowLN {
    float4 v[NV];
    __device__ __forceinline__ void load(const float* __restrict__ xr, int d, int lane) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[i] = c < d ? ldg16<NT>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // f(i, c) for every column block i of this lane that lies inside the row: v[i] holds columns c .. c + 3
    template <typename F>
    static __device__ __forceinline__ void for_cols(int d, int lane, F&& f) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) f(i, c);
        }
    }
    // statistics of the row (the butterfly of wave_sum; FAST: the same partners and order through VALU lane exchanges -- a + b
    // is commutative, so the bits do not depend on which instruction fetched the partner's value)
    template <bool FAST = false>
    __device__ __forceinline__ void stats(int d, int lane, float& mean, float& rstd, float eps) const {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        mean = (FAST ? wave_sum_valu(s) : wave_sum(s)) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) {
                const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
        rstd = 1.0f / sqrtf((FAST ? wave_sum_valu(q) : wave_sum(q)) / (float)d + eps);
    }
    __device__ __forceinline__ void scale(int i, float mean, float rstd, const float4& gg, const float4& bb) {
        v[i].x = (v[i].x - mean) * rstd * gg.x + bb.x;
        v[i].y = (v[i].y - mean) * rstd * gg.y + bb.y;
        v[i].z = (v[i].z - mean) * rstd * gg.z + bb.z;
        v[i].w = (v[i].w - mean) * rstd * gg.w + bb.w;
    }
    // FAST: the statistics' butterflies on the VALU (same partners, same order, same bits) -- for launches whose few waves wait on
    // the reductions themselves (ln_f + pool of a handful of query sequences)
    template <bool FAST = false>
    __device__ __forceinline__ void normalize(const float* __restrict__ g, const float* __restrict__ b, int d,
                                              float eps, int lane) {
        float mean, rstd;
        stats<FAST>(d, lane, mean, rstd, eps);
        for_cols(d, lane, [&](int i, int c) {
            scale(i, mean, rstd, *reinterpret_cast<const float4*>(g + c), *reinterpret_cast<const float4*>(b + c));
        });
    }
    // the same with gamma / beta already in registers (gg[i], bb[i] = the lane's float4 of column block i) and the VALU butterfly:
    // the query-sized prologues fetch every operand of the tile's rows in ONE memory round trip (qgemm.hip)
    __device__ __forceinline__ void normalize_pre(const float4* gg, const float4* bb, int d, float eps, int lane) {
        float mean, rstd;
        stats<true>(d, lane, mean, rstd, eps);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) scale(i, mean, rstd, gg[i], bb[i]);
        }
    }
};

// R rows normalised together (gamma / beta in registers): RowLN::normalize_pre on each row, with the rows' reductions interleaved
// (wave_sum_valu_multi) -- the same operations on every row, the same bits.
template <int NV, int R, bool NT>
__device__ __forceinline__ void rowln_normalize_rows(RowLN<NV, NT> (&r)[R], const float4* gg, const float4* bb, int d, float eps, int lane) {
    float s[R], q[R], mean[R], rstd[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        s[u] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s[u] += (r[u].v[i].x + r[u].v[i].y) + (r[u].v[i].z + r[u].v[i].w);
    }
    wave_sum_valu_multi<R>(s);
#pragma unroll
    for (int u = 0; u < R; ++u) {
        mean[u] = s[u] / (float)d;
        q[u] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) {
                const float a0 = r[u].v[i].x - mean[u], a1 = r[u].v[i].y - mean[u], a2 = r[u].v[i].z - mean[u], a3 = r[u].v[i].w - mean[u];
                q[u] += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
    }
    wave_sum_valu_multi<R>(q);
#pragma unroll
    for (int u = 0; u < R; ++u) rstd[u] = 1.0f / sqrtf(q[u] / (float)d + eps);
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < d) r[u].scale(i, mean[u], rstd[u], gg[i], bb[i]);
        }
}

// RMSNorm of the Llama family (HF:llama/modeling_llama.py LlamaRMSNorm): out = x * rsqrt(mean(x^2) + eps) * g -- no mean subtraction,
// no bias.  The square sum goes through the butterfly of the LayerNorm statistics; HF's order of operations: (x * rstd) first,
// then * g.  Columns past d hold zeros and add nothing to the sum.
template <int NV, bool FAST = false>
__device__ __forceinline__ void rms_normalize(RowLN<NV>& r, const float* __restrict__ g, int d, float eps, int lane) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) q += (r.v[i].x * r.v[i].x + r.v[i].y * r.v[i].y) + (r.v[i].z * r.v[i].z + r.v[i].w * r.v[i].w);
    const float rstd = 1.0f / sqrtf((FAST ? wave_sum_valu(q) : wave_sum(q)) / (float)d + eps);
    r.for_cols(d, lane, [&](int i, int c) {
        const float4 gg = *reinterpret_cast<const float4*>(g + c);
        r.v[i].x = r.v[i].x * rstd * gg.x; r.v[i].y = r.v[i].y * rstd * gg.y;
        r.v[i].z = r.v[i].z * rstd * gg.z; r.v[i].w = r.v[i].w * rstd * gg.w;
    });
}

// ---- normalisers: norm(r, d, lane) turns the loaded row into the normalised one.  Both are built from (g, b, eps) so that a kernel
// templated on the normaliser constructs either; FAST as in RowLN::normalize ----
template <bool FAST = false>
struct RowLayerNorm {
    const float *g, *b;
    float eps;
    __device__ __forceinline__ RowLayerNorm(const float* g_, const float* b_, float eps_) : g(g_), b(b_), eps(eps_) {}
    template <int NV>
    __device__ __forceinline__ void operator()(RowLN<NV>& r, int d, int lane) const { r.template normalize<FAST>(g, b, d, eps, lane); }
};
template <bool FAST = false>
struct RowRMSNorm {
    const float* g;
    float eps;
    __device__ __forceinline__ RowRMSNorm(const float* g_, const float* /* no bias: never read */, float eps_) : g(g_), eps(eps_) {}
    template <int NV>
    __device__ __forceinline__ void operator()(RowLN<NV>& r, int d, int lane) const { rms_normalize<NV, FAST>(r, g, d, eps, lane); }
};

// ---- sinks: sink(r, row, at, d, lane) stores the normalised row; at = row * d, the offset of the row in a [T][d] array ----
// out [T][d] in OutT, rounded once (fp32: stored as it is).  16-bit outputs: MUL multiplies by out_mul first (the power-of-two range
// shift of an f16 operand; the consuming GEMMs multiply their accumulators by 1 / out_mul), TRACK passes every value through the f16
// range tracker (kernels that rely on no load-time bound of the gain).  Neither costs an instruction where it is off.
template <typename OutT, bool MUL, bool TRACK>
struct RowStore {
    OutT* out;
    float out_mul;
    int* range_flag;
    template <int NV>
    __device__ __forceinline__ void operator()(const RowLN<NV>& r, int row, long at, int d, int lane) const {
        RangeTrack<OutT> range;
        r.for_cols(d, lane, [&](int i, int c) {
            if constexpr (sizeof(OutT) == 4) {
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + at + c) = r.v[i];
            } else {
                float4 v = r.v[i];
                if constexpr (MUL) { v.x *= out_mul; v.y *= out_mul; v.z *= out_mul; v.w *= out_mul; }
                if constexpr (TRACK) { range.note(v.x, v.y); range.note(v.z, v.w); }
                *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out) + at + c) =
                    make_uint2(Half<OutT>::pack2(v.x, v.y), Half<OutT>::pack2(v.z, v.w));
            }
        });
        if constexpr (TRACK && sizeof(OutT) != 4) range.finish(range_flag);
    }
};

// the row back to x in fp32 and -- the same registers, rounded once -- to the 16-bit buffer out16 [T][d], range-tracked
template <typename OutT>
struct RowStoreWriteback {
    float* x;
    OutT* out16;
    int* range_flag;
    template <int NV>
    __device__ __forceinline__ void operator()(const RowLN<NV>& r, int row, long at, int d, int lane) const {
        RangeTrack<OutT> range;
        r.for_cols(d, lane, [&](int i, int c) {
            *reinterpret_cast<float4*>(x + at + c) = r.v[i];
            range.note(r.v[i].x, r.v[i].y); range.note(r.v[i].z, r.v[i].w);
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(out16) + at + c) =
                make_uint2(Half<OutT>::pack2(r.v[i].x, r.v[i].y), Half<OutT>::pack2(r.v[i].z, r.v[i].w));
        });
        range.finish(range_flag);
    }
};

// a = row * out_mul as [hi | lo | hi] in out [T][3 d]: hi = round16(a), lo = round16(a - hi)
template <typename OutT>
struct RowStoreSplit {
    uint16_t* out;
    float out_mul;
    template <int NV>
    __device__ __forceinline__ void operator()(const RowLN<NV>& r, int row, long at, int d, int lane) const {
        uint16_t* o = out + 3 * at;
        r.for_cols(d, lane, [&](int i, int c) {
            const float v0 = r.v[i].x * out_mul, v1 = r.v[i].y * out_mul, v2 = r.v[i].z * out_mul, v3 = r.v[i].w * out_mul;
            const uint32_t h01 = Half<OutT>::pack2(v0, v1), h23 = Half<OutT>::pack2(v2, v3);
            const uint32_t l01 = Half<OutT>::pack2(v0 - Half<OutT>::lo(h01), v1 - Half<OutT>::hi(h01));
            const uint32_t l23 = Half<OutT>::pack2(v2 - Half<OutT>::lo(h23), v3 - Half<OutT>::hi(h23));
            *reinterpret_cast<uint2*>(o + c) = make_uint2(h01, h23);
            *reinterpret_cast<uint2*>(o + d + c) = make_uint2(l01, l23);
            *reinterpret_cast<uint2*>(o + 2 * d + c) = make_uint2(h01, h23);
        });
    }
};

// The power-of-two row scale of the fp8 (OCP e4m3fn) formats: the smallest 2^k with amax / 2^k <= 448, i.e. amax / 2^k in (224, 448].
// amax = m * 2^e, 1 <= m < 2 (subnormal amax: e = -127): m <= 1.75 -> 2^(e - 8), else 2^(e - 7).  amax 0, inf or NaN: 1.
__device__ __forceinline__ float fp8_pow2_scale(float amax) {
    float sc = 1.0f;
    if (amax > 0.f && amax < 3.0e38f) {
        const uint32_t u = __float_as_uint(amax);
        const int e = (int)((u >> 23) & 0xffu) - 127;
        int k = e - ((u & 0x7fffffu) > 0x600000u ? 7 : 8);
        k = k < -126 ? -126 : (k > 127 ? 127 : k);
        sc = __uint_as_float((uint32_t)(k + 127) << 23);
    }
    return sc;
}

// e4m3fn codes q [T][d] under ONE scale per row (fp8_pow2_scale of max|row|), which factors out of the consuming GEMM's k-sum
struct RowStoreFp8 {
    uint8_t* q;
    float* scale;
    template <int NV>
    __device__ __forceinline__ void operator()(const RowLN<NV>& r, int row, long at, int d, int lane) const {
        float amax = 0.f;
        r.for_cols(d, lane, [&](int i, int) {
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(r.v[i].x), fabsf(r.v[i].y)), fmaxf(fabsf(r.v[i].z), fabsf(r.v[i].w))));
        });
        const float sc = fp8_pow2_scale(wave_max(amax));
        if (lane == 0) scale[row] = sc;
        const float inv = 1.0f / sc;
        r.for_cols(d, lane, [&](int i, int c) {
            int w = __builtin_amdgcn_cvt_pk_fp8_f32(r.v[i].x * inv, r.v[i].y * inv, 0, false);
            w = __builtin_amdgcn_cvt_pk_fp8_f32(r.v[i].z * inv, r.v[i].w * inv, w, true);
            *reinterpret_cast<uint32_t*>(q + at + c) = (uint32_t)w;
        });
    }
};

// The body of every stand-alone row kernel: one wave per row (four rows per 256-thread workgroup), the row loaded into registers,
// normalised there, and handed to the sink.  All of a wave's loads precede its stores and a wave owns its row, so a sink may write
// the memory x was read from: fp32 layernorm / rmsnorm with out == x, and the write-back through x, are in place by contract.
template <int NV, typename Norm, typename Sink>
__device__ __forceinline__ void rownorm_row(const float* x, int T, int d, const Norm& norm, const Sink& sink) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int lane = threadIdx.x & 63;
    RowLN<NV> r;
    const long at = (long)row * d;
    r.load(x + at, d, lane);
    norm(r, d, lane);
    sink(r, row, at, d, lane);
}
