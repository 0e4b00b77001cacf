// The uint8 codec of the one-byte scorer tile (score64c.h), and the query prologue and row kernels of the format: a corpus held as
// uint8 codes with one range per DIMENSION (sentence-transformers' precision="uint8"; the format of sgpt_u8_quantize_rows, include/sgpt_hip.h):
//     x^[n][j] = start[j] + codes[n][j] * step[j],      codes [N][ld] bytes, ld = ceil(d / 128) * 128, pad columns hold 128.
// One byte per element as the fp8 corpus, but 256 uniform levels inside each column's own range instead of three mantissa bits under
// one scale per row: five to seven times less score error on anisotropic embeddings.
//
// Arithmetic.  The per-dimension scale folds into the QUERY, so the document operand of the MFMA is the bare code:
//     mid[j] = start[j] + 128 step[j],   c = code - 128 (an integer in [-128, 127], exact in f16)
//     <q, x^_n> = sum_j q_j mid_j + sum_j (q_j step_j) c[n][j] = qbias + qscale * <q'', c_n>
// with q'' = RNE_f16(q_j step_j / qscale), qscale a power of two per query row that puts max |q''| into [1, 2] (u8_prepare_queries_kernel
// below: q_j step_j is ~4e-5 for unit rows at d = 768, an f16 subnormal without it).  A product of an 11-bit by an 8-bit significand is
// exact in fp32; the sums accumulate in the MFMA's fp32, k ascending in slices of 32 as every scorer here.  ONE fma per score,
// fmaf(acc, qscale, qbias), at the head of the tile epilogue puts it back in the natural domain, before the NaN rule and the threshold
// compare: thresholds, candidate lists, merges and running lists are the f16 scorer's.
//
// Conversion, 2 + 2 instructions per 4 codes (the fp8 tile's count): v_perm_b32 places two code bytes under the constant 0x64 -- the
// f16 bit pattern 0x6400 | u is 1024 + u exactly (ulp 1 in [1024, 2048)) -- and v_pk_add_f16 with -1152 gives u - 128 exactly.
#include "score64c.h"

namespace {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

// 2 of 8 uint8 codes (k ascending from the low byte of c.x) -> f16 values code - 128, exact
__device__ __forceinline__ uint32_t cvt_u8x2_f16(uint32_t w, uint32_t sel) {
    const h16x2 v = __builtin_bit_cast(h16x2, __builtin_amdgcn_perm(0x64006400u, w, sel)) - h16x2{(_Float16)1152.0f, (_Float16)1152.0f};
    return __builtin_bit_cast(uint32_t, v);
}

struct U8Codec {
    typedef ScoreU8Args Args;
    static constexpr bool kRagged = true;          // any number of documents: a ragged shard needs neither scratch nor a second launch
    static __device__ __forceinline__ uint4 cvt(const uint2 c) {
        uint4 r;
        r.x = cvt_u8x2_f16(c.x, 0x07010700u);     // bytes 0, 1 of the codes under byte 7 of the pair = 0x64
        r.y = cvt_u8x2_f16(c.x, 0x07030702u);     // bytes 2, 3
        r.z = cvt_u8x2_f16(c.y, 0x07010700u);
        r.w = cvt_u8x2_f16(c.y, 0x07030702u);
        return r;
    }
    struct Lane {
        float qs[4], qb[4];                        // the two values of the fma, per query row of this lane
        __device__ __forceinline__ void before_loop(const Args& a, int fr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qs[i] = a.qscale[i * 16 + fr];
                qb[i] = a.qbias[i * 16 + fr];
            }
        }
        __device__ __forceinline__ void tile_begin(const Args&, long, int) {}
        // back to the natural domain, once per tile: score = acc * qscale + qbias (one fma)
        __device__ __forceinline__ float finish(float acc, int i, int, int) const { return __builtin_fmaf(acc, qs[i], qb[i]); }
    };
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Query prologue: one workgroup per row of the 64-row padded tile.  Row r < nq: q'_j = q_j * step_j (fp32, one rounding), e = the
// exponent with max_j |q'_j| * 2^-e in [1, 2) (0 for a zero or non-finite row), qpad[r][j] = RNE_f16(q'_j * 2^-e), qscale[r] = 2^e,
// qbias[r] = sum_j q_j * (start_j + 128 step_j) in fp32 (thread t sums columns t, t + 256, ...; the 256 partial sums are added in a fixed
// butterfly: deterministic).  Rows nq .. 63 and the pad columns d .. ld - 1 are zero, with qscale 1 and qbias 0.
__global__ __launch_bounds__(256) void u8_prepare_queries_kernel(const float* __restrict__ q, const float* __restrict__ start,
                                                                 const float* __restrict__ step, int nq, int d, int ld,
                                                                 f16_t* __restrict__ qpad, float* __restrict__ qscale,
                                                                 float* __restrict__ qbias) {
    __shared__ float red[2][4];
    const int r = blockIdx.x, t = threadIdx.x;
    f16_t* out = qpad + (long)r * ld;
    if (r >= nq) {
        for (int j = t; j < ld; j += 256) out[j].bits = 0;
        if (t == 0) { qscale[r] = 1.0f; qbias[r] = 0.0f; }
        return;
    }
    const float* row = q + (long)r * d;
    float amax = 0.f, bias = 0.f;
    bool bad = false;
    for (int j = t; j < d; j += 256) {
        const float st = step[j];
        const float qp = __fmul_rn(row[j], st);
        bad |= !(fabsf(qp) < INFINITY);
        amax = fmaxf(amax, fabsf(qp));
        bias = __fadd_rn(bias, __fmul_rn(row[j], __fadd_rn(start[j], __fmul_rn(128.0f, st))));
    }
    amax = wave_max(amax);
    bias = wave_sum(bias);
    const unsigned long long anybad = __ballot(bad);
    if ((t & 63) == 0) { red[0][t >> 6] = anybad != 0 ? INFINITY : amax; red[1][t >> 6] = bias; }
    __syncthreads();
    amax = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    bias = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    int e = 0;
    if (amax > 0.f && amax < INFINITY) { (void)frexpf(amax, &e); e -= 1; }     // amax = m * 2^(e + 1), m in [0.5, 1)
    for (int j = t; j < ld; j += 256) {
        float v = 0.f;
        if (j < d) v = ldexpf(__fmul_rn(row[j], step[j]), -e);
        out[j].bits = f32_to_h<f16_t>(v);
    }
    if (t == 0) { qscale[r] = ldexpf(1.0f, e); qbias[r] = bias; }
}

// Column min / max of fp32 rows x [n][d], NaN-propagating (a NaN anywhere in a column makes both NaN).  accumulate != 0: mn / mx go in as
// the running values of earlier blocks of rows.  One workgroup per 32 columns: 8 row lanes x 32 columns.
__global__ __launch_bounds__(256) void u8_col_minmax_kernel(const float* __restrict__ x, long n, int d, int accumulate,
                                                            float* __restrict__ mn, float* __restrict__ mx) {
    __shared__ float s_mn[8][32], s_mx[8][32];
    __shared__ int s_nan[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cl;
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    if (col < d) {
        for (long r = rl; r < n; r += 8) {
            const float v = x[r * d + col];
            nan |= v != v;
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
    }
    s_mn[rl][cl] = lo; s_mx[rl][cl] = hi; s_nan[rl][cl] = nan;
    __syncthreads();
    if (rl == 0 && col < d) {
#pragma unroll
        for (int i = 1; i < 8; ++i) { lo = fminf(lo, s_mn[i][cl]); hi = fmaxf(hi, s_mx[i][cl]); nan |= s_nan[i][cl]; }
        if (accumulate) {
            const float a = mn[col], b = mx[col];
            nan |= (a != a) | (b != b);
            lo = fminf(lo, a); hi = fmaxf(hi, b);
        }
        mn[col] = nan ? NAN : lo;
        mx[col] = nan ? NAN : hi;
    }
}

// x fp32 [n][d] -> codes [n][ld] (ld % 4 == 0; pad columns 128): one thread per 4 codes, one 4-byte store
__global__ __launch_bounds__(256) void u8_quant_rows_kernel(const float* __restrict__ x, long n, int d, int ld,
                                                            const float* __restrict__ start, const float* __restrict__ step,
                                                            uint8_t* __restrict__ codes) {
    const long per_row = ld / 4, total = n * per_row;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per_row;
        const int j0 = (int)(i - r * per_row) * 4;
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            const uint32_t c = j < d ? u8_code(x[r * d + j], start[j], step[j]) : 128u;
            w |= c << (8 * e);
        }
        *reinterpret_cast<uint32_t*>(codes + r * ld + j0) = w;
    }
}

// codes [n][ld] -> out [n][ld]: start + code * step, the product and the sum each rounded once in fp32 (no fma), then one rounding to OutT
template <typename OutT>
__global__ __launch_bounds__(256) void u8_dequant_rows_kernel(const uint8_t* __restrict__ codes, long n, int ld,
                                                              const float* __restrict__ start, const float* __restrict__ step,
                                                              OutT* __restrict__ out) {
    const long per_row = ld / 4, total = n * per_row;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / per_row;
        const int j0 = (int)(i - r * per_row) * 4;
        const uint32_t w = *reinterpret_cast<const uint32_t*>(codes + r * ld + j0);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(start[j0 + e], __fmul_rn((float)((w >> (8 * e)) & 0xffu), step[j0 + e]));
        OutT* o = out + r * ld + j0;
        if constexpr (sizeof(OutT) == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *reinterpret_cast<uint2*>(o) = make_uint2(Half<OutT>::pack2(v[0], v[1]), Half<OutT>::pack2(v[2], v[3]));
        }
    }
}

unsigned row_grid(long n, int ld) {
    const long blocks = (n * (ld / 4) + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

// ---- re-scoring of a candidate list from the codes (sgpt_u8_rescore; stage 2 of sgpt_score_topk_bits_u8) ----
// A candidate's value is <q, x^_n> = qbias + sum_j q'_j (code[n][j] - 128) with q'_j = q_j step_j and qbias = sum_j q_j mid_j: the form of
// the scorer above without the f16 rounding of q' and without its power-of-two scale, since no MFMA reads it -- everything is fp32.

// Query prologue, one workgroup per query: qs[r][j] = q_j * step_j (fp32, one rounding; zero in the pad columns d .. ld - 1) and
// qbias[r] as u8_prepare_queries_kernel sums it (thread t adds columns t, t + 256, ... in ascending order, the 256 partial sums are
// added in a fixed butterfly).  Once per call, not once per candidate.
__global__ __launch_bounds__(256) void u8_rescore_prepare_kernel(const float* __restrict__ q, const float* __restrict__ start,
                                                                 const float* __restrict__ step, int d, int ld, float* __restrict__ qs,
                                                                 float* __restrict__ qbias) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const float* row = q + (long)blockIdx.x * d;
    float* out = qs + (long)blockIdx.x * ld;
    float bias = 0.f;
    for (int j = t; j < ld; j += 256) {
        float v = 0.f;
        if (j < d) {
            const float st = step[j];
            v = __fmul_rn(row[j], st);
            bias = __fadd_rn(bias, __fmul_rn(row[j], __fadd_rn(start[j], __fmul_rn(128.0f, st))));
        }
        out[j] = v;
    }
    bias = wave_sum(bias);
    if ((t & 63) == 0) red[t >> 6] = bias;
    __syncthreads();
    if (t == 0) qbias[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// 16 codes of one 16-byte piece against the 16 q' values of the same columns: dword e of the piece feeds accumulator e, its bytes in
// ascending order.  code - 128 is exact however it is formed: the compiler takes the byte by an SDWA select, subtracts in integers and
// converts with v_cvt_f32_i32 (two instructions per code, as v_cvt_f32_ubyteN and a subtraction would be); the fmas pair up as v_pk_fma_f32.
__device__ __forceinline__ void u8_piece_fma(const uint4 w, const float (&qf)[16], float (&acc)[4]) {
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            acc[e] = __builtin_fmaf(qf[4 * e + b], (float)((ws[e] >> (8 * b)) & 0xffu) - 128.0f, acc[e]);
}

// The gather.  blockIdx.y = query, blockIdx.x = a group of 4 * CPW candidate slots; wave w of the workgroup serves slots
// 4 CPW blockIdx.x + w + 4 i, i < CPW.  A wave covers a row in rounds of 1024 columns: lane l owns the 16-byte piece l + 64 r of round r.
// Rows are ld-padded (pad codes 128, q' = 0 there), so the loop runs over ld / 16 whole pieces with no tail mask; at ld = 768 lanes
// 48 .. 63 idle in the only round.  q' of the first NR rounds sits in registers for all CPW candidates of the wave (NR * 16 floats per
// lane); rows wider than NR * 1024 columns re-read the rest of q' per candidate (any d is served; the register set covers d <= 2048).
// The CPW index loads, then the CPW * NR row loads, are issued back to back before the arithmetic: two memory latencies per wave.
// Order of the arithmetic, fixed by the slot alone (independent of nq, m and the launch shape): per lane four accumulators (one per
// dword of a piece) take their products by fma, columns ascending, rounds ascending; s = (a0 + a1) + (a2 + a3); the wave's 64 sums
// are added in the xor butterfly 32, 16, .., 1; value = s + qbias.  NaN -> -1.  A slot with idx < 0 or idx - idx_base outside [0, n_docs)
// -> (-inf, -1): no row is read for it.
template <int NR, int CPW>
__global__ __launch_bounds__(256) void u8_rescore_kernel(const float* __restrict__ qs, const float* __restrict__ qbias,
                                                         const uint8_t* __restrict__ codes, int ld, const int64_t* __restrict__ idx,
                                                         long ld_idx, int m, long idx_base, long n_docs, float* __restrict__ out_val,
                                                         int64_t* __restrict__ out_idx, long ld_out) {
    const int qi = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int np = ld >> 4;                                        // 16-byte pieces of a row
    const float* __restrict__ qrow = qs + (long)qi * ld;
    float qf[NR][16];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int p = lane + 64 * r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 v = p < np ? reinterpret_cast<const float4*>(qrow)[4 * p + e] : make_float4(0.f, 0.f, 0.f, 0.f);
            qf[r][4 * e + 0] = v.x; qf[r][4 * e + 1] = v.y; qf[r][4 * e + 2] = v.z; qf[r][4 * e + 3] = v.w;
        }
    }
    const float qb = qbias[qi];
    const int j0 = blockIdx.x * (4 * CPW) + wave;
    int64_t id[CPW];
    const uint4* row[CPW];
    uint4 w[CPW][NR];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int j = j0 + 4 * i;
        id[i] = j < m ? idx[(long)qi * ld_idx + j] : (int64_t)-1;
    }
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const long r = (long)(id[i] - idx_base);
        row[i] = id[i] >= 0 && r >= 0 && r < n_docs ? reinterpret_cast<const uint4*>(codes + r * ld) : nullptr;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int p = lane + 64 * rr;
            w[i][rr] = row[i] != nullptr && p < np ? row[i][p] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        }
    }
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int j = j0 + 4 * i;
        if (j >= m) break;                                         // (wave-uniform)
        float v = -INFINITY;
        if (row[i] != nullptr) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < NR; ++rr) u8_piece_fma(w[i][rr], qf[rr], acc);
            for (int p = lane + 64 * NR; p < np; p += 64) {        // (rows wider than the register set)
                float qx[16];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 t = reinterpret_cast<const float4*>(qrow)[4 * p + e];
                    qx[4 * e + 0] = t.x; qx[4 * e + 1] = t.y; qx[4 * e + 2] = t.z; qx[4 * e + 3] = t.w;
                }
                u8_piece_fma(row[i][p], qx, acc);
            }
            float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            s = wave_sum(s);
            s = s + qb;
            v = s != s ? -1.0f : s;
        }
        if (lane == 0) {
            out_val[(long)qi * ld_out + j] = v;
            out_idx[(long)qi * ld_out + j] = v > -INFINITY ? id[i] : (int64_t)-1;
        }
    }
}

}  // namespace

// 64 padded f16 query rows, any number of documents, rows of whole 128-code k-steps, 16-byte aligned code rows (the 16-byte loads)
bool score64u8_shape_ok(int M, long N, int K, const void* codes, long ldw) {
    return M == 64 && N > 0 && N <= 0x7fffff00L && K >= 128 && K % 128 == 0 && ((size_t)codes & 15) == 0 && ldw >= K && ldw % 16 == 0;
}

void launch_score64u8(int epi, const ScoreU8Args& a, hipStream_t s) {
    if (!score64u8_shape_ok(a.g.M, a.g.N, a.g.K, a.g.W, a.g.ldw) || (epi != EPI_SCORE && epi != EPI_SCORE_FILTER)) abort();
    launch_score64c<U8Codec>(epi, a, s);
}

void launch_u8_prepare_queries(const float* q, const float* start, const float* step, int nq, int d, int ld, void* qpad, float* qscale,
                               float* qbias, hipStream_t s) {
    hipLaunchKernelGGL(u8_prepare_queries_kernel, dim3(64), dim3(256), 0, s, q, start, step, nq, d, ld, static_cast<f16_t*>(qpad), qscale, qbias);
}

void launch_u8_col_minmax(const float* x, long n, int d, int accumulate, float* mn, float* mx, hipStream_t s) {
    hipLaunchKernelGGL(u8_col_minmax_kernel, dim3((d + 31) / 32), dim3(256), 0, s, x, n, d, accumulate, mn, mx);
}

void launch_u8_quant_rows(const float* x, long n, int d, int ld, const float* start, const float* step, uint8_t* codes, hipStream_t s) {
    hipLaunchKernelGGL(u8_quant_rows_kernel, dim3(row_grid(n, ld)), dim3(256), 0, s, x, n, d, ld, start, step, codes);
}

void launch_u8_dequant_rows(const uint8_t* codes, long n, int ld, const float* start, const float* step, void* out, int out_dtype,
                            hipStream_t s) {
    const unsigned grid = row_grid(n, ld);
    if (out_dtype == DT_BF16)
        hipLaunchKernelGGL(u8_dequant_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, codes, n, ld, start, step, static_cast<bf16_t*>(out));
    else if (out_dtype == DT_F16)
        hipLaunchKernelGGL(u8_dequant_rows_kernel<f16_t>, dim3(grid), dim3(256), 0, s, codes, n, ld, start, step, static_cast<f16_t*>(out));
    else
        hipLaunchKernelGGL(u8_dequant_rows_kernel<float>, dim3(grid), dim3(256), 0, s, codes, n, ld, start, step, static_cast<float*>(out));
}

void launch_u8_rescore_prepare(const float* q, const float* start, const float* step, int nq, int d, int ld, float* qs, float* qbias,
                               hipStream_t s) {
    hipLaunchKernelGGL(u8_rescore_prepare_kernel, dim3(nq), dim3(256), 0, s, q, start, step, d, ld, qs, qbias);
}

// qs / qbias: launch_u8_rescore_prepare's output for the same nq queries; ld % 128 == 0, codes 16-byte aligned (the 16-byte loads)
void launch_u8_rescore(const float* qs, const float* qbias, const uint8_t* codes, int ld, const int64_t* idx, long ld_idx, int nq, int m,
                       long idx_base, long n_docs, float* out_val, int64_t* out_idx, long ld_out, hipStream_t s) {
    if (ld < 128 || ld % 128 || ((size_t)codes & 15) || ((size_t)qs & 15) || nq <= 0 || m <= 0) abort();
    constexpr int CPW = 4;
    const unsigned gx = (unsigned)((m + 4 * CPW - 1) / (4 * CPW));
    for (int q0 = 0; q0 < nq; q0 += 32768) {         // (grid.y is a 16-bit count)
        const int gn = nq - q0 < 32768 ? nq - q0 : 32768;
        const auto kernel = ld <= 1024 ? u8_rescore_kernel<1, CPW> : u8_rescore_kernel<2, CPW>;
        hipLaunchKernelGGL(kernel, dim3(gx, gn), dim3(256), 0, s, qs + (long)q0 * ld, qbias + q0, codes, ld, idx + (long)q0 * ld_idx, ld_idx,
                           m, idx_base, n_docs, out_val + (long)q0 * ld_out, out_idx + (long)q0 * ld_out, ld_out);
    }
}
