// score64u8_kernel: the short-batch scorer tile of score8.hip (score64q8_kernel) over a corpus held as uint8 codes with one range per
// DIMENSION (sentence-transformers' precision="uint8"; the format of sgpt_u8_quantize_rows, include/sgpt_hip.h):
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
//
// Tile, staging and epilogues are score64q8_kernel's, statement for statement, with two differences besides the conversion: (a) no
// per-document scale; the two per-query-row values qscale / qbias are read once before the loop like the thresholds; (b) ANY number
// of documents: rows past N - 1 are fetched from row N - 1 (the look-ahead loads behind the last tile obey the same clamp), and their
// columns are dropped in both epilogues -- never stored, never appended -- so a ragged shard needs neither scratch nor a second launch.
#include "common.h"

namespace {

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

// 8 uint8 codes (k ascending from the low byte of c.x) -> 8 f16 values code - 128, exact
__device__ __forceinline__ uint32_t cvt_u8x2_f16(uint32_t w, uint32_t sel) {
    const h16x2 v = __builtin_bit_cast(h16x2, __builtin_amdgcn_perm(0x64006400u, w, sel)) - h16x2{(_Float16)1152.0f, (_Float16)1152.0f};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint4 cvt_u8x8_f16(const uint2 c) {
    uint4 r;
    r.x = cvt_u8x2_f16(c.x, 0x07010700u);     // bytes 0, 1 of the codes under byte 7 of the pair = 0x64
    r.y = cvt_u8x2_f16(c.x, 0x07030702u);     // bytes 2, 3
    r.z = cvt_u8x2_f16(c.y, 0x07010700u);
    r.w = cvt_u8x2_f16(c.y, 0x07030702u);
    return r;
}

constexpr int QCH = 16;       // 16-byte chunks per query row per k-step: 128 f16 elements

template <int EPI>
__global__ __launch_bounds__(512, 2) void score64u8_kernel(const ScoreU8Args a) {
    const GemmArgs& p = a.g;
    if (p.pred != nullptr && *p.pred == 0) return;
    __shared__ __attribute__((aligned(16))) uint4 lq[2][64 * QCH];                                   // 2 x 16 KiB of queries
    __shared__ __attribute__((aligned(16))) uint2 stage_all[EPI == EPI_SCORE_FILTER ? 8 * 256 : 1];   // filtered epilogue: 256 staged survivors per wave
    const int K = p.K, nk = K / 128, NT = (p.N + 255) / 256;      // (the last tile may be ragged)
    const long n_last = (long)p.N - 1;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const f16_t* __restrict__ Qg = static_cast<const f16_t*>(p.A);            // [64][K] (padded, pre-scaled query rows)
    const uint8_t* __restrict__ Dg = static_cast<const uint8_t*>(p.W);        // [N][ldw] codes (ldw in bytes: ld x the row stride)

    // this thread's two 16-byte pieces of a query k-step: rows t / 16 and 32 + t / 16, chunk t % 16
    const int qrow = t >> 4, qch = t & 15;
    const f16_t* qsrc = Qg + (long)qrow * p.lda + qch * 8;
    const int qdst = qrow * QCH + (qch ^ (qrow & 15));                         // (row + 32 has the same low four bits)
    auto load_q = [&](int kt, uint4& qa, uint4& qb) {
        qa = *reinterpret_cast<const uint4*>(qsrc + kt * 128);
        qb = *reinterpret_cast<const uint4*>(qsrc + 32 * p.lda + kt * 128);
    };
    auto store_q = [&](int buf, const uint4& qa, const uint4& qb) {
        lq[buf][qdst] = qa;
        lq[buf][qdst + 32 * QCH] = qb;
    };
    // this lane's 16-byte pieces of a document k-step: rows 32 w + 16 j + fr (clamped to the last document), two loads of 64 contiguous
    // bytes per row (h = 0, 1).  Lane group g takes bytes 64 h + 32 (g & 1) + 16 (g >> 1) .. + 15; frag() below trades halves between the
    // lane pairs (g, g ^ 1) so that every lane ends with its own chunk g of both slices (score8.hip has the picture).
    // (the clamp touches the last tile only: two byte offsets per row, picked by a workgroup-uniform test, so that the row address stays
    //  uniform base + lane offset as in the fp8 tile)
    long roff[2], roff_last[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long lr = wave * 32 + j * 16 + fr, last = n_last - (long)(NT - 1) * 256;
        roff[j] = lr * p.ldw + 32 * (g & 1) + 16 * (g >> 1);
        roff_last[j] = (lr < last ? lr : last) * p.ldw + 32 * (g & 1) + 16 * (g >> 1);
    }
    auto load_d = [&](int tile, int kt, uint4 (&d)[2][2]) {
        const uint8_t* base = Dg + (long)tile * 256 * p.ldw + kt * 128;
        const bool last_tile = tile == NT - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint8_t* row = base + (last_tile ? roff_last[j] : roff[j]);
#pragma unroll
            for (int h = 0; h < 2; ++h) d[j][h] = *reinterpret_cast<const uint4*>(row + h * 64);
        }
    };
    auto frag = [&](const uint4& v, int odd) {
        const auto rx = __builtin_amdgcn_permlane16_swap(v.x, v.z, false, false);
        const auto ry = __builtin_amdgcn_permlane16_swap(v.y, v.w, false, false);
        return cvt_u8x8_f16(make_uint2(rx[odd], ry[odd]));
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int tile = blockIdx.x;
    if (tile >= NT) return;
    // Two k-steps of document codes in flight behind the one being computed: three register sets whose roles rotate (score8.hip).
    // (pt, pk) = the position two steps ahead; behind the last tile it points at this workgroup's first tile again.
    auto adv = [&](int& tl, int& k2) { if (++k2 == nk) { k2 = 0; tl += gridDim.x; } };
    auto in_range = [&](int tl) { return tl < NT ? tl : (int)blockIdx.x; };
    // per query row of this lane, read once: the threshold (filtered epilogue) and the two values of the fma
    float thv[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    float qs[4], qb4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qs[i] = a.qscale[i * 16 + fr];
        qb4[i] = a.qbias[i * 16 + fr];
    }
    if constexpr (EPI == EPI_SCORE_FILTER) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i * 16 + fr < p.m_valid) thv[i] = p.thr[(long)(i * 16 + fr) * p.thr_ld];
    }
    uint4 dA[2][2], dB[2][2], dC[2][2];
    int kt = 0, pt = tile, pk = 0, buf = 0;
    {
        uint4 qa, qb;
        load_q(0, qa, qb);
        load_d(tile, 0, dA);
        adv(pt, pk);
        load_d(in_range(pt), pk, dB);
        adv(pt, pk);
        store_q(0, qa, qb);
        __syncthreads();
    }
    auto step = [&](const uint4 (&dc)[2][2], uint4 (&dn)[2][2]) __attribute__((always_inline)) {
        const long n0 = (long)tile * 256 + wave * 32;
        uint4 qa, qb;
        load_q(kt + 1 == nk ? 0 : kt + 1, qa, qb);
        load_d(in_range(pt), pk, dn);
        adv(pt, pk);
        const uint4* q_ = lq[buf];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            uint4 qf[4], df[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) df[j] = frag(dc[j][ks >> 1], ks & 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = i * 16 + fr;
                qf[i] = q_[row * QCH + ((4 * ks + g) ^ (row & 15))];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Half<f16_t>::mfma16(df[j], qf[i], acc[i][j]);   // document fragment = A-operand
        }
        store_q(buf ^ 1, qa, qb);          // the next step's queries (the readers of that buffer finished before the previous barrier)
        __syncthreads();
        buf ^= 1;
        if (kt + 1 == nk) {
            const long nleft = (long)p.N - n0 - 4 * g;
            const int nrem = nleft < 32 ? (int)nleft : 32;          // this lane's columns j * 16 + r < nrem exist (32: all of them)
            // back to the natural domain, once per tile: score = acc * qscale + qbias (one fma)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = __builtin_fmaf(acc[i][j][r], qs[i], qb4[i]);
                        // filtered epilogue: a column that does not exist is -inf, which beats no threshold (v > th is false for every th)
                        acc[i][j][r] = (EPI == EPI_SCORE_FILTER && j * 16 + r >= nrem) ? -INFINITY : v;
                    }
            // ---- epilogue, straight from the registers (score64_kernel's): lane = query row i*16 + fr, documents n0 + 16 j + 4 g .. + 3 ----
            if constexpr (EPI == EPI_SCORE_FILTER) {
                uint2_a* stage = reinterpret_cast<uint2_a*>(&stage_all[wave * 256]);
                int staged = 0;                                                // wave-uniform
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = i * 16 + fr;
                    const float th = thv[i];
                    float mx = -INFINITY;                                // fast reject on the accumulators
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[i][j][r]);
                    if (__ballot(th < -1.0f) != 0) {                      // thresholds below -1 (dot scores): the per-lane path, NaN -> -1 may survive
                        if ((mx > th || th < -1.0f) && cand_room(p.cand_cnt + m, p.cand_cap)) {
                            int c = 0;
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float v = acc[i][j][r];
                                    acc[i][j][r] = v != v ? -1.0f : v;
                                    c += acc[i][j][r] > th ? 1 : 0;
                                }
                            int slot = atomicAdd(p.cand_cnt + m, c);
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float v = acc[i][j][r];
                                    if (v > th) {
                                        if (slot < p.cand_cap) {
                                            p.cand_val[(long)m * p.cand_cap + slot] = v;
                                            p.cand_idx[(long)m * p.cand_cap + slot] = p.idx_base + n0 + j * 16 + 4 * g + r;
                                        }
                                        ++slot;
                                    }
                                }
                        }
                    } else if (__ballot(mx > th) != 0) {
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[i][j][r];
                                const bool sv = v > th;
                                const unsigned long long mask = __ballot(sv);
                                if (mask != 0) {
                                    if (sv) {
                                        const int pos = staged + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                                        if (pos < 256) stage[pos] = make_uint2((unsigned)(m << 16) | (unsigned)(j * 16 + 4 * g + r), __float_as_uint(v));
                                    }
                                    staged += __builtin_popcountll(mask);
                                }
                            }
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (staged > 0) {
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (staged <= 256) {                                       // one global round trip per flush
                        for (int e = lane; e < staged; e += 64) {
                            const uint2 ent = stage[e];
                            const int m = (int)(ent.x >> 16);
                            const int slot = atomicAdd(p.cand_cnt + m, 1);
                            if (slot < p.cand_cap) {
                                p.cand_val[(long)m * p.cand_cap + slot] = __uint_as_float(ent.y);
                                p.cand_idx[(long)m * p.cand_cap + slot] = p.idx_base + n0 + (int)(ent.x & 0xffffu);
                            }
                        }
                    } else if (lane == 0) {
                        atomicAdd(p.cand_cnt + (int)(stage[0].x >> 16), p.cand_cap + 1);   // more than the scratch holds: force the fallback
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = i * 16 + fr;
                    if (m < p.m_valid) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                            v.x = v.x != v.x ? -1.0f : v.x; v.y = v.y != v.y ? -1.0f : v.y;
                            v.z = v.z != v.z ? -1.0f : v.z; v.w = v.w != v.w ? -1.0f : v.w;
                            const long n = n0 + j * 16 + 4 * g;
                            float* o = static_cast<float*>(p.out) + (long)m * p.ldo + n;
                            if (n + 4 <= (long)p.N) *reinterpret_cast<float4*>(o) = v;
                            else {                                          // the ragged tile: the columns that exist, one by one
                                if (n < (long)p.N) o[0] = v.x;
                                if (n + 1 < (long)p.N) o[1] = v.y;
                                if (n + 2 < (long)p.N) o[2] = v.z;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        adv(tile, kt);
    };
    while (true) {         // block-uniform exits: every wave meets the same barriers
        step(dA, dC);
        if (tile >= NT) break;
        step(dB, dA);
        if (tile >= NT) break;
        step(dC, dB);
        if (tile >= NT) break;
    }
}

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

// code of one element by the rule of include/sgpt_hip.h: clamp(rint((x - start) / step), 0, 255) in fp32 (IEEE subtraction and
// division, round-half-even); step == 0, a NaN element or a NaN quotient give 128
__device__ __forceinline__ uint32_t u8_code(float x, float start, float step) {
    if (step == 0.f) return 128u;
    const float t = rintf(__fdiv_rn(__fsub_rn(x, start), step));
    if (t != t) return 128u;
    return (uint32_t)fminf(fmaxf(t, 0.f), 255.f);
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

}  // namespace

// 64 padded f16 query rows, any number of documents, rows of whole 128-code k-steps, 16-byte aligned code rows (the 16-byte loads)
bool score64u8_shape_ok(int M, long N, int K, const void* codes, long ldw) {
    return M == 64 && N > 0 && N <= 0x7fffff00L && K >= 128 && K % 128 == 0 && ((size_t)codes & 15) == 0 && ldw >= K && ldw % 16 == 0;
}

void launch_score64u8(int epi, const ScoreU8Args& a, hipStream_t s) {
    if (!score64u8_shape_ok(a.g.M, a.g.N, a.g.K, a.g.W, a.g.ldw) || (epi != EPI_SCORE && epi != EPI_SCORE_FILTER)) abort();
    static const int ncu = [] {
        int dev = 0, n = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n;
    }();
    const int NT = (a.g.N + 255) / 256;
    const int grid = NT < ncu ? NT : ncu;
    if (epi == EPI_SCORE) hipLaunchKernelGGL((score64u8_kernel<EPI_SCORE>), dim3(grid), dim3(512), 0, s, a);
    else hipLaunchKernelGGL((score64u8_kernel<EPI_SCORE_FILTER>), dim3(grid), dim3(512), 0, s, a);
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
