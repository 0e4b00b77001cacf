// score64q8_kernel: the short-batch scorer tile (score64_kernel, gemm.hip) over a corpus held as OCP e4m3fn codes [N][d] bytes
// with one power-of-two fp32 scale per document (the format of sgpt_fp8_quantize_rows).  The search pass at nq <= 64 is
// HBM-bound on the corpus stream; a code is one byte where an f16 element is two.
//
// Tile and ownership as score64_kernel: 64 padded f16 query rows x 256 documents per workgroup, persistent over tiles; wave w owns
// documents 32 w .. 32 w + 31 for all 64 queries (acc[4][2], 16 MFMAs per 32-wide k slice); a lane ends with one query row and 4
// consecutive documents per fragment.  The epilogues (EPI_SCORE, EPI_SCORE_FILTER) are score64_kernel's, statement for statement.
//
// Arithmetic.  Every e4m3 value is an f16 value (4 exponent bits, 3 mantissa bits, |v| <= 448, smallest subnormal 2^-9 -- a NORMAL
// f16), so codes are converted in registers by the hardware conversions e4m3 -> f32 -> f16 (v_cvt_pk_f32_fp8, v_cvt_pkrtz_f16_f32:
// both exact here) and feed the same v_mfma_f32_16x16x32_f16 as the f16 scorer, in the same k order (slices of 32, ascending; lane
// group g holds k = 32 s + 8 g .. + 7 of slice s).  The arithmetic conversion rather than the bit move (b & 0x80) << 8 | (b & 0x7f) << 7:
// it is two instructions per code pair where the bit move is four or five, it keeps the operands clear of f16 subnormals, and the
// NaN codes 0x7f / 0xff become NaN without a test (NaN score -> -1 in the epilogue, as the f16 scorer).  The document's scale
// multiplies the fp32 accumulators once per tile: a power of two, so the product is exactly the accumulator the f16 scorer reaches
// on the de-quantised row (code * scale in f16) as long as nothing under- or overflows -- scores are comparable bit for bit.
//
// Staging: REGISTER-staged, no LDS-DMA ring for the documents.  The MFMA A-fragment of a lane is 8 consecutive codes of one row, so
// the document bytes can go from global memory to where the conversion wants them without touching the LDS (the DMA ring of
// score64_kernel moves 16 B per lane; byte rows would use half its LDS write width and be read back as 8-byte fragments).
// profiles/r06_score64_register_ab.txt has the register-staged f16 tile within a few per cent of the DMA ring, and
// profiles/r06_dma_stream_probe.txt shows the stream rate is set by bytes in flight, not by the path they take; here a wave keeps two
// 128-element k-steps (8 KiB of codes) in flight behind the one it computes (three register sets, roles rotating): 64 KiB per CU
// outstanding with one workgroup per CU.  Loads are 16 bytes per lane, 64 contiguous bytes per row and instruction, and a
// v_permlane16_swap pair sorts the halves into fragments (load_d / frag below).  Measured on an MI355X, 1 M x 768, nq = 16, whole
// search pass (profiles/score_fp8_corpus.txt has the final numbers): 8-byte loads of a lane's own fragment (32 bytes per row and
// instruction) 0.296 ms, the same with the non-temporal hint 0.376 ms, 16-byte loads + swap 0.253 ms, with the hint 0.267 ms; the f16
// pass 0.336 ms.  Plain loads it is: the four instructions that share a 128-byte line want it kept in the vector L1.
// Plain C++ loads throughout: the compiler counts them (no hand-written waitcnt to get wrong).  Queries stay f16 in LDS: 64 rows x 128
// elements per k-step, double-buffered (2 x 16 KiB), loaded through registers by all 512 threads, one barrier per k-step; LDS rows
// are XOR-swizzled at 16-byte granularity (chunk ^= row & 15) so the 16 rows of a fragment read hit 16 different bank groups.
#include "common.h"

namespace {

// 8 e4m3fn codes (k ascending from the low byte of c.x) -> 8 f16, exact; NaN codes -> NaN
__device__ __forceinline__ uint4 cvt_e4m3x8_f16(const uint2 c) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
    const f32x2_t e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), f = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
    uint4 r;
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a[0], a[1]));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(b[0], b[1]));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(e[0], e[1]));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f[0], f[1]));
    return r;
}

constexpr int QCH = 16;       // 16-byte chunks per query row per k-step: 128 f16 elements

template <int EPI>
__global__ __launch_bounds__(512, 2) void score64q8_kernel(const Score8Args a) {
    const GemmArgs& p = a.g;
    if (p.pred != nullptr && *p.pred == 0) return;
    __shared__ __attribute__((aligned(16))) uint4 lq[2][64 * QCH];                                   // 2 x 16 KiB of queries
    __shared__ __attribute__((aligned(16))) uint2 stage_all[EPI == EPI_SCORE_FILTER ? 8 * 256 : 1];   // filtered epilogue: 256 staged survivors per wave
    const int K = p.K, nk = K / 128, NT = p.N / 256;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const f16_t* __restrict__ Qg = static_cast<const f16_t*>(p.A);            // [64][K] (padded query rows)
    const uint8_t* __restrict__ Dg = static_cast<const uint8_t*>(p.W);        // [N][ldw] codes (ldw in bytes: d x the row stride)

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
    // this lane's A-fragments of a document k-step: rows 32 w + 16 j + fr, codes 32 s + 8 g .. + 7 of the four 32-wide slices
    // this lane's 16-byte pieces of a document k-step: rows 32 w + 16 j + fr, two loads of 64 contiguous bytes per row (h = 0, 1).
    // Lane group g takes bytes 64 h + 32 (g & 1) + 16 (g >> 1) .. + 15: groups 0 and 2 hold chunks (0, 1) and (2, 3) of slice 2 h,
    // groups 1 and 3 the same chunks of slice 2 h + 1 (a chunk = the 8 codes one lane feeds one MFMA); frag() below trades halves
    // between the lane pairs (g, g ^ 1) so that every lane ends with its own chunk g of both slices.
    auto load_d = [&](int tile, int kt, uint4 (&d)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint8_t* row = Dg + ((long)tile * 256 + wave * 32 + j * 16 + fr) * p.ldw + kt * 128 + 32 * (g & 1) + 16 * (g >> 1);
#pragma unroll
            for (int h = 0; h < 2; ++h) d[j][h] = *reinterpret_cast<const uint4*>(row + h * 64);
        }
    };
    // v_permlane16_swap trades the odd 16-lane rows of its first operand with the even rows of its second: with (low, high) halves of
    // the loaded 16 bytes, result 0 is chunk g of slice 2 h on every lane (even g: its own low half; odd g: the partner's high half)
    // and result 1 chunk g of slice 2 h + 1 (even g: the partner's low half; odd g: its own high half).
    auto frag = [&](const uint4& v, int odd) {
        const auto rx = __builtin_amdgcn_permlane16_swap(v.x, v.z, false, false);
        const auto ry = __builtin_amdgcn_permlane16_swap(v.y, v.w, false, false);
        return cvt_e4m3x8_f16(make_uint2(rx[odd], ry[odd]));
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int tile = blockIdx.x;
    if (tile >= NT) return;
    // The workgroup walks its sequence of (tile, k-step) positions with TWO k-steps of document codes in flight behind the one being
    // computed: three register sets whose roles rotate (the step loop is unrolled by three, so no set is ever copied -- a copy would
    // wait for the load it copies).  (pt, pk) = the position two steps ahead; behind the last tile it points at this workgroup's first
    // tile again: valid addresses whose data nobody reads.  The queries of the next step are loaded first in each step and stored to
    // the other LDS buffer at its end: the wait for them (in-order counter) leaves the step's document loads outstanding.
    auto adv = [&](int& tl, int& k2) { if (++k2 == nk) { k2 = 0; tl += gridDim.x; } };
    auto in_range = [&](int tl) { return tl < NT ? tl : (int)blockIdx.x; };
    // the thresholds of this lane's four query rows: nothing writes them while the launch runs, so they are read once here -- a
    // load in the epilogue would be the youngest in flight, and waiting for it would drain the document stream once per tile
    float thv[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
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
    float sc[2][4];                                        // this lane's 8 documents' scales (loaded at a tile's first step, used in its epilogue)
    auto step = [&](const uint4 (&dc)[2][2], uint4 (&dn)[2][2]) __attribute__((always_inline)) {
        const long n0 = (long)tile * 256 + wave * 32;
        if (kt == 0) {      // (issued BEFORE the step's other loads: the wait for the queries at the step's end then covers them, and the
                            //  epilogue finds them landed without draining the document loads in flight)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[j][r] = a.scale[(n0 + j * 16 + 4 * g + r) * a.scale_stride];
        }
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
            // the per-document scale, once per tile: a power of two on the fp32 accumulators
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][j][r] *= sc[j][r];
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
                            *reinterpret_cast<float4*>(static_cast<float*>(p.out) + (long)m * p.ldo + n0 + j * 16 + 4 * g) = v;
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

}  // namespace

// 64 padded f16 query rows, whole 256-document tiles, d a multiple of the 128-element k-step, 8-byte aligned code rows
bool score64q8_shape_ok(int M, long N, int K, const void* codes, long ldw) {
    return M == 64 && N > 0 && N % 256 == 0 && K >= 128 && K % 128 == 0 && ((size_t)codes & 7) == 0 && ldw % 8 == 0;
}

void launch_score64q8(int epi, const Score8Args& a, hipStream_t s) {
    if (!score64q8_shape_ok(a.g.M, a.g.N, a.g.K, a.g.W, a.g.ldw) || (epi != EPI_SCORE && epi != EPI_SCORE_FILTER)) abort();
    static const int ncu = [] {
        int dev = 0, n = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n;
    }();
    const int NT = a.g.N / 256;
    const int grid = NT < ncu ? NT : ncu;
    if (epi == EPI_SCORE) hipLaunchKernelGGL((score64q8_kernel<EPI_SCORE>), dim3(grid), dim3(512), 0, s, a);
    else hipLaunchKernelGGL((score64q8_kernel<EPI_SCORE_FILTER>), dim3(grid), dim3(512), 0, s, a);
}
