// score64c_kernel: the short-batch scorer tile (score64_kernel, gemm.hip) over a corpus of ONE-BYTE codes, [N][ldw] bytes.  The search
// pass at nq <= 64 is HBM-bound on the corpus stream; a code is one byte where an f16 element is two.  The formats (e4m3 with one scale
// per document: score8.hip; uint8 with one range per dimension: scoreu8.hip) differ in a Codec, everything else is here.
//
// Tile and ownership as score64_kernel: 64 padded f16 query rows x 256 documents per workgroup, persistent over tiles; wave w owns
// documents 32 w .. 32 w + 31 for all 64 queries (acc[4][2], 16 MFMAs per 32-wide k slice); a lane ends with one query row and 4
// consecutive documents per fragment, and the epilogue is score64_kernel's (score64_epilogue.h).  Codes are converted to f16 in
// registers and feed the same v_mfma_f32_16x16x32_f16 as the f16 scorer, in the same k order (slices of 32, ascending; lane group g
// holds k = 32 s + 8 g .. + 7 of slice s).
//
// A Codec supplies
//   Args                 the launch descriptor: a GemmArgs g (g.A = 64 padded f16 query rows, g.W = the codes) plus the format's own pointers
//   kRagged              may the last tile reach past document N - 1?  true: NT = ceil(N / 256), rows past N - 1 are fetched from row
//                        N - 1 (the look-ahead loads behind the last tile obey the same clamp) and their columns are dropped in both
//                        epilogues -- never stored, never appended.  false: N is a multiple of 256 and the clamp's registers do not exist.
//   cvt(uint2) -> uint4  8 codes (k ascending from the low byte of c.x) -> 8 f16 values
//   Lane                 per-lane state with three hooks:
//     before_loop(a, fr)      once before the loop: what belongs to this lane's query rows 16 i + fr
//     tile_begin(a, n0, g)    at a tile's first k-step, BEFORE the step's other loads: what belongs to this lane's documents
//                             n0 + 16 j + 4 g + r (the wait for the queries at the step's end then covers these loads, and the epilogue
//                             finds them landed without draining the document loads in flight).  The tile does NOT clamp these
//                             indices: a codec with kRagged = true that reads per-document data here must clamp to N - 1 itself
//     finish(acc, i, j, r)    at the tile's last step: accumulator -> score, in fp32
//
// Staging: REGISTER-staged, no LDS-DMA ring for the documents.  The MFMA A-fragment of a lane is 8 consecutive codes of one row, so
// the document bytes can go from global memory to where the conversion wants them without touching the LDS (the DMA ring of
// score64_kernel moves 16 B per lane; byte rows would use half its LDS write width and be read back as 8-byte fragments).
// profiles/r06_score64_register_ab.txt has the register-staged f16 tile within a few per cent of the DMA ring, and
// profiles/r06_dma_stream_probe.txt shows the stream rate is set by bytes in flight, not by the path they take; here a wave keeps two
// 128-element k-steps (8 KiB of codes) in flight behind the one it computes (three register sets, roles rotating): 64 KiB per CU
// outstanding with one workgroup per CU.  Loads are 16 bytes per lane, 64 contiguous bytes per row and instruction, and a
// v_permlane16_swap pair sorts the halves into fragments (load_d / frag below).  Measured on an MI355X, fp8 codes, 1 M x 768, nq = 16,
// whole search pass (profiles/score_fp8_corpus.txt has the final numbers): 8-byte loads of a lane's own fragment (32 bytes per row and
// instruction) 0.296 ms, the same with the non-temporal hint 0.376 ms, 16-byte loads + swap 0.253 ms, with the hint 0.267 ms; the f16
// pass 0.336 ms.  Plain loads it is: the four instructions that share a 128-byte line want it kept in the vector L1.
// Plain C++ loads throughout: the compiler counts them (no hand-written waitcnt to get wrong).  Queries stay f16 in LDS: 64 rows x 128
// elements per k-step, double-buffered (2 x 16 KiB), loaded through registers by all 512 threads, one barrier per k-step; LDS rows
// are XOR-swizzled at 16-byte granularity (chunk ^= row & 15) so the 16 rows of a fragment read hit 16 different bank groups.
#pragma once
#include "common.h"
#include "score64_epilogue.h"

template <typename Codec, int EPI>
__global__ __launch_bounds__(512, 2) void score64c_kernel(const typename Codec::Args a) {
    constexpr int QCH = 16;       // 16-byte chunks per query row per k-step: 128 f16 elements
    constexpr bool RAGGED = Codec::kRagged;
    const GemmArgs& p = a.g;
    if (p.pred != nullptr && *p.pred == 0) return;
    __shared__ __attribute__((aligned(16))) uint4 lq[2][64 * QCH];                                   // 2 x 16 KiB of queries
    __shared__ __attribute__((aligned(16))) uint2 stage_all[EPI == EPI_SCORE_FILTER ? 8 * 256 : 1];   // filtered epilogue: 256 staged survivors per wave
    const int K = p.K, nk = K / 128, NT = RAGGED ? (p.N + 255) / 256 : p.N / 256;
    [[maybe_unused]] const long n_last = (long)p.N - 1;                      // (RAGGED)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const f16_t* __restrict__ Qg = static_cast<const f16_t*>(p.A);            // [64][K] (padded query rows)
    const uint8_t* __restrict__ Dg = static_cast<const uint8_t*>(p.W);        // [N][ldw] codes (ldw in bytes)

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
    // this lane's 16-byte pieces of a document k-step: rows 32 w + 16 j + fr, two loads of 64 contiguous bytes per row (h = 0, 1).
    // Lane group g takes bytes 64 h + 32 (g & 1) + 16 (g >> 1) .. + 15: groups 0 and 2 hold chunks (0, 1) and (2, 3) of slice 2 h,
    // groups 1 and 3 the same chunks of slice 2 h + 1 (a chunk = the 8 codes one lane feeds one MFMA); frag() below trades halves
    // between the lane pairs (g, g ^ 1) so that every lane ends with its own chunk g of both slices.
    // Whole tiles: the row address is computed per load from the tile index.  RAGGED: the clamp to the last document touches the last
    // tile only -- two byte offsets per row, kept over the loop and picked by a workgroup-uniform test, so that the row address stays
    // uniform base + lane offset.  (Two forms on purpose: whole tiles on the kept offsets measured 1.1 - 1.4 % slower on the fp8 pass
    // at nq = 64, 1 M x 768, profiles/score64_tile_refactor.txt.)
    [[maybe_unused]] long roff[2], roff_last[2];
    if constexpr (RAGGED) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long lr = wave * 32 + j * 16 + fr, last = n_last - (long)(NT - 1) * 256;
            roff[j] = lr * p.ldw + 32 * (g & 1) + 16 * (g >> 1);
            roff_last[j] = (lr < last ? lr : last) * p.ldw + 32 * (g & 1) + 16 * (g >> 1);
        }
    }
    auto load_d = [&](int tile, int kt, uint4 (&d)[2][2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint8_t* row;
            if constexpr (RAGGED) row = Dg + (long)tile * 256 * p.ldw + kt * 128 + (tile == NT - 1 ? roff_last[j] : roff[j]);
            else row = Dg + ((long)tile * 256 + wave * 32 + j * 16 + fr) * p.ldw + kt * 128 + 32 * (g & 1) + 16 * (g >> 1);
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
        return Codec::cvt(make_uint2(rx[odd], ry[odd]));
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
    typename Codec::Lane cl;
    cl.before_loop(a, fr);
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
    auto step = [&](const uint4 (&dc)[2][2], uint4 (&dn)[2][2]) __attribute__((always_inline)) {
        const long n0 = (long)tile * 256 + wave * 32;
        if (kt == 0) cl.tile_begin(a, n0, g);
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
            // accumulators -> scores, once per tile; on the filtered leg a column that does not exist becomes -inf (score64_epilogue.h)
            int nrem = 32;                                           // this lane's columns j * 16 + r < nrem exist (32: all of them)
            if constexpr (RAGGED && EPI == EPI_SCORE_FILTER) {
                const long nleft = (long)p.N - n0 - 4 * g;
                nrem = nleft < 32 ? (int)nleft : 32;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = cl.finish(acc[i][j][r], i, j, r);
                        acc[i][j][r] = j * 16 + r >= nrem ? -INFINITY : v;
                    }
            score64_epilogue<EPI, RAGGED>(p, acc, thv, n0, g, fr, lane,
                                          reinterpret_cast<uint2_a*>(stage_all) + (EPI == EPI_SCORE_FILTER ? wave * 256 : 0));
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

// one workgroup per CU, persistent over the tiles; the caller has checked the shape
template <typename Codec>
void launch_score64c(int epi, const typename Codec::Args& a, hipStream_t s) {
    const int NT = Codec::kRagged ? (a.g.N + 255) / 256 : a.g.N / 256;
    const int ncu = device_cu_count();
    const int grid = NT < ncu ? NT : ncu;
    if (epi == EPI_SCORE) hipLaunchKernelGGL((score64c_kernel<Codec, EPI_SCORE>), dim3(grid), dim3(512), 0, s, a);
    else hipLaunchKernelGGL((score64c_kernel<Codec, EPI_SCORE_FILTER>), dim3(grid), dim3(512), 0, s, a);
}
