// scorebits_kernel: the Hamming tile of the binary corpus (sgpt_score_topk_bits).  A document is a row of packed sign bits, `ldw` bytes
// apart (96 bytes at d = 768: 1/16 of an f16 row), a query a row of the same format; the score of a pair is the agreement
//     a = d - 2 * popcount(q ^ doc) = <sign q, sign doc>   (signs +-1; pad bits are zero on both sides and cancel),
// an integer in [-d, d], handed to the two scorer epilogues as an exact fp32 value: EPI_SCORE stores out[m][n], EPI_SCORE_FILTER
// appends (a, index) of every a > thr[m] to query m's candidate list (score64_kernel's contracts, so score_topk_impl's schedule,
// select, merge and predicated overflow fallback serve unchanged).
//
// Ownership: a LANE owns a document; its row sits in registers as NP pieces of VEC dwords while the queries pass over it.
// Two ways the row gets there:
//   COAL (consecutive tight rows, ldw == ldb == 16 NP, NP in {1, 2, 3, 4, 6, 8}): a tile of 256 rows is 4 NP KiB of contiguous memory.
//     The workgroup loads it with 16-byte loads whose 64 lanes cover 1 KiB of consecutive addresses, NP per lane, all issued back to
//     back and for the NEXT tile before the current one is scored, so that they are in flight behind the arithmetic (the stream rate
//     is set by bytes in flight, not by the path they take: profiles/r06_dma_stream_probe.txt, header of score8.hip).  The pieces are
//     written to LDS as they are (4 NP KiB per workgroup) and every lane reads its own row back: two barriers per tile.
//   direct (everything else: strided samples, rows with slack, dword rows, rows wider than 8 pieces): every lane loads its own row
//     from global memory, the next tile's before the current one is scored.  One instruction then touches 16 bytes of up to 64
//     different cache lines, so this path depends on the caches keeping those lines for the row's other pieces;
//     profiles/score_bits_corpus.txt, variant A, has whole 16 M-document passes on it (9.1 ms at nq = 1 against 0.38 ms as committed).
// The queries are wave-uniform: the loop over m reads the packed query row through uniform addresses (scalar loads into SGPRs; the
// 6 KiB of 64 queries stay in the scalar cache), so per (query, dword) the VALU issues one XOR and one population count
// (v_bcnt_u32_b32).  No MFMA.  LDS holds the COAL tile and, in the filtered epilogue, the 64 thresholds (read once: a global load of a
// threshold inside the loop would be the youngest vector load in flight and drain the prefetched rows).  Rows wider than NP pieces
// keep the first NP in registers and re-read the rest per query: any d is served, speed is claimed for d % 128 == 0 up to 1024.
// Documents [N, 256 * tiles) of the last tile do not exist: their lanes read the last valid row (piece) and store nothing.
#include "common.h"

namespace {

template <int VEC> struct BitPiece;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));    // (a native vector: arrays of HIP's uint4 struct went through scratch here)
template <> struct BitPiece<4> { using type = u32x4_t; };
template <> struct BitPiece<1> { using type = uint32_t; };

__device__ __forceinline__ int xor_pop(const u32x4_t x, const uint32_t* __restrict__ q, int h) {
    h += __builtin_popcount(x.x ^ q[0]);
    h += __builtin_popcount(x.y ^ q[1]);
    h += __builtin_popcount(x.z ^ q[2]);
    h += __builtin_popcount(x.w ^ q[3]);
    return h;
}
__device__ __forceinline__ int xor_pop(const uint32_t x, const uint32_t* __restrict__ q, int h) { return h + __builtin_popcount(x ^ q[0]); }

// Q: packed query rows [m_valid][qw] dwords (qw >= np * VEC, pad dwords zero); D: document rows, p.ldw BYTES apart; np: pieces per row.
// EXACT: np == NP, known at compile time -- the loop over a row's pieces is then branch-free, and a query's dwords arrive in a few
// wide scalar loads behind ONE wait (with a run-time np every piece is a uniform branch around its own scalar load and wait).
// COAL (EXACT, VEC == 4, p.ldw == 16 NP): tiles staged through LDS by coalesced loads, see above.
template <int EPI, int VEC, int NP, bool EXACT, bool COAL>
__global__ __launch_bounds__(256) void scorebits_kernel(const GemmArgs p, const uint32_t* __restrict__ Q, const char* __restrict__ D,
                                                        const int d, const int qw, const int np, const int spread) {
    using P = typename BitPiece<VEC>::type;
    if (p.pred != nullptr && *p.pred == 0) return;
    const long N = p.N, ntiles = (N + 255) / 256;
    const int nq = p.m_valid;
    auto row_of = [&](long tile) {
        long n = tile * 256 + threadIdx.x;
        if (n >= N) n = N - 1;
        return reinterpret_cast<const P*>(D + n * p.ldw);
    };
    auto load_row = [&](const P* __restrict__ row, P (&r)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) r[i] = row[EXACT || i < np ? i : 0];
    };
    long tile = blockIdx.x;
    if (tile >= ntiles) return;
    // the thresholds (at most 64 queries): nothing writes them while the launch runs, so they are read once, into LDS -- a global
    // load in the loop below would be the youngest vector load in flight, and waiting for it drains the prefetched rows
    __shared__ float thr_s[EPI == EPI_SCORE_FILTER ? 64 : 1];
    if constexpr (EPI == EPI_SCORE_FILTER) {
        if ((int)threadIdx.x < nq) thr_s[threadIdx.x] = p.thr[(long)threadIdx.x * p.thr_ld];
        __syncthreads();
    }
    P cur[NP], nxt[NP];
    __shared__ __attribute__((aligned(16))) P lds_tile[COAL ? 256 * NP : 1];
    // COAL: piece j of this thread = 16-byte piece threadIdx.x + 256 j of the tile (pieces behind the last row: the last one)
    auto load_tile = [&](long tl, P (&r)[NP]) {
        const long last = N * NP - 1;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            long i = tl * (256L * NP) + threadIdx.x + 256 * j;
            r[j] = reinterpret_cast<const P*>(D)[i < last ? i : last];
        }
    };
    auto through_lds = [&](P (&r)[NP], P (&own)[NP]) __attribute__((always_inline)) {
        __syncthreads();                                            // every lane has read its row of the previous tile
#pragma unroll
        for (int j = 0; j < NP; ++j) lds_tile[threadIdx.x + 256 * j] = r[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j) own[j] = lds_tile[threadIdx.x * NP + j];
    };
    if constexpr (COAL) {
        load_tile(tile, nxt);
        through_lds(nxt, cur);
    } else {
        load_row(row_of(tile), cur);
    }
    for (; tile < ntiles; tile += gridDim.x) {
        const long ahead = tile + gridDim.x;
        // the next tile, in flight under this tile's arithmetic
        if constexpr (COAL) load_tile(ahead < ntiles ? ahead : tile, nxt);
        else load_row(row_of(ahead < ntiles ? ahead : tile), nxt);
        const long n = tile * 256 + threadIdx.x;
        const bool live = n < N;
        const P* __restrict__ row = row_of(tile);
#pragma unroll 2
        for (int m = 0; m < nq; ++m) {
            const uint32_t* __restrict__ qr = Q + (long)m * qw;
            int h = 0;
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (EXACT || i < np) h = xor_pop(cur[i], qr + i * VEC, h);
            if constexpr (!EXACT)
                for (int i = NP; i < np; ++i) h = xor_pop(row[i], qr + i * VEC, h);   // (rows wider than the register set)
            float v = (float)(d - 2 * h);
            if constexpr (EPI == EPI_SCORE) {
                // spread (the schedule's threshold sample): a - frac, frac = 12 low bits of the column / 4096, exact in fp32.  The order
                // of the agreements is kept (they differ by 2 or more), the k-th best v has ceil(v) = the k-th best a, so the
                // inclusive threshold one ulp below it still admits exactly a >= that a -- and the select over the sample meets
                // 4096 times fewer equal keys (profiles/score_bits_corpus.txt, variant B: 16 M-document passes without this and without the sample bound)
                if (spread) v -= (float)(n & 4095) * (1.0f / 4096.0f);
            }
            if constexpr (EPI == EPI_SCORE_FILTER) {
                if (live && v > thr_s[m] && cand_room(p.cand_cnt + m, p.cand_cap)) {
                    const int slot = atomicAdd(p.cand_cnt + m, 1);
                    if (slot < p.cand_cap) {
                        p.cand_val[(long)m * p.cand_cap + slot] = v;
                        p.cand_idx[(long)m * p.cand_cap + slot] = p.idx_base + n;
                    }
                }
            } else {
                if (live) static_cast<float*>(p.out)[(long)m * p.ldo + n] = v;
            }
        }
        if constexpr (COAL) {
            through_lds(nxt, cur);                                  // (block-uniform loop: every thread meets the barriers)
        } else {
#pragma unroll
            for (int i = 0; i < NP; ++i) cur[i] = nxt[i];
        }
    }
}

template <int EPI, int VEC, int NP, bool EXACT, bool COAL = false>
void launch_one(const GemmArgs& a, int d, int qw, int np, int grid, int spread, hipStream_t s) {
    hipLaunchKernelGGL((scorebits_kernel<EPI, VEC, NP, EXACT, COAL>), dim3(grid), dim3(256), 0, s, a, static_cast<const uint32_t*>(a.A),
                       static_cast<const char*>(a.W), d, qw, np, spread);
}

template <int EPI, int NP>
void launch_exact(const GemmArgs& a, int d, int qw, int grid, int spread, hipStream_t s) {
    if (a.ldw == 16L * NP) launch_one<EPI, 4, NP, true, true>(a, d, qw, NP, grid, spread, s);     // consecutive tight rows: coalesced tiles
    else launch_one<EPI, 4, NP, true, false>(a, d, qw, NP, grid, spread, s);
}

template <int EPI>
void launch_epi(const GemmArgs& a, int d, int qw, bool vec, int grid, int spread, hipStream_t s) {
    const int words = (d + 31) / 32;
    if (vec) {
        const int np = (words + 3) / 4;
        if (np == 1) launch_exact<EPI, 1>(a, d, qw, grid, spread, s);             // d <= 128
        else if (np == 2) launch_exact<EPI, 2>(a, d, qw, grid, spread, s);        // 256
        else if (np == 3) launch_exact<EPI, 3>(a, d, qw, grid, spread, s);        // 384
        else if (np == 4) launch_exact<EPI, 4>(a, d, qw, grid, spread, s);        // 512
        else if (np == 6) launch_exact<EPI, 6>(a, d, qw, grid, spread, s);        // 768
        else if (np == 8) launch_exact<EPI, 8>(a, d, qw, grid, spread, s);        // 1024
        else launch_one<EPI, 4, 8, false>(a, d, qw, np, grid, spread, s);
    } else {
        if (words <= 4) launch_one<EPI, 1, 4, false>(a, d, qw, words, grid, spread, s);
        else launch_one<EPI, 1, 24, false>(a, d, qw, words, grid, spread, s);
    }
}

}  // namespace

// a.A: packed query rows (a.m_valid of them, qw dwords apart, zero behind ceil(d / 32) dwords up to a multiple of four); a.W / a.ldw:
// document rows and their stride in bytes (a strided sample: ldb x the stride); ldb: the bytes a row owns, ldb % 4 == 0 and
// ldb >= 4 * ceil(d / 32); a.N documents, all of them bounds-checked (no tile rounding).  epi = EPI_SCORE | EPI_SCORE_FILTER.
// spread (EPI_SCORE): scores of a threshold sample, a - (column & 4095) / 4096 (see the kernel).
void launch_scorebits(int epi, const GemmArgs& a, int d, int qw, long ldb, hipStream_t s, bool spread) {
    const int words = (d + 31) / 32;
    if ((epi != EPI_SCORE && epi != EPI_SCORE_FILTER) || (epi == EPI_SCORE_FILTER && a.m_valid > 64) || a.N <= 0 || a.m_valid <= 0 || d <= 0 || ldb % 4 || ldb < 4L * words ||
        a.ldw < ldb || a.ldw % ldb || qw < (words + 3) / 4 * 4 || ((size_t)a.W & 3))
        abort();
    const int ncu = device_cu_count();
    // 16-byte loads need 16-byte aligned rows that own whole pieces (a row of ldb % 16 == 0 bytes ends behind its last piece)
    const bool vec = ldb % 16 == 0 && ((size_t)a.W & 15) == 0;
    const long ntiles = ((long)a.N + 255) / 256;
    const int grid = (int)(ntiles < 8L * ncu ? ntiles : 8L * ncu);
    if (epi == EPI_SCORE) launch_epi<EPI_SCORE>(a, d, qw, vec, grid, spread ? 1 : 0, s);
    else launch_epi<EPI_SCORE_FILTER>(a, d, qw, vec, grid, 0, s);
}
