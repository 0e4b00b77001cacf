// IVF corpus (include/sgpt_hip.h: sgpt_ivf_lists, sgpt_ivf_centroids, sgpt_gather_rows, sgpt_ivf_search; over uint8 lists
// sgpt_u8_gather_quantize_rows, sgpt_ivf_search_u8): inverted lists over spherical k-means centroids, built and probed on the device.
//
// sgpt_ivf_lists -- the keys (list << 32 | row) are unique; the bitonic network of sort64.h sorts them ascending, which IS the stable
//   argsort of the assignment: perm = the low words, offsets[c] = the first sorted position whose key is >= c << 32.  Integers only.
// sgpt_ivf_centroids -- store-and-sum: a list is cut into chunks of IVF_SUM_ROWS rows counted from ITS first row; one wavefront per chunk
//   adds the chunk's rows in ascending order into a partial row of fp32 sums (lane l owns the 8-column pieces l, l + 64, ...: no two
//   lanes share a column, no atomics), one workgroup per list adds the list's partials in chunk order.  A long list is many chunks, so it
//   spreads over the chip; which chunk a wavefront serves comes from an exclusive scan of the lists' chunk counts (one small launch), not
//   from the host.  The order of every addition depends on the list's own rows alone.
// sgpt_ivf_search -- stage 1 is sgpt_score_topk(SGPT_F16) of the f16 queries against the f16 centroids; stage 2 (ivf_scan_kernel) is one
//   workgroup per (query, probed list, chunk of SGPT_IVF_CHUNK rows): the query in registers, each of the four wavefronts walks 64 rows in
//   16-byte pieces, the chunk's (score, position) keys are sorted in LDS and the min(k, chunk) best leave for the candidate list, which
//   the library's select kernel merges with the running list.
// sgpt_ivf_search_u8 -- the same two stages over lists of uint8 codes with one range per dimension (ivf_scan_u8_kernel): q' = q * step and
//   qbias by the prologue of sgpt_u8_rescore, once per call; a row of ld bytes is ld / 16 pieces, so 8 .. 64 lanes cover a row.
#include "host.h"
#include "sort64.h"

namespace {

constexpr int IVF_SUM_ROWS = 256;        // rows of one centroid partial (sgpt_ivf_centroids)
constexpr int IVF_THREADS = 256;
constexpr size_t IVF_CAND_BYTES = (size_t)512 << 20;   // candidate lists of one query group of sgpt_ivf_search at most (a single query may exceed it)

// ---------------------------------------------------------------------------------------------------------------------------
// lists
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IVF_THREADS) void ivf_keys_kernel(const int64_t* __restrict__ assign, int n, int nlist, int np2, u64* __restrict__ keys) {
    const int i = blockIdx.x * IVF_THREADS + threadIdx.x;
    if (i >= np2) return;
    u64 k = ~0ull;                                                   // padding sorts behind every row
    if (i < n) {
        int64_t a = assign[i];
        a = a < 0 ? 0 : (a >= nlist ? nlist - 1 : a);                // out of range: clamped
        k = ((u64)a << 32) | (uint32_t)i;
    }
    keys[i] = k;
}

__global__ __launch_bounds__(IVF_THREADS) void ivf_lists_out_kernel(const u64* __restrict__ keys, int n, int nlist, int64_t* __restrict__ offsets,
                                                                    int64_t* __restrict__ perm) {
    const int i = blockIdx.x * IVF_THREADS + threadIdx.x;
    if (i < n) perm[i] = (int64_t)(uint32_t)(keys[i] & 0xffffffffull);
    if (i <= nlist) offsets[i] = i == nlist ? n : lower_bound_key(keys, n, (u64)i << 32);
}

// ---------------------------------------------------------------------------------------------------------------------------
// centroids
// ---------------------------------------------------------------------------------------------------------------------------
// [o0, o1) of list c inside [0, n): offsets that do not describe such a range give an empty one (memory-safe, whatever the caller passed)
__device__ __forceinline__ void list_range(const int64_t* __restrict__ offsets, int c, long n, long& o0, long& o1) {
    o0 = offsets[c]; o1 = offsets[c + 1];
    if (o0 < 0 || o1 < o0 || o1 > n) { o0 = 0; o1 = 0; }
}

// cstart[c] = chunks of the lists before c (exclusive scan of ceil(len / IVF_SUM_ROWS)), cstart[nlist] = all of them.  One workgroup:
// thread t scans a contiguous span of lists, thread 0 the 256 span totals.  Integer adds.
__global__ __launch_bounds__(IVF_THREADS) void ivf_chunk_scan_kernel(const int64_t* __restrict__ offsets, int nlist, long n, int* __restrict__ cstart) {
    __shared__ int span[IVF_THREADS];
    const int t = threadIdx.x, per = (nlist + IVF_THREADS - 1) / IVF_THREADS;
    const int c0 = t * per, c1 = min(c0 + per, nlist);
    int tot = 0;
    for (int c = c0; c < c1; ++c) {
        long o0, o1;
        list_range(offsets, c, n, o0, o1);
        tot += (int)((o1 - o0 + IVF_SUM_ROWS - 1) / IVF_SUM_ROWS);
    }
    span[t] = tot;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < IVF_THREADS; ++i) { const int v = span[i]; span[i] = run; run += v; }
        cstart[nlist] = run;
    }
    __syncthreads();
    int run = span[t];
    for (int c = c0; c < c1; ++c) {
        long o0, o1;
        list_range(offsets, c, n, o0, o1);
        cstart[c] = run;
        run += (int)((o1 - o0 + IVF_SUM_ROWS - 1) / IVF_SUM_ROWS);
    }
}

// eight consecutive elements of a row as fp32
__device__ __forceinline__ void load8(const float* __restrict__ row, int p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4*>(row)[2 * p], b = reinterpret_cast<const float4*>(row)[2 * p + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const f16_t* __restrict__ row, int p, float (&v)[8]) {
    const uint4 w = reinterpret_cast<const uint4*>(row)[p];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = Half<f16_t>::lo(ws[e]); v[2 * e + 1] = Half<f16_t>::hi(ws[e]); }
}

// One wavefront per chunk of IVF_SUM_ROWS rows of a list: partial[g][:] = the sum of the chunk's rows, rows ascending.  Rows are fetched
// four at a time (their index loads, then their row loads, back to back) and added in ascending order.  A perm entry outside [0, n_x)
// adds nothing.
template <typename T>
__global__ __launch_bounds__(WAVE) void ivf_chunk_sum_kernel(const T* __restrict__ x, long n_x, int d, const int64_t* __restrict__ perm, long n,
                                                             const int64_t* __restrict__ offsets, int nlist, const int* __restrict__ cstart,
                                                             float* __restrict__ partial) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= cstart[nlist]) return;
    int lo = 0, len = nlist;                                         // the list c with cstart[c] <= g < cstart[c + 1]
    while (len > 0) {
        const int half = len >> 1;
        const bool right = cstart[lo + half + 1] <= g;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    const int c = min(lo, nlist - 1);
    long o0, o1;
    list_range(offsets, c, n, o0, o1);
    const long r0 = o0 + (long)(g - cstart[c]) * IVF_SUM_ROWS;
    const long r1 = min(r0 + IVF_SUM_ROWS, o1);
    const int np = d >> 3;
    for (int p = lane; p < np; p += WAVE) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (long r = r0; r < r1; r += 4) {
            long src[4];
            float v[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) src[u] = r + u < r1 ? (long)perm[r + u] : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (src[u] >= 0 && src[u] < n_x) load8(x + src[u] * d, p, v[u]);
                else
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + u < r1)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = __fadd_rn(acc[e], v[u][e]);
        }
        float4* out = reinterpret_cast<float4*>(partial + (long)g * d) + 2 * p;
        out[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        out[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

// One workgroup per list: out[c][j] = the list's partials added in chunk order (thread t owns columns t, t + 256, ...; d <= 4096), under
// `normalize` divided by the L2 norm of that sum -- sum of squares: per thread columns ascending, the 64 lanes in the xor butterfly, the
// four wavefronts as (w0 + w1) + (w2 + w3); one IEEE square root, one IEEE division per element.  An empty list -- and under `normalize` a
// sum whose squared norm is zero or not finite -- gives prev[c] (zeros without prev).
__global__ __launch_bounds__(IVF_THREADS) void ivf_centroid_final_kernel(const float* __restrict__ partial, int n_partial, const int* __restrict__ cstart,
                                                                         int d, const float* __restrict__ prev, int normalize, float* __restrict__ out) {
    __shared__ float red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int g0 = cstart[c], g1 = min(cstart[c + 1], n_partial);
    float s[16];
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int j = t + u * IVF_THREADS;
        s[u] = 0.f;
        if (j < d) {
            for (int g = g0; g < g1; ++g) s[u] = __fadd_rn(s[u], partial[(long)g * d + j]);
            sq = __fadd_rn(sq, __fmul_rn(s[u], s[u]));
        }
    }
    sq = wave_sum(sq);
    if ((t & 63) == 0) red[t >> 6] = sq;
    __syncthreads();
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    const bool keep = g1 <= g0 || (normalize && !(tot > 0.f && tot < INFINITY));
    const float norm = __fsqrt_rn(tot);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int j = t + u * IVF_THREADS;
        if (j < d) out[(long)c * d + j] = keep ? (prev ? prev[(long)c * d + j] : 0.f) : (normalize ? __fdiv_rn(s[u], norm) : s[u]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------------------------------------------------------
// out[p] = RNE_f16(x[perm[p]]): one thread per 8-column piece, a 16-byte store each (and 16-byte loads).  perm outside [0, n_x): a zero row.
template <typename T>
__global__ __launch_bounds__(IVF_THREADS) void ivf_gather_kernel(const T* __restrict__ x, long n_x, int d, const int64_t* __restrict__ perm, long n,
                                                                 uint4* __restrict__ out) {
    const int np = d >> 3;
    const long total = n * np;
    for (long i = (long)blockIdx.x * IVF_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * IVF_THREADS) {
        const long r = i / np;
        const int p = (int)(i - r * np);
        const long src = (long)perm[r];
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (src >= 0 && src < n_x) load8(x + src * d, p, v);
        out[i] = make_uint4(pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3]), pack_f16x2(v[4], v[5]), pack_f16x2(v[6], v[7]));
    }
}

// codes[p] = the uint8 rule (u8_code) of x[perm[p]]: one thread per 8-column piece of the ld-wide row, an 8-byte store each (16- or
// 32-byte loads).  Pieces behind column d hold 128, and so does the whole row of a perm entry outside [0, n_x).
template <typename T>
__global__ __launch_bounds__(IVF_THREADS) void ivf_gather_quant_kernel(const T* __restrict__ x, long n_x, int d, int ld, const int64_t* __restrict__ perm,
                                                                       long n, const float* __restrict__ start, const float* __restrict__ step,
                                                                       uint2* __restrict__ out) {
    const int np = ld >> 3, npd = d >> 3;
    const long total = n * np;
    for (long i = (long)blockIdx.x * IVF_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * IVF_THREADS) {
        const long r = i / np;
        const int p = (int)(i - r * np);
        const long src = (long)perm[r];
        uint32_t w[2] = {0x80808080u, 0x80808080u};
        if (p < npd && src >= 0 && src < n_x) {
            float v[8];
            load8(x + src * d, p, v);
            w[0] = w[1] = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e >> 2] |= u8_code(v[e], start[8 * p + e], step[8 * p + e]) << (8 * (e & 3));
        }
        out[i] = make_uint2(w[0], w[1]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// search, stage 2
// ---------------------------------------------------------------------------------------------------------------------------
// Selection of a work item, shared by the two scan kernels: key = (~f2key(score + 0) << 32 | position in the chunk), ascending key == score
// descending, then position -- and ids ascend inside a list, so position order is original-index order.  NaN -> -1; a position past the
// chunk's rows sorts behind every row.
__device__ __forceinline__ u64 chunk_key(float score, int rr, int nrows) {
    const float v = score != score ? -1.0f : score;
    return rr < nrows ? ((u64)(~f2key(v + 0.0f)) << 32) | (uint32_t)rr : ~0ull;
}
// The CHUNK keys in LDS are sorted by a bitonic network; the first kc leave for the item's slots of the candidate list.
__device__ __forceinline__ void chunk_select(u64* s_key, int t, int kc, const int64_t* __restrict__ ids, long r0, long idx_base,
                                             float* __restrict__ cand_v, int64_t* __restrict__ cand_i, long slot) {
    __syncthreads();
    for (int size = 2; size <= SGPT_IVF_CHUNK; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (t < SGPT_IVF_CHUNK / 2) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const bool up = (i & size) == 0;
                const u64 x = s_key[i], y = s_key[j];
                if ((x > y) == up && x != y) { s_key[i] = y; s_key[j] = x; }
            }
            __syncthreads();
        }
    if (t < kc) {
        const u64 key = s_key[t];
        float v = -INFINITY;
        int64_t id = -1;
        if (key != ~0ull) {
            v = key2f(~(uint32_t)(key >> 32));
            id = ids[r0 + (long)(uint32_t)(key & 0xffffffffull)] + idx_base;
        }
        cand_v[slot + t] = v;
        cand_i[slot + t] = v > -INFINITY ? id : (int64_t)-1;
    }
}

// 8 f16 of one 16-byte piece against the 8 query values of the same columns: dword e of the piece feeds accumulator e, low half first
__device__ __forceinline__ void f16_piece_fma(const uint4 w, const float (&qf)[8], float (&acc)[4]) {
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        acc[e] = __builtin_fmaf(qf[2 * e], Half<f16_t>::lo(ws[e]), acc[e]);
        acc[e] = __builtin_fmaf(qf[2 * e + 1], Half<f16_t>::hi(ws[e]), acc[e]);
    }
}

// blockIdx = (chunk of the list, probe slot, query).  The workgroup's item is rows [ch * CHUNK, ch * CHUNK + CHUNK) of the list
// probe[qi][pi]; an item past the list's end marks its kc output slots unused and exits.  Wavefront w serves rows 64 w .. 64 w + 63 of the
// chunk, RB rows per round: their row loads are issued back to back before the arithmetic.  A wave covers a row in rounds of 512 columns,
// lane l owning the 16-byte piece l + 64 r of round r; the query's pieces sit in registers (NR rounds: d <= 512 NR).
// Order of the arithmetic, fixed by d alone: per lane four accumulators (one per dword of a piece) take their two products by fma, low
// half first, pieces ascending; s = (a0 + a1) + (a2 + a3); the 64 lanes in the xor butterfly 32, 16, .., 1.  NaN -> -1.
// Selection: chunk_key / chunk_select above.
template <int NR, int RB>
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(const float* __restrict__ q, const uint8_t* __restrict__ rows, const int64_t* __restrict__ ids,
                                                               const int64_t* __restrict__ offsets, const int64_t* __restrict__ probe, long n_rows,
                                                               int d, int nlist, int nprobe, int nchunks, int kc, long idx_base,
                                                               float* __restrict__ cand_v, int64_t* __restrict__ cand_i, long ldc) {
    __shared__ u64 s_key[SGPT_IVF_CHUNK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ch = blockIdx.x, pi = blockIdx.y, qi = blockIdx.z;
    const long slot = (long)qi * ldc + ((long)pi * nchunks + ch) * kc;
    const int64_t li = probe[(long)qi * nprobe + pi];
    long o0 = 0, o1 = 0;
    if (li >= 0 && li < nlist) list_range(offsets, (int)li, n_rows, o0, o1);
    const long r0 = o0 + (long)ch * SGPT_IVF_CHUNK;
    if (r0 >= o1) {                                                  // (block-uniform, before the first barrier)
        if (t < kc) { cand_v[slot + t] = -INFINITY; cand_i[slot + t] = -1; }
        return;
    }
    const int nrows = (int)min((long)SGPT_IVF_CHUNK, o1 - r0);
    const int np = d >> 3;
    float qf[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int p = lane + 64 * r;
        if (p < np) load8(q + (long)qi * d, p, qf[r]);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[r][e] = 0.f;
    }
    const uint8_t* base = rows + (size_t)r0 * d * 2;
    float mine = 0.f;                                                // the score of row 64 wave + lane of the chunk
    for (int j0 = 0; j0 < 64; j0 += RB) {
        if (wave * 64 + j0 >= nrows) break;                          // (wave-uniform)
        uint4 w[RB][NR];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int rr = wave * 64 + j0 + b;
            const uint4* row = reinterpret_cast<const uint4*>(base + (size_t)rr * d * 2);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int p = lane + 64 * r;
                w[b][r] = rr < nrows && p < np ? row[p] : make_uint4(0u, 0u, 0u, 0u);
            }
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < NR; ++r) f16_piece_fma(w[b][r], qf[r], acc);
            const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
            if (lane == j0 + b) mine = s;
        }
    }
    s_key[t] = chunk_key(mine, wave * 64 + lane, nrows);
    chunk_select(s_key, t, kc, ids, r0, idx_base, cand_v, cand_i, slot);
}

template <typename... A>
void launch_ivf_scan(int d, dim3 grid, hipStream_t s, A... a) {
    if (d <= 512) hipLaunchKernelGGL((ivf_scan_kernel<1, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (d <= 1024) hipLaunchKernelGGL((ivf_scan_kernel<2, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (d <= 2048) hipLaunchKernelGGL((ivf_scan_kernel<4, 4>), grid, dim3(IVF_THREADS), 0, s, a...);
    else hipLaunchKernelGGL((ivf_scan_kernel<8, 2>), grid, dim3(IVF_THREADS), 0, s, a...);
}

// Byte B of a dword as fp32, exact: one v_cvt_f32_ubyteB.  Spelled out because the compiler otherwise turns float(byte) - 128 into an
// integer subtraction and v_cvt_f32_i32 per element, which does not pair up.
template <int B>
__device__ __forceinline__ float cvt_ubyte(uint32_t w) {
    float r;
    if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(w));
    else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(w));
    else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(w));
    else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(w));
    return r;
}
// byte B of two dwords against their two q' values: code - 128 (exact) and the fma, each for the pair at once (v_pk_add_f32, v_pk_fma_f32)
template <int B>
__device__ __forceinline__ void u8_pair_fma(uint32_t w0, uint32_t w1, const f32x2_t q, f32x2_t& acc) {
    const f32x2_t c = f32x2_t{cvt_ubyte<B>(w0), cvt_ubyte<B>(w1)} - f32x2_t{128.0f, 128.0f};
    acc = __builtin_elementwise_fma(q, c, acc);
}
// 16 codes of one 16-byte piece against the 16 q' values of the same columns: dword e of the piece feeds accumulator e, its bytes in
// ascending order; accumulators 0, 1 and 2, 3 travel as pairs (acc[h] = (a_2h, a_2h+1)), and qp[4 h + b] holds the q' of byte b of the
// dwords 2 h and 2 h + 1.  Per piece: 16 conversions, 8 packed subtractions, 8 packed fmas.
__device__ __forceinline__ void u8_piece_fma(const uint4 w, const f32x2_t (&qp)[8], f32x2_t (&acc)[2]) {
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        u8_pair_fma<0>(ws[2 * h], ws[2 * h + 1], qp[4 * h + 0], acc[h]);
        u8_pair_fma<1>(ws[2 * h], ws[2 * h + 1], qp[4 * h + 1], acc[h]);
        u8_pair_fma<2>(ws[2 * h], ws[2 * h + 1], qp[4 * h + 2], acc[h]);
        u8_pair_fma<3>(ws[2 * h], ws[2 * h + 1], qp[4 * h + 3], acc[h]);
    }
}

// The scan over lists of uint8 codes (sgpt_ivf_search_u8): ivf_scan_kernel's work items and selection, the value of sgpt_u8_rescore.
// qs / qbias: launch_u8_rescore_prepare's q' [nq][ld] and qbias [nq].  G lanes cover a row (a 16-byte piece is 16 columns, so a narrow
// row does not fill a wavefront): the wave walks 64 / G rows at once, lane group sg = lane / G on row sg of them, lane lg = lane % G
// of the group owning the pieces lg + G r of round r < NR (ld <= 16 G NR); the q' pieces sit in registers (paired for u8_piece_fma).  A round of the loop is RB
// such steps, their row loads issued back to back before the arithmetic.  Rows are ld-padded (pad codes 128, q' = 0 there): whole
// pieces, no tail mask; a piece past the row's end reads as 128s against zeros.
// Order of the arithmetic, fixed by ld alone (G and NR are functions of ld, launch_ivf_scan_u8): per lane four accumulators (one per
// dword of a piece) take their four products by fma, bytes ascending, pieces ascending; s = (a0 + a1) + (a2 + a3); the G lanes in
// the xor butterfly G / 2, .., 1; value = s + qbias.  NaN -> -1.  Lane 0 of a group writes the row's key; keys of rows the chunk does
// not have stay ~0 (every thread first marks its own slot: the four waves' slots are disjoint until the selection's barrier).
template <int G, int NR, int RB>
__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_u8_kernel(const float* __restrict__ qs, const float* __restrict__ qbias,
                                                                  const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids,
                                                                  const int64_t* __restrict__ offsets, const int64_t* __restrict__ probe, long n_rows,
                                                                  int ld, int nlist, int nprobe, int nchunks, int kc, long idx_base,
                                                                  float* __restrict__ cand_v, int64_t* __restrict__ cand_i, long ldc) {
    constexpr int SPW = WAVE / G;                                    // rows a wavefront walks at once
    static_assert(G * SPW == WAVE && 64 % (RB * SPW) == 0, "ivf_scan_u8_kernel: whole rounds over a wavefront's 64 rows");
    __shared__ u64 s_key[SGPT_IVF_CHUNK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lg = lane & (G - 1), sg = lane / G;
    const int ch = blockIdx.x, pi = blockIdx.y, qi = blockIdx.z;
    const long slot = (long)qi * ldc + ((long)pi * nchunks + ch) * kc;
    const int64_t li = probe[(long)qi * nprobe + pi];
    long o0 = 0, o1 = 0;
    if (li >= 0 && li < nlist) list_range(offsets, (int)li, n_rows, o0, o1);
    const long r0 = o0 + (long)ch * SGPT_IVF_CHUNK;
    if (r0 >= o1) {                                                  // (block-uniform, before the first barrier)
        if (t < kc) { cand_v[slot + t] = -INFINITY; cand_i[slot + t] = -1; }
        return;
    }
    const int nrows = (int)min((long)SGPT_IVF_CHUNK, o1 - r0);
    const int np = ld >> 4;
    const float* __restrict__ qrow = qs + (long)qi * ld;
    f32x2_t qp[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int p = lg + G * r;
        float4 v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p < np ? reinterpret_cast<const float4*>(qrow)[4 * p + e] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            qp[r][4 * h + 0] = f32x2_t{v[2 * h].x, v[2 * h + 1].x}; qp[r][4 * h + 1] = f32x2_t{v[2 * h].y, v[2 * h + 1].y};
            qp[r][4 * h + 2] = f32x2_t{v[2 * h].z, v[2 * h + 1].z}; qp[r][4 * h + 3] = f32x2_t{v[2 * h].w, v[2 * h + 1].w};
        }
    }
    const float qb = qbias[qi];
    s_key[t] = ~0ull;
    const uint8_t* base = codes + (size_t)r0 * ld;
    for (int j0 = 0; j0 < 64; j0 += RB * SPW) {
        if (wave * 64 + j0 >= nrows) break;                          // (wave-uniform)
        uint4 w[RB][NR];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int rr = wave * 64 + j0 + b * SPW + sg;
            const uint4* row = reinterpret_cast<const uint4*>(base + (size_t)rr * ld);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int p = lg + G * r;
                w[b][r] = rr < nrows && p < np ? row[p] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
            }
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int rr = wave * 64 + j0 + b * SPW + sg;
            f32x2_t acc[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int r = 0; r < NR; ++r) u8_piece_fma(w[b][r], qp[r], acc);
            float s = (acc[0].x + acc[0].y) + (acc[1].x + acc[1].y);
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
            s = s + qb;
            if (lg == 0 && rr < nrows) s_key[rr] = chunk_key(s, rr, nrows);
        }
    }
    chunk_select(s_key, t, kc, ids, r0, idx_base, cand_v, cand_i, slot);
}

// G and NR from ld alone: they fix the order of the arithmetic (include/sgpt_hip.h)
template <typename... A>
void launch_ivf_scan_u8(int ld, dim3 grid, hipStream_t s, A... a) {
    if (ld <= 128) hipLaunchKernelGGL((ivf_scan_u8_kernel<8, 1, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (ld <= 256) hipLaunchKernelGGL((ivf_scan_u8_kernel<16, 1, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (ld <= 512) hipLaunchKernelGGL((ivf_scan_u8_kernel<32, 1, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (ld <= 1024) hipLaunchKernelGGL((ivf_scan_u8_kernel<64, 1, 8>), grid, dim3(IVF_THREADS), 0, s, a...);
    else if (ld <= 2048) hipLaunchKernelGGL((ivf_scan_u8_kernel<64, 2, 4>), grid, dim3(IVF_THREADS), 0, s, a...);
    else hipLaunchKernelGGL((ivf_scan_u8_kernel<64, 4, 2>), grid, dim3(IVF_THREADS), 0, s, a...);
}

inline bool x_dtype_ok(int dt) { return dt == SGPT_F32 || dt == SGPT_F16; }

}  // namespace

static_assert(SGPT_IVF_CHUNK == IVF_THREADS && SGPT_IVF_CHUNK % WAVE == 0, "ivf_scan_kernel: one thread per row of a chunk");

extern "C" {

sgpt_status sgpt_ivf_lists(sgpt_ctx* c, const int64_t* assign, int64_t N, int32_t nlist, int64_t* offsets, int64_t* perm, void* stream) {
    if (!c || !assign || !offsets || !perm || N <= 0 || N > SGPT_IVF_MAX_ROWS || nlist <= 0 || nlist > SGPT_IVF_MAX_LISTS)
        return fail(c, SGPT_ERR_INVALID, "sgpt_ivf_lists: bad arguments (0 < N <= 2^30, 0 < nlist <= 65536)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)N, np2 = s64_padded(N);
    sgpt_status st = ensure(c, &c->ws7, &c->ws7_bytes, (size_t)np2 * 8);
    if (st != SGPT_OK) return st;
    u64* keys = (u64*)c->ws7;
    hipLaunchKernelGGL(ivf_keys_kernel, dim3(np2 / IVF_THREADS), dim3(IVF_THREADS), 0, s, assign, n, (int)nlist, np2, keys);
    launch_sort_u64(keys, np2, s);
    const int m = n > nlist + 1 ? n : nlist + 1;
    hipLaunchKernelGGL(ivf_lists_out_kernel, dim3((m + IVF_THREADS - 1) / IVF_THREADS), dim3(IVF_THREADS), 0, s, keys, n, (int)nlist, offsets, perm);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_ivf_centroids(sgpt_ctx* c, const void* x, int32_t x_dtype, int64_t n_x, int32_t d, const int64_t* perm, int64_t n,
                               const int64_t* offsets, int32_t nlist, const float* prev, int32_t normalize, float* out, void* stream) {
    if (!c || !x || !perm || !offsets || !out || !x_dtype_ok(x_dtype) || n_x <= 0 || n <= 0 || n > SGPT_IVF_MAX_ROWS || d <= 0 || d % 8 ||
        d > SGPT_IVF_MAX_DIM || nlist <= 0 || nlist > SGPT_IVF_MAX_LISTS || ((size_t)x & 15) || ((size_t)out & 15))
        return fail(c, SGPT_ERR_INVALID, "sgpt_ivf_centroids: bad arguments (x fp32 or f16 and 16-byte aligned, d % 8 == 0, d <= 4096, "
                                         "0 < n <= 2^30, 0 < nlist <= 65536)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // disjoint lists inside [0, n) have at most n / ROWS + nlist chunks; lists that overlap (a caller's error) lose the chunks beyond
    const long bound = n / IVF_SUM_ROWS + nlist;
    const size_t cs_b = align_up((size_t)(nlist + 1) * 4, 256);
    sgpt_status st = ensure(c, &c->ws7, &c->ws7_bytes, cs_b + (size_t)bound * d * 4);
    if (st != SGPT_OK) return st;
    int* cstart = (int*)c->ws7;
    float* partial = (float*)((char*)c->ws7 + cs_b);
    hipLaunchKernelGGL(ivf_chunk_scan_kernel, dim3(1), dim3(IVF_THREADS), 0, s, offsets, (int)nlist, (long)n, cstart);
    if (x_dtype == SGPT_F32)
        hipLaunchKernelGGL(ivf_chunk_sum_kernel<float>, dim3((unsigned)bound), dim3(WAVE), 0, s, (const float*)x, (long)n_x, (int)d, perm, (long)n,
                           offsets, (int)nlist, cstart, partial);
    else
        hipLaunchKernelGGL(ivf_chunk_sum_kernel<f16_t>, dim3((unsigned)bound), dim3(WAVE), 0, s, (const f16_t*)x, (long)n_x, (int)d, perm, (long)n,
                           offsets, (int)nlist, cstart, partial);
    hipLaunchKernelGGL(ivf_centroid_final_kernel, dim3(nlist), dim3(IVF_THREADS), 0, s, partial, (int)bound, cstart, (int)d, prev, (int)normalize, out);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_gather_rows(sgpt_ctx* c, const void* x, int32_t x_dtype, int64_t n_x, const int64_t* perm, int64_t n, int32_t d, void* out,
                             void* stream) {
    if (!c || !x || !perm || !out || !x_dtype_ok(x_dtype) || n_x <= 0 || n <= 0 || d <= 0 || d % 8 || ((size_t)x & 15) || ((size_t)out & 15))
        return fail(c, SGPT_ERR_INVALID, "sgpt_gather_rows: bad arguments (x fp32 or f16, d % 8 == 0, x and out 16-byte aligned)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)n * (d >> 3);
    const long want = (total + IVF_THREADS - 1) / IVF_THREADS;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    if (x_dtype == SGPT_F32)
        hipLaunchKernelGGL(ivf_gather_kernel<float>, dim3(grid), dim3(IVF_THREADS), 0, s, (const float*)x, (long)n_x, (int)d, perm, (long)n, (uint4*)out);
    else
        hipLaunchKernelGGL(ivf_gather_kernel<f16_t>, dim3(grid), dim3(IVF_THREADS), 0, s, (const f16_t*)x, (long)n_x, (int)d, perm, (long)n, (uint4*)out);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

// The two-stage search that sgpt_ivf_search and sgpt_ivf_search_u8 are: the shared argument checks (entry_ok: the caller's own; `bad`: its
// message for both), stage 1 by the f16 scorer's own launches, then per query group the caller's scan, the running list appended, the
// select.  ws7 = [f16 queries | probe values | probe sets | candidate values | candidate indices | head_b bytes of the caller];
// prepare(head, s) fills the caller's part once per call, scan(head, g0, gn, probe sets of the group, nchunks, kc, cv, ci, ldc, s) launches
// the work items of queries g0 .. g0 + gn.
extern "C++" {
template <class Prepare, class Scan>
static sgpt_status ivf_two_stage(sgpt_ctx* c, const char* who, const char* bad, bool entry_ok, const float* q, const void* centroids16,
                                 const int64_t* ids, const int64_t* offsets, int32_t nq, int64_t N, int32_t d, int32_t nlist, int64_t max_list,
                                 int32_t nprobe, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                                 int64_t* probe_out, void* stream, size_t head_b, Prepare prepare, Scan scan) {
    if (!entry_ok || !c || !q || !centroids16 || !ids || !offsets || !run_val || !run_idx || nq <= 0 || nq > 65535 || N <= 0 || d <= 0 || d % 8 ||
        d > SGPT_IVF_MAX_DIM || nlist <= 0 || nlist > SGPT_IVF_MAX_LISTS || max_list < 0 || max_list > N || nprobe <= 0 || nprobe > nlist ||
        nprobe > 1024 || k <= 0 || k > 1024 || n_run < 0 || n_run > k || ((size_t)q & 15) || ((size_t)centroids16 & 15))
        return fail(c, SGPT_ERR_INVALID, bad);
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nchunks = (int)((max_list + SGPT_IVF_CHUNK - 1) / SGPT_IVF_CHUNK) > 0 ? (int)((max_list + SGPT_IVF_CHUNK - 1) / SGPT_IVF_CHUNK) : 1;
    const int kc = k < SGPT_IVF_CHUNK ? k : SGPT_IVF_CHUNK;
    const long m = (long)nprobe * nchunks * kc;                      // candidate slots of a query
    if (m + k > 0x7fffff00L)
        return fail(c, SGPT_ERR_INVALID, std::string(who) + ": nprobe * ceil(max_list / SGPT_IVF_CHUNK) * min(k, chunk) does not fit the select kernel");
    const long ldc = m + k;
    long group = (long)(IVF_CAND_BYTES / ((size_t)ldc * 12));
    group = group < 1 ? 1 : (group > nq ? nq : group);
    const size_t q16_b = align_up((size_t)nq * d * 2, 256), pv_b = align_up((size_t)nq * nprobe * 4, 256), pi_b = align_up((size_t)nq * nprobe * 8, 256);
    const size_t cv_b = align_up((size_t)group * ldc * 4, 256), ci_b = align_up((size_t)group * ldc * 8, 256);
    sgpt_status st = ensure(c, &c->ws7, &c->ws7_bytes, q16_b + pv_b + pi_b + cv_b + ci_b + head_b);
    if (st != SGPT_OK) return st;
    char* b = (char*)c->ws7;
    void* q16 = b; b += q16_b;
    float* pv = (float*)b; b += pv_b;
    int64_t* pidx = (int64_t*)b; b += pi_b;
    float* cv = (float*)b; b += cv_b;
    int64_t* ci = (int64_t*)b; b += ci_b;
    char* head = b;
    // stage 1: the probe sets, by the f16 scorer's own launches
    launch_f32_to_16(q, (long)nq * d, q16, DT_F16, s);
    st = sgpt_score_topk(c, q16, centroids16, SGPT_F16, nq, nlist, d, nprobe, 0, pv, pidx, 0, nullptr, stream);
    if (st != SGPT_OK) return st;
    if (probe_out) HIPC(c, hipMemcpyAsync(probe_out, pidx, (size_t)nq * nprobe * 8, hipMemcpyDeviceToDevice, s));
    prepare(head, s);
    // stage 2, in query groups the candidate workspace holds: scan, append the running list, select
    for (long g0 = 0; g0 < nq; g0 += group) {
        const int gn = (int)(nq - g0 < group ? nq - g0 : group);
        scan(head, g0, gn, (const int64_t*)(pidx + g0 * nprobe), nchunks, kc, cv, ci, ldc, s);
        launch_list_append(run_val + g0 * k, run_idx + g0 * k, k, n_run, gn, cv, ci, ldc, (int)m, s);
        launch_topk_select(cv, ldc, 0, 0, cv, ci, (int)(m + n_run), ldc, gn, k, 0, nullptr, run_val + g0 * k, run_idx + g0 * k, s);
    }
    if (n_out) { const int64_t tot = (int64_t)n_run + N; *n_out = (int32_t)(tot < k ? tot : k); }
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}
}  // extern "C++"

sgpt_status sgpt_ivf_search(sgpt_ctx* c, const float* q, const void* centroids16, const void* rows, const int64_t* ids, const int64_t* offsets,
                            int32_t nq, int64_t N, int32_t d, int32_t nlist, int64_t max_list, int32_t nprobe, int32_t k, int64_t idx_base,
                            float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, int64_t* probe_out, void* stream) {
    auto scan = [&](char*, long g0, int gn, const int64_t* probes, int nchunks, int kc, float* cv, int64_t* ci, long ldc, hipStream_t s) {
        launch_ivf_scan(d, dim3(nchunks, nprobe, gn), s, q + g0 * d, (const uint8_t*)rows, ids, offsets, probes, (long)N, (int)d, (int)nlist,
                        (int)nprobe, nchunks, kc, (long)idx_base, cv, ci, ldc);
    };
    return ivf_two_stage(c, "sgpt_ivf_search",
                         "sgpt_ivf_search: bad arguments (0 < nq <= 65535, d % 8 == 0, d <= 4096, 0 < nlist <= 65536, "
                         "0 <= max_list <= N, 0 < nprobe <= min(nlist, 1024), 0 < k <= 1024, 0 <= n_run <= k, q / centroids16 / "
                         "rows 16-byte aligned)",
                         rows && !((size_t)rows & 15), q, centroids16, ids, offsets, nq, N, d, nlist, max_list, nprobe, k, idx_base, run_val, run_idx,
                         n_run, n_out, probe_out, stream, 0, [](char*, hipStream_t) {}, scan);
}

sgpt_status sgpt_u8_gather_quantize_rows(sgpt_ctx* c, const void* x, int32_t x_dtype, int64_t n_x, const int64_t* perm, int64_t n, int32_t d,
                                         int32_t ld, const float* start, const float* step, uint8_t* codes, void* stream) {
    if (!c || !x || !perm || !start || !step || !codes || !x_dtype_ok(x_dtype) || n_x <= 0 || n <= 0 || d <= 0 || d % 8 || d > SGPT_IVF_MAX_DIM ||
        ld % 128 || d > ld || ((size_t)x & 15) || ((size_t)codes & 15))
        return fail(c, SGPT_ERR_INVALID, "sgpt_u8_gather_quantize_rows: bad arguments (x fp32 or f16, d % 8 == 0, d <= 4096, ld % 128 == 0, "
                                         "d <= ld, x and codes 16-byte aligned)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)n * (ld >> 3);
    const long want = (total + IVF_THREADS - 1) / IVF_THREADS;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    if (x_dtype == SGPT_F32)
        hipLaunchKernelGGL(ivf_gather_quant_kernel<float>, dim3(grid), dim3(IVF_THREADS), 0, s, (const float*)x, (long)n_x, (int)d, (int)ld, perm,
                           (long)n, start, step, (uint2*)codes);
    else
        hipLaunchKernelGGL(ivf_gather_quant_kernel<f16_t>, dim3(grid), dim3(IVF_THREADS), 0, s, (const f16_t*)x, (long)n_x, (int)d, (int)ld, perm,
                           (long)n, start, step, (uint2*)codes);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

// head of ws7 = [q' fp32 [nq][ld] | qbias fp32 [nq]]: the prologue of sgpt_u8_rescore, once per call
sgpt_status sgpt_ivf_search_u8(sgpt_ctx* c, const float* q, const void* centroids16, const uint8_t* codes, const float* start, const float* step,
                               const int64_t* ids, const int64_t* offsets, int32_t nq, int64_t N, int32_t d, int32_t ld, int32_t nlist,
                               int64_t max_list, int32_t nprobe, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run,
                               int32_t* n_out, int64_t* probe_out, void* stream) {
    const bool ok = codes && start && step && ld > 0 && ld % 128 == 0 && d <= ld && ld <= SGPT_IVF_MAX_DIM && !((size_t)codes & 15);
    const size_t qs_b = ok && nq > 0 ? align_up((size_t)nq * ld * 4, 256) : 0;
    auto prepare = [&](char* head, hipStream_t s) {
        launch_u8_rescore_prepare(q, start, step, nq, d, ld, (float*)head, (float*)(head + qs_b), s);
    };
    auto scan = [&](char* head, long g0, int gn, const int64_t* probes, int nchunks, int kc, float* cv, int64_t* ci, long ldc, hipStream_t s) {
        launch_ivf_scan_u8(ld, dim3(nchunks, nprobe, gn), s, (const float*)head + g0 * ld, (const float*)(head + qs_b) + g0, codes, ids, offsets,
                           probes, (long)N, (int)ld, (int)nlist, (int)nprobe, nchunks, kc, (long)idx_base, cv, ci, ldc);
    };
    return ivf_two_stage(c, "sgpt_ivf_search_u8",
                         "sgpt_ivf_search_u8: bad arguments (0 < nq <= 65535, d % 8 == 0, d <= 4096, ld % 128 == 0, d <= ld <= 4096, "
                         "0 < nlist <= 65536, 0 <= max_list <= N, 0 < nprobe <= min(nlist, 1024), 0 < k <= 1024, 0 <= n_run <= k, q / "
                         "centroids16 / codes 16-byte aligned)",
                         ok, q, centroids16, ids, offsets, nq, N, d, nlist, max_list, nprobe, k, idx_base, run_val, run_idx, n_run, n_out,
                         probe_out, stream, qs_b + (ok && nq > 0 ? align_up((size_t)nq * 4, 256) : 0), prepare, scan);
}

}  // extern "C"
