// USEB evaluation on the device (include/sgpt_hip.h::sgpt_eval_groups, sgpt_eval_pairs).
//
// sgpt_eval_groups -- the re-ranking tasks (AskUbuntu, SciDocs): a CSR of candidate groups over a pool of embedded sentences is
// scored, ranked and reduced to its metric sums in one call.
//   * A pair's score is always taken by ONE wavefront with ONE summation order that depends on d alone: lane l adds the products of
//     elements l + 64 (4 t + u) into accumulator u (u = 0 .. 3, t ascending), the four are joined as (a0 + a1) + (a2 + a3) and the
//     lanes by the xor butterfly of wave_sum.  So the same two rows give the same bits wherever the pair stands.
//   * Rank order is the ascending order of a 64-bit key: the high word falls as the score rises (NaN: the largest word, so NaN
//     ranks last; -0 is folded into +0), the low word is the candidate's position inside its group, so equal scores keep the
//     order the caller listed them in (Python's stable sorted(..., reverse=True)).  Keys are unique: the order is total.
//   * Groups of <= 64 candidates: one wavefront per group, GR_WAVES groups per workgroup, key in a register, a 21-step bitonic
//     exchange across the lanes.  Groups of 65 .. 1024: one workgroup per group, keys in LDS (8 KiB), bitonic sort with a
//     barrier per step, wave 0 reduces.  Which kernel serves a group depends on its size alone.
//   * The sums are eval.hip's: lane l of chunk c looks at rank 64 c + l + 1, hits@i is a ballot prefix plus the carry of the
//     earlier chunks (exact), a chunk's 64 float terms are summed by the xor butterfly and the chunks added in ascending order.
//
// sgpt_eval_pairs -- TwitterPara: the global rank statistics of n scored pairs.
//   * (score key, index) 64-bit keys are sorted ascending by the bitonic network of sort64.h: tiles of 2048 keys in LDS for the strides
//     below 2048, one global compare-exchange launch per stride above.  The keys are unique, so the result is the one sorted order.
//   * A tie group is found from the sorted keys (neighbour compare, binary search only inside a group of equal scores):
//     rank2 = first + last 1-based rank of the group = twice the averaged rank.
//   * Positives and used rows at or above each threshold come from a three-launch inclusive scan of the (positive, used) flags
//     in sorted order (64-bit integer adds: exact in any order); the average-precision numerator is summed in fp64, 256 terms by
//     an LDS tree per workgroup and the workgroup partials by one workgroup in a fixed order.
// No float atomics anywhere; the only atomic is the vector atomicOr of the NaN flag.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/sgpt_hip.h"
#include "common.h"
#include "ctx.h"
#include "sort64.h"

namespace {

constexpr int GR_WAVES = 4;              // small groups per workgroup
constexpr int GR_THREADS = GR_WAVES * WAVE;
constexpr int GR_SMALL = WAVE;           // <= this: a wavefront per group
constexpr int PR_TILE = S64_TILE;        // keys sorted in LDS by one workgroup (sort64.h)
constexpr int PR_THREADS = S64_THREADS;
constexpr int PR_SCAN = 1024;            // flags scanned by one workgroup (4 per thread)
constexpr int PR_FLAG_WORD = 33;         // word of the ctx's 256-byte flag block that collects the NaN check (32: sgpt_eval_ranked)

__device__ __forceinline__ int popc_below_incl(u64 m, int lane) {   // set bits of m at lanes 0 .. lane
    return __popcll(m & (~0ull >> (63 - lane)));
}

// ---------------------------------------------------------------------------------------------------------------------------
// groups
// ---------------------------------------------------------------------------------------------------------------------------
struct GroupArgs {
    const float* emb; int n_rows, d, mode;
    const float* scores_in;
    int G; const int* grp_off; int n_cand;
    const int* q_row; const int* cand_row; const int* cand_rel; const int* R_extra;
    const int* ideal_off; const int* ideal_rel; int n_ideal;
    float* out_scores; int* out_order; int* out_hits1; int* out_hits5; int* out_first; int* out_R;
    float* out_sp; float* out_dcg; float* out_idcg;
};

// rank key of candidate `pos` of a group: ascending key == descending score, then ascending position; NaN last
__device__ __forceinline__ u64 rank_key(float s, int pos) {
    const uint32_t hi = s != s ? 0xffffffffu : ~f2key(s + 0.0f);
    return ((u64)hi << 32) | (uint32_t)pos;
}

template <int MODE>
__device__ __forceinline__ float pair_score_mode(const float* __restrict__ x, const float* __restrict__ y, int d, int lane) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, xx[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < d; i0 += 4 * WAVE) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * WAVE + lane;
            if (i < d) {
                const float xv = x[i], yv = y[i];
                if (MODE == SGPT_NEG_L2) {
                    const float df = xv - yv;
                    acc[u] += df * df;
                } else {
                    acc[u] += xv * yv;
                    if (MODE == SGPT_COS) { xx[u] += xv * xv; yy[u] += yv * yv; }
                }
            }
        }
    }
    const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (MODE == SGPT_NEG_L2) return -sqrtf(s);
    if (MODE == SGPT_COS) {
        const float nx = wave_sum((xx[0] + xx[1]) + (xx[2] + xx[3])), ny = wave_sum((yy[0] + yy[1]) + (yy[2] + yy[3]));
        return s / (fmaxf(sqrtf(nx), 1e-8f) * fmaxf(sqrtf(ny), 1e-8f));
    }
    return s;
}

// score of (query row q, candidate row r), the same value on every lane; a row outside [0, n_rows) gives NaN (ranks last)
__device__ __forceinline__ float pair_score(const GroupArgs& a, int q, int r, int lane) {
    if (q < 0 || q >= a.n_rows || r < 0 || r >= a.n_rows) return __uint_as_float(0x7fc00000u);
    const float* x = a.emb + (long)q * a.d;
    const float* y = a.emb + (long)r * a.d;
    if (a.mode == SGPT_COS) return pair_score_mode<SGPT_COS>(x, y, a.d, lane);
    if (a.mode == SGPT_DOT) return pair_score_mode<SGPT_DOT>(x, y, a.d, lane);
    return pair_score_mode<SGPT_NEG_L2>(x, y, a.d, lane);
}

// [o0, o0 + n) of group g, or n = -1 when the offsets do not describe a range inside the candidate arrays
__device__ __forceinline__ int group_range(const GroupArgs& a, int g, int& o0) {
    o0 = a.grp_off[g];
    const int o1 = a.grp_off[g + 1];
    return (o0 < 0 || o1 < o0 || o1 > a.n_cand) ? -1 : o1 - o0;
}

// One wavefront: the sorted keys of a group (key_at(r): key of 0-based rank r, asked for r < n only) -> its outputs.
template <typename KeyAt>
__device__ __forceinline__ void group_reduce(const GroupArgs& a, int g, int o0, int n, int lane, KeyAt key_at) {
    int carry = 0, first = 0, h1 = 0, h5 = 0;
    float sp = 0.f, dcg = 0.f, idcg = 0.f;
    for (int c0 = 0; c0 < n; c0 += WAVE) {
        const int r = c0 + lane;
        const bool valid = r < n;
        const int pos = valid ? (int)(uint32_t)(key_at(r) & 0xffffffffull) : 0;
        if (valid && a.out_order) a.out_order[o0 + r] = pos;
        const int grade = valid ? a.cand_rel[o0 + pos] : 0;
        const bool rel = valid && grade > 0;
        const u64 m = __ballot(rel);
        const int h_i = carry + popc_below_incl(m, lane);            // hits@(r + 1)
        dcg += wave_sum(rel ? (float)grade / log2f((float)(r + 2)) : 0.f);
        sp += wave_sum(rel ? (float)h_i / (float)(r + 1) : 0.f);
        if (c0 == 0) { h1 = __popcll(m & 1ull); h5 = __popcll(m & 0x1full); }
        if (first == 0 && m) first = c0 + (int)__builtin_ctzll(m) + 1;
        carry += __popcll(m);
    }
    if (a.ideal_off && a.ideal_rel) {
        const int j0 = min(max(a.ideal_off[g], 0), a.n_ideal);
        const int nj = max(min(a.ideal_off[g + 1], a.n_ideal) - j0, 0);
        for (int c0 = 0; c0 < nj; c0 += WAVE) {
            const int j = c0 + lane;
            const int gr = j < nj ? a.ideal_rel[j0 + j] : 0;
            const u64 m = __ballot(gr > 0);
            if (m == 0) break;                                       // descending: nothing but non-positive grades from here on
            idcg += wave_sum(gr > 0 ? (float)gr / log2f((float)(j + 2)) : 0.f);
        }
    }
    if (lane == 0) {
        a.out_hits1[g] = h1; a.out_hits5[g] = h5; a.out_first[g] = first;
        a.out_R[g] = carry + (a.R_extra ? max(a.R_extra[g], 0) : 0);
        a.out_sp[g] = sp; a.out_dcg[g] = dcg; a.out_idcg[g] = idcg;
    }
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(v & 0xffffffffull), mask, WAVE);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, WAVE);
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(GR_THREADS) void groups_wave_kernel(GroupArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int g = blockIdx.x * GR_WAVES + wave;
    if (g >= a.G) return;                                            // no barrier in this kernel
    int o0;
    const int n = group_range(a, g, o0);
    if (n < 0 || n > SGPT_EVAL_MAX_GROUP) {                          // not a servable group (caller error): marked, nothing else touched
        if (lane == 0) {
            a.out_hits1[g] = 0; a.out_hits5[g] = 0; a.out_first[g] = 0; a.out_R[g] = -1;
            a.out_sp[g] = 0.f; a.out_dcg[g] = 0.f; a.out_idcg[g] = 0.f;
        }
        return;
    }
    if (n > GR_SMALL) return;                                        // larger groups: groups_block_kernel
    float s = 0.f;
    if (a.scores_in) {
        if (lane < n) s = a.scores_in[o0 + lane];
    } else {
        const int q = n > 0 ? a.q_row[g] : 0;
        for (int j = 0; j < n; ++j) {
            const float sc = pair_score(a, q, a.cand_row[o0 + j], lane);
            if (lane == j) s = sc;
        }
    }
    if (lane < n && a.out_scores) a.out_scores[o0 + lane] = s;
    u64 key = lane < n ? rank_key(s, lane) : ~0ull;
    for (int size = 2; size <= WAVE; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const u64 other = shfl_xor_u64(key, stride);
            const bool up = (lane & size) == 0, low = (lane & stride) == 0;
            const bool take_min = up == low;                         // the lower lane of an ascending pair keeps the smaller key
            key = take_min ? (other < key ? other : key) : (other > key ? other : key);
        }
    group_reduce(a, g, o0, n, lane, [&](int) { return key; });       // n <= 64: rank r sits in lane r
}

__global__ __launch_bounds__(PR_THREADS) void groups_block_kernel(GroupArgs a) {
    __shared__ u64 s_key[SGPT_EVAL_MAX_GROUP];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    const int g = blockIdx.x;
    int o0;
    const int n = group_range(a, g, o0);
    if (n <= GR_SMALL || n > SGPT_EVAL_MAX_GROUP) return;            // block-uniform, before the first barrier
    int np2 = 2 * WAVE;
    while (np2 < n) np2 <<= 1;
    if (a.scores_in) {
        for (int j = t; j < n; j += PR_THREADS) {
            const float s = a.scores_in[o0 + j];
            s_key[j] = rank_key(s, j);
            if (a.out_scores) a.out_scores[o0 + j] = s;
        }
    } else {
        const int q = a.q_row[g];
        for (int j = wave; j < n; j += PR_THREADS / WAVE) {
            const float s = pair_score(a, q, a.cand_row[o0 + j], lane);
            if (lane == 0) {
                s_key[j] = rank_key(s, j);
                if (a.out_scores) a.out_scores[o0 + j] = s;
            }
        }
    }
    for (int j = n + t; j < np2; j += PR_THREADS) s_key[j] = ~0ull;
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = t; p < (np2 >> 1); p += PR_THREADS) {
                const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
                const bool up = (i & size) == 0;
                const u64 x = s_key[i], y = s_key[j];
                if ((x > y) == up && x != y) { s_key[i] = y; s_key[j] = x; }
            }
            __syncthreads();
        }
    if (wave == 0) group_reduce(a, g, o0, n, lane, [&](int r) { return s_key[r]; });
}

// ---------------------------------------------------------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void pairs_keys_kernel(const float* __restrict__ score, int n, int np2, u64* __restrict__ keys,
                                                                int* __restrict__ flag) {
    const int i = blockIdx.x * PR_THREADS + threadIdx.x;
    bool bad = false;
    if (i < np2) {
        u64 k = ~0ull;                                               // padding sorts behind every score
        if (i < n) {
            const float s = score[i];
            bad = s != s;
            k = ((u64)(bad ? 0xffffffffu : f2key(s + 0.0f)) << 32) | (uint32_t)i;
        }
        keys[i] = k;
    }
    if (__ballot(bad) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(flag, 1);
}

// (positive << 32 | used) of sorted position p
__device__ __forceinline__ u64 pair_flags(const u64* __restrict__ keys, const int* __restrict__ label, int n, int p) {
    if (p >= n) return 0ull;
    const int l = label[(uint32_t)(keys[p] & 0xffffffffull)];
    return l < 0 ? 0ull : (l > 0 ? (1ull << 32) | 1ull : 1ull);
}

// inclusive scan over the workgroup's PR_THREADS values (Hillis-Steele in LDS); every thread also gets the total
__device__ __forceinline__ u64 block_scan_incl(u64 v, u64* sh, int t, u64& total) {
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < PR_THREADS; o <<= 1) {
        const u64 add = t >= o ? sh[t - o] : 0ull;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const u64 r = sh[t];
    total = sh[PR_THREADS - 1];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(PR_THREADS) void pairs_block_sums_kernel(const u64* __restrict__ keys, const int* __restrict__ label, int n,
                                                                      u64* __restrict__ bsum) {
    __shared__ u64 sh[PR_THREADS];
    const int t = threadIdx.x, p0 = blockIdx.x * PR_SCAN + t * 4;
    u64 v = 0;
    for (int u = 0; u < 4; ++u) v += pair_flags(keys, label, n, p0 + u);
    u64 total;
    block_scan_incl(v, sh, t, total);
    if (t == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(PR_THREADS) void pairs_scan_sums_kernel(u64* __restrict__ bsum, int nblk) {     // one workgroup: exclusive scan in place
    __shared__ u64 sh[PR_THREADS];
    const int t = threadIdx.x;
    u64 carry = 0;
    for (int c0 = 0; c0 < nblk; c0 += PR_THREADS) {
        const u64 v = c0 + t < nblk ? bsum[c0 + t] : 0ull;
        u64 total;
        const u64 incl = block_scan_incl(v, sh, t, total);
        if (c0 + t < nblk) bsum[c0 + t] = carry + incl - v;
        carry += total;
    }
}

__global__ __launch_bounds__(PR_THREADS) void pairs_scan_kernel(const u64* __restrict__ keys, const int* __restrict__ label, int n,
                                                                const u64* __restrict__ bsum, u64* __restrict__ incl_out) {
    __shared__ u64 sh[PR_THREADS];
    const int t = threadIdx.x, p0 = blockIdx.x * PR_SCAN + t * 4;
    u64 f[4], v = 0;
    for (int u = 0; u < 4; ++u) { v += pair_flags(keys, label, n, p0 + u); f[u] = v; }
    u64 total;
    const u64 before = block_scan_incl(v, sh, t, total) - v + bsum[blockIdx.x];
    for (int u = 0; u < 4; ++u) incl_out[p0 + u] = before + f[u];
}

__global__ __launch_bounds__(PR_THREADS) void pairs_rank_kernel(const u64* __restrict__ keys, const u64* __restrict__ incl, int n,
                                                                int* __restrict__ rank2, double* __restrict__ partial) {
    __shared__ double sh[PR_THREADS];
    const int t = threadIdx.x, p = blockIdx.x * PR_THREADS + t;
    double term = 0.0;
    if (p < n) {
        const u64 k = keys[p];
        const uint32_t hi = (uint32_t)(k >> 32);
        // the tie group [s, e) of sorted positions that p belongs to
        int s = p, e = p + 1;
        if (p > 0 && (uint32_t)(keys[p - 1] >> 32) == hi) s = lower_bound_key(keys, n, (u64)hi << 32);
        if (p + 1 < n && (uint32_t)(keys[p + 1] >> 32) == hi) e = hi == 0xffffffffu ? n : lower_bound_key(keys, n, (u64)(hi + 1u) << 32);
        rank2[(uint32_t)(k & 0xffffffffull)] = s + e + 1;            // (s + 1) + e: first + last 1-based rank of the group
        if (p == s) {
            const u64 tot = incl[n - 1], cs = s > 0 ? incl[s - 1] : 0ull, ce = incl[e - 1];
            const long tp = (long)(tot >> 32) - (long)(cs >> 32);                               // positives at or above this threshold
            const long nn = (long)(tot & 0xffffffffull) - (long)(cs & 0xffffffffull);           // used rows at or above it
            const long dtp = (long)(ce >> 32) - (long)(cs >> 32);                               // positives of this group
            if (dtp > 0 && nn > 0) term = (double)dtp * (double)tp / (double)nn;
        }
    }
    sh[t] = term;
    __syncthreads();
    for (int o = PR_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(PR_THREADS) void pairs_final_kernel(const double* __restrict__ partial, int n_part, const u64* __restrict__ incl,
                                                                 int n, long long* __restrict__ n_pos, long long* __restrict__ n_used,
                                                                 double* __restrict__ ap_num) {
    __shared__ double sh[PR_THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < n_part; i += PR_THREADS) acc += partial[i];
    sh[t] = acc;
    __syncthreads();
    for (int o = PR_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const u64 tot = incl[n - 1];
        *n_pos = (long long)(tot >> 32);
        *n_used = (long long)(tot & 0xffffffffull);
        *ap_num = sh[0];
    }
}

#define HIPC(ctx, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return SGPT_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

sgpt_status fail(sgpt_ctx* c, const std::string& m) {
    if (c) c->err = m;
    return SGPT_ERR_INVALID;
}

// grow-only evaluation workspace (ctx.h: ws5)
sgpt_status ensure_ws5(sgpt_ctx* c, size_t need) {
    if (c->ws5_bytes >= need) return SGPT_OK;
    if (c->ws5) { HIPC(c, hipDeviceSynchronize()); HIPC(c, hipFree(c->ws5)); c->ws5 = nullptr; c->ws5_bytes = 0; }
    need = (need + (need >> 3) + (1 << 20) - 1) >> 20 << 20;
    if (hipMalloc(&c->ws5, need) != hipSuccess) {
        c->ws5 = nullptr;
        c->err = "hipMalloc evaluation workspace failed";
        return SGPT_ERR_OOM;
    }
    c->ws5_bytes = need;
    c->generation++;
    return SGPT_OK;
}

}  // namespace

extern "C" sgpt_status sgpt_eval_groups(sgpt_ctx* c, const float* emb, int32_t n_rows, int32_t d, int32_t mode, const float* scores_in,
                                        int32_t G, const int32_t* grp_off, int32_t n_cand, int32_t max_group, const int32_t* q_row,
                                        const int32_t* cand_row, const int32_t* cand_rel, const int32_t* R_extra,
                                        const int32_t* ideal_off, const int32_t* ideal_rel, int32_t n_ideal, float* out_scores,
                                        int32_t* out_order, int32_t* out_hits1, int32_t* out_hits5, int32_t* out_first, int32_t* out_R, float* out_sp,
                                        float* out_dcg, float* out_idcg, void* stream) {
    if (!c) return SGPT_ERR_INVALID;
    if (G < 0 || n_cand < 0 || max_group < 0 || n_ideal < 0)
        return fail(c, "sgpt_eval_groups: G, n_cand, max_group and n_ideal must not be negative");
    if (max_group > SGPT_EVAL_MAX_GROUP)
        return fail(c, "sgpt_eval_groups: a group of " + std::to_string(max_group) + " candidates; at most " +
                           std::to_string(SGPT_EVAL_MAX_GROUP) + " are served");
    if (!scores_in) {
        if (mode != SGPT_COS && mode != SGPT_DOT && mode != SGPT_NEG_L2)
            return fail(c, "sgpt_eval_groups: mode must be SGPT_COS, SGPT_DOT or SGPT_NEG_L2");
        if (n_rows < 0 || d < 1) return fail(c, "sgpt_eval_groups: n_rows >= 0 and d >= 1 are required");
    }
    if ((ideal_off == nullptr) != (ideal_rel == nullptr)) return fail(c, "sgpt_eval_groups: ideal_off and ideal_rel go together");
    if (G == 0) return SGPT_OK;
    if (!grp_off || !out_hits1 || !out_hits5 || !out_first || !out_R || !out_sp || !out_dcg || !out_idcg)
        return fail(c, "sgpt_eval_groups: null pointer");
    if (n_cand > 0 && (!cand_rel || (!scores_in && (!emb || !cand_row || !q_row)))) return fail(c, "sgpt_eval_groups: null pointer");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    GroupArgs a;
    a.emb = emb; a.n_rows = n_rows; a.d = d; a.mode = mode; a.scores_in = scores_in;
    a.G = G; a.grp_off = grp_off; a.n_cand = n_cand;
    a.q_row = q_row; a.cand_row = cand_row; a.cand_rel = cand_rel; a.R_extra = R_extra;
    a.ideal_off = ideal_off; a.ideal_rel = ideal_rel; a.n_ideal = n_ideal;
    a.out_scores = out_scores; a.out_order = out_order; a.out_hits1 = out_hits1; a.out_hits5 = out_hits5; a.out_first = out_first;
    a.out_R = out_R; a.out_sp = out_sp; a.out_dcg = out_dcg; a.out_idcg = out_idcg;
    hipLaunchKernelGGL(groups_wave_kernel, dim3((G + GR_WAVES - 1) / GR_WAVES), dim3(GR_THREADS), 0, s, a);
    HIPC(c, hipGetLastError());
    // both kernels see every group and pick by its size on the device: max_group is never trusted for that
    hipLaunchKernelGGL(groups_block_kernel, dim3(G), dim3(PR_THREADS), 0, s, a);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

extern "C" sgpt_status sgpt_eval_pairs(sgpt_ctx* c, const float* score, const int32_t* label, int32_t n, int32_t check_nan,
                                       int32_t* out_rank2, int64_t* out_n_pos, int64_t* out_n_used, double* out_ap_num, void* stream) {
    if (!c) return SGPT_ERR_INVALID;
    if (n < 0 || n > SGPT_EVAL_MAX_PAIRS)
        return fail(c, "sgpt_eval_pairs: 0 <= n <= " + std::to_string(SGPT_EVAL_MAX_PAIRS) + " is required");
    if (!out_n_pos || !out_n_used || !out_ap_num) return fail(c, "sgpt_eval_pairs: null pointer");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIPC(c, hipMemsetAsync(out_n_pos, 0, sizeof(int64_t), s));
        HIPC(c, hipMemsetAsync(out_n_used, 0, sizeof(int64_t), s));
        HIPC(c, hipMemsetAsync(out_ap_num, 0, sizeof(double), s));
        return SGPT_OK;
    }
    if (!score || !label || !out_rank2) return fail(c, "sgpt_eval_pairs: null pointer");
    int np2 = PR_TILE;
    while (np2 < n) np2 <<= 1;
    const int nblk = np2 / PR_SCAN, n_part = np2 / PR_THREADS;
    sgpt_status st = ensure_ws5(c, ((size_t)np2 * 2 + nblk + n_part) * 8);
    if (st != SGPT_OK) return st;
    u64* keys = (u64*)c->ws5;
    u64* incl = keys + np2;
    u64* bsum = incl + np2;
    double* partial = (double*)(bsum + nblk);
    int* flag = c->range_flag + PR_FLAG_WORD;
    HIPC(c, hipMemsetAsync(flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(pairs_keys_kernel, dim3(np2 / PR_THREADS), dim3(PR_THREADS), 0, s, score, n, np2, keys, flag);
    launch_sort_u64(keys, np2, s);
    hipLaunchKernelGGL(pairs_block_sums_kernel, dim3(nblk), dim3(PR_THREADS), 0, s, keys, label, n, bsum);
    hipLaunchKernelGGL(pairs_scan_sums_kernel, dim3(1), dim3(PR_THREADS), 0, s, bsum, nblk);
    hipLaunchKernelGGL(pairs_scan_kernel, dim3(nblk), dim3(PR_THREADS), 0, s, keys, label, n, bsum, incl);
    hipLaunchKernelGGL(pairs_rank_kernel, dim3(n_part), dim3(PR_THREADS), 0, s, keys, incl, n, out_rank2, partial);
    hipLaunchKernelGGL(pairs_final_kernel, dim3(1), dim3(PR_THREADS), 0, s, partial, n_part, incl, n, (long long*)out_n_pos,
                       (long long*)out_n_used, out_ap_num);
    HIPC(c, hipGetLastError());
    if (check_nan) {
        int h = 0;
        HIPC(c, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
        if (h) return fail(c, "sgpt_eval_pairs: a score is NaN (check_nan)");
    }
    return SGPT_OK;
}
