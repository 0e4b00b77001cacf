// Retrieval metrics taken where the ranked lists already live (include/sgpt_hip.h::sgpt_eval_ranked).
//
// The reference driver hands the search result -- Dict[qid, Dict[doc_id, float]], k = 1000 + 1 entries per query -- to
// beir.EvaluateRetrieval.evaluate (biencoder/beir/beir_dense_retriever.py:446), which needs, per query and cut, a handful of
// sums over the ranked list: hits@k, the rank of the first relevant document, DCG@k, IDCG@k and the sum of precisions at the
// relevant ranks.  This kernel takes those sums from the device-resident [nq, K] lists that sgpt_topk_merge /
// sgpt_exchange_topk leave behind, so an evaluation run moves nq x nk x a few words to the host instead of nq x K pairs.
//
// One wavefront per query, EV_WAVES queries per workgroup.  Lane l of chunk c looks at rank i = 64 c + l + 1:
//   - the corpus position idx[q][i - 1] is looked up in the query's judged positions (sorted ascending; a lower-bound binary
//     search through L2, or through LDS when the query has more than EV_STAGE_MIN judgements and at most EV_STAGE_MAX);
//   - hits@i is the ballot prefix of "relevant" plus the count carried from the earlier chunks (integers: exact);
//   - the float sums have ONE order whatever the launch geometry: the xor-butterfly sum of a chunk's 64 terms (terms past the
//     cut or past the end of the list are zeros), chunks added in ascending order.  Cut j's running values live in lane j, so
//     no per-thread array is indexed at run time (no scratch).
// A position < 0 is padding and ends the list.  No float atomics; the only atomic is the vector atomicOr of the order check.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/sgpt_hip.h"
#include "common.h"
#include "ctx.h"

namespace {

constexpr int EV_WAVES = 4;              // queries per workgroup
constexpr int EV_STAGE_MIN = 256;        // more judgements than this: the judged positions are staged in LDS ...
constexpr int EV_STAGE_MAX = 2048;       // ... when they fit (4 waves x 2048 x 8 B = 64 KiB); longer lists are searched in L2
constexpr int EV_FLAG_WORD = 32;         // word of the ctx's 256-byte flag block that collects the order check (16: sgpt_row_crest)

struct EvalCuts { int nk; int k[SGPT_EVAL_MAX_CUTS]; };

// first j in [0, n) with list[j] >= key (n if none)
template <typename P>
__device__ __forceinline__ int lower_bound(P list, int n, int64_t key) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = list[lo + half] < key;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

__device__ __forceinline__ int popc_below_incl(unsigned long long m, int lane) {   // set bits of m at lanes 0 .. lane
    return __popcll(m & (~0ull >> (63 - lane)));
}

__global__ __launch_bounds__(EV_WAVES * WAVE) void eval_ranked_kernel(
    const int64_t* __restrict__ idx, const float* __restrict__ val, int nq, int K, const int* __restrict__ qoff,
    const int64_t* __restrict__ qpos, const int* __restrict__ qrel, const int* __restrict__ ideal, EvalCuts cuts,
    int check_order, int* __restrict__ order_flag, int* __restrict__ out_hits, int* __restrict__ out_first,
    float* __restrict__ out_dcg, float* __restrict__ out_idcg, float* __restrict__ out_sp, int* __restrict__ out_R) {
    __shared__ int64_t sh_pos[EV_WAVES][EV_STAGE_MAX];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int q = blockIdx.x * EV_WAVES + wave;
    const bool active = q < nq;
    const int qc = active ? q : 0;                                   // every load below is addressed in bounds
    const int j0 = qoff[qc];
    const int nj = active ? max(qoff[qc + 1] - j0, 0) : 0;
    const int64_t* jpos = qpos + j0;
    const bool staged = nj > EV_STAGE_MIN && nj <= EV_STAGE_MAX;
    if (staged)
        for (int j = lane; j < nj; j += WAVE) sh_pos[wave][j] = jpos[j];
    __syncthreads();
    if (!active) return;

    const int nk = cuts.nk;
    const int my_k = lane < nk ? cuts.k[lane] : 0;                   // lane j owns cut j
    const int kmax = __shfl(my_k, nk - 1, WAVE);
    const int64_t* row_i = idx + (long)q * K;
    const float* row_v = val + (long)q * K;                          // read only under check_order (val may be null otherwise)

    // ---- R and IDCG@k from the query's grades in descending order ----
    int R = 0, jdone = 0;
    float idcg = 0.f;
    for (int c0 = 0; c0 < nj; c0 += WAVE) {
        const int j = c0 + lane;
        const int g = ideal[j0 + min(j, nj - 1)];
        const bool pos = j < nj && g > 0;
        const unsigned long long m = __ballot(pos);
        R += __popcll(m);
        if (m == 0) break;                                           // descending: nothing but non-positive grades from here on
        if (c0 >= kmax) continue;
        const float term = pos ? (float)g / log2f((float)(j + 2)) : 0.f;
        const float full = wave_sum(term);
        for (int t = jdone; t < nk; ++t) {
            const int kt = __shfl(my_k, t, WAVE);
            const float s = kt >= c0 + WAVE ? full : wave_sum(j < kt ? term : 0.f);
            if (lane == t) idcg += s;
            if (kt <= c0 + WAVE) jdone = t + 1;                      // cut t lies inside (or at the end of) this chunk: complete
        }
    }

    // ---- the ranked list ----
    int hits = 0, first = 0, carry = 0, done = 0;                    // carry: relevant documents in the chunks before this one
    float dcg = 0.f, sp = 0.f;
    int bad = 0;
    const int n_scan = check_order ? K : kmax;                       // the order check covers the whole row, the sums stop at the deepest cut
    for (int c0 = 0; c0 < n_scan && (check_order || done < nk); c0 += WAVE) {
        const int r = c0 + lane;                                     // 0-based rank
        const int rc = min(r, K - 1);
        const int64_t p = row_i[rc];
        const unsigned long long padm = __ballot(r < K && p < 0);
        const int n_end = padm ? c0 + (int)__builtin_ctzll(padm) : K;   // the list ends at the first padding entry
        const bool valid = r < n_end;
        int g = 0;
        if (valid && nj > 0 && done < nk) {
            const int at = staged ? lower_bound(&sh_pos[wave][0], nj, p) : lower_bound(jpos, nj, p);
            const int atc = min(at, nj - 1);
            const int64_t found = staged ? sh_pos[wave][atc] : jpos[atc];
            if (at < nj && found == p) g = qrel[j0 + atc];
        }
        if (check_order) {
            const int r1 = min(r + 1, K - 1);
            const float a = row_v[rc], b = row_v[r1];
            const int64_t p1 = row_i[r1];
            if (valid && r + 1 < K && p1 >= 0 && !(a >= b)) bad = 1;
        }
        const bool rel = valid && g > 0;
        const unsigned long long m = __ballot(rel);
        const int h_i = carry + popc_below_incl(m, lane);            // hits@(r + 1)
        const float t_dcg = rel ? (float)g / log2f((float)(r + 2)) : 0.f;
        const float t_sp = rel ? (float)h_i / (float)(r + 1) : 0.f;
        const float full_dcg = wave_sum(t_dcg), full_sp = wave_sum(t_sp);
        for (int t = done; t < nk; ++t) {
            const int kt = __shfl(my_k, t, WAVE);
            const bool whole = kt >= c0 + WAVE;
            const unsigned long long mk = whole ? m : (m & (~0ull >> (63 - (kt - c0 - 1))));   // kt > c0 here: cuts ascend
            const float s_dcg = whole || m == 0 ? full_dcg : wave_sum(r < kt ? t_dcg : 0.f);
            const float s_sp = whole || m == 0 ? full_sp : wave_sum(r < kt ? t_sp : 0.f);
            if (lane == t) {
                dcg += s_dcg; sp += s_sp; hits += __popcll(mk);
                if (first == 0 && mk) first = c0 + (int)__builtin_ctzll(mk) + 1;
            }
            if (kt <= c0 + WAVE) done = t + 1;
        }
        carry += __popcll(m);
        if (padm) break;
    }

    if (lane < nk) {
        const long o = (long)q * nk + lane;
        out_hits[o] = hits; out_first[o] = first; out_dcg[o] = dcg; out_idcg[o] = idcg; out_sp[o] = sp;
    }
    if (lane == 0) out_R[q] = R;
    if (check_order && __ballot(bad) && lane == 0) atomicOr(order_flag, 1);
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

}  // namespace

extern "C" sgpt_status sgpt_eval_ranked(sgpt_ctx* c, const int64_t* idx, const float* val, int32_t nq, int32_t K,
                                        const int32_t* qrel_off, const int64_t* qrel_pos, const int32_t* qrel_rel,
                                        const int32_t* ideal_rel, const int32_t* k_values, int32_t nk, int32_t check_order,
                                        int32_t* out_hits, int32_t* out_first, float* out_dcg, float* out_idcg, float* out_sp,
                                        int32_t* out_R, void* stream) {
    if (!c) return SGPT_ERR_INVALID;
    if (nq < 0 || K <= 0) return fail(c, "sgpt_eval_ranked: nq >= 0 and K >= 1 are required");
    if (!k_values || nk < 1 || nk > SGPT_EVAL_MAX_CUTS)
        return fail(c, "sgpt_eval_ranked: between 1 and " + std::to_string(SGPT_EVAL_MAX_CUTS) + " cuts are required");
    EvalCuts cuts;
    cuts.nk = nk;
    for (int t = 0; t < SGPT_EVAL_MAX_CUTS; ++t) cuts.k[t] = 0;
    for (int t = 0; t < nk; ++t) {
        if (k_values[t] < 1 || (t > 0 && k_values[t] <= k_values[t - 1]))
            return fail(c, "sgpt_eval_ranked: k_values must be positive and strictly ascending");
        if (k_values[t] > K)
            return fail(c, "sgpt_eval_ranked: cut " + std::to_string(k_values[t]) + " is deeper than the lists (K = " +
                               std::to_string(K) + ")");
        cuts.k[t] = k_values[t];
    }
    if (nq == 0) return SGPT_OK;
    if (!idx || !qrel_off || !qrel_pos || !qrel_rel || !ideal_rel || !out_hits || !out_first || !out_dcg || !out_idcg || !out_sp ||
        !out_R || (check_order && !val))
        return fail(c, "sgpt_eval_ranked: null pointer");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int* flag = c->range_flag + EV_FLAG_WORD;
    if (check_order) HIPC(c, hipMemsetAsync(flag, 0, sizeof(int), s));
    const int blocks = (nq + EV_WAVES - 1) / EV_WAVES;
    hipLaunchKernelGGL(eval_ranked_kernel, dim3(blocks), dim3(EV_WAVES * WAVE), 0, s, idx, val, nq, K, qrel_off, qrel_pos,
                       qrel_rel, ideal_rel, cuts, check_order ? 1 : 0, flag, out_hits, out_first, out_dcg, out_idcg, out_sp,
                       out_R);
    HIPC(c, hipGetLastError());
    if (check_order) {
        int h = 0;
        HIPC(c, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
        if (h) return fail(c, "sgpt_eval_ranked: a ranked list is not sorted by descending score (check_order)");
    }
    return SGPT_OK;
}
