// The epilogue of the 64-query-row scorer tiles: score64_kernel (gemm.hip, f16 / bf16 rows) and score64c_kernel (score64c.h, one-byte
// codes).  Device-only.  A wave owns 32 documents n0 .. n0 + 31 for all 64 padded query rows; scores leave the registers directly:
// lane = query row m = 16 i + fr, documents n0 + 16 j + 4 g .. + 3 in acc[i][j].  A NaN score counts as -1 (exact_search.py:99).
//   EPI_SCORE         out[m][n] = score, rows m < p.m_valid.
//   EPI_SCORE_FILTER  (score, p.idx_base + n) of every score STRICTLY above thv[i] is appended to query m's candidate list (the running
//                     k-th best is a lower bound of the final one, and a later document never displaces an equal score); thv[i] = +inf
//                     for a padded row, which so never appends.  stage = this wave's 256 uint2 of LDS.
// RAGGED: the tile may reach past document p.N - 1.  EPI_SCORE stores only the columns that exist; on the filtered leg the caller has
// set the columns that do not exist to -inf, which beats no threshold (v > th is false for every th), so that leg is the same code.
// acc is zero on return: the next tile accumulates into it.
#pragma once
#include "common.h"

template <int EPI, bool RAGGED>
__device__ __forceinline__ void score64_epilogue(const GemmArgs& p, f32x4 (&acc)[4][2], const float (&thv)[4], const long n0, const int g,
                                                 const int fr, const int lane, uint2_a* stage) {
    if constexpr (EPI == EPI_SCORE_FILTER) {
        // Survivors are staged in LDS at positions the ballot itself gives (staged + mbcnt: no atomics) and appended in one flush per
        // tile; a row block whose lanes all fail the fast reject costs one scalar branch (gemm256_epilogue.inc has the measurements).
        int staged = 0;                                                // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = i * 16 + fr;
            const float th = thv[i];
            float mx = -INFINITY;                                // fast reject on the raw accumulators: fmaxf drops NaNs
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc[i][j][r]);
            // thresholds below -1 (dot scores): the per-lane path, NaN -> -1 may survive.  The rare leg: the staged one falls through.
            if (__builtin_expect(__ballot(th < -1.0f) != 0, 0)) {
                // cand_room is read only AFTER the lane has found a survivor (or cannot rule one out): a capacity load in front of the
                // test would put a global round trip on every row of every tile (see cand_room, common.h).  A list already over capacity
                // is recomputed by the fallback anyway, so its atomics are skipped.
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
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the staged entries are in LDS (one wave: in order)
            // ONE global round trip per flush: each lane takes one staged entry, and the atomicAdd itself says whether the list still
            // has room (a capacity load in front of it would be a second dependent round trip).
            if (staged <= 256) {
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
                // The overflow signal.  The storm case (every document beats the threshold) is bounded by the stage: a wave that
                // staged more than it holds appends nothing and pushes one list past its capacity with one atomic -- raw count > cap
                // is what cand_merge flags, and the chunk is recomputed by the fallback.
                atomicAdd(p.cand_cnt + (int)(stage[0].x >> 16), p.cand_cap + 1);
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
                    const long n = n0 + (j * 16 + 4 * g);
                    float* o = static_cast<float*>(p.out) + (long)m * p.ldo + n;
                    if (!RAGGED || n + 4 <= (long)p.N) *reinterpret_cast<float4*>(o) = v;
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
