// The context object behind `sgpt_ctx*` (include/sgpt_hip.h), shared by the host translation units (host.h) and comm.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

struct sgpt_ctx {
    int device = 0;
    std::string err;
    // grow-only workspaces
    void* ws = nullptr; size_t ws_bytes = 0;        // encoder activations
    void* ws2 = nullptr; size_t ws2_bytes = 0;      // scorer: score chunk + ping-pong top-k
    void* ws3 = nullptr; size_t ws3_bytes = 0;      // multi-GPU exchange staging (comm.hip)
    void* ws4 = nullptr; size_t ws4_bytes = 0;      // refined / binary-corpus scorer: 16-bit or packed queries, stage-1 lists, candidate list, saved running list, flag
    void* ws5 = nullptr; size_t ws5_bytes = 0;      // evaluation (useb_eval.hip): sort keys, flag scan, block partials of sgpt_eval_pairs
    void* ws6 = nullptr; size_t ws6_bytes = 0;      // fp8 corpus (sgpt_score_topk_q8): f16 rows of the de-quantised block / ragged tail
    void* ws7 = nullptr; size_t ws7_bytes = 0;      // IVF corpus (ivf.hip): sort keys, chunk partials; f16 queries, probe sets, candidate lists of sgpt_ivf_search
    size_t filt_flag_off = 0; int filt_chunks = 0;   // scorer: overflow flags (offset into ws2, which only grows) of the last pass's filtered chunks (sgpt_score_overflow_count)
    void* comm = nullptr;                         // ncclComm_t of this ctx (sgpt_comm_init), one per process / GPU
    int comm_rank = 0, comm_world = 0;
    // bumped whenever a library-owned buffer that launched kernels point into is re-allocated (workspace growth,
    // learnt pooling weights): a hipGraph captured earlier holds stale pointers once this moves (sgpt_ctx_generation)
    uint64_t generation = 0;
    int* range_flag = nullptr;                      // device int: an f16 activation left the representable range (ctx-level ops: sgpt_linear*)
    int kgroups = 1;                                // low-latency mode: 2 = k-groups for query-sized launches (sgpt_ctx_set_low_latency)
    int force256 = 0;                               // tile policy: 1 = 256x256 tiles even for small problems (sgpt_ctx_set_tile_policy)
    int no_qpath = 0;                               // tile policy 2: query- / mid-sized layouts keep the bulk path's small-tile kernels (A/B, tests)
    int cu_cap = 0;                                 // persistent 256x256 GEMM: workgroups per launch at most (0 = one per CU; sgpt_ctx_set_gemm_cu_cap)
    int qtile = 0;                                  // sgpt_linear_query only: k > 0 = the k-th candidate tile of qgemm.hip (0 = the launcher's choice; sgpt_ctx_set_query_tile)
    // a bulk encode call as two chains of whole sequences (encode.hip; sgpt_ctx_set_encode_chains): 0 = the library's default,
    // 1 = one chain, 2 = two wherever the conditions hold; chain_min_rows > 0 replaces the row threshold.  Chain A runs on the
    // caller's stream, chain B on chain_stream (non-blocking); chain_ev = fork, chain B's start, join.  Created by the first
    // call that is cut (chain_init), destroyed with the context.
    int chains = 0, chain_min_rows = 0;
    hipStream_t chain_stream = nullptr;
    hipEvent_t chain_ev[3] = {nullptr, nullptr, nullptr};
    int64_t chain_calls = 0;                        // calls that ran as two chains (sgpt_ctx_encode_chain_calls)
    // GEMM profiling (bench.py roofline)
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    std::vector<double> ev_flops;
    int64_t prof_launches = 0; double prof_ms = 0, prof_flops = 0;
};
