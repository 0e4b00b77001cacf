// What the host translation units of the C ABI share (ctx.hip, model.hip, encode.hip, score.hip, ops.hip): the model object behind
// `sgpt_model*`, the operand classes of a block, error / workspace helpers and the profiled GEMM launches.  Internal to csrc/:
// include/sgpt_hip.h does not include it, sgpt_model stays opaque outside.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sgpt_hip.h"
#include "common.h"
#include "ctx.h"


struct LayerW {
    void* w_qkv = nullptr;   // [3d, d]  (q rows, k rows, v rows)
    // split-precision copies, rows [W_hi | W_hi | W_lo] of 3 x the input width: w_qkv3 [2d or 3d, 3d] (qk_split alone: the q and k
    // rows; split_weights: q, k and v rows), w_o3 [d, 3d], w_fc3 [ffn, 3d], w_proj3 [d, 3 ffn]
    void *w_qkv3 = nullptr, *w_o3 = nullptr, *w_fc3 = nullptr, *w_proj3 = nullptr;
    void* w_o = nullptr;     // [d, d]
    void* w_fc = nullptr;    // [ffn, d]
    void* w_proj = nullptr;  // [d, ffn]
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *b_o, *b_fc, *b_proj;
    float* b_qkv = nullptr;  // BLOOM: [3d] de-interleaved (q | k | v) projection bias
    // SGPT_FP8W: w_* hold e4m3fn codes, s_* the per-output-channel power-of-two scales
    float *s_qkv = nullptr, *s_o = nullptr, *s_fc = nullptr, *s_proj = nullptr;
    int is_local = 0;
};

struct sgpt_model {
    sgpt_ctx* ctx;
    sgpt_model_desc d;
    std::vector<LayerW> L;
    float *wte = nullptr, *wpe = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    float *rot_sin = nullptr, *rot_cos = nullptr;   // GPT-J rotary tables [max_pos, rotary_dim/2]
    float *emb_ln_g = nullptr, *emb_ln_b = nullptr, *alibi = nullptr;   // BLOOM: embedding LayerNorm, ALiBi slopes [H]
    float* zero_bias = nullptr;                      // [max(d, ffn)] zeros: bias-free projections (GPT-J out_proj)
    float* pool_w = nullptr; int pool_w_n = 0;       // learntmean position weights (sgpt_model_set_pool_weights)
    float *lm_w = nullptr, *lm_b = nullptr;           // LM head [vocab, d] (+bias): tied to the embedding unless "lm_head.*" was given
    void* dq[4] = {nullptr, nullptr, nullptr, nullptr};   // SGPT_FP8W / FP8M: bf16 scratch for the current block's qkv / o / fc / proj
    // SGPT_FP8M (fp8 MFMA on the MLP projections): per-block power-of-two scale of the GELU output's e4m3 codes, set by
    // calibration; h_amax = device float bits [n_layers] collected while `calibrating`
    std::vector<float> act_scale;      // [2 * n_layers]: GELU-output scales, then attention-context scales
    unsigned* h_amax = nullptr;        // device float bits [2 * n_layers], same order
    bool calibrating = false;
    // SGPT_F16 range shifts: operand class c of block l is STORED as value * 2^-shift[l * RS_N + c] (classes: RS_*), the
    // consuming launches multiply their fp32 accumulators back (exact).  All 0 until a load-time bound or a run-time
    // magnitude asks for more (sgpt_model_range_adapt).  range_dev: device words [0] = flag (bit 0: an f16 store reached
    // RANGE_LIMIT, bit 1: an e4m3 code saturated), [1 + l * RS_N + c] = fp32 bits of the largest offending magnitude.
    std::vector<int> shift;
    unsigned* range_dev = nullptr;
    std::vector<int> ln_floor;         // [n_layers]: the LayerNorm shift sgpt_model_load derived from the parameters (set_range_shifts may not go below)
    // Precision plan: operand class c of block l enters its consumer as a split-precision (hi + lo) pair when prec[l * PC_N + c]
    // != 0 (classes: PC_*).  crest_dev: device fp32 bits [n_layers * RS_N] collected while `probing` (sgpt_model_precision_probe_*).
    std::vector<int> prec;
    bool split_all = false;            // the split copies of all four matrices exist (sgpt_model_desc.split_weights)
    int qkv3_rows = 0;                 // row blocks of w_qkv3: 2 (q, k: qk_split alone) | 3 (q, k, v: split_weights) | 0 (none)
    unsigned* crest_dev = nullptr;
    bool probing = false;
    std::vector<void*> allocs;
};

// operand classes of a block: LayerNorm-1 output, q | k | v (and the attention context, a convex combination of v rows),
// LayerNorm-2 output, GELU output
enum { RS_LN1 = 0, RS_QKV = 1, RS_LN2 = 2, RS_H = 3, RS_N = 4 };
// precision classes (include/sgpt_hip.h SGPT_PC_*): LayerNorm-1 output -> Q / K (/ V) projection; q | k | v | p inside the attention;
// attention context -> out-projection; LayerNorm-2 output -> fc1; GELU output -> fc2
enum { PC_LN1 = SGPT_PC_LN1, PC_ATT = SGPT_PC_ATT, PC_CTX = SGPT_PC_CTX, PC_LN2 = SGPT_PC_LN2, PC_H = SGPT_PC_H, PC_N = SGPT_PREC_CLASSES };
constexpr int RS_MAX_SHIFT = 40;
static inline float pow2f(int k) { return std::ldexp(1.0f, k); }

#define HIPC(ctx, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return SGPT_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

// (one namespace of their own: the library exports its C++ symbols, and these names are short)
namespace sgpt_host {

inline sgpt_status fail(sgpt_ctx* c, sgpt_status st, const std::string& m) {
    if (c) c->err = m;
    return st;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// environment switches of the measurement scripts: compiled in only with -DSGPT_EXPERIMENTS (libsgpt_hip_exp.so)
#ifdef SGPT_EXPERIMENTS
inline const char* exp_env(const char* name) { return getenv(name); }
#else
inline const char* exp_env(const char*) { return nullptr; }
#endif

// grow-only workspace (ctx.hip)
sgpt_status ensure(sgpt_ctx* c, void** p, size_t* have, size_t need);

struct Prof {  // brackets one GEMM launch with events when profiling is on
    sgpt_ctx* c; hipStream_t s; bool on; size_t slot = 0;
    Prof(sgpt_ctx* c_, hipStream_t s_, double flops) : c(c_), s(s_), on(c_->prof) {
        if (!on) return;
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            c->ev_pool.emplace_back(a, b);
            c->ev_flops.push_back(0);
        }
        slot = c->ev_used++;
        c->ev_flops[slot] = flops;
        (void)hipEventRecord(c->ev_pool[slot].first, s);
    }
    ~Prof() { if (on) (void)hipEventRecord(c->ev_pool[slot].second, s); }
};

// profiled launches with the per-ctx policies (ctx.hip)
void gemm(sgpt_ctx* c, int dtype, int epi, int out_dtype, const GemmArgs& a0, hipStream_t s);
// query-sized projection (qgemm.hip); false = not served, the caller launches gemm()
bool qgemm(sgpt_ctx* c, int dtype, int epi, int out_dtype, const QGemmArgs& a, hipStream_t s);

}  // namespace sgpt_host
using namespace sgpt_host;
