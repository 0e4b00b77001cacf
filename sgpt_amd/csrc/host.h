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
    float* b_qkv = nullptr;  // BLOOM: [3d] de-interleaved (q | k | v) projection bias; SGPT_ARCH_LLAMA: [d_q + 2 d_kv] when the model has one (Qwen2)
    float *qn_g = nullptr, *kn_g = nullptr;   // SGPT_ARCH_LLAMA: per-head RMSNorm gains of q and k [head_dim] when the model has them (Qwen3)
    // SGPT_FP8W: w_* hold e4m3fn codes, s_* the per-output-channel power-of-two scales (a converted SGPT_ARCH_LLAMA model,
    // sgpt_model.proj8: all but w_o / s_o)
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
    bool bidir = false;                // SGPT_ARCH_LLAMA: every query sees every key of its sequence (sgpt_model_set_attention(0))
    // SGPT_ARCH_LLAMA, SGPT_BF16: 1 once sgpt_model_set_projections(1) has turned w_qkv / w_fc / w_proj of every layer into e4m3fn codes with
    // s_qkv / s_fc / s_proj (w_o stays 16-bit); the forward then runs block_llama_q8 (encode.hip).  One-way.
    int proj8 = 0;
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

// ---- what a model family is: one row per SGPT_ARCH_* value ("What a family consists of") ----
// A family that does not build a feature says so in its row and nowhere else: every refusal of model.hip / encode.hip reads this table,
// and outside it only the loader dispatch (model.hip) and the block dispatch (encode.hip) look at `arch` for these families.
enum { WIN_ANY, WIN_ZERO, WIN_NONNEG };            // sgpt_model_desc.window: any value | must be 0 | >= 0
struct Family {
    const char *name, *prefix, *wte, *lnf;   // name in messages; state dict: layer prefix, embedding tensor, final norm (null: it has none)
    int norm_kind;                     // final norm inside the pool (launch_lnf_pool): 0 LayerNorm | 1 RMSNorm
    // post_ln: every block ends in the LayerNorm that writes the residual stream (the fp32 blocks never write `a`).  swiglu: fc1 yields
    // gate | up columns ([T][2 ffn] scratch).  slack_f32: the fp32 forward zeroes the slack rows behind q | k | v -- the Llama fp32 forward
    // has never issued that memset ("the kernel reads no key past its query") and keeps not issuing it: to be settled on its own.
    bool post_ln, swiglu, slack_f32;
    // what the family builds: fp8 modes, split-precision operands, f16 range shifts, the precision probe, the query path, pooling modes
    bool fp8, split, shifts, probe, qpath, learntmean, cls;
    const char* no_lm;                 // sgpt_lm_logprobs: why it is refused (null: the LM head is built)
    // head dims its 16-bit attention serves: 64 and 128, with dh256 also 256 (the library-wide rule of check_desc); without it dh_rule
    // is the family's refusal of anything else, and dh_all: it holds for SGPT_F32 models too.  window: WIN_*.  gqa: n_kv_heads may
    // differ from n_heads.
    bool dh256; const char* dh_rule; bool dh_all; int window; bool gqa;
    // sgpt_model_set_attention: why the family's attention mode is not the caller's to set (null: it is -- causal or bidirectional)
    const char* attn_fixed;
};
constexpr Family FAMILIES[] = {
    // name, prefix, wte, lnf, norm_kind | post_ln, swiglu, slack_f32 | fp8, split, shifts, probe, qpath, learntmean, cls | no_lm |
    // dh256, dh_rule, dh_all, window, gqa | attn_fixed     (the bools of a row are grouped as in this line: 3, then 7, then dh256)
    {"SGPT_ARCH_GPTNEO", "h.", "wte.weight", "ln_f", 0, false, false, true,  true, true, true, true, true, true, true,  nullptr, true, nullptr, false, WIN_ANY, false, "stays causal"},
    {"SGPT_ARCH_GPTJ", "h.", "wte.weight", "ln_f", 0, false, false, true,  true, true, true, true, true, true, true,  nullptr, true, nullptr, false, WIN_ANY, false, "stays causal"},
    {"SGPT_ARCH_BLOOM", "h.", "word_embeddings.weight", "ln_f", 0, false, false, true,  true, true, true, true, true, true, true,  nullptr, true, nullptr, false, WIN_ANY, false, "stays causal"},
    {"SGPT_ARCH_BERT", "encoder.layer.", "embeddings.word_embeddings.weight", nullptr, 0, true, false, true,  false, false, false, false, false, false, true,
     "SGPT_ARCH_BERT carries no causal LM head", false, "16-bit bidirectional attention supports head_dim 64 or 128", false, WIN_ZERO, false,
     "is bidirectional by architecture"},
    {"SGPT_ARCH_LLAMA", "layers.", "embed_tokens.weight", "norm", 1, false, true, false,  false, false, false, false, false, false, false,
     "not built for SGPT_ARCH_LLAMA (the LM head of this family is not loaded)", false, "head_dim 64 or 128", true, WIN_NONNEG, true, nullptr},
};
constexpr int N_FAMILIES = sizeof(FAMILIES) / sizeof(FAMILIES[0]);
static_assert(SGPT_ARCH_GPTNEO == 0 && SGPT_ARCH_GPTJ == 1 && SGPT_ARCH_BLOOM == 2 && SGPT_ARCH_BERT == 3 && SGPT_ARCH_LLAMA == 4 && N_FAMILIES == 5, "FAMILIES is indexed by SGPT_ARCH_*");
inline const Family& family(int arch) { return FAMILIES[arch]; }
// head dim of a descriptor: SGPT_ARCH_LLAMA carries an explicit one in rotary_dim (0 = d_model / n_heads), so n_heads * head_dim -- the
// query width d_q -- need not be d_model there
inline int head_dim(const sgpt_model_desc& d) { return d.arch == SGPT_ARCH_LLAMA && d.rotary_dim > 0 ? d.rotary_dim : d.d_model / d.n_heads; }
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
