// C ABI (include/sgpt_hip.h): packed weights (load / free), learnt pooling weights, FP8M calibration, the f16 range guard and
// the precision plan of a model, the attention mode and the fp8 projections of a Llama-family model.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
#include "host.h"

namespace {

// Every refusal sgpt_model_load makes on the descriptor alone.  The order is part of the ABI's behaviour: where a descriptor breaks
// several rules, the first one here answers.  The family rules come from the family's row (host.h).
sgpt_status check_desc(sgpt_ctx* c, const sgpt_model_desc* d) {
    if (d->arch < 0 || d->arch >= N_FAMILIES) return fail(c, SGPT_ERR_INVALID, "arch must be SGPT_ARCH_GPTNEO, SGPT_ARCH_GPTJ, SGPT_ARCH_BLOOM, SGPT_ARCH_BERT or SGPT_ARCH_LLAMA");
    const Family& F = family(d->arch); const std::string fam = std::string(F.name) + ": ";
    const int dm = d->d_model, ffn = d->d_ffn, H = d->n_heads, cd = d->compute_dtype;
    if (dm % 128 || ffn % 128 || H <= 0 || dm % H) return fail(c, SGPT_ERR_INVALID, "d_model and d_ffn must be multiples of 128");
    const int dh = head_dim(*d);
    const bool fp8 = cd == SGPT_FP8W || cd == SGPT_FP8M, split = d->qk_split != 0 || d->split_weights != 0;
    if (cd != SGPT_F32 && dh != 64 && dh != 128 && dh != 256) return fail(c, SGPT_ERR_INVALID, "16-bit attention supports head_dim 64, 128 or 256");
    if (dh > 256 || dh % 4) return fail(c, SGPT_ERR_INVALID, "head_dim must be <= 256 and a multiple of 4");
    if (dm > 4096) return fail(c, SGPT_ERR_INVALID, "d_model > 4096 not supported");
    if (cd != SGPT_BF16 && cd != SGPT_F32 && cd != SGPT_F16 && !fp8) return fail(c, SGPT_ERR_INVALID, "bad compute_dtype");
    if (d->arch == SGPT_ARCH_GPTJ && (d->rotary_dim <= 0 || d->rotary_dim > dh || d->rotary_dim % 2)) return fail(c, SGPT_ERR_INVALID, "GPT-J needs an even rotary_dim in (0, head_dim]");
    if (split && cd != SGPT_F16 && cd != SGPT_BF16) return fail(c, SGPT_ERR_INVALID, "qk_split / split_weights apply to SGPT_F16 / SGPT_BF16 models");
    // (a family without them has one arithmetic per operand format: no fp8 storage / MFMA, no split-precision operands)
    if (fp8 && !F.fp8) return fail(c, SGPT_ERR_INVALID, fam + "compute_dtype SGPT_F32, SGPT_F16 or SGPT_BF16 (no fp8 mode for this family)");
    if (split && !F.split) return fail(c, SGPT_ERR_INVALID, fam + "qk_split / split_weights (split-precision operands) are not available for this family");
    if (!F.dh256 && (F.dh_all || cd != SGPT_F32) && dh != 64 && dh != 128) return fail(c, SGPT_ERR_INVALID, fam + F.dh_rule);
    if (F.gqa && (d->n_kv_heads < 0 || (d->n_kv_heads > 0 && H % d->n_kv_heads))) return fail(c, SGPT_ERR_INVALID, fam + "n_heads % n_kv_heads == 0 (0 = n_heads)");
    if (F.window == WIN_ZERO && d->window != 0) return fail(c, SGPT_ERR_INVALID, fam + "window must be 0");
    if (F.window == WIN_NONNEG && d->window < 0) return fail(c, SGPT_ERR_INVALID, fam + "window >= 0");
    if (!F.gqa && d->n_kv_heads != 0 && d->n_kv_heads != H) return fail(c, SGPT_ERR_INVALID, "n_kv_heads (grouped K / V) belongs to SGPT_ARCH_LLAMA");
    // an explicit head dim (SGPT_ARCH_LLAMA, rotary_dim > 0): the query width n_heads * head_dim is the K of the out-projection
    if (d->arch == SGPT_ARCH_LLAMA && d->rotary_dim > 0 && (H * d->rotary_dim) % 128)
        return fail(c, SGPT_ERR_INVALID, fam + "n_heads * rotary_dim (the query width) must be a multiple of 128");
    if (d->arch == SGPT_ARCH_LLAMA && d->rotary_dim > 0 && H * d->rotary_dim > 4096)
        return fail(c, SGPT_ERR_INVALID, fam + "n_heads * rotary_dim (the query width) > 4096 not supported");
    return SGPT_OK;
}

// One sgpt_model_load at work: the caller's tensors by name, the model being filled, the packed format and the running status.  A
// failure is recorded in `st` (the last one answers) and ends the layer loop of the family's loader.
struct Loader {
    sgpt_ctx* c; const sgpt_model_desc* d; sgpt_model* m;
    std::unordered_map<std::string, const sgpt_tensor_view*> byname;
    unsigned* stats;           // SGPT_F16 range audit: [0] = max|matmul weight|, [1] = max|LayerNorm gamma|, [2] = max|LayerNorm beta|
    bool fp8, f16, bf;         // bf: 16-bit packed weights (bf16 or f16)
    size_t esz; int dm, ffn, H, dh; sgpt_status st;

    const float* find(const std::string& name, int64_t numel) {
        auto it = byname.find(name);
        if (it == byname.end()) { st = fail(c, SGPT_ERR_MISSING, "missing weight tensor: " + name); return nullptr; }
        if (it->second->numel != numel) { st = fail(c, SGPT_ERR_INVALID, "wrong numel for " + name); return nullptr; }
        return it->second->ptr;
    }
    void* dalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { st = fail(c, SGPT_ERR_OOM, "hipMalloc weights failed"); return nullptr; }
        m->allocs.push_back(p);
        return p;
    }
    float* copy_f32(const std::string& name, int64_t numel) {
        const float* src = find(name, numel);
        if (!src) return nullptr;
        float* dst = (float*)dalloc(numel * 4);
        if (!dst) return nullptr;
        if (hipMemcpyAsync(dst, src, numel * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess) st = fail(c, SGPT_ERR_HIP, "memcpy " + name);
        return dst;
    }
    // LayerNorm parameters whose output is rounded to the 16-bit GEMM operand format
    void copy_ln(const std::string& base, float** g, float** b) {
        *g = copy_f32(base + ".weight", dm);
        *b = copy_f32(base + ".bias", dm);
        if (f16 && *g && *b) { launch_absmax(*g, dm, stats + 1, 0); launch_absmax(*b, dm, stats + 2, 0); }
    }
    // matmul weight [rows, cols] -> packed dtype at row `row_off` of dst (fp8: codes + one scale per row)
    void pack_rows(const float* src, int64_t rows, int64_t cols, void* dst, int64_t row_off, float* scale) {
        const int64_t off = row_off * cols, numel = rows * cols;
        if (fp8) launch_fp8_quant_rows(src, rows, cols, (uint8_t*)dst + off, scale + row_off, 0);
        else if (bf) {
            launch_f32_to_16(src, numel, (bf16_t*)dst + off, f16 ? DT_F16 : DT_BF16, 0);
            if (f16) launch_absmax(src, numel, stats + 0, 0);
        }
        else if (hipMemcpyAsync((float*)dst + off, src, numel * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess)
            st = fail(c, SGPT_ERR_HIP, "memcpy weight");
    }
    void pack_w(const std::string& name, int64_t rows, int64_t cols, void* dst, int64_t row_off, float* scale) {
        const float* src = find(name, rows * cols);
        if (src) pack_rows(src, rows, cols, dst, row_off, scale);
    }
    // the split-precision copy [W_hi | W_hi | W_lo] of a whole matrix
    void pack3(const std::string& name, int64_t rows, int64_t cols, void* dst3) {
        const float* src = find(name, rows * cols);
        if (src) launch_pack_split_rows(src, rows, cols, dst3, f16 ? DT_F16 : DT_BF16, 0);
    }
    // the four packed matrices of a block: w_qkv [qkv_rows, d], w_o [d, o_cols], w_fc [fc_rows, d], w_proj [d, ffn]
    void alloc_w(LayerW& l, size_t qkv_rows, size_t fc_rows, size_t o_cols) {
        l.w_qkv = dalloc(qkv_rows * dm * esz); l.w_o = dalloc((size_t)dm * o_cols * esz);
        l.w_fc = dalloc(fc_rows * dm * esz); l.w_proj = dalloc((size_t)dm * ffn * esz);
    }
    // What follows a family's own embedding tensors, in the order the tensors have always been read: the LM head, the final norm the
    // family's row names, the zero bias vector.
    void head() {
        const Family& F = family(d->arch);
        // LM head of the cross-encoder scorer (crossencoder/beir/sgptce.py): GPT-Neo / BLOOM tie it to the embedding
        // (HF tie_word_embeddings), GPT-J carries lm_head.weight / lm_head.bias
        m->lm_w = m->wte;
        if (byname.count("lm_head.weight")) {
            m->lm_w = copy_f32("lm_head.weight", (int64_t)d->vocab * dm);
            if (byname.count("lm_head.bias")) m->lm_b = copy_f32("lm_head.bias", d->vocab);
        }
        if (F.lnf) m->lnf_g = copy_f32(std::string(F.lnf) + ".weight", dm);
        if (F.lnf && F.norm_kind == 0) m->lnf_b = copy_f32(std::string(F.lnf) + ".bias", dm);       // (an RMSNorm is a gain, no bias)
        m->zero_bias = (float*)dalloc((size_t)(ffn > dm ? ffn : dm) * 4);
        if (m->zero_bias && hipMemsetAsync(m->zero_bias, 0, (size_t)(ffn > dm ? ffn : dm) * 4, 0) != hipSuccess)
            st = fail(c, SGPT_ERR_HIP, "memset zero_bias");
        m->L.resize(d->n_layers);
    }
};

// GPT-Neo / GPT-J / BLOOM.  HF state-dict names:
//   GPT-Neo h.N.attn.attention.{q,k,v,out}_proj / mlp.c_fc / mlp.c_proj          (HF:gpt_neo:84-87,302-303)
//   GPT-J   h.N.attn.{q,k,v,out}_proj (no biases) / mlp.fc_in / mlp.fc_out          (HF:gptj:98-101,368-369)
//   BLOOM   h.N.self_attention.{query_key_value,dense} / mlp.dense_h_to_4h / mlp.dense_4h_to_h,
//           input_layernorm / post_attention_layernorm                               (HF:bloom:197-198,320-322,351-354)
void load_decoder(Loader& L) {
    sgpt_model* m = L.m; const sgpt_model_desc* d = L.d;
    const int dm = L.dm, ffn = L.ffn, H = L.H, dh = L.dh;
    const bool gptj = d->arch == SGPT_ARCH_GPTJ, bloom = d->arch == SGPT_ARCH_BLOOM, fp8 = L.fp8;
    if (gptj) {
        m->rot_sin = L.copy_f32("rotary.sin", (int64_t)d->max_pos * (d->rotary_dim / 2));
        m->rot_cos = L.copy_f32("rotary.cos", (int64_t)d->max_pos * (d->rotary_dim / 2));
    } else if (bloom) {
        m->emb_ln_g = L.copy_f32("word_embeddings_layernorm.weight", dm);
        m->emb_ln_b = L.copy_f32("word_embeddings_layernorm.bias", dm);
        m->alibi = L.copy_f32("alibi.slopes", H);
    } else {
        m->wpe = L.copy_f32("wpe.weight", (int64_t)d->max_pos * dm);
    }
    L.head();
    const std::string attn = gptj ? "attn." : "attn.attention.";
    const std::string fc1 = bloom ? "mlp.dense_h_to_4h" : (gptj ? "mlp.fc_in" : "mlp.c_fc");
    const std::string fc2 = bloom ? "mlp.dense_4h_to_h" : (gptj ? "mlp.fc_out" : "mlp.c_proj");
    const std::string ln1 = bloom ? "input_layernorm" : "ln_1", ln2 = bloom ? "post_attention_layernorm" : "ln_2";
    float* stage = bloom ? (float*)L.dalloc((size_t)3 * dm * dm * 4) : nullptr;   // BLOOM: fp32 staging for the de-interleaved fused QKV weight
    const bool split_all = m->d.split_weights != 0, split = m->d.qk_split != 0 || split_all;
    const int dt16 = L.f16 ? DT_F16 : DT_BF16;
    for (int i = 0; i < d->n_layers && L.st == SGPT_OK; ++i) {
        const std::string p = family(d->arch).prefix + std::to_string(i) + ".";
        LayerW& l = m->L[i];
        l.is_local = (gptj || bloom) ? 0 : (d->layer_is_local ? d->layer_is_local[i] : (i & 1));
        L.copy_ln(p + ln1, &l.ln1_g, &l.ln1_b);
        if (!gptj) L.copy_ln(p + ln2, &l.ln2_g, &l.ln2_b);
        else l.ln2_g = l.ln2_b = nullptr;
        const std::string wo = p + (bloom ? std::string("self_attention.dense") : attn + "out_proj");
        l.b_o = gptj ? m->zero_bias : L.copy_f32(wo + ".bias", dm);
        l.b_fc = L.copy_f32(p + fc1 + ".bias", ffn);
        l.b_proj = L.copy_f32(p + fc2 + ".bias", dm);
        L.alloc_w(l, (size_t)3 * dm, ffn, dm);
        if (fp8) {
            l.s_qkv = (float*)L.dalloc((size_t)3 * dm * 4); l.s_o = (float*)L.dalloc((size_t)dm * 4);
            l.s_fc = (float*)L.dalloc((size_t)ffn * 4); l.s_proj = (float*)L.dalloc((size_t)dm * 4);
        }
        if (L.st != SGPT_OK) break;
        if (split) { l.w_qkv3 = L.dalloc((size_t)(split_all ? 3 : 2) * dm * 3 * dm * 2); if (!l.w_qkv3) break; }
        if (split_all) {
            l.w_o3 = L.dalloc((size_t)dm * 3 * dm * 2); l.w_fc3 = L.dalloc((size_t)ffn * 3 * dm * 2); l.w_proj3 = L.dalloc((size_t)dm * 3 * ffn * 2);
            if (!l.w_o3 || !l.w_fc3 || !l.w_proj3) break;
        }
        if (bloom) {
            const float* wq = L.find(p + "self_attention.query_key_value.weight", (int64_t)3 * dm * dm);
            const float* bq = L.find(p + "self_attention.query_key_value.bias", (int64_t)3 * dm);
            l.b_qkv = (float*)L.dalloc((size_t)3 * dm * 4);
            if (!wq || !bq || !l.b_qkv || !stage) break;
            launch_qkv_deinterleave(wq, stage, H, dh, dm, 0);          // rows [h,3,dh] -> [q | k | v]
            launch_qkv_deinterleave(bq, l.b_qkv, H, dh, 1, 0);
            L.pack_rows(stage, (int64_t)3 * dm, dm, l.w_qkv, 0, l.s_qkv);
            if (split) launch_pack_split_rows(stage, (long)(split_all ? 3 : 2) * dm, dm, l.w_qkv3, dt16, 0);      // q and k (and v) rows
        } else {
            if (split) L.pack3(p + attn + "q_proj.weight", dm, dm, l.w_qkv3);
            if (split) L.pack3(p + attn + "k_proj.weight", dm, dm, (bf16_t*)l.w_qkv3 + (size_t)dm * 3 * dm);
            if (L.st != SGPT_OK) break;
            if (split_all) L.pack3(p + attn + "v_proj.weight", dm, dm, (bf16_t*)l.w_qkv3 + (size_t)2 * dm * 3 * dm);
            L.pack_w(p + attn + "q_proj.weight", dm, dm, l.w_qkv, 0, l.s_qkv);
            L.pack_w(p + attn + "k_proj.weight", dm, dm, l.w_qkv, dm, l.s_qkv);
            L.pack_w(p + attn + "v_proj.weight", dm, dm, l.w_qkv, (int64_t)2 * dm, l.s_qkv);
        }
        L.pack_w(wo + ".weight", dm, dm, l.w_o, 0, l.s_o);
        if (split_all) L.pack3(wo + ".weight", dm, dm, l.w_o3);
        L.pack_w(p + fc1 + ".weight", ffn, dm, l.w_fc, 0, l.s_fc);
        L.pack_w(p + fc2 + ".weight", dm, ffn, l.w_proj, 0, l.s_proj);
        if (split_all) { L.pack3(p + fc1 + ".weight", ffn, dm, l.w_fc3); L.pack3(p + fc2 + ".weight", dm, ffn, l.w_proj3); }
    }
}

// BERT  encoder.layer.N.attention.self.{query,key,value} / attention.output.{dense,LayerNorm} / intermediate.dense /
//       output.{dense,LayerNorm}; `pooler.*` is not read                         (HF:bert/modeling_bert.py BertLayer)
// ln1 = the LayerNorm behind the attention (attention.output.LayerNorm), ln2 = the one behind the MLP (output.LayerNorm)
void load_bert(Loader& L) {
    sgpt_model* m = L.m; const sgpt_model_desc* d = L.d;
    const int dm = L.dm, ffn = L.ffn;
    // position table with token_type_embeddings[0] already added by the caller (single-segment inputs; include/sgpt_hip.h)
    m->wpe = L.copy_f32("embeddings.position_embeddings.weight", (int64_t)d->max_pos * dm);
    L.copy_ln("embeddings.LayerNorm", &m->emb_ln_g, &m->emb_ln_b);
    L.head();
    for (int i = 0; i < d->n_layers && L.st == SGPT_OK; ++i) {
        const std::string p = family(d->arch).prefix + std::to_string(i) + ".";
        LayerW& l = m->L[i];
        l.is_local = 0;
        L.copy_ln(p + "attention.output.LayerNorm", &l.ln1_g, &l.ln1_b);
        L.copy_ln(p + "output.LayerNorm", &l.ln2_g, &l.ln2_b);
        l.b_o = L.copy_f32(p + "attention.output.dense.bias", dm);
        l.b_fc = L.copy_f32(p + "intermediate.dense.bias", ffn);
        l.b_proj = L.copy_f32(p + "output.dense.bias", dm);
        l.b_qkv = (float*)L.dalloc((size_t)3 * dm * 4);
        L.alloc_w(l, (size_t)3 * dm, ffn, dm);
        if (L.st != SGPT_OK) break;
        const char* qkv[3] = {"query", "key", "value"};
        for (int j = 0; j < 3 && L.st == SGPT_OK; ++j) {          // fused [q rows | k rows | v rows], biases alike
            L.pack_w(p + "attention.self." + qkv[j] + ".weight", dm, dm, l.w_qkv, (int64_t)j * dm, nullptr);
            const float* bj = L.find(p + "attention.self." + qkv[j] + ".bias", dm);
            if (bj && hipMemcpyAsync(l.b_qkv + (size_t)j * dm, bj, (size_t)dm * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess)
                L.st = fail(L.c, SGPT_ERR_HIP, "memcpy qkv bias");
        }
        L.pack_w(p + "attention.output.dense.weight", dm, dm, l.w_o, 0, nullptr);
        L.pack_w(p + "intermediate.dense.weight", ffn, dm, l.w_fc, 0, nullptr);
        L.pack_w(p + "output.dense.weight", dm, ffn, l.w_proj, 0, nullptr);
    }
}

// LLAMA layers.N.input_layernorm / self_attn.{qkv_proj (q | k | v rows fused by the caller), o_proj} / post_attention_layernorm /
//       mlp.{gate_up_proj (gate rows, then up rows), down_proj}             (HF:llama/modeling_llama.py LlamaDecoderLayer)
// Optional, decided on layer 0 and then required of every layer: self_attn.qkv_proj.bias [d_q + 2 d_kv] (HF:qwen2/modeling_qwen2.py
// Qwen2Attention) and self_attn.{q_norm,k_norm}.weight [head_dim], both or neither (HF:qwen3/modeling_qwen3.py Qwen3Attention).
// The RMSNorm gains carry no load-time bound (the f16 stores of the norm kernels are range-tracked at run time): shifts stay 0.
void load_llama(Loader& L) {
    sgpt_model* m = L.m; const sgpt_model_desc* d = L.d;
    const int dm = L.dm, ffn = L.ffn; const int64_t dq = (int64_t)L.H * L.dh, dkv = (int64_t)m->d.n_kv_heads * L.dh;
    // no position table: half-split rotary on q / k (tables from the host, include/sgpt_hip.h)
    m->rot_sin = L.copy_f32("rotary.sin", (int64_t)d->max_pos * (L.dh / 2));
    m->rot_cos = L.copy_f32("rotary.cos", (int64_t)d->max_pos * (L.dh / 2));
    L.head();
    const std::string p0 = std::string(family(d->arch).prefix) + "0.self_attn.";
    const bool has_bias = L.byname.count(p0 + "qkv_proj.bias") != 0;
    const bool has_norm = L.byname.count(p0 + "q_norm.weight") != 0 || L.byname.count(p0 + "k_norm.weight") != 0;
    for (int i = 0; i < d->n_layers && L.st == SGPT_OK; ++i) {
        const std::string p = family(d->arch).prefix + std::to_string(i) + ".";
        LayerW& l = m->L[i];
        l.is_local = d->layer_is_local ? d->layer_is_local[i] : (d->window > 0 ? 1 : 0);
        l.ln1_g = L.copy_f32(p + "input_layernorm.weight", dm);
        l.ln2_g = L.copy_f32(p + "post_attention_layernorm.weight", dm);
        l.ln1_b = l.ln2_b = l.b_fc = nullptr;
        l.b_o = l.b_proj = m->zero_bias;       // the residual epilogue reads a bias vector: zeros
        // a later layer that has what layer 0 lacks: the tensor layer 0 misses is named
        if (!has_bias && L.byname.count(p + "self_attn.qkv_proj.bias")) L.st = fail(L.c, SGPT_ERR_MISSING, "missing weight tensor: " + p0 + "qkv_proj.bias");
        if (!has_norm && (L.byname.count(p + "self_attn.q_norm.weight") || L.byname.count(p + "self_attn.k_norm.weight")))
            L.st = fail(L.c, SGPT_ERR_MISSING, "missing weight tensor: " + p0 + "q_norm.weight");
        if (L.st != SGPT_OK) break;
        if (has_bias) l.b_qkv = L.copy_f32(p + "self_attn.qkv_proj.bias", dq + 2 * dkv);
        if (has_norm) {
            l.qn_g = L.copy_f32(p + "self_attn.q_norm.weight", L.dh);
            l.kn_g = L.copy_f32(p + "self_attn.k_norm.weight", L.dh);
            if (L.f16 && l.qn_g && l.kn_g) { launch_absmax(l.qn_g, L.dh, L.stats + 1, 0); launch_absmax(l.kn_g, L.dh, L.stats + 1, 0); }
        }
        L.alloc_w(l, dq + 2 * dkv, (size_t)2 * ffn, dq);
        if (L.st != SGPT_OK) break;
        L.pack_w(p + "self_attn.qkv_proj.weight", dq + 2 * dkv, dm, l.w_qkv, 0, nullptr);
        L.pack_w(p + "self_attn.o_proj.weight", dm, dq, l.w_o, 0, nullptr);
        L.pack_w(p + "mlp.gate_up_proj.weight", (int64_t)2 * ffn, dm, l.w_fc, 0, nullptr);
        L.pack_w(p + "mlp.down_proj.weight", dm, ffn, l.w_proj, 0, nullptr);
    }
}

// What every model has behind its layers: fp8 de-quantisation scratch, FP8M activation scales, range shifts, the precision plan, the
// crest and range words.
void load_tail(Loader& L) {
    sgpt_model* m = L.m; const sgpt_model_desc* d = L.d;
    const int dm = L.dm, ffn = L.ffn;
    auto zeroed = [&](size_t bytes) {
        void* p = L.dalloc(bytes);
        if (p && hipMemsetAsync(p, 0, bytes, 0) != hipSuccess) L.st = fail(L.c, SGPT_ERR_HIP, "memset");
        return (unsigned*)p;
    };
    if (L.fp8 && L.st == SGPT_OK) {
        m->dq[0] = L.dalloc((size_t)3 * dm * dm * 2); m->dq[1] = L.dalloc((size_t)dm * dm * 2);
        m->dq[2] = L.dalloc((size_t)ffn * dm * 2); m->dq[3] = L.dalloc((size_t)dm * ffn * 2);
    }
    if (d->compute_dtype == SGPT_FP8M && L.st == SGPT_OK) {
        m->act_scale.assign(2 * (size_t)d->n_layers, 0.0f);   // 0 = not calibrated
        m->h_amax = zeroed((size_t)d->n_layers * 8);
    }
    m->shift.assign((size_t)d->n_layers * RS_N, 0);
    m->ln_floor.assign((size_t)d->n_layers, 0);
    m->prec.assign((size_t)d->n_layers * PC_N, 0);
    m->split_all = d->split_weights != 0;
    m->qkv3_rows = d->split_weights != 0 ? 3 : (d->qk_split != 0 ? 2 : 0);
    if (d->qk_split != 0)              // the round-3 switch: the Q / K projection of every block contracts over hi + lo pairs
        for (int i = 0; i < d->n_layers; ++i) m->prec[(size_t)i * PC_N + PC_LN1] = 1;
    if (L.st == SGPT_OK && L.bf && !L.fp8) m->crest_dev = zeroed((size_t)d->n_layers * RS_N * 4);
    if (L.st == SGPT_OK) m->range_dev = zeroed((size_t)(1 + d->n_layers * RS_N) * 4);
}

// SGPT_F16, after the weights are packed.  f16 has 5 exponent bits.  A LayerNorm output is bounded by max|gamma| * sqrt(d) + max|beta|
// (|x_hat| <= sqrt(d-1)): when that bound can leave the format the LayerNorm outputs are stored under a power-of-two down-shift that
// the consuming GEMMs undo on their fp32 accumulators (exact; sgpt_model.shift).  Activations behind the GEMMs are range-checked on the
// device at run time (RangeTrack in the store epilogues -> sgpt_model_range_check / sgpt_model_range_adapt).  Only a weight outside
// the format is refused.
void audit_f16_range(Loader& L) {
    unsigned h[4] = {0, 0, 0, 0};
    if (L.st == SGPT_OK && hipMemcpy(h, L.stats, 12, hipMemcpyDeviceToHost) != hipSuccess) L.st = fail(L.c, SGPT_ERR_HIP, "range audit");
    (void)hipFree(L.stats);
    float wmax, gmax, bmax;
    memcpy(&wmax, &h[0], 4); memcpy(&gmax, &h[1], 4); memcpy(&bmax, &h[2], 4);
    const float bound = gmax * sqrtf((float)L.dm) + bmax;
    if (L.st == SGPT_OK && (!(wmax < 65504.f) || !std::isfinite(bound)))
        L.st = fail(L.c, SGPT_ERR_RANGE, "SGPT_F16: a matmul weight exceeds the f16 range (or a LayerNorm parameter is not finite); load with SGPT_BF16");
    // (a family without range shifts keeps 0: its norm kernels carry a run-time range tracker instead of relying on this bound)
    if (L.st != SGPT_OK || bound < 32768.f || !family(L.d->arch).shifts) return;
    int k = (int)std::ceil(std::log2(bound / 16384.f));
    k = k < 1 ? 1 : k;
    if (k > RS_MAX_SHIFT) L.st = fail(L.c, SGPT_ERR_RANGE, "SGPT_F16: LayerNorm parameters beyond any usable range shift; load with SGPT_BF16");
    for (int i = 0; i < L.d->n_layers && L.st == SGPT_OK; ++i) {
        L.m->shift[(size_t)i * RS_N + RS_LN1] = L.m->shift[(size_t)i * RS_N + RS_LN2] = k;
        L.m->ln_floor[i] = k;
    }
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------
sgpt_status sgpt_model_load(sgpt_ctx* c, const sgpt_model_desc* d, const sgpt_tensor_view* tv, size_t nt, sgpt_model** out) {
    if (!c || !d || !tv || !out) return SGPT_ERR_INVALID;
    *out = nullptr;
    HIPC(c, hipSetDevice(c->device));
    if (sgpt_status st = check_desc(c, d)) return st;
    const int cd = d->compute_dtype;
    Loader L{};                // (st = SGPT_OK)
    L.c = c; L.d = d; L.dm = d->d_model; L.ffn = d->d_ffn; L.H = d->n_heads; L.dh = head_dim(*d);
    L.fp8 = cd == SGPT_FP8W || cd == SGPT_FP8M; L.f16 = cd == SGPT_F16; L.bf = cd == SGPT_BF16 || L.f16;
    L.esz = L.fp8 ? 1 : (L.bf ? 2 : 4);
    if (L.f16 && hipMalloc((void**)&L.stats, 16) != hipSuccess) return fail(c, SGPT_ERR_OOM, "hipMalloc failed");
    if (L.f16) (void)hipMemsetAsync(L.stats, 0, 16, 0);
    for (size_t i = 0; i < nt; ++i) L.byname[tv[i].name] = &tv[i];
    sgpt_model* m = L.m = new sgpt_model();
    m->ctx = c; m->d = *d; m->d.layer_is_local = nullptr;
    if (m->d.n_kv_heads == 0) m->d.n_kv_heads = L.H;
    m->wte = L.copy_f32(family(d->arch).wte, (int64_t)d->vocab * L.dm);
    // the family's own embedding tensors, L.head(), its layers
    (d->arch == SGPT_ARCH_BERT ? load_bert : d->arch == SGPT_ARCH_LLAMA ? load_llama : load_decoder)(L);
    load_tail(L);
    if (L.st == SGPT_OK && hipDeviceSynchronize() != hipSuccess) L.st = fail(c, SGPT_ERR_HIP, "sync after weight pack");
    if (L.f16) audit_f16_range(L);
    if (L.st != SGPT_OK) { sgpt_model_free(m); return L.st; }
    *out = m;
    return SGPT_OK;
}

void sgpt_model_free(sgpt_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipDeviceSynchronize();
    for (void* p : m->allocs) (void)hipFree(p);
    delete m;
}

sgpt_status sgpt_model_set_pool_weights(sgpt_model* m, const float* w, int32_t n) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (!w || n <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_pool_weights: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());      // an in-flight encode may still read the previous table
    if (n > m->pool_w_n) {
        float* p = nullptr;
        if (hipMalloc((void**)&p, (size_t)n * 4) != hipSuccess) return fail(c, SGPT_ERR_OOM, "hipMalloc pool weights failed");
        m->allocs.push_back(p);           // the old, smaller table is released with the model
        m->pool_w = p;
        c->generation++;                  // captured graphs still point at the old table
    }
    m->pool_w_n = n;
    HIPC(c, hipMemcpy(m->pool_w, w, (size_t)n * 4, hipMemcpyDeviceToDevice));
    return SGPT_OK;
}

// The attention mode of a loaded model (not a descriptor field: the descriptor of a model does not change with it).  The family's row
// says whose it is to set; the block functions read m->bidir (encode.hip: attn_llama).
sgpt_status sgpt_model_set_attention(sgpt_model* m, int32_t causal) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    const Family& F = family(m->d.arch);
    if (causal != 0 && causal != 1) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_attention: causal 0 | 1");
    if (F.attn_fixed)
        return fail(c, SGPT_ERR_INVALID, std::string("sgpt_model_set_attention: the attention mode belongs to SGPT_ARCH_LLAMA models; ") + F.name + " " + F.attn_fixed);
    if (!causal && m->d.window > 0)
        for (const LayerW& l : m->L)
            if (l.is_local)
                return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_attention: bidirectional attention with an applied sliding window (window " +
                            std::to_string(m->d.window) + " on a layer of this model) is not built");
    if (m->bidir != (causal == 0)) c->generation++;       // captured graphs carry the old attention launches
    m->bidir = causal == 0;
    return SGPT_OK;
}

sgpt_status sgpt_model_calibrate_begin(sgpt_model* m) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (m->d.compute_dtype != SGPT_FP8M) return fail(c, SGPT_ERR_INVALID, "calibration applies to SGPT_FP8M models");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    HIPC(c, hipMemset(m->h_amax, 0, (size_t)m->d.n_layers * 8));
    m->calibrating = true;
    return SGPT_OK;
}

sgpt_status sgpt_model_calibrate_end(sgpt_model* m, float margin, float* scales_out) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (m->d.compute_dtype != SGPT_FP8M || !m->calibrating) return fail(c, SGPT_ERR_INVALID, "sgpt_model_calibrate_end without _begin");
    m->calibrating = false;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    const int ns = 2 * m->d.n_layers;
    std::vector<float> amax(ns);
    HIPC(c, hipMemcpy(amax.data(), m->h_amax, (size_t)ns * 4, hipMemcpyDeviceToHost));
    if (!(margin >= 1.0f)) margin = 2.0f;
    for (int i = 0; i < ns; ++i) {
        // smallest power of two with margin * amax / scale <= 448 (head-room: later batches may exceed the sample's range;
        // a saturated code raises bit 1 of the range flag)
        const float need = amax[i] * margin / 448.0f;
        float sc = 1.0f;
        if (need > 0.f && std::isfinite(need)) sc = std::exp2(std::ceil(std::log2(need)));
        m->act_scale[i] = sc;
        if (scales_out) scales_out[i] = sc;
    }
    return SGPT_OK;
}

sgpt_status sgpt_model_set_act_scales(sgpt_model* m, const float* scales, int32_t n) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (m->d.compute_dtype != SGPT_FP8M || !scales || n != 2 * m->d.n_layers) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_act_scales: needs 2 * n_layers scales");
    for (int i = 0; i < n; ++i) {
        int e = 0;
        if (!(scales[i] > 0.f) || std::frexp(scales[i], &e) != 0.5f) return fail(c, SGPT_ERR_INVALID, "activation scales must be powers of two");
        m->act_scale[i] = scales[i];
    }
    return SGPT_OK;
}

// ---- SGPT_F16 range guard, per model --------------------------------------------------------------------------------
sgpt_status sgpt_model_range_check(sgpt_model* m, int32_t* flagged, int32_t reset, void* stream) {
    if (!m || !flagged) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned h = 0;
    HIPC(c, hipMemcpyAsync(&h, m->range_dev, 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (reset && h) HIPC(c, hipMemsetAsync(m->range_dev, 0, (size_t)(1 + m->d.n_layers * RS_N) * 4, s));
    *flagged = (int32_t)h;
    return SGPT_OK;
}

sgpt_status sgpt_model_range_adapt(sgpt_model* m, int32_t* n_raised, void* stream) {
    if (!m || !n_raised) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    *n_raised = 0;
    if (m->d.compute_dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "sgpt_model_range_adapt applies to SGPT_F16 models");
    if (!family(m->d.arch).shifts)
        return fail(c, SGPT_ERR_INVALID, "sgpt_model_range_adapt: SGPT_ARCH_BERT / SGPT_ARCH_LLAMA run without range shifts; a flagged f16 model must be loaded with SGPT_BF16 or SGPT_F32");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int n = m->d.n_layers * RS_N;
    std::vector<unsigned> h((size_t)n + 1);
    HIPC(c, hipMemcpyAsync(h.data(), m->range_dev, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    int raised = 0;
    for (int i = 0; i < n; ++i) {
        if (!h[i + 1]) continue;
        float amax;
        memcpy(&amax, &h[i + 1], 4);
        // the stored magnitude was amax >= RANGE_LIMIT: bring it to <= 16384 (a factor of two of head-room for later
        // batches); infinite (the fp32 value itself overflowed f16 by an unknown factor): 8 binary orders per attempt
        int need = std::isfinite(amax) ? (int)std::ceil(std::log2(amax / 16384.f)) : 8;
        need = need < 1 ? 1 : need;
        if (m->shift[i] + need > RS_MAX_SHIFT)
            return fail(c, SGPT_ERR_RANGE, "SGPT_F16: an activation class needs a range shift beyond 2^40; load with SGPT_BF16");
        m->shift[i] += need;
        ++raised;
    }
    if (raised) {
        HIPC(c, hipMemsetAsync(m->range_dev + 1, 0, (size_t)n * 4, s));
        const unsigned keep = h[0] & ~1u;                 // bit 0 handled; fp8 saturation bits stay
        HIPC(c, hipMemcpyAsync(m->range_dev, &keep, 4, hipMemcpyHostToDevice, s));
        HIPC(c, hipStreamSynchronize(s));
        c->generation++;                                  // captured graphs carry the old factors as kernel arguments
    }
    *n_raised = raised;
    return SGPT_OK;
}

sgpt_status sgpt_model_get_range_shifts(sgpt_model* m, int32_t* shifts, int32_t n) {
    if (!m || !shifts || n != m->d.n_layers * RS_N) return m ? fail(m->ctx, SGPT_ERR_INVALID, "sgpt_model_get_range_shifts: n must be 4 * n_layers") : SGPT_ERR_INVALID;
    for (int i = 0; i < n; ++i) shifts[i] = m->shift[i];
    return SGPT_OK;
}

sgpt_status sgpt_model_set_range_shifts(sgpt_model* m, const int32_t* shifts, int32_t n) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (m->d.compute_dtype != SGPT_F16 || !shifts || n != m->d.n_layers * RS_N)
        return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_range_shifts: SGPT_F16 models, n = 4 * n_layers");
    if (!family(m->d.arch).shifts)
        return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_range_shifts: SGPT_ARCH_BERT / SGPT_ARCH_LLAMA run without range shifts");
    for (int i = 0; i < n; ++i)
        if (shifts[i] < 0 || shifts[i] > RS_MAX_SHIFT) return fail(c, SGPT_ERR_INVALID, "range shifts must lie in [0, 40]");
    // the LayerNorm kernels have no run-time range tracker: their shifts may not go below the bound sgpt_model_load derived
    // from THIS checkpoint's parameters (shifts pinned from another checkpoint would overflow to inf unnoticed)
    for (int i = 0; i < n; ++i) {
        const int cls = i % RS_N, blk = i / RS_N;
        if ((cls == RS_LN1 || cls == RS_LN2) && shifts[i] < m->ln_floor[blk])
            return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_range_shifts: a LayerNorm shift below the bound of this checkpoint's LayerNorm parameters (block " +
                        std::to_string(blk) + ": at least " + std::to_string(m->ln_floor[blk]) + ")");
    }
    for (int i = 0; i < n; ++i) m->shift[i] = shifts[i];
    c->generation++;
    return SGPT_OK;
}

// ---- precision plan: split-precision (hi + lo) operand classes per block ----------------------------------------------
sgpt_status sgpt_model_set_precision(sgpt_model* m, const int32_t* plan, int32_t n) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    const int cd = m->d.compute_dtype;
    if (!plan || n != m->d.n_layers * PC_N) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: n must be 5 * n_layers");
    const int dh = m->d.d_model / m->d.n_heads;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const int cls = i % PC_N, v = plan[i];
        if (v < 0 || v > (cls == PC_LN1 ? 3 : 1)) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: entries are 0 | 1 (LayerNorm-1 class: 0 ... 3)");
        any |= v != 0;
        const bool legacy_ok = cls == PC_LN1 && (v == 1 || v == 3 || (v == 2 && m->qkv3_rows == 3)) && m->L[i / PC_N].w_qkv3 != nullptr;
        if (v != 0 && cls != PC_ATT && !m->split_all && !legacy_ok)      // (the attention class splits activations only)
            return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: the model was loaded without split weight copies (sgpt_model_desc.split_weights)");
        if (cls == PC_ATT && v != 0 && (m->d.arch == SGPT_ARCH_GPTJ || !attn_x3_supported(dh)))
            return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: split-precision attention needs head_dim 64 or 128 and no rotary embedding (GPT-Neo / BLOOM)");
        if (cls == PC_LN2 && m->d.arch == SGPT_ARCH_GPTJ && v != 0 && plan[i - PC_LN2 + PC_LN1] == 0)
            return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: GPT-J's MLP reads ln_1's output: a split fc1 needs a split LayerNorm-1 entry");
    }
    if (any && !family(m->d.arch).split)
        return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision: no split-precision operands for SGPT_ARCH_BERT / SGPT_ARCH_LLAMA");
    if (any && cd != SGPT_F16 && cd != SGPT_BF16) return fail(c, SGPT_ERR_INVALID, "sgpt_model_set_precision applies to SGPT_F16 / SGPT_BF16 models");
    for (int i = 0; i < n; ++i) m->prec[i] = plan[i];
    c->generation++;                                      // captured graphs carry the old launch sequence
    return SGPT_OK;
}

sgpt_status sgpt_model_get_precision(sgpt_model* m, int32_t* plan, int32_t n) {
    if (!m || !plan || n != m->d.n_layers * PC_N) return m ? fail(m->ctx, SGPT_ERR_INVALID, "sgpt_model_get_precision: n must be 5 * n_layers") : SGPT_ERR_INVALID;
    for (int i = 0; i < n; ++i) plan[i] = m->prec[i];
    return SGPT_OK;
}

// The [W_hi | W_hi | W_lo] copies of sgpt_model_desc.split_weights are 3 x the 16-bit weight bytes on top of the plain copy
// (+35 GB at GPT-J-6B shape).  A model whose probe settled on plain operands gives them back here; a later plan
// that needs them is refused by sgpt_model_set_precision as for a model loaded without them.  The round-3 qk_split copies
// (q and k rows) stay when a plan entry still reads them.
sgpt_status sgpt_model_release_split_weights(sgpt_model* m, int64_t* bytes_freed) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (bytes_freed) *bytes_freed = 0;
    if (!m->split_all) return SGPT_OK;
    bool qk_used = false;
    for (int i = 0; i < m->d.n_layers; ++i)
        for (int cls = 0; cls < PC_N; ++cls) {
            const int v = m->prec[(size_t)i * PC_N + cls];
            if (v == 0 || cls == PC_ATT) continue;
            if (cls == PC_LN1) { qk_used = true; continue; }            // any LayerNorm-1 level reads w_qkv3 (level 2: its V rows too): kept whole
            return fail(c, SGPT_ERR_INVALID, "sgpt_model_release_split_weights: the installed precision plan reads the split copies");
        }
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    const size_t dm = m->d.d_model, ffn = m->d.d_ffn;
    int64_t freed = 0;
    auto drop = [&](void*& p, size_t bytes) {
        if (!p) return;
        for (size_t i = 0; i < m->allocs.size(); ++i)
            if (m->allocs[i] == p) { m->allocs[i] = m->allocs.back(); m->allocs.pop_back(); break; }
        (void)hipFree(p);
        p = nullptr;
        freed += (int64_t)bytes;
    };
    for (int i = 0; i < m->d.n_layers; ++i) {
        LayerW& l = m->L[i];
        drop(l.w_o3, dm * 3 * dm * 2); drop(l.w_fc3, ffn * 3 * dm * 2); drop(l.w_proj3, dm * 3 * ffn * 2);
        if (!qk_used) drop(l.w_qkv3, 3 * dm * 3 * dm * 2);
    }
    if (!qk_used) m->qkv3_rows = 0;
    m->split_all = false;
    c->generation++;
    if (bytes_freed) *bytes_freed = freed;
    return SGPT_OK;
}

// The arithmetic of a loaded Llama-family model's projections (not a descriptor field, not a compute dtype: sgpt_model_set_attention is
// the model for this).  kind 1: layer by layer, the bf16 rows of w_qkv, w_fc and w_proj become e4m3fn codes + one power-of-two scale per
// output row (the rule and the RNE codes of sgpt_fp8_quantize_rows on the bf16 values), and the 16-bit allocation goes back to the
// device as its layer is done -- the peak is one layer's codes on top of the model.  w_o stays 16-bit: its operand, the attention
// context, has no per-row scale.  The block functions read m->proj8 (encode.hip: pick_block).
sgpt_status sgpt_model_set_projections(sgpt_model* m, int32_t kind, int64_t* bytes_freed) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (bytes_freed) *bytes_freed = 0;
    const sgpt_model_desc& d = m->d;
    const char* who = "sgpt_model_set_projections: ";
    if (d.arch != SGPT_ARCH_LLAMA)
        return fail(c, SGPT_ERR_INVALID, std::string(who) + "fp8 projections belong to SGPT_ARCH_LLAMA models (" + family(d.arch).name + " has its fp8 compute dtypes or none)");
    if (d.compute_dtype != SGPT_BF16) return fail(c, SGPT_ERR_INVALID, std::string(who) + "the model must be loaded with SGPT_BF16");
    const int dh = head_dim(d), dq = d.n_heads * dh, dkv = d.n_kv_heads * dh;
    const std::pair<const char*, int> widths[] = {{"d_model", d.d_model}, {"d_q + d_kv", dq + dkv}, {"d_kv", dkv}, {"d_ffn", d.d_ffn}};
    for (const auto& w : widths)
        if (w.second % 256)
            return fail(c, SGPT_ERR_INVALID, std::string(who) + w.first + " = " + std::to_string(w.second) + " is not a multiple of 256 (the fp8 MFMA kernel's tile)");
    if (kind != 0 && kind != 1) return fail(c, SGPT_ERR_INVALID, std::string(who) + "kind 0 (16-bit) | 1 (fp8)");
    if (kind == 0 && m->proj8 != 0) return fail(c, SGPT_ERR_INVALID, std::string(who) + "the conversion is one-way: the 16-bit weights are gone (load the model again)");
    if (kind == 1 && m->proj8 != 0) return fail(c, SGPT_ERR_INVALID, std::string(who) + "the model is converted already");
    if (kind == 0) return SGPT_OK;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());      // an in-flight encode still reads the 16-bit weights
    int64_t freed = 0;
    bool oom = false;
    // one matrix [rows, cols]: codes + scales allocated, quantised from the bf16 rows, the pointers swapped; the old allocation is `old`
    auto convert = [&](void*& w, float*& sc, size_t rows, size_t cols, void*& old) {
        void* q = nullptr; float* s = nullptr;
        if (hipMalloc(&q, rows * cols) != hipSuccess || hipMalloc((void**)&s, rows * 4) != hipSuccess) {
            (void)hipGetLastError();
            if (q) (void)hipFree(q);
            oom = true;
            return;
        }
        m->allocs.push_back(q); m->allocs.push_back(s);
        launch_fp8_quant_rows_bf16(w, (long)rows, (long)cols, q, s, 0);
        old = w; w = q; sc = s;
        freed += (int64_t)(rows * cols * 2) - (int64_t)(rows * cols + rows * 4);
    };
    m->proj8 = -1;                        // (until every layer is done: a model converted in part encodes nothing, plan() refuses it)
    c->generation++;                      // captured graphs carry the 16-bit launches and pointers
    for (LayerW& l : m->L) {
        void* old[3] = {nullptr, nullptr, nullptr};
        convert(l.w_qkv, l.s_qkv, (size_t)dq + 2 * dkv, d.d_model, old[0]);
        if (!oom) convert(l.w_fc, l.s_fc, (size_t)2 * d.d_ffn, d.d_model, old[1]);
        if (!oom) convert(l.w_proj, l.s_proj, d.d_model, d.d_ffn, old[2]);
        HIPC(c, hipDeviceSynchronize());  // the quantiser has read the rows that go back now
        for (void* p : old) {
            if (!p) continue;
            for (size_t i = 0; i < m->allocs.size(); ++i)
                if (m->allocs[i] == p) { m->allocs[i] = m->allocs.back(); m->allocs.pop_back(); break; }
            (void)hipFree(p);
        }
        if (oom) return fail(c, SGPT_ERR_OOM, std::string(who) + "hipMalloc failed part of the way: the model is unusable, free it and load it again");
    }
    HIPC(c, hipGetLastError());
    m->proj8 = 1;
    if (bytes_freed) *bytes_freed = freed;
    return SGPT_OK;
}

sgpt_status sgpt_model_get_projections(sgpt_model* m, int32_t* kind) {
    if (!m || !kind) return m ? fail(m->ctx, SGPT_ERR_INVALID, "sgpt_model_get_projections: kind is NULL") : SGPT_ERR_INVALID;
    *kind = m->proj8 == 1 ? 1 : 0;
    return SGPT_OK;
}

sgpt_status sgpt_model_precision_probe_begin(sgpt_model* m) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (!m->crest_dev || !family(m->d.arch).probe) return fail(c, SGPT_ERR_INVALID, "the precision probe applies to SGPT_F16 / SGPT_BF16 models of the decoder families");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    HIPC(c, hipMemset(m->crest_dev, 0, (size_t)m->d.n_layers * RS_N * 4));
    m->probing = true;
    c->generation++;                                      // a graph captured while probing must not outlive the probe
    return SGPT_OK;
}

sgpt_status sgpt_model_precision_probe_end(sgpt_model* m, float* crest_out) {
    if (!m) return SGPT_ERR_INVALID;
    sgpt_ctx* c = m->ctx;
    if (!m->probing) return fail(c, SGPT_ERR_INVALID, "sgpt_model_precision_probe_end without _begin");
    m->probing = false;
    c->generation++;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    if (crest_out) HIPC(c, hipMemcpy(crest_out, m->crest_dev, (size_t)m->d.n_layers * RS_N * 4, hipMemcpyDeviceToHost));
    return SGPT_OK;
}

}  // extern "C"
