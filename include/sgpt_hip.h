/*
 * sgpt_hip.h -- C ABI of the MI355X (gfx950) SGPT bi-encoder retrieval hot path.
 *
 * The reference (Muennighoff/sgpt) has NO native layer: the hot path is Python that
 * reaches implicit PyTorch/cuBLAS kernels through HuggingFace `AutoModel`, `torch.mm`
 * and `torch.topk`.  Each entry point below names the reference call site whose device
 * work it replaces (paths relative to /root/reference; HF: = huggingface transformers,
 * the un-vendored dependency that holds the transformer arithmetic).  The Python side
 * (sgpt_amd/_lib.py) binds these with ctypes; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer marked "device" is a HIP device pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); the library allocates only its own workspace and
 *     its packed copy of the weights, both tied to the ctx / model handle;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream) and performs no hidden device synchronisation, except
 *     sgpt_ctx_create / sgpt_model_load / *_destroy / *_free and workspace growth;
 *   - no C++ exception crosses the ABI: functions return SGPT_OK (0) or a negative
 *     sgpt_status; sgpt_last_error(ctx) returns a message for the last failure on ctx;
 *   - calls on one ctx must be issued from one thread onto ONE stream at a time: the activation / scorer workspaces are
 *     per-ctx scratch shared by every model and call on it (use one ctx per stream for concurrent streams);
 *   - a ctx is bound to one HIP device and is re-entrant per ctx, not thread-safe
 *     (the reference runs one single-threaded Python process per GPU,
 *     sentence_transformers/SentenceTransformer.py:275-283).
 */
#ifndef SGPT_HIP_H
#define SGPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGPT_ABI_VERSION 27

/* The longest sequence (ABI v23): the token rows one sequence may own in the packed layout of sgpt_encode*, sgpt_attention_ex and
 * sgpt_attention_gqa (max_alloc_len <= SGPT_MAX_SEQ_LEN; a larger value is SGPT_ERR_INVALID, nothing launched).  32 768 is the
 * context of Qwen3-Embedding; up to ABI v22 the bound was 2048, the position table of the SGPT checkpoints.  A model's own bound is
 * its descriptor's max_pos (positions at or above it are clamped by the kernels and refused by the Python host); the descriptor
 * and the rotary tables hold min(max_position_embeddings, SGPT_MAX_SEQ_LEN) rows.  The plain sgpt_attention entry keeps 2048. */
#define SGPT_MAX_SEQ_LEN 32768

typedef int sgpt_status;
#define SGPT_OK 0
#define SGPT_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define SGPT_ERR_HIP (-2)         /* a HIP runtime call failed */
#define SGPT_ERR_MISSING (-3)     /* a required weight tensor was not supplied */
#define SGPT_ERR_OOM (-4)
#define SGPT_ERR_COMM (-6)        /* an RCCL call failed */
#define SGPT_ERR_RANGE (-5)       /* SGPT_F16: a matmul weight does not fit the f16 range, or an activation class is beyond every range shift */

typedef struct sgpt_ctx sgpt_ctx;
typedef struct sgpt_model sgpt_model;

enum { SGPT_F32 = 0, SGPT_BF16 = 1, SGPT_FP8W = 2, SGPT_F16 = 3, SGPT_FP8M = 4 };   /* element types; FP8W / FP8M: model compute_dtype only */
enum { SGPT_ARCH_GPTNEO = 0, SGPT_ARCH_GPTJ = 1, SGPT_ARCH_BLOOM = 2, SGPT_ARCH_BERT = 3, SGPT_ARCH_LLAMA = 4 };
/* SGPT_ARCH_BERT (ABI v13): HF BertModel (HF:bert/modeling_bert.py) -- the baseline of the reference's own scripts
 * (biencoder/beir/beir_dense_retriever.py:36 defaults --modelname to bert-base-uncased; :131-132 frame [CLS] ... [SEP]).
 *   x = LN_emb(wte[id] + wpe'[pos]);  per layer: q | k | v = x W^T + b; ctx = softmax(q.k^T / sqrt(dh)) v over ALL keys of the
 *   sequence (bidirectional: causality follows from the arch); x = LN(x + ctx Wo^T + bo); x = LN(x + gelu(x W1^T + b1) W2^T + b2)
 *   with the erf GELU.  Post-LayerNorm: there is no ln_f, apply_final_ln is ignored, hidden state i of sgpt_encode_layers is
 *   the input of block i (i = 0: the embedding LayerNorm's output) and state L the last block's output, as HF numbers them.
 *   Descriptor: attn_scale = 1 / sqrt(head_dim), window = 0, ln_eps from the config (1e-12), layer_is_local NULL, rotary_dim 0.
 *   Token types are all 0 on this path (single-segment inputs): the CALLER adds token_type_embeddings[0] to every row of the
 *   position table and passes the sum as "embeddings.position_embeddings.weight" (sgpt_amd/model.py does); the pooler head is
 *   not read.  compute_dtype SGPT_F32 | SGPT_F16 | SGPT_BF16; SGPT_FP8W / SGPT_FP8M, qk_split, split_weights and any non-zero
 *   precision plan are refused (SGPT_ERR_INVALID), as are SGPT_POOL_LEARNTMEAN, sgpt_lm_logprobs and the precision probe.
 *   SGPT_F16 runs WITHOUT range shifts: every kernel that rounds an activation to f16 (the write-back LayerNorms included)
 *   records |v| >= 32768 in the model's guard word as for the other families, but sgpt_model_range_adapt and
 *   sgpt_model_set_range_shifts refuse -- a flagged model is reloaded as SGPT_BF16 / SGPT_F32.  16-bit head_dim 64 | 128.
 *   Every layout (T_pad % 32) runs the bulk projection kernels: the query-sized kernels' LayerNorm prologues assume pre-LN. */
/* SGPT_ARCH_LLAMA (ABI v15): HF LlamaModel and MistralModel (HF:llama/modeling_llama.py, HF:mistral/modeling_mistral.py) -- the two differ
 * only in the window.  Pre-norm decoder, causal unless sgpt_model_set_attention says otherwise (ABI v24, below), no bias anywhere, x the fp32 residual stream:
 *   a = RMSNorm_1(x);  q | k | v = a W^T with n_heads query heads and n_kv_heads key / value heads (grouped K / V: query head h reads
 *   key / value head h / (n_heads / n_kv_heads));  q, k <- half-split rotary (rotate_half: x[i] pairs with x[i + head_dim / 2]);
 *   x += softmax(q.k^T / sqrt(dh), causal, window) v Wo^T;  a = RMSNorm_2(x);  x += (silu(a Wgate^T) * (a Wup^T)) Wdown^T;
 *   hidden state i of sgpt_encode_layers is the input of block i, state L the final RMSNorm of the last block's output.
 *   RMSNorm(x) = x * rsqrt(mean(x^2) + ln_eps) * g (ln_eps = rms_norm_eps).  The MLP runs UNFUSED: one fc1 launch of N = 2 d_ffn
 *   (gate rows, then up rows) into a workspace, then one row kernel for silu(gate) * up (sgpt_swiglu).
 *   Descriptor: n_kv_heads (n_heads % n_kv_heads == 0; 0 = n_heads), attn_scale = 1 / sqrt(head_dim), window = the sliding window
 *   (key j visible to query i iff i - window < j <= i; 0 = none) applied on the layers layer_is_local marks, rotary_dim = head_dim.
 *   Tensors: see sgpt_tensor_view.  compute_dtype SGPT_F32 | SGPT_F16 | SGPT_BF16; SGPT_FP8W / SGPT_FP8M, qk_split, split_weights, any
 *   non-zero precision plan, the precision probe, range shifts (sgpt_model_range_adapt / _set_range_shifts: a flagged f16 model is
 *   reloaded as SGPT_BF16 / SGPT_F32), SGPT_POOL_LEARNTMEAN and sgpt_lm_logprobs are refused (SGPT_ERR_INVALID).  head_dim 64 | 128.
 *   Every layout runs the bulk projection kernels (the query-sized kernels' prologues are LayerNorm).
 *   ABI v16 -- HF Qwen2Model and Qwen3Model (HF:qwen2/modeling_qwen2.py, HF:qwen3/modeling_qwen3.py) are this family with three facts
 *   more, none of them a descriptor field of its own:
 *   head_dim: for this arch rotary_dim > 0 IS the head dim and rotary_dim == 0 means d_model / n_heads.  n_heads * head_dim (the query
 *   width d_q) need not equal d_model: q has d_q columns, k and v d_kv = n_kv_heads * head_dim, the fused weight is [d_q + 2 d_kv, d]
 *   and o_proj [d, d_q].  d_q % 128 == 0 and d_q <= 4096, head_dim 64 | 128 as before.
 *   QKV bias (Qwen2): when "layers.N.self_attn.qkv_proj.bias" fp32 [d_q + 2 d_kv] (q | k | v, fused by the caller) is given, it is
 *   added to the projection; o_proj and the MLP carry none.
 *   q / k norm (Qwen3): when "layers.N.self_attn.q_norm.weight" and "layers.N.self_attn.k_norm.weight" fp32 [head_dim] are given, every
 *   query and key head is RMS-normalised over head_dim (ln_eps, the gain shared by the heads) before the rotary -- one fused row
 *   kernel, sgpt_qknorm_rope_half.  Presence is decided on layer 0 and holds for every layer; one gain without the other, or a layer
 *   that disagrees with layer 0, is SGPT_ERR_MISSING by name.
 *   ABI v24 -- the bidirectional embedders built on these backbones (GritLM, gte-Qwen2-instruct, LLM2Vec: `is_causal: false`) are this
 *   family with one property set AFTER load, sgpt_model_set_attention(model, 0): in every layer every query row of a sequence sees
 *   keys [0, seq_len[b]) of that sequence (the non-causal kernels of SGPT_ARCH_BERT with grouped K / V); rotary, the q / k norm, the
 *   bias and the projections are untouched.  Not a descriptor field: the descriptor of a model is the same in both modes.  Such
 *   models usually pool the tokens behind an instruction prompt: sgpt_encode_pool_from.
 *   ABI v25 -- fp8 projections, a second property set AFTER load on an SGPT_BF16 model, sgpt_model_set_projections(model, 1, ..): the
 *   Q | K | V, gate | up and down projections on the e4m3 MFMA with dynamic per-token activation scales and per-channel weight scales,
 *   no calibration; the out-projection, the attention and everything else as above.  Composes with both attention modes and pool_lo. */
enum { SGPT_POOL_WEIGHTEDMEAN = 0, SGPT_POOL_MEAN = 1, SGPT_POOL_LASTTOKEN = 2, SGPT_POOL_LEARNTMEAN = 3,
       SGPT_POOL_CLS = 4 };   /* ABI v13: the first token row of each sequence (Pooling.py:103-105 `pooling_mode_cls_token`); sgpt_encode*, sgpt_pool */
enum { SGPT_COS = 0, SGPT_DOT = 1, SGPT_NEG_L2 = 2 };   /* SGPT_NEG_L2 (ABI v11): -||x - y||_2, sgpt_eval_groups only */

/* Model hyper-parameters = the fields of HF GPTNeoConfig the forward pass reads
 * (HF:gpt_neo/configuration_gpt_neo.py; values of the SGPT checkpoints in SURVEY.md 8). */
typedef struct {
    int32_t arch;            /* SGPT_ARCH_GPTNEO (SGPT-125M/1.3B/2.7B) | SGPT_ARCH_GPTJ (SGPT-5.8B) | SGPT_ARCH_BLOOM (sgpt-bloom-7b1) */
    int32_t n_layers;
    int32_t d_model;         /* multiple of 128 */
    int32_t n_heads;         /* d_model / n_heads in {64, 128} */
    int32_t d_ffn;           /* multiple of 128 */
    int32_t vocab;
    int32_t max_pos;
    int32_t window;          /* GPT-Neo local-attention window (256) */
    float ln_eps;            /* 1e-5 */
    float attn_scale;        /* 1.0 for GPT-Neo (no 1/sqrt(dh), HF:gpt_neo:110); 1/sqrt(dh) for GPT-J (HF:gptj:148) and BLOOM (HF:bloom:186) */
    int32_t compute_dtype;   /* SGPT_F16 : IEEE half MFMA operands (weights, LN output, q/k/v, probabilities, context, GELU
                                           output), fp32 accumulate/residual/LN/softmax -- the same MFMA rate as bf16 with 3
                                           more mantissa bits: the mode that meets the 1e-3 cosine bar against the fp32
                                           reference.  Range-managed: every operand class of a block (LayerNorm
                                           outputs, q | k | v + attention context, GELU output) is stored under a power-of-two
                                           down-shift (0 by default) that the consuming GEMM undoes on its fp32 accumulators
                                           -- exact, the f16 analogue of the e4m3 scales of SGPT_FP8M.  sgpt_model_load
                                           derives the LayerNorm shifts from the parameters and refuses only weights outside
                                           the format (SGPT_ERR_RANGE); every kernel that rounds an activation to f16 records
                                           |v| >= 32768 in a per-model device word (sgpt_model_range_check), from which
                                           sgpt_model_range_adapt raises the shifts of exactly the classes that overflowed;
                                SGPT_BF16: bf16 MFMA operands, fp32 accumulate/residual/LN/softmax;
                                SGPT_F32 : exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), the parity gate;
                                SGPT_FP8W: the six matmul weights per block are STORED as OCP e4m3fn with one
                                           power-of-two fp32 scale per output channel (the
                                           reference loads sgpt-bloom-7b1 8-bit through bitsandbytes) and
                                           de-quantised -- exactly -- to bf16 per block; arithmetic as SGPT_BF16;
                                SGPT_FP8M: weights stored as SGPT_FP8W, and the four projections of every block COMPUTED in fp8:
                                           v_mfma_f32_16x16x128_f8f6f4 on e4m3 x e4m3 operands at twice the bf16 MFMA rate
                                           (BASELINE configs[4]).  The LayerNorms emit e4m3 codes with one power-of-two scale
                                           per row, the GELU output and the attention context are re-quantised under one
                                           calibrated power-of-two scale per block (sgpt_model_calibrate_begin / _end), scales
                                           are applied to the fp32 accumulators; q / k / V^T, softmax and P.V stay bf16 / fp32,
                                           the residual stream fp32.  Shapes that do not fit the 256x256x256 fp8 tile
                                           run the SGPT_FP8W arithmetic.  Cannot meet the 1e-3 bar (3 mantissa bits): the
                                           tests report max |dcos| and top-10 overlap against the fp32 oracle instead */
    const uint8_t* layer_is_local;  /* host, [n_layers]: 1 = sliding-window layer (HF:gpt_neo:66) */
    int32_t rotary_dim;      /* GPT-J: leading dims of every head that get rotary position embedding (64).  SGPT_ARCH_LLAMA (ABI v16):
                                the head dim, n_heads * rotary_dim need not be d_model; 0 = d_model / n_heads */
    int32_t qk_split;        /* SGPT_F16 / SGPT_BF16 only.  1 = split-precision Q / K projection: the LayerNorm output a and the
                                Wq / Wk weights enter the projection as hi + lo pairs of 16-bit values (a_hi.W_hi + a_lo.W_hi +
                                a_hi.W_lo: one GEMM over K' = 3 d on the same MFMA), i.e. to ~2^-22 instead of 2^-11 each; q / k
                                are stored in 16 bits as before.  For GPT-Neo (attention without 1/sqrt(dh), HF:gpt_neo:110) the
                                path LayerNorm -> Wq / Wk -> q / k carries 80 % of the 16-bit deviation at d = 2048:
                                SGPT-1.3B shape goes from 8.2e-4 / 1.09e-3 (cosine / embedding) to well inside the 1e-3 bar, for
                                three times the FLOPs of one of the five projections.  0 (default) = off.  (= precision plan entry
                                SGPT_PC_LN1 = 1 in every block, see sgpt_model_set_precision) */
    int32_t split_weights;   /* SGPT_F16 / SGPT_BF16 only.  1 = also keep [W_hi | W_hi | W_lo] copies of all four matmul weights of
                                every block (3 x the 16-bit weight bytes on top of the plain copy) so that sgpt_model_set_precision
                                can move any operand class of any block to split precision after load.  0 (default) = off */
    int32_t n_kv_heads;      /* ABI v15, SGPT_ARCH_LLAMA only: key / value heads (grouped K / V), n_heads % n_kv_heads == 0; 0 = n_heads */
} sgpt_model_desc;

/* One named fp32 weight tensor under its HF state-dict name
 * (GPT-Neo: "wte.weight", "wpe.weight", "h.0.attn.attention.q_proj.weight", ..., "ln_f.bias";
 *  GPT-J:   "wte.weight", "h.0.attn.q_proj.weight", "h.0.mlp.fc_in.weight", ..., plus the rotary tables
 *           "rotary.sin" / "rotary.cos" fp32[max_pos, rotary_dim/2] = HF create_sinusoidal_positions,
 *           HF:gptj/modeling_gptj.py:47-50, computed by the host so they match the reference bit for bit;
 *  BERT:    "embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight" (token_type_embeddings[0] added by the
 *           caller), "embeddings.LayerNorm.{weight,bias}", "encoder.layer.0.attention.self.{query,key,value}.{weight,bias}" (fused
 *           to [3d, d] by the library), "encoder.layer.0.attention.output.{dense,LayerNorm}.*", "encoder.layer.0.intermediate.dense.*",
 *           "encoder.layer.0.output.{dense,LayerNorm}.*";
 *  LLAMA:   "embed_tokens.weight", "layers.0.input_layernorm.weight", "layers.0.self_attn.qkv_proj.weight" (q_proj | k_proj | v_proj
 *           rows fused by the caller, [d + 2 d_kv, d] with d_kv = n_kv_heads * head_dim), "layers.0.self_attn.o_proj.weight",
 *           "layers.0.post_attention_layernorm.weight", "layers.0.mlp.gate_up_proj.weight" (gate_proj rows, then up_proj rows,
 *           [2 d_ffn, d]), "layers.0.mlp.down_proj.weight", "norm.weight", plus "rotary.sin" / "rotary.cos" fp32[max_pos, head_dim/2]
 *           (angle = pos * rope_theta^(-2i / head_dim), computed by the host); no biases but the optional
 *           "layers.0.self_attn.qkv_proj.bias" [d_q + 2 d_kv]; optional "layers.0.self_attn.{q_norm,k_norm}.weight" [head_dim]
 *           (ABI v16, see SGPT_ARCH_LLAMA; with an explicit head dim the fused weight is [d_q + 2 d_kv, d], o_proj [d, d_q]);
 *  BLOOM:   "word_embeddings.weight", "word_embeddings_layernorm.*", "h.0.self_attention.query_key_value.{weight,bias}"
 *           (fused, head-interleaved [n_head, 3, head_dim] rows, HF:bloom:214 -- de-interleaved by the library),
 *           "h.0.self_attention.dense.*", "h.0.mlp.dense_h_to_4h.*", ..., plus "alibi.slopes" fp32[n_head]
 *           (HF build_alibi_tensor, HF:bloom:62-79)). */
typedef struct {
    const char* name;
    const float* ptr;        /* device, contiguous fp32 */
    int64_t numel;
} sgpt_tensor_view;

/* -- lifetime ------------------------------------------------------------------------- */
int sgpt_abi_version(void);
sgpt_status sgpt_ctx_create(int hip_device, sgpt_ctx** out);
void sgpt_ctx_destroy(sgpt_ctx* ctx);
const char* sgpt_last_error(const sgpt_ctx* ctx);

/* Replaces AutoModel.from_pretrained(...).to(device) (biencoder/beir/beir_dense_retriever.py:123;
 * sentence_transformers/models/Transformer.py:38).  Copies / packs the weights into
 * library-owned device memory (fused [3d,d] QKV; bf16 rounding (RNE) of the six matmul
 * weights per block when compute_dtype == SGPT_BF16); the caller may free its tensors after
 * return. */
sgpt_status sgpt_model_load(sgpt_ctx* ctx, const sgpt_model_desc* desc,
                            const sgpt_tensor_view* tensors, size_t n_tensors, sgpt_model** out);
void sgpt_model_free(sgpt_model* model);

/* SGPT_FP8M activation-scale calibration.  Between _begin and _end every sgpt_encode on the model runs the SGPT_FP8W
 * arithmetic and records max |gelu output| and max |attention context| per block; _end turns the maxima into per-block
 * power-of-two scales (smallest 2^k with margin * max / 2^k <= 448; margin >= 1, default 2) and returns them (host
 * float[2 * n_layers]: the GELU-output scales, then the context scales; may be NULL).  sgpt_model_set_act_scales installs
 * scales computed elsewhere (2 * n_layers powers of two).  A later batch that saturates the e4m3 range raises bit 1 of the
 * flag read by sgpt_range_check. */
sgpt_status sgpt_model_calibrate_begin(sgpt_model* model);
sgpt_status sgpt_model_calibrate_end(sgpt_model* model, float margin, float* scales_out);
sgpt_status sgpt_model_set_act_scales(sgpt_model* model, const float* scales, int32_t n_scales);

/* -- a2+a3+a4: forward + pool --------------------------------------------------------- */
/* Replaces, in ONE call and with no hidden-state D2H:
 *   AutoModel(**tokens, output_hidden_states=True)   beir_dense_retriever.py:204-205 / Transformer.py:72
 *     = HF GPTNeoModel.forward                       HF:gpt_neo/modeling_gpt_neo.py:398-505
 *   hidden_state = all_hidden_states[layeridx]       beir_dense_retriever.py:233
 *   weightedmean / mean / lasttoken pooling          beir_dense_retriever.py:238-282; Pooling.py:99-125
 *   optional F.normalize                             SentenceTransformer.py:248-249
 *
 * Token layout (varlen, no FLOPs on padding): sequence b owns rows
 * [seq_off[b], seq_off[b+1]) of the packed token axis; its seq_len[b] real tokens come
 * first.  seq_off[] are even (ABI <= v5 asked for multiples of 8; any such layout is still valid), seq_off[B] <= T_pad, T_pad is a multiple of 32
 * (ABI <= v7: 128; rows past seq_off[B] are filler: computed by the row-wise kernels, never attended to).  Layouts of at most
 * 4096 rows take the query- / mid-sized kernels (csrc/qgemm.hip: tiles of 32 .. 128 rows, LayerNorm inside the projections); same bits.
 *   ids      device int32[T_pad]  token ids (filler rows: any valid id)
 *   pos      device int32[T_pad]  absolute position id = pad_left[b] + t  (HF:gpt_neo:451 uses
 *                                 the PADDED index arange(S); filler rows: 0)
 *   pad_left device int32[B]      left-padding of the reference batch (0 for right-padded
 *                                 GPT-2 tokenizers); the pooling weight of token t is
 *                                 pad_left[b] + t + 1 (Pooling.py:104-112, padded index)
 *   n_layers_run  number of blocks to run (n_layers for layeridx=-1)
 *   apply_final_ln  1 = ln_f (hidden_states[-1]); 0 = raw residual (hidden_states[i<L])
 *   out      device fp32[B, d_model]
 *   hidden_out  optional device fp32[T_pad, d_model]: the selected hidden state per token
 */
sgpt_status sgpt_encode(sgpt_model* model, const int32_t* ids, const int32_t* pos,
                        const int32_t* seq_off, const int32_t* seq_len, const int32_t* pad_left,
                        int32_t B, int32_t T_pad, int32_t max_alloc_len,
                        int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln,
                        int32_t normalize, float* out, float* hidden_out, void* stream);

/* sgpt_encode with the sequence starts of the layout in HOST memory as well (ABI v22): seq_off_host int32[B + 1] holds the values
 * of seq_off[] -- the library trusts that and cannot check it.  Knowing where the sequences start without reading the device,
 * the call may run its forward as two chains of whole sequences (sgpt_ctx_set_encode_chains below); NULL, or a layout the
 * conditions there refuse, is sgpt_encode itself.  Same results bit for bit either way. */
sgpt_status sgpt_encode_host_layout(sgpt_model* model, const int32_t* ids, const int32_t* pos,
                                    const int32_t* seq_off, const int32_t* seq_len, const int32_t* pad_left,
                                    int32_t B, int32_t T_pad, int32_t max_alloc_len,
                                    int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln,
                                    int32_t normalize, float* out, float* hidden_out, const int32_t* seq_off_host, void* stream);

/* sgpt_encode_host_layout with the pooled rows starting behind a prefix (ABI v24): pool_lo device int32[B] (NULL = zeros = the call
 * above exactly, bit for bit) -- sequence b is pooled over its token rows t in [min(max(pool_lo[b], 0), seq_len[b]), seq_len[b]): the
 * tokens behind an instruction prompt (sentence-transformers `include_prompt: false`, GritLM, LLM2Vec).  mean: over that range.
 * weightedmean: the weight of row t stays pad_left[b] + t + 1, the PADDED position index (Pooling.py) -- the weights do not restart
 * behind the prompt.  lasttoken: row seq_len[b] - 1 whatever pool_lo says.  An empty range is a zero row (the clamped denominator),
 * not NaN.  SGPT_POOL_CLS and SGPT_POOL_LEARNTMEAN with a non-NULL pool_lo are SGPT_ERR_INVALID.  seq_off_host may be NULL; in a call
 * that runs as two chains each chain reads its own sequences' entries. */
sgpt_status sgpt_encode_pool_from(sgpt_model* model, const int32_t* ids, const int32_t* pos,
                                  const int32_t* seq_off, const int32_t* seq_len, const int32_t* pad_left,
                                  int32_t B, int32_t T_pad, int32_t max_alloc_len,
                                  int32_t pool_mode, int32_t n_layers_run, int32_t apply_final_ln,
                                  int32_t normalize, float* out, float* hidden_out, const int32_t* seq_off_host,
                                  const int32_t* pool_lo, void* stream);

/* The attention mode of an SGPT_ARCH_LLAMA model (ABI v24), set after load.  causal = 1: the default, today's path bit for bit.
 * causal = 0: bidirectional -- see SGPT_ARCH_LLAMA above.  SGPT_ERR_INVALID, by name: for every other arch (SGPT_ARCH_BERT is
 * bidirectional by architecture, the GPT families stay causal), and with causal = 0 for a model whose descriptor applies a sliding
 * window on any layer (window > 0 on a layer layer_is_local marks; a Mistral window the loader of the caller folded away is not in
 * the descriptor, and inside a folded window the window hides nothing in either direction).  Graphs captured before a change are
 * stale (sgpt_ctx_generation moves). */
sgpt_status sgpt_model_set_attention(sgpt_model* model, int32_t causal);

/* The arithmetic of an SGPT_ARCH_LLAMA model's projections (ABI v25), set after load; no compute dtype, no descriptor field, no
 * calibration pass.  kind 0: 16-bit, the model as loaded (legal only on a model never converted: a no-op).  kind 1: fp8 -- layer by
 * layer w_qkv [d_q + 2 d_kv, d], w_fc [2 ffn, d] and w_proj [d, ffn] become e4m3fn codes with one power-of-two fp32 scale per output
 * row (sgpt_fp8_quantize_rows' rule and RNE codes, taken from the bf16 values the model holds), and each 16-bit allocation is freed as
 * its layer is done.  *bytes_freed (or NULL): the 16-bit bytes of the three matrices minus codes and scales, over all layers.  ONE-WAY.
 * The forward of a converted model: RMSNorm and SwiGLU write e4m3fn codes under one DYNAMIC power-of-two scale per token row
 * (sgpt_rmsnorm_fp8, sgpt_swiglu_fp8); q | k, V^T, gate | up and the down-projection run on the fp8 MFMA (sgpt_linear_fp8 epi 0 / 4 /
 * 0 / 2 with a_scale = the row scales); rotary, the q / k norm, the attention in either mode, pooling and the out-projection are the
 * 16-bit model's -- w_o stays 16-bit, its operand (the attention context) has no row scale.  sgpt_encode* then takes layouts of
 * T_pad % 256 == 0 only (SGPT_ERR_INVALID otherwise: no other path is left).  Graphs captured before the call are stale.
 * SGPT_ERR_INVALID, each by its own message: any arch but SGPT_ARCH_LLAMA; a compute dtype other than SGPT_BF16; d_model, d_q + d_kv,
 * d_kv or d_ffn not a multiple of 256; kind outside 0 | 1; kind 0 after a conversion; a second conversion.
 * sgpt_model_get_projections: *kind = 0 | 1. */
sgpt_status sgpt_model_set_projections(sgpt_model* model, int32_t kind, int64_t* bytes_freed);
sgpt_status sgpt_model_get_projections(sgpt_model* model, int32_t* kind);

/* All L+1 hidden states pooled in ONE forward: the `meanmean` / `lasttokenmean` methods
 * (beir_dense_retriever.py:243-257, 284-301; useb_dense_retriever.py:219-302) average the pooled vector of
 * every entry of `all_hidden_states`.  Entry i < L is the input of block i (raw residual stream), entry L is
 * ln_f of the last block's output (HF:gpt_neo:475-505).  Same token layout as sgpt_encode.
 *   out_layers device fp32[n_layers+1, B, d_model] (or NULL); normalize applies to every entry;
 *   out_mean   device fp32[B, d_model] (or NULL): the average of the L+1 entries = the method's embedding. */
sgpt_status sgpt_encode_layers(sgpt_model* model, const int32_t* ids, const int32_t* pos,
                               const int32_t* seq_off, const int32_t* seq_len, const int32_t* pad_left,
                               int32_t B, int32_t T_pad, int32_t max_alloc_len, int32_t pool_mode,
                               int32_t normalize, float* out_layers, float* out_mean, void* stream);

/* sgpt_encode_layers with pool_lo (ABI v24; see sgpt_encode_pool_from): every one of the L + 1 hidden states is pooled over the same range. */
sgpt_status sgpt_encode_layers_pool_from(sgpt_model* model, const int32_t* ids, const int32_t* pos,
                                         const int32_t* seq_off, const int32_t* seq_len, const int32_t* pad_left,
                                         int32_t B, int32_t T_pad, int32_t max_alloc_len, int32_t pool_mode,
                                         int32_t normalize, float* out_layers, float* out_mean, const int32_t* pool_lo, void* stream);

/* Trained position weights for SGPT_POOL_LEARNTMEAN: `position_weights` of
 * models/WeightedMeanPooling.py:21-39 (the reference reads them from 1_WeightedMeanPooling/pytorch_model.bin,
 * useb_dense_retriever.py:253-270).  Token t of a sequence is weighted by weights[pad_left + t]; the weight sum
 * is clamped at 1e-9.  The n fp32 values are copied (device pointer); n must cover the longest padded sequence. */
sgpt_status sgpt_model_set_pool_weights(sgpt_model* model, const float* weights, int32_t n);

/* Cross-encoder scoring: log P(target | prefix) under the LM head for selected token rows.
 * Replaces, for the rows that matter, `F.log_softmax(model(inps)[0], dim=-1)` + `torch.gather` + `argmax`
 * of crossencoder/beir/sgptce.py:233-255.  hidden = the post-ln_f hidden states of sgpt_encode (`hidden_out`,
 * fp32 [T_pad, d_model]); row_idx[i] = the token row whose next-token distribution is asked for, targets[i] the
 * token id to score.  The LM head is the embedding matrix (GPT-Neo, BLOOM: tied) or "lm_head.weight" /
 * "lm_head.bias" when those tensors were passed to sgpt_model_load (GPT-J).  Logits are computed in exact-fp32 MFMA.
 *   out_logprob device fp32[n]; out_greedy device int32[n] (argmax token, first maximum) or NULL.
 * Contract (the entry has no row count of `hidden` and cannot check the first point):
 *   - every row_idx[i] must lie in [0, T_pad): the gather reads row row_idx[i] of `hidden` and does NOT clamp -- an index outside
 *     the allocation is an out-of-bounds read (SGPTModel.lm_logprobs checks the indices on the host before it uploads them);
 *     targets[i] outside [0, vocab) is clamped to the nearest valid id (a bad target scores a wrong token);
 *   - d_model % 4 == 0 (sgpt_model_load guarantees % 128) and `hidden` 16-byte aligned with row stride d_model: rows are
 *     copied in 16-byte pieces;
 *   - the n rows are processed in chunks of 1024: per chunk a gather into a staging buffer, the fp32 GEMM [rows, vocab] with
 *     leading dimension roundup(vocab, 4) (+ bias), and the log-softmax.  Staging buffer and logits chunk live in the context's
 *     scorer workspace (1024 x roundup(vocab, 4) x 4 bytes: 206 MB at vocab 50 257), which grows on demand (a growth
 *     synchronises the device) and is reused by every call: calls on one context must be ordered on one stream, and the pad
 *     columns [vocab, roundup(vocab, 4)) of the logits are never written nor read.  The call overwrites what the last score +
 *     top-k pass left in that workspace: sgpt_score_overflow_count no longer describes that pass afterwards;
 *   - a row's result does not depend on n, on the row's position in its chunk or on the order of row_idx (every tile of the
 *     fp32 GEMM sums k ascending; the opt-in low-latency mode of a context, sgpt_ctx_set_low_latency, gives this up).
 * SGPT_ERR_INVALID (nothing launched): null model / hidden / row_idx / targets / out_logprob, n <= 0, a family without LM head. */
sgpt_status sgpt_lm_logprobs(sgpt_model* model, const float* hidden, const int32_t* row_idx, const int32_t* targets,
                             int32_t n, float* out_logprob, int32_t* out_greedy, void* stream);

/* Stand-alone pooling over caller-supplied hidden states (USEB layer sweeps, parity tests).
 * Replaces Pooling.forward (sentence_transformers/models/Pooling.py:99-125,129-164) and
 * CustomEmbedder.embed_batcher's pooling branch (beir_dense_retriever.py:238-282).
 *   hidden device [B,S,d], fp32, bf16 or f16 (hidden_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16; any other
 *   code is SGPT_ERR_INVALID); mask device int32[B,S] (0/1, any padding side);
 *   weights follow the padded index t+1; weight sum clamped at 1e-9 (Pooling.py:122).
 *   pool_mode SGPT_POOL_WEIGHTEDMEAN | _MEAN | _LASTTOKEN | _CLS (row 0 of every sequence, whatever the mask: Pooling.py:103-105). */
sgpt_status sgpt_pool(sgpt_ctx* ctx, const void* hidden, int32_t hidden_dtype, const int32_t* mask,
                      int32_t B, int32_t S, int32_t d, int32_t pool_mode, float* out, void* stream);
/* Same with per-position weights (SGPT_POOL_LEARNTMEAN): pos_weights device fp32[>= S]. */
sgpt_status sgpt_pool_learnt(sgpt_ctx* ctx, const void* hidden, int32_t hidden_dtype, const int32_t* mask,
                             int32_t B, int32_t S, int32_t d, const float* pos_weights, float* out, void* stream);

/* Row-wise x / max(||x||_2, 1e-12): torch.nn.functional.normalize(p=2, dim=1)
 * (sentence_transformers/util.py:41-42, 66-70).  out_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16 (any other code
 * is SGPT_ERR_INVALID); the 16-bit outputs are the fp32 result rounded once (RNE).  out may alias in when
 * out_dtype == SGPT_F32. */
sgpt_status sgpt_l2_normalize(sgpt_ctx* ctx, const float* in, int64_t n, int32_t d,
                              void* out, int32_t out_dtype, void* stream);

/* Row-wise scores of two [n, d] fp32 matrices (ABI v8): out[i] = dot(a[i], b[i]) -- util.pairwise_dot_score,
 * sentence_transformers/util.py:66-76 -- or, cosine != 0, the same sum over rows normalised as sgpt_l2_normalize does --
 * util.pairwise_cos_sim, util.py:79-91 (`pairwise_dot_score(normalize_embeddings(a), normalize_embeddings(b))`).
 * The reference's own cases: tests/test_util.py:69-76. */
sgpt_status sgpt_pairwise_scores(sgpt_ctx* ctx, const float* a, const float* b, int64_t n, int32_t d, int32_t cosine,
                                 float* out, void* stream);

/* fp32 -> bf16 / f16 (RNE) element-wise; used to keep a corpus shard in HBM in the scorer's 16-bit operand format
 * (out_dtype SGPT_BF16 | SGPT_F16; normalised embeddings are in [-1, 1], inside either range). */
sgpt_status sgpt_f32_to_16(sgpt_ctx* ctx, const float* in, int64_t numel, void* out, int32_t out_dtype, void* stream);
sgpt_status sgpt_f32_to_bf16(sgpt_ctx* ctx, const float* in, int64_t numel, void* out, void* stream);

/* Range guards.  The reference's fp32 CPU path cannot overflow, so the 16-bit / 8-bit paths must never do so silently.
 * sgpt_model_range_check: *flagged = the model's guard word since the last reset --
 *     bit 0: an sgpt_encode* call on this SGPT_F16 model rounded an activation of magnitude >= 32768 (or +-inf) to f16: the
 *            results of the affected calls are not trustworthy; call sgpt_model_range_adapt and re-run them;
 *     bit 1: an SGPT_FP8M GELU output saturated its e4m3 codes;  bit 2: an SGPT_FP8M attention context did (re-calibrate).
 *   Per model: a flag raised by one model is never attributed to another one sharing the ctx.  Synchronises `stream` (one
 *   4-byte read-back); the Python host calls it once per encode_ids().
 * sgpt_model_range_adapt (SGPT_F16): reads the magnitudes the flagged launches recorded per (block, operand class), raises
 *   the power-of-two shift of each such class so that the recorded maximum lands at <= 16384, clears bit 0 and returns the
 *   number of classes raised through *n_raised (0: nothing recorded).  Shifts never decrease; a class that would need more
 *   than 2^40 returns SGPT_ERR_RANGE.  Bumps sgpt_ctx_generation (captured graphs carry the factors as kernel arguments).
 * sgpt_model_get/set_range_shifts: the 4 * n_layers exponents (per block: LayerNorm-1 output, q | k | v, LayerNorm-2 output,
 *   GELU output) -- to pin the shifts found on one run for reproducible embeddings on the next (a shift changes results only
 *   through f16 subnormals: |v| * 2^-k < 6.1e-5).  A LayerNorm shift below the bound sgpt_model_load derived from this
 *   checkpoint's LayerNorm parameters is refused (the LayerNorm kernels carry no run-time tracker), and a pooled embedding
 *   that is not finite raises bit 0 whatever produced it.
 * sgpt_range_check: the same bit 0 for the ctx-level stand-alone ops (sgpt_linear with f16 output). */
sgpt_status sgpt_model_range_check(sgpt_model* model, int32_t* flagged, int32_t reset, void* stream);
sgpt_status sgpt_model_range_adapt(sgpt_model* model, int32_t* n_raised, void* stream);
sgpt_status sgpt_model_get_range_shifts(sgpt_model* model, int32_t* shifts, int32_t n);
sgpt_status sgpt_model_set_range_shifts(sgpt_model* model, const int32_t* shifts, int32_t n);
sgpt_status sgpt_range_check(sgpt_ctx* ctx, int32_t* flagged, int32_t reset, void* stream);

/* Precision plan (ABI v6): which operand classes of which blocks enter their MFMAs as split-precision pairs.
 * The reference runs fp32 everywhere (beir_dense_retriever.py:123,204-205; Transformer.py:38,72), so it has no checkpoint
 * on which 11-bit operands are not enough; this path does (real GPT-Neo checkpoints carry outlier channels: a row whose
 * energy sits in one or two entries puts their whole relative rounding error on the dot product).  A split class is stored
 * as hi = round16(v) and lo = round16(v - hi) -- a [hi | lo | hi] row of 3 K that the UNCHANGED 16-bit GEMM contracts
 * against [W_hi | W_hi | W_lo] (a_hi.W_hi + a_lo.W_hi + a_hi.W_lo: the product to ~2^-22 instead of 2^-11 per operand, at
 * a third of the 16-bit MFMA rate and ~5 x the exact-fp32 MFMA mode).
 *   plan: host int32[n_layers][SGPT_PREC_CLASSES], per block
 *     SGPT_PC_LN1  LayerNorm-1 output -> Q / K / V projection: 0 = plain, 1 = Q and K split (V from the hi block), 2 = Q, K, V,
 *                  3 = Q and K with the ACTIVATION alone split ([a_hi | a_lo] . [W_hi | W_hi]: K' = 2 d, half the extra FLOPs of 1)
 *     SGPT_PC_ATT  inside the attention: q, k, V^T and the probabilities as hi + lo pairs (logits and P.V as three MFMA
 *                  passes each; head_dim 64 / 128, GPT-Neo and BLOOM)
 *     SGPT_PC_CTX  attention context -> out-projection
 *     SGPT_PC_LN2  LayerNorm-2 output -> fc1 (GPT-J's parallel block reads ln_1's output: needs LN1 != 0 there)
 *     SGPT_PC_H    GELU output -> fc2
 *   Every class but LN1 = 1 / 3 (qk_split is enough) and ATT (activations only) needs sgpt_model_desc.split_weights.  All ones (LN1 = 2) = the "f16x3" mode: embeddings within
 *   ~1e-5 of the fp32 reference on any checkpoint the f16 RANGE guard accepts.  Changing the plan bumps sgpt_ctx_generation.
 * sgpt_model_precision_probe_begin / _end: between the two calls every sgpt_encode on the model also records, per block and
 *   class (LayerNorm-1 output, attention context, LayerNorm-2 output, GELU output: 4 * n_layers floats), the largest crest
 *   factor max|v| / rms(v) over the rows of the operand -- 4-10 for a well-conditioned row, ~sqrt(K / 2) when two entries carry
 *   the row.  The host turns them into a plan (sgpt_amd/model.py: classes above 12 / 20 are split, and with them the
 *   attention of the block; by default any such class moves the whole model to f16x3).  The recording launches are extra
 *   kernels: results of the probed calls are unchanged.
 * sgpt_split16: fp32 rows [n, d] -> 16-bit rows [n, 3 d] for a split-precision SCORER on the same kernels: layout 0 =
 *   [hi | lo | hi] (documents), layout 1 = [hi | hi | lo] (queries); sgpt_scores / sgpt_score_topk over d' = 3 d then give
 *   q_hi.c_hi + q_hi.c_lo + q_lo.c_hi.  (Normalised embeddings that two channels dominate lose up to 4e-4 of cosine to the
 *   16-bit corpus format alone.)
 * sgpt_linear_split: sgpt_linear (epi 0 | 1 | 4, 16-bit output) with the split store epilogue: hi at out, lo at out + lo_delta,
 *   a second hi at out + hi2_delta when != 0 (element offsets; ldo = leading dimension of out): kernel-level tests. */
#define SGPT_PREC_CLASSES 5
enum { SGPT_PC_LN1 = 0, SGPT_PC_ATT = 1, SGPT_PC_CTX = 2, SGPT_PC_LN2 = 3, SGPT_PC_H = 4 };
sgpt_status sgpt_model_set_precision(sgpt_model* model, const int32_t* plan, int32_t n);
sgpt_status sgpt_model_get_precision(sgpt_model* model, int32_t* plan, int32_t n);
/* sgpt_model_release_split_weights: give the [W_hi | W_hi | W_lo] copies of sgpt_model_desc.split_weights back (3 x the 16-bit
 *   weight bytes: +0.5 GB at SGPT-125M, +35 GB at GPT-J-6B shape) once the plan is known not to need them -- what the host does when
 *   the probe of precision='auto' settles on plain operands.  Refused while the installed plan reads the out-projection / fc1 /
 *   fc2 copies (context, LayerNorm-2, GELU classes); the Q / K / V copy stays when a LayerNorm-1 entry (precise_qk) reads it; afterwards
 *   sgpt_model_set_precision refuses plans that would, exactly as for a model loaded without split_weights.  bytes_freed may
 *   be NULL.  (The reference keeps one fp32 copy of the weights: `AutoModel.from_pretrained`, beir_dense_retriever.py:123.) */
sgpt_status sgpt_model_release_split_weights(sgpt_model* model, int64_t* bytes_freed);
sgpt_status sgpt_model_precision_probe_begin(sgpt_model* model);
sgpt_status sgpt_model_precision_probe_end(sgpt_model* model, float* crest_out /* host float[4 * n_layers] or NULL */);
 /* sgpt_row_crest: the probe's statistic for caller-owned 16-bit rows [n, d] (leading dimension ld): max over the rows of
 *   max|v| / rms(v), returned to the host (synchronises `stream`).  The search host uses it on the gathered query embeddings --
 *   identical on every rank -- to decide whether a 16-bit corpus is kept as split pairs. */
sgpt_status sgpt_row_crest(sgpt_ctx* ctx, const void* x, int32_t dtype, int64_t n, int32_t d, int64_t ld, float* crest_out,
                           void* stream);
sgpt_status sgpt_split16(sgpt_ctx* ctx, const float* in, int64_t n, int32_t d, int32_t layout, void* out, int32_t out_dtype,
                         void* stream);
sgpt_status sgpt_linear_split(sgpt_ctx* ctx, int32_t dtype, int32_t epi, const void* A, const void* W, const float* bias,
                              void* out, int64_t ldo, int64_t lo_delta, int64_t hi2_delta, int32_t M, int32_t N, int32_t K,
                              void* stream);

/* hipGraph support.  sgpt_ctx_generation changes whenever a library-owned buffer that launched kernels point into is
 * re-allocated (workspace growth, a larger learnt-pooling table): a graph captured at generation g must be re-captured
 * (or refused) once the value differs.  sgpt_ctx_reserve grows the encoder / scorer workspaces to at least the given
 * sizes up front so that no growth happens while graphs are alive. */
uint64_t sgpt_ctx_generation(const sgpt_ctx* ctx);
sgpt_status sgpt_ctx_reserve(sgpt_ctx* ctx, size_t encode_bytes, size_t score_bytes);

/* fp8 weight storage (SGPT_FP8W) building blocks, exported for parity tests and for callers that keep
 * their own quantised checkpoints.  w device fp32[rows, cols] (cols % 4 == 0) -> codes uint8[rows, cols]
 * (OCP e4m3fn, round-to-nearest-even) + scale fp32[rows], scale = the smallest power of two with
 * max|w_row| / scale <= 448.  De-quantisation code * scale is exact in bf16 and in fp32 (out_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16; in
 * f16 exact while code * scale is an f16 value -- the rows of a quantised corpus, sgpt_score_topk_q8); the NaN codes 0x7f / 0xff,
 * which the quantiser emits for NaN input only, de-quantise to NaN. */
sgpt_status sgpt_fp8_quantize_rows(sgpt_ctx* ctx, const float* w, int64_t rows, int64_t cols,
                                   uint8_t* codes, float* scale, void* stream);
sgpt_status sgpt_fp8_dequantize_rows(sgpt_ctx* ctx, const uint8_t* codes, const float* scale, int64_t rows,
                                     int64_t cols, void* out, int32_t out_dtype, void* stream);

/* -- a7: scoring ---------------------------------------------------------------------- */
/* Replaces cos_sim / dot_score = torch.mm(a, b.T) (sentence_transformers/util.py:24-63;
 * beir.util, imported at custommodels/exact_search.py:9): out[i][j] = <a_i, b_j>, NaN kept.
 * For cosine the caller normalises first (sgpt_l2_normalize), exactly as util.py:41-43.
 *   a device [na,d], b device [nb,d], both of `dtype` (fp32: exact fp32 MFMA; bf16 / f16: 16-bit MFMA,
 *   fp32 accumulate); d multiple of 4 (fp32) / 8 (16-bit); out device fp32[na, ldo], ldo >= nb, ldo%4==0. */
sgpt_status sgpt_scores(sgpt_ctx* ctx, const void* a, const void* b, int32_t dtype,
                        int64_t na, int64_t nb, int32_t d, float* out, int64_t ldo, void* stream);

/* -- a7+a8: fused chunked score + top-k ------------------------------------------------ */
/* Replaces the body of the corpus-chunk loop of DenseRetrievalExactSearch.search
 * (custommodels/exact_search.py:96-108): scores = q . corpus^T ; scores[isnan] = -1 ;
 * topk(min(k, n)) -- and, when run_val/run_idx already hold `n_run` entries per query from
 * earlier chunks, the heapq.nlargest merge of :121-132 (the set of the k best of old+new).
 *   q       device [nq,d] of `dtype`;  corpus device [N,d] of `dtype`
 *   idx_base  global index of corpus row 0 (rank offset when the corpus is sharded)
 *   run_val device fp32[nq,k], run_idx device int64[nq,k]: in = running best (first n_run
 *           columns valid), out = new running best, sorted by descending score
 *           (ties: ascending index); unused tail = (-inf, -1).
 *   returns through *n_out (host) the number of valid columns = min(k, n_run + N).
 * Long corpora (bf16 or f16, d % 64 == 0, d >= 128, k <= 1024, N >= two chunks): only the first chunk's scores are materialised;
 * later chunks double in length and their GEMM epilogue appends just the scores above the query's running k-th
 * best to a candidate list that a small merge kernel folds into the running top-k.  The result is identical to
 * the materialised loop; a candidate-list overflow raises a device flag on which a materialised recomputation of
 * the call is predicated (its kernels exit at once otherwise), so the call stays asynchronous on `stream`. */
sgpt_status sgpt_score_topk(sgpt_ctx* ctx, const void* q, const void* corpus, int32_t dtype,
                            int32_t nq, int64_t N, int32_t d, int32_t k, int64_t idx_base,
                            float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                            void* stream);

/* sgpt_score_topk_q8 (ABI v18): sgpt_score_topk over a corpus held as fp8 -- half the bytes of a 16-bit corpus in memory and
 * per search pass.
 *   format    codes device uint8 [N, d]: OCP e4m3fn; scale device fp32 [N]: one power of two per document, document n =
 *             code[n][:] * scale[n].  The rule of sgpt_fp8_quantize_rows: scale = the smallest power of two with max|row| / scale <= 448,
 *             codes round-to-nearest-even (NaN -> the NaN code).  Rows come from sgpt_l2_normalize (fp32 out) + sgpt_fp8_quantize_rows.
 *   q         device f16 [nq, d], 16-byte aligned.
 *   exactness every e4m3 value is an f16 value, so the kernel feeds the f16 MFMA with exactly the de-quantised corpus (the scale, a
 *             power of two, multiplies the fp32 accumulator): the result equals sgpt_score_topk(SGPT_F16) on the de-quantised rows bit
 *             for bit (as long as code * scale is an f16 value, which holds for unit rows).  The only approximation is the quantisation:
 *             |s_fp8 - s| <= 2^-4 sum_i |q_i c_i| + 2^-10 scale sum_i |q_i| per score (e4m3 round-to-nearest, relative 2^-4 per element;
 *             elements below half the smallest subnormal 2^-9 scale flush to zero), on top of the f16 scorer's own arithmetic.
 *   shapes    nq <= 64 and d % 128 == 0 (codes 8-byte aligned): every whole 256-document tile streams through the one-byte tile (score64c.h), which
 *             reads the codes themselves; a ragged tail (< 256 documents) is de-quantised to f16 scratch.  Everything else (nq > 64:
 *             MFMA-bound; other d): blocks of at most 131 072 documents are de-quantised to f16 workspace and scored by the f16 path,
 *             the running list chained -- the memory saving holds, no speed is claimed.
 *   result    as sgpt_score_topk: rows sorted descending, ties to the lowest index, NaN scores (a NaN code) -> -1, running list in/out.
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers, d % 8, k <= 0, n_run > k, q not 16-byte aligned. */
sgpt_status sgpt_score_topk_q8(sgpt_ctx* ctx, const void* q, const uint8_t* codes, const float* scale, int32_t nq, int64_t N, int32_t d,
                               int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                               void* stream);

/* Binary (1-bit) corpus (ABI v19): packed sign bits, Hamming search, re-scoring of an over-fetched candidate list -- the recipe known
 * as quantize_embeddings(precision="ubinary") + Hamming search + rescoring.  96 bytes per document at d = 768: 1/16 of f16 rows.
 * The candidates are re-scored from the sign bits or an fp8 copy (sgpt_score_topk_bits: one query matrix, so an fp8 copy serves uncentred
 * bits only) or from a uint8 copy (sgpt_score_topk_bits_u8, ABI v21, below the uint8 corpus: raw queries plus the centre, so it serves
 * centred bits too).
 *   format    bits device uint8 [N, ldb], ldb % 4 == 0, ldb >= 4 * ceil(d / 32).  Dimension i of a document is bit 7 - i % 8 of byte
 *             i / 8 (the order of numpy.packbits); a bit is 1 exactly when the element is > 0 (NaN, +0, -0 give 0); bits d .. 8 ldb - 1
 *             are zero.  bits[:, :ceil(d / 8)] equals numpy.packbits(x > 0, axis=-1).
 * sgpt_pack_sign_bits: rows x - center (center device fp32 [d], or NULL: rows x) of x device fp32 [n, d] -> that format, pad bits
 * included.  SGPT_ERR_INVALID: null pointers, n <= 0, d <= 0, a bad ldb. */
sgpt_status sgpt_pack_sign_bits(sgpt_ctx* ctx, const float* x, int64_t n, int32_t d, const float* center /* fp32[d] or NULL */,
                                uint8_t* bits, int64_t ldb, void* stream);

/* sgpt_score_topk_bits (ABI v19): two-stage search over a binary corpus.
 *   q         device fp32 [nq, d]: normalised by the caller, and centred if the corpus was; the call packs its sign bits itself.
 *   stage 1   always fresh on this call's N documents: agreement a = d - 2 * hamming(sign q, bits[n]) = <sign q, sign d_n> (signs +-1), an
 *             integer; the candidate list is the min(kp, N) best by (a descending, index ascending) -- exact, whatever ties there are.
 *             The Hamming tile (csrc/scorebits.hip) streams the rows through registers under sgpt_score_topk's filtered schedule; a
 *             candidate-list overflow (integer scores tie at the threshold) takes the same predicated, sync-free fallback.
 *   mode 0    Hamming only, kp == k: value float(a) / float(d), one IEEE fp32 division; order a descending, ties to the lowest index.
 *   mode 1    sign re-scoring, no extra memory: value <q, s_n> / sqrt(d), s_n the document's +-1 sign vector over its d true dimensions,
 *             accumulated in fp32.
 *   mode 2    fp8 re-scoring: codes / scale = the same documents in the format of sgpt_score_topk_q8, code rows ceil(d / 8) * 8 bytes
 *             apart (the padded width the quantiser produced); value <q, code_n * scale_n> in fp32; a NaN code gives -1.
 *             Modes 1 and 2 order by value descending, ties to the lowest index.  k <= kp <= 1024.
 *   result    as sgpt_score_topk: this call's list is merged with the running list (run_val / run_idx, n_run) into the new top-k, unused
 *             tail (-inf, -1), *n_out = min(k, n_run + N), a NaN value becomes -1.  The running list must hold values of the SAME mode
 *             (and the same d for mode 0): values of different modes are not comparable.
 *   shapes    any nq >= 1 (queries beyond 64 are served in groups of 64, each re-streaming the rows), any d >= 1, any N >= 1; speed is
 *             claimed for d % 128 == 0 (16-byte loads need ldb % 16 == 0 and 16-byte aligned bits; a dword path serves the rest).
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers; ldb < 4 * ceil(d / 32) or ldb % 4; k <= 0, kp < k, kp > 1024,
 * mode 0 with kp != k; mode outside 0..2; mode 2 without codes or scale; n_run < 0 or n_run > k. */
sgpt_status sgpt_score_topk_bits(sgpt_ctx* ctx, const float* q, const uint8_t* bits, int64_t ldb, int32_t nq, int64_t N, int32_t d,
                                 int32_t k, int32_t kp, int32_t mode, const uint8_t* codes, const float* scale, int64_t idx_base,
                                 float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream);

/* uint8 corpus (ABI v20): scalar quantisation with one range per DIMENSION -- quantize_embeddings(precision="uint8") of
 * sentence-transformers.  One byte per element as the fp8 corpus; 256 uniform levels inside each column's own range instead of three
 * mantissa bits under one scale per row, which suits anisotropic embeddings (a few channels carry the row) far better.
 *   format    codes device uint8 [N, ld], ld = ceil(d / 128) * 128, columns d .. ld - 1 hold 128; start, step device fp32 [ld], pad columns
 *             start = step = 0.  Document n is x^[n][j] = start[j] + codes[n][j] * step[j].  With mid = start + 128 * step and
 *             c = code - 128 this is mid[j] + c * step[j]; codes - 128 as int8 are sentence-transformers' "int8" codes.
 *   rule      codes = clamp(rint((x - start) / step), 0, 255) in fp32: IEEE subtraction and division, round-half-even; step == 0 or a NaN
 *             element gives 128.  Elements outside [start, start + 255 step] clamp to the ends (ranges taken from a calibration sample).
 *   ranges    start = the column minimum, step = (max - min) / 255 in fp32.
 * sgpt_u8_col_minmax: column min / max of x device fp32 [n, d] into col_min / col_max [d]; NaN-propagating (a NaN in a column makes both
 *   NaN); accumulate != 0: the two arrays go in holding the result of earlier blocks of rows, so blocks chain.
 * sgpt_u8_quantize_rows: x device fp32 [n, d] -> codes [n, ld] by the rule, pad columns included (start / step are read for j < d).
 * sgpt_u8_dequantize_rows: codes [n, ld] -> out [n, ld] (SGPT_F32 | SGPT_BF16 | SGPT_F16, 16-byte aligned): start + code * step with the
 *   product and the sum each rounded once in fp32 (no fused multiply-add), then one rounding to the output format.
 * SGPT_ERR_INVALID: null pointers, n <= 0, d <= 0, ld % 128, d > ld, codes not 4-byte aligned. */
sgpt_status sgpt_u8_col_minmax(sgpt_ctx* ctx, const float* x, int64_t n, int32_t d, int32_t accumulate, float* col_min, float* col_max,
                               void* stream);
sgpt_status sgpt_u8_quantize_rows(sgpt_ctx* ctx, const float* x, int64_t n, int32_t d, int32_t ld, const float* start, const float* step,
                                  uint8_t* codes, void* stream);
sgpt_status sgpt_u8_dequantize_rows(sgpt_ctx* ctx, const uint8_t* codes, int64_t n, int32_t ld, const float* start, const float* step,
                                    void* out, int32_t out_dtype, void* stream);

/* sgpt_u8_prepare_queries (ABI v20; test entry): the query prologue sgpt_score_topk_u8 runs itself.  q device fp32 [nq, d], nq <= 64.
 *   q'_j = q_j * step_j (fp32); e = the exponent with max_j |q'_j| * 2^-e in [1, 2) (0 for a zero or non-finite row);
 *   qpad f16 [64, ld]: row r < nq holds RNE_f16(q'_j * 2^-e), rows nq .. 63 and columns d .. ld - 1 are zero;
 *   qscale fp32 [64] = 2^e (1 for rows >= nq); qbias fp32 [64] = sum_j q_j * mid_j accumulated in fp32 (0 for rows >= nq).
 * The power-of-two scale is needed: q_j * step_j is ~4e-5 for unit rows at d = 768, an f16 subnormal. */
sgpt_status sgpt_u8_prepare_queries(sgpt_ctx* ctx, const float* q, const float* start, const float* step, int32_t nq, int32_t d, int32_t ld,
                                    void* qpad, float* qscale, float* qbias, void* stream);

/* sgpt_score_topk_u8 (ABI v20): sgpt_score_topk over a uint8 corpus.
 *   q         device fp32 [nq, d], 1 <= nq <= 64 per call (larger batches: groups of 64, each re-streaming the corpus).
 *   score     <q, x^_n> = qbias + qscale * <q'', c_n>: the kernel (csrc/scoreu8.hip) streams the code bytes, turns them into the exact f16
 *             integers code - 128 and feeds the f16 MFMA with the pre-scaled query q''; products of an 11-bit by an 8-bit significand
 *             are exact in fp32, sums accumulate in fp32 with k ascending, and ONE fma, score = fmaf(acc, qscale, qbias), returns to the
 *             natural domain before the NaN rule (NaN -> -1) and the threshold compare.  The result equals sgpt_score_topk(SGPT_F16) of
 *             q'' against the f16 rows codes - 128, followed by that fma, bit for bit.
 *   error     arithmetic: |score - exact(q'', qscale, qbias, codes)| <= d 2^-23 qscale sum_j |q''_j c_j| + 2^-23 |score|;
 *             quantisation, rows inside the ranges: |<q, x^> - <q, x>| <= sum_j |q_j| step_j / 2 (+ |q_j| times the clamp distance outside).
 *   shapes    any N >= 1 (rows past the last document of a ragged 256-document tile are fetched from the last row and their columns
 *             dropped: no scratch, no tail launch), any d >= 1 with ld = ceil(d / 128) * 128; codes 16-byte aligned.
 *   result    as sgpt_score_topk: rows sorted descending, ties to the lowest index, running list in/out, *n_out = min(k, n_run + N).
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers; nq > 64; ld % 128; d > ld; codes not 16-byte aligned; k <= 0;
 * n_run < 0 or n_run > k. */
sgpt_status sgpt_score_topk_u8(sgpt_ctx* ctx, const float* q, const uint8_t* codes, const float* start, const float* step, int32_t nq,
                               int64_t N, int32_t d, int32_t ld, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx,
                               int32_t n_run, int32_t* n_out, void* stream);

/* Binary corpus with a uint8 second stage (ABI v21): binary retrieval + int8 re-scoring -- the Hamming search of sgpt_score_topk_bits,
 * its candidates re-scored from a uint8 copy of the same documents, on a centred corpus or not.
 *
 * sgpt_u8_rescore: the second stage alone -- the values of caller-given candidate lists against a uint8 corpus (the candidates may come
 * from any first stage).
 *   q         device fp32 [nq, d]; codes / start / step / ld: the uint8 corpus above (N documents, codes 16-byte aligned).
 *   idx       device int64 [nq, m], rows ld_idx >= m apart: candidate document indices idx_base + n, 0 <= n < N.
 *   value     out_val[i][j] = <q_i, x^_n> = qbias_i + sum_j q'_ij (code[n][j] - 128), q'_ij = q_ij * step_j (fp32, one rounding),
 *             qbias_i = sum_j q_ij * mid_j, mid_j = start_j + 128 * step_j (fp32; thread t of 256 adds columns t, t + 256, ... in
 *             ascending order, the 256 partial sums are added in a fixed tree).  One launch computes q' and qbias per call; the gather kernel
 *             (csrc/scoreu8.hip) reads the code rows in 16-byte pieces, lane l of a wave owning pieces l, l + 64, ...: four fp32
 *             accumulators per lane (one per dword of a piece) take their products by fma with columns ascending, are added as
 *             (a0 + a1) + (a2 + a3), the 64 lanes in a fixed butterfly, then qbias.  The order depends on ld alone -- not on nq, m, the
 *             slot a candidate sits in or the launch shape: equal inputs give equal bits.  code - 128 and its conversion to fp32 are exact.  NaN -> -1.
 *   error     |value - <q, x^_n> in exact arithmetic| <= (d + 2) 2^-23 (sum_j |q_j step_j c_nj| + sum_j |q_j mid_j|) + 2^-23 |value|,
 *             c = code - 128: every partial sum passes at most d inexact additions (a pad column adds an exact zero), q' and
 *             q_j * mid_j round once and mid_j once more, each rounding relative 2^-24, with the customary factor 2 for the
 *             second-order terms; the last addition rounds the value itself.
 *   result    out_val / out_idx [nq, m], slot for slot, NOT sorted: out_idx = idx.  A slot with idx < 0 or idx - idx_base outside [0, N)
 *             gives (-inf, -1) and reads no row.
 *   shapes    any nq, m, N >= 1, any d >= 1 with ld = ceil(d / 128) * 128; q' stays in registers for d <= 2048 and is re-read beyond.
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers; nq, N, d or m <= 0; ld % 128; d > ld; ld_idx < m; codes not
 * 16-byte aligned. */
sgpt_status sgpt_u8_rescore(sgpt_ctx* ctx, const float* q, const uint8_t* codes, const float* start, const float* step, int32_t nq, int64_t N,
                            int32_t d, int32_t ld, const int64_t* idx, int64_t ld_idx, int32_t m, int64_t idx_base, float* out_val,
                            int64_t* out_idx, void* stream);

/* sgpt_score_topk_bits_u8 (ABI v21): sgpt_score_topk_bits with that second stage.
 *   q         device fp32 [nq, d]: normalised by the caller and RAW -- not centred, unlike sgpt_score_topk_bits.
 *   center    device fp32 [d] or NULL: what the corpus bits were centred on.
 *   bits/ldb  as sgpt_score_topk_bits; codes / start / step / ld: the same N documents as a uint8 corpus (rows from sgpt_u8_quantize_rows of
 *             the UNcentred rows), codes 16-byte aligned.
 *   stage 1   that of sgpt_score_topk_bits on the matrix q - center (one IEEE fp32 subtraction per element, taken by sgpt_pack_sign_bits'
 *             kernel as it packs the query bits): the same Hamming tile, schedule and predicated fallback, the same candidate list index
 *             for index.
 *   stage 2   sgpt_u8_rescore's value of every candidate from the raw q (its arithmetic, order and error bound); NaN -> -1; order by value
 *             descending, ties to the lowest index.
 *   result    as sgpt_score_topk_bits: merged with the running list (which must hold values of this entry), unused tail (-inf, -1),
 *             *n_out = min(k, n_run + N).
 *   shapes    any nq >= 1, any d >= 1, any N >= 1, k <= kp <= 1024.
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers (center may be NULL); ldb < 4 * ceil(d / 32) or ldb % 4; ld % 128;
 * d > ld; codes not 16-byte aligned; k <= 0, kp < k, kp > 1024; n_run < 0 or n_run > k. */
sgpt_status sgpt_score_topk_bits_u8(sgpt_ctx* ctx, const float* q, const float* center /* fp32[d] or NULL */, const uint8_t* bits, int64_t ldb,
                                    const uint8_t* codes, const float* start, const float* step, int32_t ld, int32_t nq, int64_t N, int32_t d,
                                    int32_t k, int32_t kp, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                                    void* stream);

/* IVF corpus (ABI v26; csrc/ivf.hip): an inverted-file index over f16 rows -- spherical k-means cuts the L2-normalised corpus into nlist
 * lists, a query scores the centroids and scans only its nprobe best lists, with full-precision (f16 row, fp32 accumulate) scores for the
 * rows it reads.  Cosine only.
 *   format    centroids16 device f16 [nlist, d] (the f16 rounding of unit fp32 centroids); rows device f16 [N, d] in list-major order: list c
 *             is rows[offsets[c] .. offsets[c + 1]); ids device int64 [N]: the original row number of every stored row, ascending inside
 *             every list; offsets device int64 [nlist + 1], offsets[0] = 0, offsets[nlist] = N.
 *   limits    d % 8 == 0, d <= SGPT_IVF_MAX_DIM, nlist <= SGPT_IVF_MAX_LISTS, N <= SGPT_IVF_MAX_ROWS.
 *
 * sgpt_ivf_lists: an assignment -> the lists.  assign device int64 [N] -> perm device int64 [N], the STABLE argsort of assign (rows of a
 *   list in ascending row number), and offsets device int64 [nlist + 1], the exclusive prefix of the list sizes.  Integer arithmetic only
 *   (a device sort of the unique keys list << 32 | row): the result is the one exact answer.  An assignment outside [0, nlist) is clamped
 *   to the nearest end (memory-safe; the row lands in list 0 or nlist - 1).
 *   SGPT_ERR_INVALID: null pointers, N <= 0 or > SGPT_IVF_MAX_ROWS, nlist <= 0 or > SGPT_IVF_MAX_LISTS.
 *
 * sgpt_ivf_centroids: out[c] = the sum of x[perm[p]] over offsets[c] <= p < offsets[c + 1]; with normalize != 0 divided by its L2 norm.
 *   x         device [n_x, d], x_dtype SGPT_F32 | SGPT_F16 (f16 elements are widened exactly), 16-byte aligned; perm device int64 [n], offsets
 *             device int64 [nlist + 1] inside [0, n]; prev device fp32 [nlist, d] or NULL; out device fp32 [nlist, d].
 *   order     fixed by the list alone.  The list is cut into chunks of 256 rows counted from its own first row; a chunk's rows are added in
 *             ascending order into a partial sum (fp32, one rounding per addition, no fused operation), the list's partials are added in
 *             chunk order.  A long list is many chunks on many compute units.  No float atomics.  The bits of out[c] do not depend on
 *             nlist, on where the list sits in perm, or on the launch shape.  normalize: the squared norm is summed columns t, t + 256, ...
 *             ascending per thread t, the 256 threads in a fixed tree; one IEEE square root, one IEEE division per element.
 *   fallback  an empty list -- and under normalize a sum whose squared norm is zero or not finite -- gives prev[c] (zeros if prev is NULL).
 *             A perm entry outside [0, n_x) adds nothing; offsets that are no range inside [0, n] give an empty list.
 *   SGPT_ERR_INVALID: null pointers (prev may be NULL), another x_dtype, d % 8, d > SGPT_IVF_MAX_DIM, n or n_x <= 0, n > SGPT_IVF_MAX_ROWS,
 *   nlist <= 0 or > SGPT_IVF_MAX_LISTS, x or out not 16-byte aligned.
 *
 * sgpt_gather_rows: out[p] = RNE_f16(x[perm[p]]), p < n: x device [n_x, d] (SGPT_F32 | SGPT_F16), out device f16 [n, d], 16-byte loads and
 *   stores (d % 8 == 0, both 16-byte aligned).  A perm entry outside [0, n_x) gives a zero row.  SGPT_ERR_INVALID: null pointers, another
 *   x_dtype, d % 8, n or n_x <= 0, alignment.
 *
 * sgpt_ivf_search: the two-stage search.
 *   q         device fp32 [nq, d], L2-normalised by the caller, 16-byte aligned.
 *   stage 1   the probe set of a query is sgpt_score_topk(SGPT_F16) of RNE_f16(q) against centroids16 with k = nprobe: the same launches,
 *             so the same bits and the same order (score descending, ties to the lowest list).  probe_out (device int64 [nq, nprobe] or
 *             NULL) receives the probe sets.
 *   stage 2   one work item per (query, probed list, chunk of SGPT_IVF_CHUNK rows of that list); items past a list's end exit at once.  The
 *             grid comes from max_list (HOST: the longest list), so the call never synchronises; rows of a list beyond max_list are not
 *             scanned.
 *   value     sum_j q_j * float(row_j) in fp32: a wavefront walks the row in 16-byte pieces (8 elements), lane l owning pieces l, l + 64, ...;
 *             per lane four accumulators (one per dword of a piece) take their two products by fma, low half first, pieces ascending;
 *             s = (a0 + a1) + (a2 + a3); the 64 lanes are added in the xor butterfly 32, 16, .., 1.  The order depends on d alone: the same
 *             (q, row) pair gives the same bits in any list, position, nq, nprobe or launch shape.  NaN -> -1.
 *   error     |value - <q, row> in exact arithmetic| <= gamma_n sum_j |q_j row_j|, n = 2 ceil(d / 512) + 8, gamma_n = n u / (1 - n u),
 *             u = 2^-24: a partial sum passes at most 2 ceil(d / 512) fmas, 2 joining and 6 butterfly additions.
 *   select    every item keeps its min(k, SGPT_IVF_CHUNK) best by the library order (score descending, then original index ascending --
 *             ids ascend inside a list); the items' pairs and the running list go through the select kernel of sgpt_topk_merge.
 *   result    as sgpt_score_topk: rows sorted, tail (-inf, -1), indices ids[...] + idx_base, running list in/out.  *n_out = min(k, n_run + N):
 *             the host cannot know how many rows were probed, so slots that found no row are (-inf, -1) inside that count.
 *   shapes    any nq <= 65535 (in groups when the candidate workspace asks for it); speed is claimed for nq <= 64 only: a list probed by
 *             several queries is streamed once per query.
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers (probe_out may be NULL); nq <= 0 or > 65535; N <= 0; d % 8 or
 * d > SGPT_IVF_MAX_DIM; nlist <= 0 or > SGPT_IVF_MAX_LISTS; max_list < 0 or > N; nprobe <= 0, > nlist or > 1024; k <= 0 or > 1024; n_run < 0 or
 * > k; q, centroids16 or rows not 16-byte aligned. */
#define SGPT_IVF_CHUNK 256
#define SGPT_IVF_MAX_DIM 4096
#define SGPT_IVF_MAX_LISTS 65536
#define SGPT_IVF_MAX_ROWS (1 << 30)
sgpt_status sgpt_ivf_lists(sgpt_ctx* ctx, const int64_t* assign, int64_t N, int32_t nlist, int64_t* offsets, int64_t* perm, void* stream);
sgpt_status sgpt_ivf_centroids(sgpt_ctx* ctx, const void* x, int32_t x_dtype, int64_t n_x, int32_t d, const int64_t* perm, int64_t n,
                               const int64_t* offsets, int32_t nlist, const float* prev /* fp32[nlist, d] or NULL */, int32_t normalize,
                               float* out, void* stream);
sgpt_status sgpt_gather_rows(sgpt_ctx* ctx, const void* x, int32_t x_dtype, int64_t n_x, const int64_t* perm, int64_t n, int32_t d, void* out,
                             void* stream);
sgpt_status sgpt_ivf_search(sgpt_ctx* ctx, const float* q, const void* centroids16, const void* rows, const int64_t* ids,
                            const int64_t* offsets, int32_t nq, int64_t N, int32_t d, int32_t nlist, int64_t max_list, int32_t nprobe,
                            int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                            int64_t* probe_out /* int64[nq, nprobe] or NULL */, void* stream);

/* IVF corpus over uint8 lists (ABI v27; csrc/ivf.hip): the index above with the uint8 codes of the uint8 corpus (one range per DIMENSION,
 * sgpt_u8_quantize_rows) in its lists instead of f16 rows -- IVF-SQ8: ld bytes per stored row instead of 2 d.
 *   format    centroids16, ids, offsets as above; codes device uint8 [N, ld] in list-major order, ld = ceil(d / 128) * 128, pad columns hold
 *             128; start, step device fp32 [ld], pad columns 0.  Stored row n stands for x^[n][j] = start[j] + codes[n][j] * step[j].
 *
 * sgpt_u8_gather_quantize_rows: codes[p] = the rule of sgpt_u8_quantize_rows applied to x[perm[p]], p < n.
 *   format    x device [n_x, d], x_dtype SGPT_F32 | SGPT_F16 (f16 elements are widened exactly), 16-byte aligned; perm device int64 [n];
 *             start, step device fp32 [ld] (read for j < d); codes device uint8 [n, ld], 16-byte aligned.
 *   value     codes[p][j] = clamp(rint((x[perm[p]][j] - start[j]) / step[j]), 0, 255) in fp32 (IEEE subtraction and division,
 *             round-half-even; step == 0 or a NaN element gives 128) for j < d, 128 for d <= j < ld.  A perm entry outside [0, n_x) gives a
 *             row of 128s.  Integer codes: no error beyond the rule's own.
 *   result    bit-equal to sgpt_u8_quantize_rows of the gathered rows as fp32.  An index build needs the f16 rows once plus the codes,
 *             never a second list-major f16 copy.
 *   shapes    any n, n_x >= 1; one thread per 8 columns, 16- or 32-byte loads and one 8-byte store each.
 *   SGPT_ERR_INVALID (nothing launched, outputs untouched): null pointers, another x_dtype, d <= 0, d % 8, d > SGPT_IVF_MAX_DIM, ld % 128,
 *   d > ld, n or n_x <= 0, x or codes not 16-byte aligned.
 *
 * sgpt_ivf_search_u8: sgpt_ivf_search over such lists.
 *   q         device fp32 [nq, d], L2-normalised by the caller, 16-byte aligned.
 *   stage 1   that of sgpt_ivf_search, launch for launch: equal q and centroids16 give the same probe sets, bit for bit, as the f16 index.
 *   stage 2   the work items of sgpt_ivf_search: one per (query, probed list, chunk of SGPT_IVF_CHUNK rows), the grid from max_list, no host
 *             synchronisation; rows of a list beyond max_list are not scanned.
 *   value     <q_i, x^_n> = qbias_i + sum_j q'_ij (code_nj - 128), q'_ij = q_ij * step_j (fp32, one rounding), qbias_i = sum_j q_ij * mid_j,
 *             mid_j = start_j + 128 * step_j: q' and qbias are those of sgpt_u8_rescore, made by its prologue in one launch per call.
 *             code - 128 and its conversion to fp32 are exact; accumulation is fp32; NaN -> -1.
 *   order     fixed by ld alone.  G(ld) lanes of a wavefront cover a row, G = 8 for ld = 128, 16 for ld = 256, 32 for ld = 384 and 512, 64
 *             beyond (a wavefront walks 64 / G rows at once): lane l of the G owns the 16-byte pieces l, l + G, ...; per lane four
 *             accumulators (one per dword of a piece) take their four products by fma, bytes ascending, pieces ascending;
 *             s = (a0 + a1) + (a2 + a3); the G lanes are added in the xor butterfly G / 2, .., 1; value = s + qbias.  The same
 *             (q, code row) pair gives the same bits in any list, position, nq, nprobe or launch shape.
 *   error     |value - <q, x^_n> in exact arithmetic| <= gamma_n (sum_j |q_j step_j c_nj| + sum_j |q_j mid_j|), c = code - 128,
 *             gamma_n = n u / (1 - n u), u = 2^-24, n = max(4 ceil(ld / (16 G)) + log2(G) + 4, ceil(d / 256) + 12): a product passes the
 *             rounding of q', at most 4 ceil(ld / (16 G)) fmas, 2 joining and log2(G) butterfly additions and the addition of qbias; a
 *             term of qbias the two roundings of mid, its product, at most ceil(d / 256) + 8 additions of the prologue and that last
 *             addition.  Quantisation: as sgpt_score_topk_u8.
 *   select    as sgpt_ivf_search: every item keeps its min(k, SGPT_IVF_CHUNK) best (score descending, then original index ascending), the
 *             items' pairs and the running list go through the select kernel of sgpt_topk_merge, in the same query groups.
 *   result    as sgpt_ivf_search: rows sorted, indices ids[...] + idx_base, running list in/out (it must hold values of this entry);
 *             *n_out = min(k, n_run + N), slots that found no row are (-inf, -1) inside that count.
 *   shapes    any nq <= 65535; speed is claimed for nq <= 64 only, as there.
 * SGPT_ERR_INVALID (nothing launched, outputs untouched): everything sgpt_ivf_search refuses (codes in the place of rows); null start or
 * step; ld % 128; d > ld; ld > SGPT_IVF_MAX_DIM; codes not 16-byte aligned. */
sgpt_status sgpt_u8_gather_quantize_rows(sgpt_ctx* ctx, const void* x, int32_t x_dtype, int64_t n_x, const int64_t* perm, int64_t n, int32_t d,
                                         int32_t ld, const float* start, const float* step, uint8_t* codes, void* stream);
sgpt_status sgpt_ivf_search_u8(sgpt_ctx* ctx, const float* q, const void* centroids16, const uint8_t* codes, const float* start,
                               const float* step, const int64_t* ids, const int64_t* offsets, int32_t nq, int64_t N, int32_t d, int32_t ld,
                               int32_t nlist, int64_t max_list, int32_t nprobe, int32_t k, int64_t idx_base, float* run_val,
                               int64_t* run_idx, int32_t n_run, int32_t* n_out, int64_t* probe_out /* int64[nq, nprobe] or NULL */,
                               void* stream);

/* Diagnostics (ABI v19): of the filtered chunks of the LAST score + top-k pass on this context (sgpt_score_topk, _q8, _u8; _bits: its last
 * query group), how many overflowed their candidate lists and were recomputed by the predicated fallback.  Synchronises `stream`. */
sgpt_status sgpt_score_overflow_count(sgpt_ctx* ctx, int32_t* n_chunks, int32_t* n_overflowed, void* stream);

/* sgpt_score_topk_refined (ABI v7): the reference's fp32 scoring + top-k (`torch.mm(a, b.T)`, util.py:41-43,63; `torch.topk`,
 * exact_search.py:96-108) -- fp32 scores of the returned documents, the fp32 top-k set -- at the speed of the 16-bit scorer.
 *   q         device fp32 [nq, d]; corpus32 device fp32 [N, d]; corpus16 device 16-bit [N, d] = corpus32 rounded (sgpt_f32_to_16
 *             or sgpt_l2_normalize with a 16-bit output); dtype16 SGPT_F16 | SGPT_BF16
 *   stage 1   the filtered 16-bit scorer (sgpt_score_topk on 16-bit copies) takes k' = k + head-room candidates per query;
 *   stage 2   every candidate is re-scored in exact fp32 from corpus32, merged with the running list, top-k (ties: ascending index).
 *   margin    the caller's bound 2 eps on |s16 - s32| for its rows: 2.5e-3 for L2-normalised rows with SGPT_F16 copies (two
 *             roundings of relative 2^-11, Cauchy-Schwarz; subnormal flushes and both fp32 accumulations inside the slack); scale by
 *             max|q| max|d| for un-normalised rows.  When the (k')-th best 16-bit score of a query is not more than `margin` below
 *             its k-th best, outsiders could still reach the fp32 top-k: a device flag is raised and the call's exact-fp32
 *             materialise-and-select pass, every launch predicated on that flag, redoes the chunk -- exact either way, and
 *             asynchronous on `stream` unless fallback_flag_out (host int32*, may be NULL) is given: then the call synchronises and
 *             reports 1 if the exact pass ran, 0 if not, -1 if the call went straight to the exact pass (k' would not fit).
 *   run_val / run_idx / n_run / n_out as sgpt_score_topk (fp32 scores throughout). */
sgpt_status sgpt_score_topk_refined(sgpt_ctx* ctx, const float* q, const float* corpus32, const void* corpus16, int32_t dtype16,
                                    int32_t nq, int64_t N, int32_t d, int32_t k, int64_t idx_base, float margin,
                                    float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, int32_t* fallback_flag_out,
                                    void* stream);

/* k best of m candidate (score, index) pairs per query: the cross-rank / cross-chunk merge
 * (exact_search.py:121-132 heapq.nlargest).  Candidates with idx < 0 are ignored, and so is
 * the candidate whose idx == exclude_idx[q] (the `corpus_id != query_id` rule of :118;
 * exclude_idx may be NULL).
 *   val device fp32[nq,m], idx device int64[nq,m] -> out_val fp32[nq,k], out_idx int64[nq,k]
 *   (sorted descending; tail (-inf,-1)).
 * The order, here and in every list this library returns (sgpt_topk, sgpt_score_topk*, sgpt_exchange_topk, sgpt_fold_gathered_topk):
 * higher score first, equal scores by ascending index, whatever the candidate's position in the row or the row's length.  It is
 * total: -0.0 and +0.0 are equal scores, a positive NaN ranks above +inf and a negative NaN below -inf.  A candidate whose score is
 * -inf counts as an unused slot: it comes back as (-inf, -1), like an ignored candidate, behind every score above -inf -- a list
 * never holds an index behind its first -1.  A (score, idx) pair that the candidates repeat is returned as often as it occurs.
 * k > 2048: the same k pairs, in NO particular order (unused slots anywhere among them). */
sgpt_status sgpt_topk_merge(sgpt_ctx* ctx, const float* val, const int64_t* idx, int32_t nq,
                            int32_t m, int32_t k, const int64_t* exclude_idx,
                            float* out_val, int64_t* out_idx, void* stream);

/* -- a9 / 8e: multi-GPU exchange steps on RCCL (one process per GPU, xGMI) ---------------------------------------------- */
/* One communicator per ctx.  Rank 0 creates the 128-byte id (ncclGetUniqueId), the host carries it to the other ranks by
 * any means (sgpt_amd/dist.py: one torch.distributed broadcast, the only use of torch.distributed on this path), every rank
 * calls sgpt_comm_init (collective, blocking: ncclCommInitRank).  sgpt_ctx_destroy tears the communicator down.
 *
 * sgpt_allgather_rows replaces the reference's two-step util.mismatched_sizes_all_gather
 * (sentence_transformers/util.py:326-347: all-gather the sizes, pad to the maximum, all-gather the rows): rank r contributes
 * counts[r] rows of row_bytes bytes (counts: host int64[world], known to every rank because shards are a pure function of the
 * global length list -- SentenceTransformer.py:159-163, or the token-balanced cut of sgpt_amd/st.py); out device
 * [sum(counts)][row_bytes] receives the blocks in rank order.  Equal counts: ONE ncclAllGather straight into `out`; ragged:
 * padded to the largest block through the exchange workspace and compacted.  Asynchronous on `stream`.
 *
 * sgpt_exchange_topk is the last step of the corpus-sharded search: every rank holds the k best (score, global
 * index) pairs per query of ITS corpus shard (sgpt_score_topk with idx_base = the shard's first global index); the lists are
 * all-gathered (two ncclAllGathers in one group) and the k_out best of the world * k candidates per query are selected by
 * the library's merge kernel on the same stream -- the heapq.nlargest merge of exact_search.py:121-132 including the
 * `corpus_id != query_id` rule (:118) through exclude_idx (device int64[nq] or NULL).  Ties -> lowest index: every rank gets
 * identical results.  val device fp32[nq,k], idx device int64[nq,k] -> out_val fp32[nq,k_out], out_idx int64[nq,k_out].
 *
 * sgpt_fold_gathered_topk is the rank-local half of that step on its own (no communicator needed): gathered_val / gathered_idx
 * device [world][nq][k] in rank order, as an all-gather delivers them -> the same k_out best per query.  For callers that move
 * the lists with their own transport, and for testing the fold of a many-rank world on one GPU. */
#define SGPT_COMM_ID_BYTES 128
sgpt_status sgpt_comm_unique_id(uint8_t* id /* [SGPT_COMM_ID_BYTES], host */);
sgpt_status sgpt_comm_init(sgpt_ctx* ctx, const uint8_t* id, int32_t rank, int32_t world);
sgpt_status sgpt_comm_destroy(sgpt_ctx* ctx);
int32_t sgpt_comm_world(const sgpt_ctx* ctx);     /* 0 = no communicator */
int32_t sgpt_comm_rank(const sgpt_ctx* ctx);
sgpt_status sgpt_allgather_rows(sgpt_ctx* ctx, const void* local, const int64_t* counts, int64_t row_bytes, void* out,
                                void* stream);
/* The same result through the RAGGED branch whatever the counts are (pad to the largest block, gather into the exchange
 * workspace, compact in rank order): lets a world of one -- or equal shards -- exercise the code path unequal shards take. */
sgpt_status sgpt_allgather_rows_padded(sgpt_ctx* ctx, const void* local, const int64_t* counts, int64_t row_bytes, void* out,
                                       void* stream);
sgpt_status sgpt_exchange_topk(sgpt_ctx* ctx, const float* val, const int64_t* idx, int32_t nq, int32_t k, int32_t k_out,
                               const int64_t* exclude_idx, float* out_val, int64_t* out_idx, void* stream);
sgpt_status sgpt_fold_gathered_topk(sgpt_ctx* ctx, const float* gathered_val, const int64_t* gathered_idx, int32_t world,
                                    int32_t nq, int32_t k, int32_t k_out, const int64_t* exclude_idx, float* out_val,
                                    int64_t* out_idx, void* stream);

/* Plain top-k over a materialised score matrix: torch.topk(scores, k, dim=1)
 * (exact_search.py:102-108; util.semantic_search util.py:241).  NaN -> -1 first (:99).  Rows need no alignment (16-byte aligned rows
 * are read with 16-byte loads).  Order, -inf scores and k > 2048 as documented at sgpt_topk_merge: sorted for k <= 2048, columns
 * beyond n and scores of -inf are (-inf, -1). */
sgpt_status sgpt_topk(sgpt_ctx* ctx, const float* scores, int32_t nq, int64_t n, int64_t ld,
                      int32_t k, int64_t idx_base, float* out_val, int64_t* out_idx, void* stream);

/* -- evaluation: retrieval metrics from device-resident ranked lists (ABI v10; csrc/eval.hip) ---------------------------- */
/* Replaces, for an evaluation run, the D2H copy of the result lists, the Dict[qid, Dict[doc_id, float]] built from them and the
 * pytrec_eval pass of beir.EvaluateRetrieval.evaluate (biencoder/beir/beir_dense_retriever.py:442-446), and the Python loops of
 * InformationRetrievalEvaluator.compute_metrics (sentence_transformers/evaluation/InformationRetrievalEvaluator.py:189-271):
 * the per-query, per-cut sums every one of those metrics is made of, taken from the lists sgpt_topk_merge / sgpt_exchange_topk
 * leave on the device.
 *   idx      device int64[nq, K]  corpus positions in rank order (descending score, ties by ascending position -- the order
 *            documented above for run_idx / out_idx); a position < 0 is padding and ENDS the list
 *   val      device fp32[nq, K]   the scores; read only when check_order != 0 (may be NULL otherwise)
 *   qrel_off device int32[nq + 1] CSR offsets of the judgements: query q owns entries [qrel_off[q], qrel_off[q + 1])
 *   qrel_pos device int64[]       judged corpus positions, ascending within a query; a judged document that is not in the corpus
 *            carries a position no list can hold (INT64_MAX): it counts in R and never matches
 *   qrel_rel device int32[]       the grade of each entry of qrel_pos (relevant: grade > 0; the gain of a grade is max(grade, 0))
 *   ideal_rel device int32[]      the same CSR layout: the query's grades sorted descending (the ideal ranking of IDCG)
 *   k_values HOST int32[nk]       the cuts: positive, strictly ascending, k_values[nk - 1] <= K, nk <= SGPT_EVAL_MAX_CUTS
 * Outputs, device, [nq, nk] unless noted, with n = length of the list and i counting ranks from 1:
 *   out_hits  int32  relevant documents among ranks 1 .. min(k, n)
 *   out_first int32  rank of the first relevant document if it is <= k, else 0
 *   out_dcg   fp32   sum_{i <= min(k, n)} max(rel_i, 0) / log2(i + 1)
 *   out_idcg  fp32   the same sum over ideal_rel
 *   out_sp    fp32   sum over the relevant ranks i <= min(k, n) of hits@i / i   (average precision x R)
 *   out_R     int32[nq]  judged documents with grade > 0
 * The integer outputs are exact.  The float sums are taken in one fixed order (64 consecutive ranks by an xor butterfly, the
 * groups in ascending order), so they do not depend on the launch geometry; no float atomics.
 * check_order != 0: the call also verifies val[i] >= val[i + 1] over the entries of every list and, if a row breaks it, returns
 *   SGPT_ERR_INVALID (one device word ORed by the kernel, read back: the call then synchronises `stream`).  Lists that come
 *   from the scorer are sorted by construction; lists packed by a caller may not be.  0: asynchronous like every other call.
 * Exactly equal scores are ties; trec_eval's tie-break by document id is not reproduced.  nq == 0 is a valid, empty call. */
#define SGPT_EVAL_MAX_CUTS 16
sgpt_status sgpt_eval_ranked(sgpt_ctx* ctx, const int64_t* idx, const float* val, int32_t nq, int32_t K,
                             const int32_t* qrel_off, const int64_t* qrel_pos, const int32_t* qrel_rel,
                             const int32_t* ideal_rel, const int32_t* k_values, int32_t nk, int32_t check_order,
                             int32_t* out_hits, int32_t* out_first, float* out_dcg, float* out_idcg, float* out_sp,
                             int32_t* out_R, void* stream);

/* -- evaluation, USEB: grouped re-ranking and pair statistics (ABI v11; csrc/useb_eval.hip) ----------------------------- */
/* sgpt_eval_groups: score, rank and reduce candidate groups.  Replaces, per query, the 21-sentence embedder call, the D2H copy,
 * the host matmul, `rank_by_score` and `ap_score` / `reciprocal_rank` of useb/evaluators/askubuntu.py:139-155, and the per-query
 * scoring plus the pytrec_eval pass of useb/evaluators/scidocs.py:67-90: every unique sentence is embedded once, the task is a CSR
 * of groups over those rows, and one call leaves the per-group sums every metric of the two tasks is made of.
 *   emb       device fp32[n_rows, d]  one row per unique sentence; not read (may be NULL) when scores_in is given
 *   mode      SGPT_COS     x.y / (max(|x|, 1e-8) max(|y|, 1e-8))   (F.cosine_similarity, scidocs.py:80)
 *             SGPT_DOT     x.y                                       (torch.matmul of the embeddings, askubuntu.py:147)
 *             SGPT_NEG_L2  -||x - y||_2                              (scidocs.py:79)
 *   scores_in device fp32[n_cand] or NULL: when given, candidate j's score is scores_in[j] and emb, q_row, cand_row, mode are not
 *             used (re-rankers that score elsewhere -- the cross-encoder's log-probabilities -- share the ranking and the sums)
 *   G, grp_off  number of groups; device int32[G + 1] CSR offsets: group g owns candidates [grp_off[g], grp_off[g + 1])
 *   n_cand    HOST: grp_off[G], the length of the per-candidate arrays
 *   max_group HOST: the size of the largest group (the caller built the CSR).  Above SGPT_EVAL_MAX_GROUP: SGPT_ERR_INVALID,
 *             nothing launched.  The kernels do not rely on it: a group that is larger than SGPT_EVAL_MAX_GROUP all the same, or
 *             whose offsets leave [0, n_cand], is a caller error they answer with out_R[g] = -1 and zeros in the group's other
 *             [G] outputs (its per-candidate outputs are not written; no access out of bounds).
 *   q_row     device int32[G]       embedding row of the group's query
 *   cand_row  device int32[n_cand]  embedding row of each candidate; a row outside [0, n_rows) scores NaN
 *   cand_rel  device int32[n_cand]  grade of each candidate (relevant: grade > 0; gain: max(grade, 0))
 *   R_extra   device int32[G] or NULL: relevant judged documents that are NOT among the candidates; they count in out_R, as in
 *             trec_eval and as sgpt_eval_ranked counts judged documents outside the corpus
 *   ideal_off, ideal_rel  device int32[G + 1] / int32[n_ideal]: CSR of each group's judged grades sorted descending (IDCG); both
 *             NULL when NDCG is not wanted (out_idcg is then 0)
 *   n_ideal   HOST: the length of ideal_rel; a group's range is clipped to [0, n_ideal)
 * Ranking: descending score, equal scores (-0 == +0) to the lower position inside the group -- Python's stable
 * sorted(..., reverse=True) of `rank_by_score`; a caller that lists candidates by descending document id gets trec_eval's
 * tie-break.  NaN scores rank last (after -inf), among themselves by position.
 * Outputs (device; per candidate in the group's CSR range, or [G]); i counts ranks from 1, n = size of the group:
 *   out_scores fp32[n_cand] or NULL   the score of each candidate (input order)
 *   out_order  int32[n_cand] or NULL  out_order[grp_off[g] + i - 1] = group-local index of the candidate at rank i
 *   out_hits1, out_hits5 int32[G]     relevant candidates among the first min(1, n) / min(5, n) ranks
 *   out_first  int32[G]               rank of the first relevant candidate, 0 if none
 *   out_R      int32[G]               relevant candidates + R_extra
 *   out_sp     fp32[G]                sum over the relevant ranks i of hits@i / i   (full list)
 *   out_dcg, out_idcg fp32[G]         sum_i max(rel_i, 0) / log2(i + 1) over the ranked list / over ideal_rel (full lists)
 * Integer outputs are exact.  A score depends on the values of the two rows, d and the mode only (one wavefront, one fixed
 * summation order), so the same pair scored twice gives the same bits whatever its position, group or grid; the float sums are
 * taken as in sgpt_eval_ranked (64 consecutive ranks by an xor butterfly, the chunks in ascending order).  No float atomics,
 * no allocation, asynchronous on `stream`.  G == 0 is a valid, empty call; a group may be empty (all outputs 0, R = R_extra).
 * SGPT_ERR_INVALID: max_group > SGPT_EVAL_MAX_GROUP, negative G / n_cand / max_group / n_ideal, unknown mode, d < 1, ideal_off without
 * ideal_rel or the reverse, a required pointer NULL. */
#define SGPT_EVAL_MAX_GROUP 1024
sgpt_status sgpt_eval_groups(sgpt_ctx* ctx, const float* emb, int32_t n_rows, int32_t d, int32_t mode, const float* scores_in,
                             int32_t G, const int32_t* grp_off, int32_t n_cand, int32_t max_group, const int32_t* q_row,
                             const int32_t* cand_row, const int32_t* cand_rel, const int32_t* R_extra,
                             const int32_t* ideal_off, const int32_t* ideal_rel, int32_t n_ideal, float* out_scores,
                             int32_t* out_order, int32_t* out_hits1, int32_t* out_hits5, int32_t* out_first, int32_t* out_R, float* out_sp,
                             float* out_dcg, float* out_idcg, void* stream);

/* sgpt_eval_pairs: global ranking statistics of n scored pairs.  Replaces what follows the cosine in
 * useb/evaluators/twitterpara.py:110-117 (the cosine itself is sgpt_pairwise_scores): the D2H copy of the scores,
 * sklearn.metrics.average_precision_score and the ranking half of scipy.stats.spearmanr.
 *   score  device fp32[n]
 *   label  device int32[n]   > 0 positive, 0 negative, < 0 left out of the average precision but still ranked (`is_para is None`)
 *   check_nan  != 0: a NaN score makes the call return SGPT_ERR_INVALID (one device word ORed by the kernel, read back: the call
 *          then synchronises `stream`, as check_order of sgpt_eval_ranked does).  0: asynchronous; NaN then sorts above every
 *          number and the statistics mean nothing.
 * Outputs (device):
 *   out_rank2  int32[n]  twice the 1-based ascending rank of score[i], ties averaged: 2 x scipy.stats.rankdata (an exact integer;
 *              -0 == +0).  Spearman is host arithmetic: the float64 Pearson correlation of out_rank2 with the doubled ranks of
 *              the gold scores (sums of squared ranks reach n^3 / 3: not a device fp32 sum).
 *   out_n_pos, out_n_used  int64 scalars: rows with label > 0, rows with label >= 0
 *   out_ap_num fp64 scalar: with the used rows sorted by descending score, tie groups j = 1 .. ending at count N_j and holding
 *              TP_j positives cumulatively, sum_j (TP_j - TP_{j-1}) TP_j / N_j.  average_precision_score = out_ap_num / out_n_pos
 *              (equal scores are one threshold, as in scikit-learn); undefined for n_pos == 0, where out_ap_num is 0.
 *              Accumulated in fp64: 256 terms by an LDS tree per workgroup, the partials by one workgroup in a fixed order.
 * A full device sort of 64-bit (score, index) keys (bitonic; the keys are unique), so nothing depends on launch geometry; no
 * float atomics; workspace from the ctx (grow-only, 2 x 8 bytes per key of the next power of two >= max(n, 2048)).
 * n == 0 is a valid call (the three scalars become 0).  SGPT_ERR_INVALID: n < 0 or n > SGPT_EVAL_MAX_PAIRS, a NULL pointer,
 * a NaN score under check_nan. */
#define SGPT_EVAL_MAX_PAIRS (1 << 24)
sgpt_status sgpt_eval_pairs(sgpt_ctx* ctx, const float* score, const int32_t* label, int32_t n, int32_t check_nan,
                            int32_t* out_rank2, int64_t* out_n_pos, int64_t* out_n_used, double* out_ap_num, void* stream);

/* -- the projection GEMM with its fused epilogues, as a stand-alone op ----------------------------------------------- */
/* out = epilogue(A . W^T): the nn.Linear calls of the transformer blocks (HF:gpt_neo:141-143,155,304-309) with the
 * element-wise tail fused -- exactly the kernels sgpt_encode launches, exposed for kernel-level parity tests and for
 * callers that assemble their own blocks.  A device [M,K], W device [N,K] (both row-major, `dtype` SGPT_F32 / SGPT_BF16 /
 * SGPT_F16), fp32 accumulation.
 *   epi 0: out[M,N] = acc (+ bias if given)              out_dtype = dtype (16-bit) or SGPT_F32
 *   epi 1: out[M,N] = gelu_new(acc + bias)               out_dtype = dtype           (HF NewGELUActivation)
 *   epi 2: out[M,N] = resid + acc + bias                 fp32; out may alias resid (the residual stream, in place)
 *   epi 4: out[N,M] = acc (+ bias[n])                    16-bit transposed store (V^T for the attention P.V operand), M % 128 == 0
 *   epi 9: out[M,N] = gelu(acc + bias), 0.5 u (1 + erf(u / sqrt 2))   out_dtype = dtype   (ABI v13; HF GELUActivation, the BERT family)
 * bias device fp32[N]; resid device fp32[M,N].  M % 256 == 0, N % 256 == 0, K % 64 == 0 with at least half a wave of
 * 256x256 tiles take the LDS-DMA throughput kernel, everything else the 128x128 / 64x64 register-staged one; both
 * feed every output element the same MFMA sequence, so the result does not depend on which one ran.
 * Accepted shapes: any M >= 1 (epi 4: M % 128 == 0); K % 8 == 0 for 16-bit operands, K % 4 == 0 for fp32 (rows of A and W
 * are read in 16-byte chunks; a K that is no multiple of the kernel's k-step is zero-filled inside the kernel); N % 4 == 0
 * for epi 1, 2, 4 and 9, any N >= 1 for epi 0 (the LM head, N = 50257) -- out is then a dense [M,N] array whose rows are
 * not 8- / 16-byte aligned, which the vector stores of the epilogue allow.  fp32 operands give fp32 output and have no
 * epi 4.  Anything else is SGPT_ERR_INVALID and leaves out untouched (tests/test_gpu_linear_edges.py). */
sgpt_status sgpt_linear(sgpt_ctx* ctx, int32_t dtype, int32_t epi, int32_t out_dtype, const void* A, const void* W,
                        const float* bias, const float* resid, void* out, int32_t M, int32_t N, int32_t K, void* stream);

/* The query- / mid-sized projection kernels of sgpt_encode, stand-alone (ABI v8; csrc/qgemm.hip: layouts of at most 4096 token rows --
 * `SentenceTransformer.encode("one query")`, SentenceTransformer.py:143-146; USEB's 21-sentence batches,
 * useb/useb/useb/evaluators/askubuntu.py:144-148), for kernel-level parity tests.  16-bit operands (dtype SGPT_BF16 | SGPT_F16),
 * fp32 accumulation, W device [N, K] row-major.
 *   A != NULL: A device [M, K] in `dtype`.
 *   x != NULL: the LayerNorm prologue -- A = nn.LayerNorm(K, eps)(x) rounded to `dtype` (x device fp32 [M, K]: the residual stream;
 *              HF:gpt_neo:317-319,385), computed by the projection itself; epi 7 and 1 only.
 *   epi 0: out[M,N] = acc (+ bias if given)         epi 1: out[M,N] = gelu_new(acc + bias)        (out in `dtype`)
 *   epi 2: out[M,N] = resid + acc + bias, fp32 (out may alias resid)
 *   epi 7: the fused Q | K | V projection: columns [0, n_split) -> out[M, n_split] row-major, columns [n_split, N) -> out_vt[N - n_split, M]
 *          (V^T, the attention kernel's P.V operand).
 * Same bits as sgpt_linear (+ the LayerNorm kernel) on the same operands.  SGPT_ERR_INVALID if the shape is not served. */
sgpt_status sgpt_linear_query(sgpt_ctx* ctx, int32_t dtype, int32_t epi, const void* A, const float* x, const float* ln_gamma,
                              const float* ln_beta, float ln_eps, const void* W, const float* bias, const float* resid, void* out,
                              void* out_vt, int32_t n_split, int32_t M, int32_t N, int32_t K, void* stream);

/* The bulk fused Q | K | V projection of sgpt_encode, stand-alone (ABI v14; kernel-level tests: tests/test_gpu_linear_256.py): ONE launch
 * of the persistent 256x256 kernel over all N = 3 d columns -- the q_proj, k_proj and v_proj nn.Linear calls of GPTNeoSelfAttention.forward,
 * HF:gpt_neo:141-143 -- the column tiles below n_split stored row-major, the V column tiles computed with swapped operand roles and stored
 * transposed; the launch the 16-bit block of csrc/encode.hip makes for a bulk batch of a model without a QKV bias.
 *   A device [M, K], W device [N, K], row-major, `dtype` SGPT_BF16 | SGPT_F16 (lda == ldw == K), no bias, fp32 accumulation
 *   out     device [M, n_split]      (q | k)           out_vt  device [N - n_split, M]   (V^T), both in `dtype`
 * Served: M, N and n_split multiples of 256, 0 < n_split < N, K % 64 == 0, K >= 128, and more than 128 q | k tiles
 * ((M / 256) (n_split / 256) > 128) -- anything else is SGPT_ERR_INVALID and nothing is launched.
 * Same bits as sgpt_linear epi 0 on W[0 : n_split] and epi 4 on W[n_split : N]. */
sgpt_status sgpt_linear_qkv(sgpt_ctx* ctx, int32_t dtype, const void* A, const void* W, void* out, void* out_vt, int32_t n_split,
                            int32_t M, int32_t N, int32_t K, void* stream);

/* The attention kernels of sgpt_encode, stand-alone (ABI v9; kernel-level tests): causal (+ sliding-window) softmax attention
 * over packed variable-length sequences -- GPTNeoSelfAttention._attn (HF:gpt_neo:105-130) with BLOOM's ALiBi bias
 * (HF:bloom:45-89).  Sequence b owns token rows [seq_off[b], seq_off[b+1]) (seq_off device int32[B+1], even entries, every
 * difference <= max_alloc_len, seq_off[B] <= T); key j (counted from the sequence start) is visible to query i iff j <= i and,
 * window > 0, j > i - window.  score = scale * q.k + alibi[h] * j (alibi device fp32[H] or NULL), exact softmax, P.V.
 *   dtype SGPT_BF16 | SGPT_F16: q, k device [T][ldq] (head h at columns h * dh ..), v = V^T device [H * dh][ldvt] (ldvt >= T),
 *     out device [T][ldo] in `dtype`: the 16-bit MFMA kernel.  dh 64 | 128 | 256.
 *   dtype SGPT_F32: q, k, v device fp32 [T][ldq] (ldvt unused), out fp32 [T][ldo]: the exact-fp32 kernel.
 *   out_fp8 = 1 (bf16 only): out holds e4m3fn codes of ctx / out_scale ([T][ldo] bytes); a saturated code (or NaN) ORs 4
 *     (bit 2, as sgpt_model_range_check) into *range_flag (device int32, may be NULL).
 *   ctx_lo_delta != 0 (16-bit; "MODE 1"): the context also leaves as lo = round16(v - hi) at out + ctx_lo_delta and, when
 *     ctx_hi2_delta != 0, a second copy of hi at out + ctx_hi2_delta (element offsets).
 *   x3 = 1 (16-bit, dh 64 | 128; "MODE 2"): q | k and V^T enter as hi + lo pairs, the lo halves qk_lo_delta / v_lo_delta
 *     elements behind the hi halves (same leading dimensions).
 * Over-read contract: the key tiles read up to 64 rows past the last sequence's allocation -- k rows (and their lo halves)
 *   up to T + 63, V^T elements r * ldvt + c for c < T + 64 -- as masked keys whose p = 0 multiplies them: they must be readable
 *   and finite (0 * NaN = NaN).  Query fragments load q rows up to T + 255 (never used past a sequence): readable.  Only the
 *   out rows of the allocations [seq_off[b], seq_off[b+1]) are written.
 * SGPT_ERR_INVALID (nothing launched) for: head_dim other than 64 | 128 | 256, T % 32, max_alloc_len odd or above 2048,
 *   out_fp8 with f16 / fp32 operands or with a split-precision mode, x3 at head_dim 256, split modes with fp32 operands,
 *   misaligned pointers / leading dimensions.
 * This entry keeps the bound of ABI <= v22, max_alloc_len <= 2048, and its message; sgpt_attention_ex (causal = 1) and
 *   sgpt_attention_gqa are the same kernels up to SGPT_MAX_SEQ_LEN rows per sequence.  fp32 above 2048 rows: a second kernel takes
 *   the keys in chunks of 2048 with an online softmax across chunks; a row that sees at most 2048 keys keeps the bits of the
 *   one-chunk kernel. */
sgpt_status sgpt_attention(sgpt_ctx* ctx, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                           void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t dh,
                           int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                           float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                           int64_t ctx_lo_delta, int64_t ctx_hi2_delta, void* stream);

/* sgpt_attention_ex (ABI v13): sgpt_attention with the bidirectional mode of SGPT_ARCH_BERT (HF:bert/modeling_bert.py BertSelfAttention).
 *   causal = 1, seq_len = NULL: sgpt_attention exactly (the same kernels, the same bits).
 *   causal = 0: every query row of sequence b sees keys j in [0, seq_len[b]) of that sequence -- seq_len device int32[B], clamped
 *     into [0, seq_off[b+1] - seq_off[b]]; NULL = the whole allocation -- and nothing of its neighbours on the packed axis.  A
 *     sequence of no keys gives zero rows.  window = 0 and alibi = NULL; out_fp8, x3 and the split context are refused
 *     (SGPT_ERR_INVALID), as is 16-bit head_dim 256.  Over-read contract as sgpt_attention.
 *   max_alloc_len even, in [2, SGPT_MAX_SEQ_LEN] (ABI v23; sgpt_attention_gqa too). */
sgpt_status sgpt_attention_ex(sgpt_ctx* ctx, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                              void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t dh,
                              int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                              float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                              int64_t ctx_lo_delta, int64_t ctx_hi2_delta, int32_t causal, const int32_t* seq_len, void* stream);

/* sgpt_attention_gqa (ABI v15): causal sgpt_attention with grouped K / V (SGPT_ARCH_LLAMA): k holds n_kv_heads heads ([T, >= n_kv_heads *
 *   head_dim] rows of leading dimension ldq), v = V^T [n_kv_heads * head_dim, ldvt] (16-bit) or [T, ...] rows (fp32); query head h
 *   reads key / value head h / (H / n_kv_heads).  Only the addresses differ: the result is bit for bit that of sgpt_attention on
 *   explicitly replicated K and V^T, and n_kv_heads == H is sgpt_attention itself.  window as sgpt_attention.  H % n_kv_heads != 0,
 *   alibi, out_fp8, x3 and the split context are refused (SGPT_ERR_INVALID), as is 16-bit head_dim 256. */
sgpt_status sgpt_attention_gqa(sgpt_ctx* ctx, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                               void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t n_kv_heads,
                               int32_t dh, int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                               float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                               int64_t ctx_lo_delta, int64_t ctx_hi2_delta, void* stream);

/* sgpt_attention_gqa_ex (ABI v24): sgpt_attention_gqa with the trailing causal / seq_len of sgpt_attention_ex, same meaning: causal = 1
 *   and seq_len = NULL is sgpt_attention_gqa exactly; causal = 0 is the bidirectional attention of an SGPT_ARCH_LLAMA model after
 *   sgpt_model_set_attention(0) -- bit for bit sgpt_attention_ex(causal = 0) on explicitly replicated K / V^T, at any length up to
 *   SGPT_MAX_SEQ_LEN (16-bit: the same 64-key tile loop, run to the sequence end; fp32 above 2048 rows: the chunked kernel).  causal = 0
 *   refuses window, alibi, out_fp8, x3, the split context and 16-bit head_dim 256.  max_alloc_len even, in [2, SGPT_MAX_SEQ_LEN]. */
sgpt_status sgpt_attention_gqa_ex(sgpt_ctx* ctx, int32_t dtype, const void* q, const void* k, const void* v, int64_t ldq, int64_t ldvt,
                                  void* out, int64_t ldo, const int32_t* seq_off, int32_t B, int32_t T, int32_t H, int32_t n_kv_heads,
                                  int32_t dh, int32_t window, float scale, const float* alibi, int32_t max_alloc_len, int32_t out_fp8,
                                  float out_scale, int32_t* range_flag, int32_t x3, int64_t qk_lo_delta, int64_t v_lo_delta,
                                  int64_t ctx_lo_delta, int64_t ctx_hi2_delta, int32_t causal, const int32_t* seq_len, void* stream);

/* The encoder's row kernels, stand-alone (ABI v12; kernel-level tests: tests/test_gpu_rowops.py compares each with a float64
 * restatement of the same operation).  These are the launches sgpt_encode / sgpt_lm_logprobs make between their GEMMs, on
 * caller-owned device buffers.  Every entry returns SGPT_ERR_INVALID, with nothing launched, for a null pointer, a row width
 * the kernels do not serve or an enum outside its range.  Indices the kernels read from device memory (ids, pos, targets) are
 * clamped into their tables: a bad index gives the result of the nearest valid one, never an out-of-bounds read.
 *
 * sgpt_embed: out fp32[T, d] = wte[ids[t]] + wpe[pos[t]] -- `inputs_embeds + position_embeds`, HF:gpt_neo/modeling_gpt_neo.py:444,
 *   462-463; wpe NULL = the token rows alone (GPT-J, HF:gptj/modeling_gptj.py:484; BLOOM).  d % 4 == 0; ids clamped into
 *   [0, vocab), pos into [0, max_pos).
 * sgpt_layernorm: nn.LayerNorm(eps) over rows of x fp32[T, d] (HF:gpt_neo:317-319,385,492), d % 4 == 0, d <= 4096.
 *   out_dtype SGPT_F32 | SGPT_BF16 | SGPT_F16: out [T, d], the normalised row rounded once (RNE) to the format.  out_mul: a
 *   positive power of two that multiplies an SGPT_F16 output before the rounding (the range shift of sgpt_model_desc
 *   .compute_dtype SGPT_F16); 1 for the other formats.  split = 1 (16-bit only): out [T, 3 d] = [hi | lo | hi] with
 *   hi = round16(v), lo = round16(v - hi), v = out_mul * LayerNorm(x) -- the operand of the split-precision projections
 *   (sgpt_model_desc.qk_split).  out may alias x for SGPT_F32 (BLOOM's embedding LayerNorm, HF:bloom/modeling_bloom.py:499).
 * sgpt_layernorm_writeback (ABI v13): the LayerNorm of a post-LN block (SGPT_ARCH_BERT): x fp32[T, d] <- nn.LayerNorm(eps)(x) IN PLACE
 *   and, from the same registers, out16 [T, d] = the normalised row rounded once (RNE) to out_dtype SGPT_BF16 | SGPT_F16 -- the
 *   next projection's operand.  An f16 value of magnitude >= 32768 raises bit 0 of sgpt_range_check.
 * sgpt_rmsnorm (ABI v15; SGPT_ARCH_LLAMA): out [T, d] = x * rsqrt(mean(x^2) + eps) * gamma in fp32, rounded once to out_dtype (SGPT_F32:
 *   not at all; out may alias x).  An f16 value of magnitude >= 32768 raises bit 0 of sgpt_range_check.
 * sgpt_swiglu (ABI v15): out [T, ffn] = silu(gu[:, :ffn]) * gu[:, ffn:] for gu [T, 2 ffn] of `dtype` (the fc1 output of the Llama MLP:
 *   gate columns, then up columns), fp32 arithmetic, one rounding to `dtype`; ffn % 8 (16-bit) / 4 (fp32).  f16 range flag as above.
 * sgpt_rope_half (ABI v15): HF rotate_half rotary embedding in place on buf [T, ld]: for the H query heads at column 0 and the H_kv key
 *   heads at column k_off, i < head_dim / 2: (x[i], x[i + head_dim/2]) <- (x[i] c - x[i + head_dim/2] s, x[i + head_dim/2] c + x[i] s)
 *   with s, c = sin_t / cos_t [max_pos, head_dim/2] at row pos[t] (clamped into the table, as sgpt_rope).  head_dim % 8.
 * sgpt_qknorm_rope_half (ABI v16): the per-head q / k RMSNorm of HF Qwen3Attention.forward (HF:qwen3/modeling_qwen3.py: `q_norm(q_proj(x)
 *   .view(.., head_dim))`, `k_norm(..)`, then apply_rotary_pos_emb) fused with sgpt_rope_half, in place on buf [T, ld]: every one of
 *   the H query heads at column 0 and the H_kv key heads at column k_off becomes n = x * rsqrt(mean_over_head_dim(x^2) + eps) * g in
 *   fp32 (g = q_gamma for query heads, k_gamma for key heads, fp32 [head_dim], 16-byte aligned), then sgpt_rope_half's rotation of n,
 *   rounded once to dtype.  head_dim 64 | 128; otherwise sgpt_rope_half's rules.  An f16 value of magnitude >= 32768 raises bit 0 of
 *   sgpt_range_check.
 * sgpt_lnf_pool_ex (ABI v15): sgpt_lnf_pool with a trailing norm_kind: 0 = LayerNorm (sgpt_lnf_pool exactly), 1 = RMSNorm(gamma)
 *   (beta is not read).
 * sgpt_lnf_pool_range (ABI v24): sgpt_lnf_pool_ex with pool_lo device int32[B] (NULL = zeros = sgpt_lnf_pool_ex exactly): the pooled
 *   rows of sequence i are t in [min(max(pool_lo[i], 0), seq_len[i]), seq_len[i]) -- see sgpt_encode_pool_from.  A non-NULL pool_lo
 *   with SGPT_POOL_LEARNTMEAN is refused.
 * sgpt_lnf_pool: the final LayerNorm fused with the pooling of a packed batch (layout of sgpt_encode: sequence i holds rows
 *   [seq_off[i], seq_off[i] + seq_len[i]) of x fp32[T_pad, d]; rows outside are never read).  apply_ln: ln_f (HF:gpt_neo:492)
 *   on every row first.  mode SGPT_POOL_*: weightedmean sum_t (P + t + 1) h_t / max(sum_t (P + t + 1), 1e-9) with P =
 *   pad_left[i] (NULL = 0; weights follow the PADDED index, Pooling.py:99-125, beir_dense_retriever.py:258-270), mean
 *   (Pooling.py:117-125), lasttoken (row seq_len - 1, beir_dense_retriever.py:271-282), learntmean w_t = pos_weights[min(P + t,
 *   n_weights - 1)] (WeightedMeanPooling.py:21-39).  normalize: x / max(||x||, 1e-12) (SentenceTransformer.py:248-249).
 *   out fp32[B, d]; a sequence of length 0 gives a zero row.  nonfinite_flag (or NULL): device word, bit 0 is OR-ed in when a
 *   pooled row holds NaN / inf.  pad_left entries are >= 0 (the caller's contract).
 * sgpt_rope: GPT-J rotary embedding in place (HF:gptj/modeling_gptj.py:57-67,190-210): for every row t < T, head h < H and pair
 *   i < rotary_dim / 2, (x[2i], x[2i+1]) <- (x[2i] c - x[2i+1] s, x[2i+1] c + x[2i] s) with s, c = sin / cos[pos[t]][i] (tables fp32
 *   [max_pos, rotary_dim / 2], create_sinusoidal_positions :47-50), on the columns h * head_dim + 2i of q (column 0) and k (column
 *   k_off) of buf [T, ld] (dtype SGPT_F32 | SGPT_BF16 | SGPT_F16; 16-bit results rounded once).  Columns >= rotary_dim of a head
 *   and everything outside the q / k blocks are not touched.  rotary_dim even, <= head_dim; head_dim, ld, k_off even;
 *   k_off >= H * head_dim; ld >= k_off + H * head_dim.  pos clamped into [0, max_pos).
 * sgpt_logprob_rows: out_logprob[r] = log_softmax(logits[r, :V])[targets[r]], out_greedy[r] (or NULL) = argmax, first maximum
 *   (F.log_softmax + torch.gather + argmax, crossencoder/beir/sgptce.py:233,243,255); logits fp32 [n, ld], ld >= V, columns
 *   [V, ld) are never read.  targets clamped into [0, V). */
sgpt_status sgpt_embed(sgpt_ctx* ctx, const int32_t* ids, const int32_t* pos, const float* wte, const float* wpe, int32_t T,
                       int32_t d, int32_t vocab, int32_t max_pos, float* out, void* stream);
sgpt_status sgpt_layernorm(sgpt_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t T, int32_t d, float eps,
                           void* out, int32_t out_dtype, float out_mul, int32_t split, void* stream);
sgpt_status sgpt_layernorm_writeback(sgpt_ctx* ctx, float* x, const float* gamma, const float* beta, int32_t T, int32_t d, float eps,
                                     void* out16, int32_t out_dtype, void* stream);
sgpt_status sgpt_rmsnorm(sgpt_ctx* ctx, const float* x, const float* gamma, int32_t T, int32_t d, float eps, void* out, int32_t out_dtype,
                         void* stream);
sgpt_status sgpt_swiglu(sgpt_ctx* ctx, const void* gu, int32_t dtype, int32_t T, int32_t ffn, void* out, void* stream);
sgpt_status sgpt_rope_half(sgpt_ctx* ctx, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos, const float* sin_t,
                           const float* cos_t, int32_t T, int32_t H, int32_t H_kv, int32_t head_dim, int32_t max_pos, void* stream);
sgpt_status sgpt_qknorm_rope_half(sgpt_ctx* ctx, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos,
                                  const float* sin_t, const float* cos_t, int32_t T, int32_t H, int32_t H_kv, int32_t head_dim,
                                  int32_t max_pos, const float* q_gamma, const float* k_gamma, float eps, void* stream);
sgpt_status sgpt_lnf_pool_ex(sgpt_ctx* ctx, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                             const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                             int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                             int32_t* nonfinite_flag, int32_t norm_kind, void* stream);
sgpt_status sgpt_lnf_pool_range(sgpt_ctx* ctx, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                                const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                                int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                                int32_t* nonfinite_flag, int32_t norm_kind, const int32_t* pool_lo, void* stream);
sgpt_status sgpt_lnf_pool(sgpt_ctx* ctx, const float* x, const float* gamma, const float* beta, const int32_t* seq_off,
                          const int32_t* seq_len, const int32_t* pad_left, int32_t B, int32_t d, float eps, int32_t apply_ln,
                          int32_t mode, int32_t normalize, const float* pos_weights, int32_t n_weights, float* out,
                          int32_t* nonfinite_flag, void* stream);
sgpt_status sgpt_rope(sgpt_ctx* ctx, void* buf, int32_t dtype, int64_t ld, int64_t k_off, const int32_t* pos, const float* sin,
                      const float* cos, int32_t T, int32_t H, int32_t head_dim, int32_t rotary_dim, int32_t max_pos, void* stream);
sgpt_status sgpt_logprob_rows(sgpt_ctx* ctx, const float* logits, int64_t ld, int32_t V, const int32_t* targets, int32_t n,
                              float* out_logprob, int32_t* out_greedy, void* stream);

/* The fp8-MFMA building blocks of SGPT_FP8M, stand-alone (kernel-level tests, custom blocks).
 * sgpt_layernorm_fp8: nn.LayerNorm(x)[T,d] -> e4m3fn codes + one power-of-two scale per row (true value = code * scale).
 * sgpt_linear_fp8:    acc = (A8 . W8^T)[m][n] * a_scale[m] * a_scalar * w_scale[n]   (A8 [M,K], W8 [N,K] e4m3fn codes, fp32
 *                     accumulate; a_scale NULL = 1; M, N, K multiples of 256)
 *     epi 0: out 16-bit[M,N] = acc (+ bias if given)          (out_dtype SGPT_BF16 | SGPT_F16)
 *     epi 1: out u8[M,N] = e4m3( gelu_new(acc + bias) / out_scale ), saturating at +-448
 *     epi 2: out fp32[M,N] = resid + acc + bias (out may alias resid)
 *     epi 4: out 16-bit[N,M] = acc (+ bias[n])                (transposed store: V^T) */
sgpt_status sgpt_layernorm_fp8(sgpt_ctx* ctx, const float* x, const float* gamma, const float* beta, int32_t T, int32_t d,
                               float eps, uint8_t* codes, float* row_scale, void* stream);
sgpt_status sgpt_linear_fp8(sgpt_ctx* ctx, int32_t epi, int32_t out_dtype, const uint8_t* A, const float* a_scale,
                            float a_scalar, const uint8_t* W, const float* w_scale, const float* bias, const float* resid,
                            void* out, float out_scale, int32_t M, int32_t N, int32_t K, void* stream);
/* The two quantising row kernels of the fp8 projections of SGPT_ARCH_LLAMA (ABI v25; sgpt_model_set_projections), stand-alone.
 * sgpt_rmsnorm_fp8: sgpt_rmsnorm's fp32 row (x * rsqrt(mean(x^2) + eps) * gamma) -> e4m3fn codes [T, d] + one power-of-two scale per
 *   row, exactly as sgpt_layernorm_fp8 quantises: scale = the smallest 2^k with max|row| / 2^k <= 448 (1 for a zero row), codes =
 *   RNE e4m3fn(value / scale), true value = code * scale.  d % 4 == 0, d <= 4096; x / gamma 16-byte aligned.
 * sgpt_swiglu_fp8:  gu [T, 2 ffn] of dtype SGPT_BF16 | SGPT_F16 (gate columns, then up columns) -> codes [T, ffn] + row_scale [T] of
 *   h = silu(gate) * up, computed in fp32 with sgpt_swiglu's expression and NOT rounded to 16 bits in between; one scale per row by the
 *   same rule.  ffn % 16 == 0; gu and codes 16-byte aligned, codes a buffer of its own.  A row of zeros: scale 1, zero codes. */
sgpt_status sgpt_rmsnorm_fp8(sgpt_ctx* ctx, const float* x, const float* gamma, int32_t T, int32_t d, float eps, uint8_t* codes,
                             float* row_scale, void* stream);
sgpt_status sgpt_swiglu_fp8(sgpt_ctx* ctx, const void* gu, int32_t dtype, int32_t T, int32_t ffn, uint8_t* codes, float* row_scale,
                            void* stream);

/* -- measurement ----------------------------------------------------------------------- */
/* bench.py's live roofline: when enabled, every GEMM launched by sgpt_encode /
 * sgpt_scores / sgpt_score_topk is bracketed by hipEvents on the launch stream;
 * sgpt_prof_read synchronises and returns launches, summed milliseconds and summed
 * algorithmic FLOPs (2*M*N*K of the un-padded problem) since the last reset. */
sgpt_status sgpt_prof_enable(sgpt_ctx* ctx, int32_t on);
sgpt_status sgpt_prof_read(sgpt_ctx* ctx, int64_t* launches, double* ms, double* flops, int32_t reset);

/* Per-ctx run-time policies (the library holds no process-global mutable state and reads no environment variable).
 * sgpt_ctx_set_low_latency: on = 1 lets GEMM launches that have fewer 64x64 tiles than workgroup slots (query-sized batches)
 *   split each tile's k range over two groups of waves that run concurrently and add their fp32 accumulators in a fixed
 *   order (launches with >= 6 k-steps of 128 elements per group).  It was worth 16 % on a 16-query SGPT-125M encode before
 *   the query-sized launches got 128-element k-steps (round 3), ~1 % since (0.82 -> 0.81 ms).  Deterministic, but the sum is no longer the k-ascending
 *   one every other kernel produces, so with the mode on an embedding depends (at 16-bit operand-rounding level, <= 5e-4 on
 *   normalised bf16 embeddings) on whether its batch was small enough to take this path.  Off (default), every batch size
 *   produces identical bits.  Returns the previous setting.
 * sgpt_ctx_set_tile_policy: 0 (default) = problems with less than half a wave of 256x256 tiles take the 128x128 / 64x64
 *   register-staged kernel; 1 = keep the 256x256 LDS-DMA kernel wherever the shape allows (kernel-level tests of
 *   single-tile shapes; identical bits either way); 2 = layouts small enough for the query- / mid-sized kernels (csrc/qgemm.hip)
 *   keep the small-tile register-staged kernels of the bulk path (same-box A/Bs, tests; identical bits).  Returns the previous policy. */
 /* sgpt_ctx_set_gemm_cu_cap: n > 0 = the persistent 256x256 projection kernel launches at most n workgroups (rounded down to
 *   a multiple of 8; 0 = one per CU, the default) -- for two contexts that run their calls half a block out of phase on two
 *   streams, so that one pipeline's LayerNorm / attention / embed kernels find free CUs while the other is in its k-loops
 *   (scripts/dual_stream_probe.py).  The fp8 projection kernel (sgpt_linear_fp8, SGPT_FP8M blocks) honours it
 *   in the same way.  Results do not depend on it.  Returns the previous value. */
 /* sgpt_ctx_set_query_tile (kernel tests): k > 0 = sgpt_linear_query launches the k-th candidate tile of csrc/qgemm.hip instead of
 *   the one its cost rule picks from the CU count -- plain kernels k = 1 .. 7 = 32x16 (256-element stages), 32x32, 32x64, 64x32,
 *   64x64, 128x64, 128x128; with the LayerNorm prologue k = 1 .. 3 = 32x32, 32x64, 64x64.  A tile that does not serve the shape
 *   (N or n_split no multiple of its width, K / stage length no multiple of its ring depth, M <= 32 on a taller tile, k > 3 with
 *   the prologue, LDS) is the entry's "not served" SGPT_ERR_INVALID with nothing launched.  0 (default) = the launcher chooses.
 *   Read by sgpt_linear_query alone: sgpt_encode's launches do not see it.  Identical bits whichever tile runs.  Returns the
 *   previous value; k outside 0 .. 7 changes nothing and returns -1. */
/* sgpt_ctx_set_encode_chains (ABI v22): a bulk sgpt_encode_host_layout call as two chains of whole sequences, A = token rows [0, r)
 *   on the caller's stream and B = [r, T_pad) on a stream the context owns, so that one chain's LayerNorm / attention / embedding
 *   launches and the ramps of its projection launches fall into the other's k-loops.  Chain B starts half a block behind chain A.
 *   Fork and join are events on the caller's stream: work issued on it after the call is ordered behind both chains, the host
 *   never waits.  Weights and workspace are shared (the chains own disjoint row ranges), every kernel computes a row or a sequence
 *   independently of the rest of its launch: identical bits.
 *   n: 0 = the library's default (two chains: +2.1 % on the 1024 x 128-token calls of bench.py) | 1 = one chain |
 *   2 = two chains; two chains run wherever ALL of these hold: a GPT-Neo / GPT-J / BLOOM model with bf16 or f16 operands (no fp8 mode, no split-precision plan, no
 *   calibration or precision probe riding on the call); pooled embeddings only (no hidden_out); T_pad >= min_rows (0 = 131072, the
 *   measured call) and a multiple of 256; r = the sequence start nearest T_pad / 2 that is a multiple of 256 rows and lies in
 *   [T_pad / 3, 2 T_pad / 3] exists; both halves take the 256x256 kernel on all projections; the caller's stream is not
 *   capturing (a captured graph never gets parallel branches: the call is recorded as one chain).
 *   With sgpt_prof_enable on, event pairs are recorded on the stream of their launch: the summed milliseconds of two overlapping
 *   chains may exceed wall time.  Returns the previous n (-1 and no change: bad arguments).
 * sgpt_ctx_encode_chain_calls: how many calls on this context ran as two chains so far. */
int32_t sgpt_ctx_set_encode_chains(sgpt_ctx* ctx, int32_t n, int32_t min_rows);
int64_t sgpt_ctx_encode_chain_calls(const sgpt_ctx* ctx);
int32_t sgpt_ctx_set_gemm_cu_cap(sgpt_ctx* ctx, int32_t n);
int32_t sgpt_ctx_set_low_latency(sgpt_ctx* ctx, int32_t on);
int32_t sgpt_ctx_set_tile_policy(sgpt_ctx* ctx, int32_t policy);
int32_t sgpt_ctx_set_query_tile(sgpt_ctx* ctx, int32_t k);

/* Micro-benchmark of one GEMM launch configuration (library-owned pseudo-random operands, never
 * zeros): average milliseconds per launch over `iters` launches.  epi: 0 store, 1 bias+gelu,
 * 2 bias+residual, 3 score, 4 V^T store (see sgpt_amd/csrc/common.h GemmEpi). */
sgpt_status sgpt_bench_gemm(sgpt_ctx* ctx, int32_t dtype, int32_t epi, int32_t out_dtype,
                            int32_t M, int32_t N, int32_t K, int32_t iters, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* SGPT_HIP_H */
