"""One `Family` row per model family in `FAMILIES` (the counterpart of `struct Family` in csrc/host.h), and `SGPTConfig`, which the rows'
parsers fill.  Outside this module nothing compares `model_type` with a literal; this module imports nothing of the model."""
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_SEQ_LEN = _lib.SGPT_MAX_SEQ_LEN   # tokens per sequence sgpt_encode takes (include/sgpt_hip.h): 32 768
# Mistral: a sliding_window of at least this many tokens (or of the whole position table) is folded away -- the rule the window kernels
# were accepted under when 2048 was the longest sequence; the fold then caps the positions at the window (see _parse_llama)
WINDOW_FOLD = 2048


@dataclass
class SGPTConfig:
    """The fields of HF GPTNeoConfig the forward reads (HF:gpt_neo/configuration_gpt_neo.py)."""
    vocab_size: int = 50257
    max_position_embeddings: int = 2048
    hidden_size: int = 768
    num_layers: int = 12
    num_heads: int = 12
    intermediate_size: Optional[int] = None
    window_size: int = 256
    attention_layers: Optional[List[str]] = None
    layer_norm_epsilon: float = 1e-5
    model_type: str = "gpt_neo"          # a Family.model_type: "gpt_neo" (SGPT-125M/1.3B/2.7B) | "gptj" (SGPT-5.8B) | "bloom" | "bert" | "llama"
    # GPT-J: HF GPTJConfig.rotary_dim (64).  "llama": the head dim where the config gives one (Qwen3: num_heads * head_dim need not be
    # hidden_size); 0 = hidden_size // num_heads.  Read it through head_dim(cfg)
    rotary_dim: int = 0
    num_kv_heads: Optional[int] = None    # "llama" only: key / value heads (grouped K / V); None = num_heads
    rope_theta: float = 10000.0           # "llama" only: base of the rotary frequencies

    def __post_init__(self):
        if self.num_kv_heads is None:
            self.num_kv_heads = self.num_heads
        if self.intermediate_size is None:
            self.intermediate_size = 4 * self.hidden_size
        if self.attention_layers is None:
            self.attention_layers = ["global" if i % 2 == 0 else "local" for i in range(self.num_layers)]

    @classmethod
    def from_hf_dict(cls, c: dict) -> "SGPTConfig":
        mt = c.get("model_type", "gpt_neo")
        for fam in FAMILIES:
            if mt in fam.hf_model_types:
                return fam.parse_config(c)
        raise NotImplementedError(f"model_type {mt!r}: GPT-Neo, GPT-J, BLOOM, BERT and Llama / Mistral are the families built here")


def table_rows(cfg: SGPTConfig) -> int:
    """Rows of the descriptor's max_pos and of the host rotary tables: positions past MAX_SEQ_LEN cannot be reached (gte-Qwen2's 131 072
    would be a 67 MB table of them).  Also the longest sequence a model takes: SGPTModel.max_seq_len."""
    return min(cfg.max_position_embeddings, MAX_SEQ_LEN)


def head_dim(cfg: SGPTConfig) -> int:
    """The width of one attention head: a Llama-family config may carry its own in `rotary_dim`, every other one is hidden_size // num_heads."""
    if cfg.model_type == "llama" and cfg.rotary_dim:
        return cfg.rotary_dim
    return cfg.hidden_size // cfg.num_heads


# ---- HF config.json -> SGPTConfig, per family ----
def _parse_gpt_neo(c: dict) -> SGPTConfig:
    layers = c.get("attention_layers")
    if layers is None and c.get("attention_types"):
        layers = [kind for pattern, rep in c["attention_types"] for _ in range(rep) for kind in pattern]
    return SGPTConfig(vocab_size=c["vocab_size"], max_position_embeddings=c["max_position_embeddings"], hidden_size=c["hidden_size"],
                      num_layers=c["num_layers"], num_heads=c["num_heads"], intermediate_size=c.get("intermediate_size"),
                      window_size=c.get("window_size", 256), attention_layers=layers, layer_norm_epsilon=c.get("layer_norm_epsilon", 1e-5))


def _parse_gptj(c: dict) -> SGPTConfig:   # HF GPTJConfig field names (HF:gptj/configuration_gptj.py)
    return SGPTConfig(vocab_size=c["vocab_size"], max_position_embeddings=c["n_positions"], hidden_size=c["n_embd"], num_layers=c["n_layer"],
                      num_heads=c["n_head"], intermediate_size=c.get("n_inner"), layer_norm_epsilon=c.get("layer_norm_epsilon", 1e-5),
                      model_type="gptj", rotary_dim=c.get("rotary_dim") or c["n_embd"] // c["n_head"], window_size=0,
                      attention_layers=["global"] * c["n_layer"])


def _parse_bloom(c: dict) -> SGPTConfig:  # HF BloomConfig (HF:bloom/configuration_bloom.py): ALiBi, no position table
    return SGPTConfig(vocab_size=c["vocab_size"], max_position_embeddings=2048, hidden_size=c["hidden_size"], num_layers=c["n_layer"],
                      num_heads=c["n_head"], intermediate_size=4 * c["hidden_size"], layer_norm_epsilon=c.get("layer_norm_epsilon", 1e-5),
                      model_type="bloom", window_size=0, attention_layers=["global"] * c["n_layer"])


def _parse_bert(c: dict) -> SGPTConfig:   # HF BertConfig (HF:bert/configuration_bert.py): the baseline of the reference's own scripts
    if c.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"bert: hidden_act {c.get('hidden_act')!r} (only 'gelu', the erf form, is built)")
    if c.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError(f"bert: position_embedding_type {c.get('position_embedding_type')!r} (only 'absolute')")
    if c.get("type_vocab_size", 2) < 1:
        raise NotImplementedError("bert: type_vocab_size must be >= 1 (token type 0 is folded into the position table)")
    return SGPTConfig(vocab_size=c["vocab_size"], max_position_embeddings=c["max_position_embeddings"],
                      hidden_size=c["hidden_size"], num_layers=c["num_hidden_layers"], num_heads=c["num_attention_heads"],
                      intermediate_size=c["intermediate_size"], layer_norm_epsilon=c.get("layer_norm_eps", 1e-12),
                      model_type="bert", window_size=0, attention_layers=["global"] * c["num_hidden_layers"])


def _parse_llama(c: dict) -> SGPTConfig:
    """HF LlamaConfig / MistralConfig / Qwen2Config / Qwen3Config: one family here (model_type "llama").  Mistral adds the window; Qwen2 a
    bias on q / k / v and Qwen3 a per-head q / k norm, both read off the tensors and not off the config; Qwen3 its own head_dim."""
    mt = c["model_type"]
    qwen = mt in ("qwen2", "qwen3")
    L, H, d = c["num_hidden_layers"], c["num_attention_heads"], c["hidden_size"]
    if c.get("hidden_act", "silu") != "silu":
        raise NotImplementedError(f"{mt}: hidden_act {c.get('hidden_act')!r} (only 'silu', the SwiGLU MLP, is built)")
    # (Qwen2Config has no such switches: its q / k / v bias is part of the model; Qwen3's attention_bias would bias o_proj too)
    for key in ("attention_bias", "mlp_bias"):
        if c.get(key) and mt != "qwen2":
            raise NotImplementedError(f"{mt}: {key} = true (the biased variants are not built)")
    if qwen and c.get("use_sliding_window"):
        raise NotImplementedError(f"{mt}: use_sliding_window = true (the per-layer window of the Qwen models is not built)")
    rs = c.get("rope_scaling")
    if rs is None and isinstance(c.get("rope_parameters"), dict) and c["rope_parameters"].get("rope_type", "default") != "default":
        rs = c["rope_parameters"]
    if rs is not None and rs.get("rope_type", rs.get("type", "default")) != "default":
        raise NotImplementedError(f"{mt}: rope_scaling {rs!r} (only the default rotary frequencies are built)")
    if not qwen and c.get("head_dim") is not None and c["head_dim"] * H != d:
        raise NotImplementedError(f"{mt}: head_dim {c['head_dim']} with head_dim * num_attention_heads != hidden_size {d}")
    if d > 4096:
        raise NotImplementedError(f"{mt}: hidden_size {d} > 4096 (the row kernels hold one row of at most 4096 columns per wave)")
    dh = c.get("head_dim") if qwen else None           # Llama / Mistral: head_dim * H == d holds, the config keeps rotary_dim 0
    if qwen and (dh or d // H) not in (64, 128):
        raise NotImplementedError(f"{mt}: head_dim {dh or d // H} (the attention and the head norm of this family are built for 64 and 128)")
    theta = c.get("rope_theta")
    if theta is None and isinstance(c.get("rope_parameters"), dict):
        theta = c["rope_parameters"].get("rope_theta")
    # Mistral: key j is visible to query i iff j > i - sliding_window (HF sliding_window_overlay) -- the window rule of the
    # GPT-Neo local layers, on every layer.  A window of min(max_position_embeddings, WINDOW_FOLD) tokens or more is folded to 0, the
    # no-window kernels (Mistral-7B-v0.1's 4096) -- and a model whose window was folded away takes sequences of at most sliding_window
    # tokens, inside which the window hides nothing: its max_position_embeddings is capped there, so that pack() refuses a longer
    # sequence with the ordinary message (Mistral-7B-v0.1 / e5-mistral: 4096 tokens).  `sliding_window: null` (v0.2 on): no window, the
    # whole table.  A missing key is HF MistralConfig's default, 4096
    sw = c.get("sliding_window", 4096) if mt == "mistral" else None
    max_pos = c["max_position_embeddings"]
    window = 0 if (sw is None or sw >= min(max_pos, WINDOW_FOLD)) else int(sw)
    if window < 0:
        raise NotImplementedError(f"{mt}: sliding_window {sw!r}")
    if sw is not None and window == 0:
        max_pos = min(max_pos, int(sw))
    return SGPTConfig(vocab_size=c["vocab_size"], max_position_embeddings=max_pos, hidden_size=d, num_layers=L,
                      num_heads=H, intermediate_size=c["intermediate_size"], layer_norm_epsilon=c.get("rms_norm_eps", 1e-6),
                      model_type="llama", window_size=window, attention_layers=["local" if window else "global"] * L,
                      num_kv_heads=c.get("num_key_value_heads") or H, rope_theta=float(theta if theta is not None else 10000.0),
                      rotary_dim=int(dh or 0))


# ---- state dict -> the tensors include/sgpt_hip.h lists for the family, host tables included ----
def _as_f32(a) -> torch.Tensor:
    return a.detach().to(torch.float32).cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float32))


def bert_state_dict(weights) -> dict:
    """HF BertModel / BertFor* state dict -> the tensors include/sgpt_hip.h asks for under SGPT_ARCH_BERT: the `bert.` prefix and
    the `pooler.*` / `cls.*` heads are dropped, `embeddings.position_ids` / `token_type_ids` buffers too, and -- token types are
    all 0 on this path (single-segment inputs, biencoder/beir/beir_dense_retriever.py:128-136) -- row 0 of
    `embeddings.token_type_embeddings.weight` is added to every row of the position table (one fp32 add per element, the order
    HF sums them in: inputs + token_type, then + position, differs by one rounding from this one)."""
    out = {}
    for k, v in weights.items():
        k2 = k[len("bert."):] if k.startswith("bert.") else k
        if k2.startswith(("pooler.", "cls.", "classifier.")) or k2.endswith(("position_ids", "token_type_ids")) or k.startswith("cls."):
            continue
        out[k2] = v
    tt = out.pop("embeddings.token_type_embeddings.weight", None)
    if tt is not None:
        pos = out["embeddings.position_embeddings.weight"]
        out["embeddings.position_embeddings.weight"] = _as_f32(pos) + _as_f32(tt)[0][None, :]
    return out


def llama_state_dict(weights) -> dict:
    """HF LlamaModel / LlamaForCausalLM / Mistral* / Qwen2* / Qwen3* state dict -> the tensors include/sgpt_hip.h asks for under
    SGPT_ARCH_LLAMA: the `model.` prefix and `lm_head.*` are dropped (as are `rotary_emb.inv_freq` buffers of older checkpoints), q_proj |
    k_proj | v_proj are stacked into `self_attn.qkv_proj.weight` [d_q + 2 d_kv, d] -- their biases, where the model has all three
    (Qwen2), into `self_attn.qkv_proj.bias` -- and gate_proj | up_proj into `mlp.gate_up_proj.weight` [2 ffn, d] (gate rows first).
    `self_attn.q_norm.weight` / `k_norm.weight` (Qwen3) pass through.  Any other bias tensor of a projection means a biased variant,
    which is not built."""
    flat = {}
    for k, v in weights.items():
        k2 = k[len("model."):] if k.startswith("model.") else k
        if k.startswith("lm_head.") or k2.endswith("rotary_emb.inv_freq"):
            continue
        if k2.endswith("_proj.bias") and not k2.endswith(tuple("self_attn." + n + "_proj.bias" for n in ("q", "k", "v", "qkv"))):
            raise NotImplementedError(f"llama: {k} (the biased variants are not built)")
        flat[k2] = v
    qkv = ("q_proj", "k_proj", "v_proj")
    part_bias = tuple("self_attn." + n + ".bias" for n in qkv)
    for k in flat:                                       # a q / k / v bias: all three or none
        if k.endswith(part_bias) and any(k[: k.rindex("self_attn.")] + b not in flat for b in part_bias):
            raise NotImplementedError(f"llama: {k} without the other two of q_proj / k_proj / v_proj .bias (a QKV bias is all three)")
    out, fuse = {}, (("self_attn.", qkv, "qkv_proj"), ("mlp.", ("gate_proj", "up_proj"), "gate_up_proj"))
    for k, v in flat.items():
        if k.endswith(part_bias):                        # fused behind its q_proj.weight
            continue
        for mod, parts, fused in fuse:
            if k.endswith(mod + parts[0] + ".weight"):
                base = k[: -len(parts[0] + ".weight")]
                out[base + fused + ".weight"] = torch.cat([_as_f32(flat[base + n + ".weight"]) for n in parts], dim=0)
                if parts is qkv and base + "q_proj.bias" in flat:
                    out[base + fused + ".bias"] = torch.cat([_as_f32(flat[base + n + ".bias"]) for n in parts], dim=0)
                break
        else:
            if not any(k.endswith(mod + n + ".weight") for mod, parts, _ in fuse for n in parts):
                out[k] = v
    return out


def rotary_tables_half(max_pos: int, head_dim: int, theta: float = 10000.0):
    """sin, cos fp32 [max_pos, head_dim / 2] of HF LlamaRotaryEmbedding (default rope): inv_freq[i] = theta^(-2i / head_dim) as
    `1.0 / (base ** (arange(0, dim, 2, int64).float() / dim))`, angle = position * inv_freq in float32."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv_freq[None, :].to(torch.float32)
    return ang.sin().numpy().astype(np.float32), ang.cos().numpy().astype(np.float32)


def alibi_slopes(n_head: int) -> np.ndarray:
    """HF build_alibi_tensor slopes (HF:bloom/modeling_bloom.py:62-79) in float32."""
    import math
    f32 = np.float32
    cp2 = 2 ** math.floor(math.log2(n_head))
    base = f32(2 ** (-(2 ** -(math.log2(cp2) - 3))))
    slopes = np.power(base, np.arange(1, 1 + cp2, dtype=np.int32).astype(f32)).astype(f32)
    if cp2 != n_head:
        extra_base = f32(2 ** (-(2 ** -(math.log2(2 * cp2) - 3))))
        nrem = min(cp2, n_head - cp2)
        slopes = np.concatenate([slopes, np.power(extra_base, np.arange(1, 1 + 2 * nrem, 2, dtype=np.int32).astype(f32)).astype(f32)])
    return slopes.astype(f32)


def rotary_tables(max_pos: int, dim: int):
    """HF create_sinusoidal_positions (HF:gptj/modeling_gptj.py:47-50) in float32: sin, cos [max_pos, dim/2]."""
    f32 = np.float32
    inv_freq = (f32(1.0) / (f32(10000.0) ** (np.arange(0, dim, 2).astype(f32) / f32(dim)))).astype(f32)
    ang = (np.arange(max_pos).astype(f32)[:, None] * inv_freq[None, :]).astype(f32)
    return np.sin(ang).astype(f32), np.cos(ang).astype(f32)


@dataclass(frozen=True)
class Family:
    """One model family.  The flags default to what the SGPT decoders build; a row names what its family does not."""
    # identity
    model_type: str                       # SGPTConfig.model_type
    hf_model_types: Tuple[str, ...]       # HF config.json `model_type` values parsed into this family
    arch: int                             # SGPT_ARCH_* (include/sgpt_hip.h)
    name: str                             # as messages spell it
    parse_config: Callable[[dict], SGPTConfig]
    # descriptor facts
    # scaled_logits: attn_scale = 1 / sqrt(head_dim) (HF:gptj:148, HF:bloom:186).  False: 1.0 (HF:gpt_neo:110) -- the logits grow with the
    # width, so default_precise_qk() may turn the structural precise_qk rule on
    scaled_logits: bool = True
    # rotary_dim: "none" (0) | "config" (cfg.rotary_dim) | "head_dim" (head_dim(cfg): the family's own head dim travels in the descriptor's
    # rotary_dim, include/sgpt_hip.h).  Rotary runs in place on 16-bit q / k: split-precision attention
    # is built for "none" only
    rotary_dim: str = "none"
    grouped_kv: bool = False              # n_kv_heads travels in the descriptor
    # weights
    # prepare_weights(cfg, weights): HF names -> the tensor names include/sgpt_hip.h lists for the family, the family's host tables
    # (rotary sin / cos, ALiBi slopes) added behind them
    prepare_weights: Callable[[SGPTConfig, dict], dict] = lambda cfg, weights: weights
    keeps_lm_head: bool = False           # `lm_head*` tensors are loaded (the other decoders tie the head to the embedding)
    # what the family builds
    # sgpt_modes: what was built for the SGPT checkpoints -- dtype 'fp8' / 'fp8mfma'; split-precision operands (precision 'x3' / 'auto' /
    # 'auto-class', precise_qk), with the 'auto' probe as the default of dtype 'f16'; f16 range shifts; `learntmean`, the trained position
    # weights.  False: one arithmetic per operand format (include/sgpt_hip.h), nothing to probe for, a range flag is final
    sgpt_modes: bool = True
    dtype_advice: str = ""                # the dtypes the fp8 refusal advises, in the family's order
    parallel_block: bool = False          # one LayerNorm feeds attention and MLP: LayerNorm-2 follows LayerNorm-1 in a per-class plan
    no_lm_head: Optional[str] = None      # the refusal of lm_logprobs where the family has no LM head
    # attention: the mode the family runs, and whether SGPTModel(attention=) may choose the other one (sgpt_model_set_attention,
    # include/sgpt_hip.h: the Llama family alone -- the bidirectional embedders built on its backbones)
    native_attention: str = "causal"
    attention_switch: bool = False
    fp8_projections: bool = False         # SGPTModel(projections='fp8'): calibration-free fp8 projections, set after load (sgpt_model_set_projections)
    # tokenizer
    framing: str = "brackets"             # "brackets" (specb / speca allowed, nothing added) | "cls_sep" | "bos_eos"


_ROTARY = ("rotary.sin", "rotary.cos")
FAMILIES = (
    Family("gpt_neo", ("gpt_neo",), _lib.SGPT_ARCH_GPTNEO, "GPT-Neo", _parse_gpt_neo, scaled_logits=False),
    Family("gptj", ("gptj",), _lib.SGPT_ARCH_GPTJ, "GPT-J", _parse_gptj, rotary_dim="config", keeps_lm_head=True, parallel_block=True,
           prepare_weights=lambda c, w: dict(w, **dict(zip(_ROTARY, rotary_tables(table_rows(c), c.rotary_dim))))),
    Family("bloom", ("bloom",), _lib.SGPT_ARCH_BLOOM, "BLOOM", _parse_bloom,
           prepare_weights=lambda c, w: dict(w, **{"alibi.slopes": alibi_slopes(c.num_heads)})),
    Family("bert", ("bert",), _lib.SGPT_ARCH_BERT, "BERT", _parse_bert, prepare_weights=lambda c, w: bert_state_dict(w), sgpt_modes=False,
           native_attention="bidirectional", framing="cls_sep", dtype_advice="'f16', 'bf16' or 'fp32'", no_lm_head="lm_logprobs: a BERT model carries no causal LM head"),
    Family("llama", ("llama", "mistral", "qwen2", "qwen3"), _lib.SGPT_ARCH_LLAMA, "Llama / Mistral", _parse_llama, rotary_dim="head_dim", grouped_kv=True,
           prepare_weights=lambda c, w: dict(llama_state_dict(w), **dict(zip(_ROTARY, rotary_tables_half(
               table_rows(c), head_dim(c), c.rope_theta)))),
           sgpt_modes=False, attention_switch=True, fp8_projections=True, framing="bos_eos", dtype_advice="'bf16', 'f16' or 'fp32'",
           no_lm_head="lm_logprobs is not built for Llama / Mistral models (their LM head is not loaded)"),
)
FRAMED = {"cls_sep": "is framed [CLS] ... [SEP]", "bos_eos": "takes its tokenizer's BOS / EOS"}   # Family.framing, as a refusal of the brackets puts it


def family(model_type: str) -> Family:
    """The row of a `SGPTConfig.model_type`."""
    for fam in FAMILIES:
        if fam.model_type == model_type:
            return fam
    raise ValueError(f"model_type {model_type!r}: SGPTConfig.model_type is one of {[f.model_type for f in FAMILIES]}")


ATTENTION_MODES = ("causal", "bidirectional")


def check_attention(cfg: SGPTConfig, attention: str) -> str:
    """SGPTModel's attention= argument, or its refusal: 'bidirectional' is the Llama family's to choose, and not over an applied window."""
    fam = family(cfg.model_type)
    if attention not in ATTENTION_MODES:
        raise ValueError(f"attention must be 'causal' or 'bidirectional', not {attention!r}")
    if attention == "bidirectional" and not fam.attention_switch:
        fixed = "is bidirectional by architecture" if fam.native_attention == "bidirectional" else "stays causal"
        raise ValueError(f"attention='bidirectional' is a mode of the Llama / Mistral / Qwen family: a {fam.name} model {fixed}")
    if attention == "bidirectional" and cfg.window_size > 0 and "local" in cfg.attention_layers:
        raise ValueError(f"attention='bidirectional' over an applied sliding window (window_size {cfg.window_size}) is not built: "
                         "only a window the config parser folded away (at least min(max_position_embeddings, "
                         f"{WINDOW_FOLD}) tokens) runs bidirectionally")
    return attention


PROJECTION_MODES = (None, "fp8")
PROJECTION_TILE = 256          # the fp8 MFMA kernel's tile: every projection width of a converted model is a multiple of it


def check_projections(cfg: SGPTConfig, dtype: str, projections: Optional[str]) -> Optional[str]:
    """SGPTModel's projections= argument, or its refusal: 'fp8' (sgpt_model_set_projections) is the Llama family's, on a 'bf16' model
    whose projection widths are multiples of 256."""
    fam = family(cfg.model_type)
    if projections not in PROJECTION_MODES:
        raise ValueError(f"projections must be None or 'fp8', not {projections!r}")
    if projections is None:
        return None
    if not fam.fp8_projections:
        raise ValueError(f"projections='fp8' is a mode of the Llama / Mistral / Qwen family: a {fam.name} model has "
                         + ("dtype 'fp8' / 'fp8mfma'" if fam.sgpt_modes else "no fp8 mode"))
    if dtype != "bf16":
        raise ValueError(f"projections='fp8' converts a dtype='bf16' model, not dtype={dtype!r}")
    dh = head_dim(cfg)
    widths = (("hidden_size", cfg.hidden_size), ("num_heads * head_dim", cfg.num_heads * dh),
              ("num_kv_heads * head_dim", cfg.num_kv_heads * dh), ("intermediate_size", cfg.intermediate_size))
    for name, w in widths:
        if w % PROJECTION_TILE:
            raise ValueError(f"projections='fp8' needs {name} to be a multiple of {PROJECTION_TILE}: this model has {name} = {w}")
    return projections


def attention_from_hf_dict(c: dict, attention: Optional[str] = None) -> str:
    """from_pretrained's attention=None: 'bidirectional' iff the folder's raw config.json says `is_causal: false` (GritLM, gte-Qwen2,
    LLM2Vec checkpoints), else 'causal'; an explicit argument wins.  The key stays out of SGPTConfig."""
    if attention is not None:
        return attention
    return "bidirectional" if c.get("is_causal", True) is False else "causal"


def family_of(model) -> Family:
    """The row of a model object (SGPTModel, or a stand-in with a `cfg`; one without, or without a model_type, is a GPT model)."""
    return family(getattr(getattr(model, "cfg", None), "model_type", FAMILIES[0].model_type))


def max_seq_len_of(model) -> Optional[int]:
    """SGPTModel.max_seq_len of a model object or a stand-in with a `cfg`: the longest sequence it encodes, min(max_position_embeddings,
    MAX_SEQ_LEN).  None where the object names no position range (nothing to clamp to)."""
    cfg = getattr(model, "cfg", None)
    return table_rows(cfg) if getattr(cfg, "max_position_embeddings", None) else None


# ---- seeded random-init weights under HF state-dict names (fixtures, benches: no checkpoints exist offline) ----
def synthetic_llama_weights(cfg: SGPTConfig, seed: int = 0, std: float = 0.02) -> Dict[str, np.ndarray]:
    """Seeded random-init weights under HF LlamaModel state-dict names (fixtures, benches: no checkpoints exist offline)."""
    rng = np.random.default_rng(seed)
    d, ffn = cfg.hidden_size, cfg.intermediate_size
    dkv = cfg.num_kv_heads * (d // cfg.num_heads)
    f32 = np.float32

    def nrm(*shape, s=std):
        return (rng.standard_normal(shape, dtype=np.float32) * f32(s)).astype(f32)

    w = {"embed_tokens.weight": nrm(cfg.vocab_size, d)}
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        w[p + "input_layernorm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[p + "self_attn.q_proj.weight"] = nrm(d, d)
        w[p + "self_attn.k_proj.weight"] = nrm(dkv, d)
        w[p + "self_attn.v_proj.weight"] = nrm(dkv, d)
        w[p + "self_attn.o_proj.weight"] = nrm(d, d)
        w[p + "post_attention_layernorm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[p + "mlp.gate_proj.weight"] = nrm(ffn, d)
        w[p + "mlp.up_proj.weight"] = nrm(ffn, d)
        w[p + "mlp.down_proj.weight"] = nrm(d, ffn)
    w["norm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
    return w


def synthetic_qwen_weights(cfg: SGPTConfig, seed: int = 0, qkv_bias: bool = False, qk_norm: bool = False, std: float = 0.02,
                            bias_std: float = 0.1, gain_std: float = 0.1) -> Dict[str, np.ndarray]:
    """Seeded random-init weights under HF Qwen2Model (qkv_bias) / Qwen3Model (qk_norm) state-dict names, a generator stream of its own
    (synthetic_llama_weights keeps the one its fixtures record).  The q / k / v biases have std 0.1 -- five times the weights', so that
    a dropped bias cannot pass a parity test -- and the head-norm gains are 1 + 0.1 N(0, 1)."""
    rng = np.random.default_rng(seed)
    d, ffn, dh = cfg.hidden_size, cfg.intermediate_size, head_dim(cfg)
    dq, dkv = cfg.num_heads * dh, cfg.num_kv_heads * dh
    f32 = np.float32

    def nrm(*shape, s=std):
        return (rng.standard_normal(shape, dtype=np.float32) * f32(s)).astype(f32)

    w = {"embed_tokens.weight": nrm(cfg.vocab_size, d)}
    for i in range(cfg.num_layers):
        p = f"layers.{i}."
        w[p + "input_layernorm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        for n, rows in (("q", dq), ("k", dkv), ("v", dkv)):
            w[p + f"self_attn.{n}_proj.weight"] = nrm(rows, d)
            if qkv_bias:
                w[p + f"self_attn.{n}_proj.bias"] = nrm(rows, s=bias_std)
        if qk_norm:
            w[p + "self_attn.q_norm.weight"] = (1.0 + nrm(dh, s=gain_std)).astype(f32)
            w[p + "self_attn.k_norm.weight"] = (1.0 + nrm(dh, s=gain_std)).astype(f32)
        w[p + "self_attn.o_proj.weight"] = nrm(d, dq)
        w[p + "post_attention_layernorm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[p + "mlp.gate_proj.weight"] = nrm(ffn, d)
        w[p + "mlp.up_proj.weight"] = nrm(ffn, d)
        w[p + "mlp.down_proj.weight"] = nrm(d, ffn)
    w["norm.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
    return w


def synthetic_bert_weights(cfg: SGPTConfig, seed: int = 0, std: float = 0.02) -> Dict[str, np.ndarray]:
    """Seeded random-init weights under HF BertModel state-dict names (bench, tests: no checkpoints exist offline)."""
    rng = np.random.default_rng(seed)
    d, ffn = cfg.hidden_size, cfg.intermediate_size
    f32 = np.float32

    def nrm(*shape, s=std):
        return (rng.standard_normal(shape, dtype=np.float32) * f32(s)).astype(f32)

    def ln(name):
        w[name + ".weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[name + ".bias"] = nrm(d, s=0.05)

    w = {"embeddings.word_embeddings.weight": nrm(cfg.vocab_size, d),
         "embeddings.position_embeddings.weight": nrm(cfg.max_position_embeddings, d, s=std / 2),
         "embeddings.token_type_embeddings.weight": nrm(2, d, s=std / 2)}
    ln("embeddings.LayerNorm")
    for i in range(cfg.num_layers):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            w[p + f"attention.self.{n}.weight"] = nrm(d, d)
            w[p + f"attention.self.{n}.bias"] = nrm(d, s=0.02)
        w[p + "attention.output.dense.weight"] = nrm(d, d)
        w[p + "attention.output.dense.bias"] = nrm(d, s=0.02)
        ln(p + "attention.output.LayerNorm")
        w[p + "intermediate.dense.weight"] = nrm(ffn, d)
        w[p + "intermediate.dense.bias"] = nrm(ffn, s=0.02)
        w[p + "output.dense.weight"] = nrm(d, ffn)
        w[p + "output.dense.bias"] = nrm(d, s=0.02)
        ln(p + "output.LayerNorm")
    return w


def synthetic_weights(cfg: SGPTConfig, seed: int = 0, std: float = 0.02) -> Dict[str, np.ndarray]:
    """Seeded random-init weights under HF GPT-Neo state-dict names (no checkpoints exist offline).
    Same generator stream as oracle/sgpt_oracle.py::synth_weights so the CPU oracle and the GPU read
    identical bytes; duplicated here because product code must not import the oracle."""
    rng = np.random.default_rng(seed)
    d, ffn = cfg.hidden_size, cfg.intermediate_size
    f32 = np.float32

    def nrm(*shape, s=std):
        return (rng.standard_normal(shape, dtype=np.float32) * f32(s)).astype(f32)

    w = {"wte.weight": nrm(cfg.vocab_size, d), "wpe.weight": nrm(cfg.max_position_embeddings, d, s=std / 2)}
    for i in range(cfg.num_layers):
        p = f"h.{i}."
        w[p + "ln_1.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[p + "ln_1.bias"] = nrm(d, s=0.05)
        w[p + "attn.attention.q_proj.weight"] = nrm(d, d)
        w[p + "attn.attention.k_proj.weight"] = nrm(d, d)
        w[p + "attn.attention.v_proj.weight"] = nrm(d, d)
        w[p + "attn.attention.out_proj.weight"] = nrm(d, d)
        w[p + "attn.attention.out_proj.bias"] = nrm(d, s=0.02)
        w[p + "ln_2.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
        w[p + "ln_2.bias"] = nrm(d, s=0.05)
        w[p + "mlp.c_fc.weight"] = nrm(ffn, d)
        w[p + "mlp.c_fc.bias"] = nrm(ffn, s=0.02)
        w[p + "mlp.c_proj.weight"] = nrm(d, ffn)
        w[p + "mlp.c_proj.bias"] = nrm(d, s=0.02)
    w["ln_f.weight"] = (1.0 + nrm(d, s=0.1)).astype(f32)
    w["ln_f.bias"] = nrm(d, s=0.05)
    return w
