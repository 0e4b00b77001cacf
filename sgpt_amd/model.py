"""SGPT encoder on the HIP layer: weights -> sgpt_model_load, token lists -> packed varlen
batches -> sgpt_encode (GPT-Neo forward + pool + optional normalise in one C call).

Replaces the device leg of CustomEmbedder.embed / embed_batcher
(biencoder/beir/beir_dense_retriever.py:158-314) and of SentenceTransformer._encode
(sentence_transformers/SentenceTransformer.py:217-255)."""
import ctypes as C
import itertools
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (ModelDesc, TensorView, POOL_MODES, SGPT_BF16, SGPT_F16, SGPT_F32, SGPT_FP8M, SGPT_FP8W, SgptRangeError,
                   SGPT_PREC_CLASSES, PC_LN1, PC_ATT, PC_CTX, PC_LN2, PC_H)
from .families import (MAX_SEQ_LEN, SGPTConfig, attention_from_hf_dict, check_attention, check_projections, alibi_slopes, bert_state_dict, family, head_dim, llama_state_dict, rotary_tables,  # noqa: F401
                       rotary_tables_half, table_rows, synthetic_bert_weights, synthetic_llama_weights, synthetic_qwen_weights, synthetic_weights)
from .runtime import Context, get_context, _p, _stream_ptr

# Precision probe thresholds: crest factor max|v| / rms(v) of an operand row above which 11-bit operands are not trusted.
# Well-conditioned rows measure 5-7 (LayerNorm outputs, attention context) and 8-10 (GELU outputs: half the entries near
# zero) at any depth / width (seeded SGPT-125M and 1.3B shapes); a row that two outlier channels carry measures ~sqrt(K / 2)
# (K = 768: 20-28 on the engineered-outlier fixture, GELU outputs 55): twice the clean level separates the two.
CREST_LIMIT_LN = 12.0
CREST_LIMIT_H = 20.0
PROBE_MAX_ROWS = 8192   # token rows of the probe forward (a bounded sample of the first call's sequences)

# Sequence starts on the packed token axis: multiples of ALIGN rows.  The only kernel that cares is the attention's V^T tile
# staging (16-byte loads along the token axis), and a dwordx4 load needs dword alignment = an EVEN token offset, not 16 bytes.
# Round 4, same box (scripts/small_batch_profile.py / mid_batch_profile.py, bench.py varlen leg), ALIGN 8 / 4 / 2: 1000 queries of
# 4..32 tokens 6.44 / 4.93 / 4.85 ms (21 760 / 19 968 / 18 944 padded rows), 128 queries 1.57 / 1.53 / 1.52 ms, lengths
# U{16..128} 62.8 / 63.4 / 63.9 k sentences/s; bit-identical embeddings per sequence (a sequence's arithmetic does not see its offset).
ALIGN = 2
TOKEN_TILE = 256   # GEMM M tile (256x256 LDS-DMA kernel)
# Query-sized batches (round 6, csrc/qgemm.hip): a layout of at most QUERY_ROWS token rows is padded to QUERY_TILE-row tiles
# only -- its projections run on 32-row tiles, and one 18-token query no longer pays for 256 rows.
QUERY_ROWS = 512
QUERY_TILE = 32


def pad_rows(total: int, row_tile: Optional[int] = None) -> int:
    """Token rows of a packed layout holding `total` allocated rows (include/sgpt_hip.h: T_pad % 32 == 0).
    row_tile: a fixed tile instead (dtype='fp8mfma' keeps 256: its MFMA kernels only take 256-row tiles, and a layout they do not
    fit would silently run the fp8-storage arithmetic)."""
    tile = row_tile or (QUERY_TILE if total <= QUERY_ROWS else TOKEN_TILE)
    return (int(total) + tile - 1) // tile * tile


@dataclass
class PackedBatch:
    """Device-resident packed token layout of include/sgpt_hip.h::sgpt_encode."""
    ids: torch.Tensor
    pos: torch.Tensor
    seq_off: torch.Tensor
    seq_len: torch.Tensor
    pad_left: torch.Tensor
    B: int
    T_pad: int
    max_alloc: int
    n_tokens: int  # real tokens (for throughput accounting)
    max_pos: int = 0  # largest position id (pad_left + len - 1): bounds the learntmean weight table
    arena: Optional[torch.Tensor] = None  # the one int32 device buffer the five views above slice (graph replays refill it in one copy)
    n_real: int = 0  # sequences that are the caller's (B minus the bucket's filler sequences)
    off_host: Optional[np.ndarray] = None  # host int32[B + 1] copy of seq_off: lets the library cut a bulk call into two chains without reading the device
    pool_lo: Optional[torch.Tensor] = None  # int32[B] first pooled token of every sequence (pack(pool_from=)); None: every token is pooled


def _flatten(seqs, total: int) -> np.ndarray:
    """Ragged token lists -> one int32 vector, at C speed: a [B,S] ndarray is a reshape, lists of ndarrays a
    concatenate, lists of lists one itertools.chain pass (no per-token Python bytecode)."""
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:
        return _to_i32(seqs).reshape(-1)
    if len(seqs) and isinstance(seqs[0], np.ndarray):
        return _to_i32(np.concatenate(seqs))
    # (Python ints beyond int32 make numpy raise OverflowError here instead of wrapping)
    return np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int32, count=total)


def _to_i32(a: np.ndarray) -> np.ndarray:
    """Narrow token ids to int32 without letting an id >= 2^31 wrap into the vocabulary range (the range check of
    SGPTModel.pack runs on the narrowed values)."""
    if a.dtype != np.int32 and a.size and (int(a.max()) > np.iinfo(np.int32).max or int(a.min()) < np.iinfo(np.int32).min):
        raise ValueError("token id out of range")
    return np.ascontiguousarray(a, dtype=np.int32)


def pack_layout(seqs, pad_left: Optional[Sequence[int]] = None, bucket: Optional[Tuple[int, int, int]] = None,
                row_tile: Optional[int] = None, pool_from=None) -> dict:
    """Sizes and offsets of the packed layout (no token data yet).
    bucket = (B_cap, T_cap, A_cap): pad the layout to that capacity -- B_cap - B one-token filler sequences behind the real
    ones, T_pad = T_cap, max_alloc = A_cap -- so that every batch of the bucket launches the same grids (hipGraph replay).
    The filler rows are computed and dropped; `n_real` says how many output rows are the caller's.
    pool_from: one int, or one per sequence -- the first pooled token, counted from the sequence start with its frame (BOS, [CLS])
    included: the tokens of an instruction prompt in front of it are encoded and not pooled.  None: no such array in the layout."""
    B = len(seqs)
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:
        lens = np.full(B, seqs.shape[1], dtype=np.int64)
    else:
        lens = np.fromiter(map(len, seqs), dtype=np.int64, count=B)
    if B == 0 or (lens <= 0).any():
        raise ValueError("Empty items should be cleaned prior to running")  # beir_dense_retriever.py:180-181
    pl = np.zeros(B, dtype=np.int32) if pad_left is None else np.asarray(pad_left, dtype=np.int32)
    pf = None
    if pool_from is not None:
        pf = np.asarray(pool_from)
        if pf.dtype.kind not in "iu" or pf.ndim > 1 or (pf.ndim == 1 and pf.shape[0] != B):
            raise ValueError("pool_from: one int, or one int per sequence")
        pf = np.full(B, int(pf), dtype=np.int64) if pf.ndim == 0 else pf.astype(np.int64)
        if (pf < 0).any():
            raise ValueError("pool_from counts tokens from the sequence start: it cannot be negative")
        pf = np.minimum(pf, lens).astype(np.int32)          # (the kernel clamps too: an empty range is a zero row)
    n_real, n_tokens = B, int(lens.sum())
    max_pos = int((lens + pl.astype(np.int64)).max()) - 1
    if bucket is not None:
        B_cap, T_cap, A_cap = bucket
        if B_cap < B or T_cap != pad_rows(T_cap, row_tile) or A_cap % ALIGN:
            raise ValueError(f"bucket {bucket} cannot hold {B} sequences (T_cap % {TOKEN_TILE}, or % {QUERY_TILE} up to "
                             f"{QUERY_ROWS} rows; A_cap % {ALIGN})")
        lens = np.concatenate([lens, np.ones(B_cap - B, dtype=np.int64)])
        pl = np.concatenate([pl, np.zeros(B_cap - B, dtype=np.int32)])
        if pf is not None:
            pf = np.concatenate([pf, np.zeros(B_cap - B, dtype=np.int32)])
        B = B_cap
    alloc = (lens + ALIGN - 1) // ALIGN * ALIGN
    off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(alloc, out=off[1:])
    T_pad = pad_rows(int(off[-1]), row_tile)
    max_alloc = int(alloc.max())
    if bucket is not None:
        if T_pad > bucket[1] or max_alloc > bucket[2]:
            raise ValueError(f"packed layout (T_pad {T_pad}, max_alloc {max_alloc}) does not fit bucket {bucket}")
        T_pad, max_alloc = bucket[1], bucket[2]
    return dict(B=B, lens=lens, alloc=alloc, off=off, T_pad=T_pad, pl=pl, n_tokens=n_tokens, n_real=n_real,
                max_alloc=max_alloc, max_pos=max_pos, pool_lo=pf)


def arena_ints(lay: dict) -> int:
    """int32 words of the one-buffer host/device image: [ids T_pad | pos T_pad | seq_off B+1 | seq_len B | pad_left B], and behind them
    [pool_lo B] where the layout has one (pack_layout(pool_from=))."""
    return 2 * lay["T_pad"] + (3 if lay.get("pool_lo") is None else 4) * lay["B"] + 1


def fill_arena(seqs, lay: dict, arena: np.ndarray):
    """Writes the packed layout of include/sgpt_hip.h::sgpt_encode into `arena` (int32, >= arena_ints words; pure index
    arithmetic, vectorised).  Returns (largest, smallest) token id: the caller validates them against the vocabulary."""
    B, T_pad, lens, off, pl = lay["B"], lay["T_pad"], lay["lens"], lay["off"], lay["pl"]
    n = lay["n_tokens"]
    ids, pos = arena[:T_pad], arena[T_pad: 2 * T_pad]
    ids[:] = 0
    pos[:] = 0
    flat = _flatten(seqs, n)
    if flat.shape[0] != n:
        raise ValueError("ragged token input does not match its lengths")
    hi_lo = (int(flat.max()), int(flat.min()))
    if B > lay["n_real"]:                                     # bucket fillers: one token (id 0) each
        flat = np.concatenate([flat, np.zeros(B - lay["n_real"], dtype=np.int32)])
        n = flat.shape[0]
    if (lens == lens[0]).all() and lens[0] % ALIGN == 0:      # rectangular, aligned: rows are already in place
        ids[:n] = flat
        pos[:n] = (np.arange(n, dtype=np.int64) % lens[0] + np.repeat(pl.astype(np.int64), lens)).astype(np.int32)
    else:
        within = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        rows = np.repeat(off[:-1], lens) + within            # destination row of every real token: seq_off[b] + t
        ids[rows] = flat
        pos[rows] = (within + np.repeat(pl.astype(np.int64), lens)).astype(np.int32)
    o = 2 * T_pad
    arena[o: o + B + 1] = off
    arena[o + B + 1: o + 2 * B + 1] = lens
    arena[o + 2 * B + 1: o + 3 * B + 1] = pl
    if lay.get("pool_lo") is not None:
        arena[o + 3 * B + 1: o + 4 * B + 1] = lay["pool_lo"]
    return hi_lo


def pack_host(seqs: Sequence[Sequence[int]], pad_left: Optional[Sequence[int]] = None,
              bucket: Optional[Tuple[int, int, int]] = None, pool_from=None):
    """Token lists -> numpy arrays of the packed layout (host side; the dict form used by tests)."""
    lay = pack_layout(seqs, pad_left, bucket, pool_from=pool_from)
    arena = np.empty(arena_ints(lay), dtype=np.int32)
    fill_arena(seqs, lay, arena)
    B, T_pad = lay["B"], lay["T_pad"]
    o = 2 * T_pad
    return dict(ids=arena[:T_pad], pos=arena[T_pad:o], seq_off=arena[o: o + B + 1], seq_len=arena[o + B + 1: o + 2 * B + 1],
                pad_left=arena[o + 2 * B + 1: o + 3 * B + 1], B=B, T_pad=T_pad, max_alloc=lay["max_alloc"],
                n_tokens=lay["n_tokens"], max_pos=lay["max_pos"], n_real=lay["n_real"], arena=arena,
                pool_lo=None if lay["pool_lo"] is None else arena[o + 3 * B + 1: o + 4 * B + 1])


class _Staging:
    """Two pinned int32 host arenas used alternately for the H2D copy of packed batches: the copy of batch i+1 is
    filled while the copy of batch i is still in flight (an event per arena says when it may be overwritten)."""

    def __init__(self, device):
        self.device = device
        self.bufs = [None, None]
        self.events = [None, None]
        self.turn = 0

    def acquire(self, n_int: int):
        i = self.turn
        self.turn ^= 1
        if self.events[i] is not None:
            self.events[i].synchronize()                    # the previous copy out of this arena has completed
        if self.bufs[i] is None or self.bufs[i].numel() < n_int:
            cap = max(n_int + n_int // 4, 1 << 16)
            self.bufs[i] = torch.empty(cap, dtype=torch.int32).pin_memory()
        return i, self.bufs[i]

    def release(self, i: int):
        ev = self.events[i] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.events[i] = ev


# precise_qk -> (LayerNorm-1 class level, attention class, context class) in every block
PRECISE_QK_PLANS = {"full": (1, 0, 0), "logits": (0, 1, 0), "act+logits": (3, 1, 0), "full+logits": (1, 1, 0),
                    "qkv+logits": (2, 1, 0), "attn": (2, 1, 1)}


def default_precise_qk(cfg: "SGPTConfig", dtype: str):
    """precise_qk=None: the cheapest variant that holds BOTH reference fixtures of the model's shape inside the 1e-3 bar with
    >= 25 % of margin, measured on MI355X (max |cos - ref| / max |normalised emb - ref|; first fixture, second seed;
    sentences/s of round 4, profiles/r04_precise_qk.txt, profiles/r05_parity.jsonl):
      SGPT-1.3B shape (24 layers, d 2048)   plain        8.2e-4 / 1.09e-3   7.6e-4 / 1.43e-3   @ 3590
                                            'logits'     6.7e-4 / 8.3e-4    7.0e-4 / 9.6e-4    @ 3428  (round 4's default: the second
                                                                                                        seed leaves it 4 % of margin)
                                            'act+logits' 6.0e-4 / 7.2e-4    5.4e-4 / 7.5e-4    @ 2967  <- default (round 5)
                                            'full'       5.0e-4 / 7.7e-4    6.4e-4 / 7.9e-4    @ 2800
                                            'full+logits' 3.3e-4 / 4.3e-4   3.5e-4 / 4.6e-4    @ 2706
      SGPT-2.7B shape (32 layers, d 2560)   plain        1.11e-3 / 2.21e-3  1.47e-3 / 2.25e-3  @ 1788
                                            'full+logits' 5.1e-4 / 8.0e-4   5.4e-4 / 9.8e-4    @ 1337  (round 4's default; second seed --
                                                                                                        160-300-token documents, the local
                                                                                                        window live -- at 2 % of margin)
                                            'qkv+logits' 4.6e-4 / 6.9e-4    4.9e-4 / 7.4e-4    @ 1214  <- default (round 5)
                                            'attn'       3.4e-4 / 5.0e-4    3.3e-4 / 5.9e-4    @ 1100
    GPT-Neo only (no 1/sqrt(dh) in its attention, HF:gpt_neo:110: the logits grow with the width); GPT-J / BLOOM sit at 6e-5
    and SGPT-125M at 3.2e-4 without any of it."""
    if dtype != "f16" or family(cfg.model_type).scaled_logits or cfg.hidden_size < 2048:
        return False
    if head_dim(cfg) not in (64, 128):
        return "full"      # the split-precision attention exists for head_dim 64 / 128: the split Q / K projection alone (round 3's default)
    return "act+logits" if cfg.hidden_size < 2560 else "qkv+logits"


def check_args(cfg: SGPTConfig, dtype: str, precise_qk, precision):
    """SGPTModel's dtype / precise_qk / precision, defaults filled in -- or the refusal, before anything touches the device."""
    fam = family(cfg.model_type)
    if dtype in ("fp16", "float16", "half"):
        dtype = "f16"
    if precision is None:
        precision = "auto" if (dtype == "f16" and fam.sgpt_modes) else "plain"
    if precision not in ("plain", "x3", "auto", "auto-class"):
        raise ValueError("precision must be 'plain', 'x3', 'auto' or 'auto-class'")
    if precision != "plain" and dtype not in ("f16", "bf16"):
        raise ValueError("precision applies to dtype 'f16' / 'bf16'")
    if precise_qk is None:
        precise_qk = default_precise_qk(cfg, dtype)
    if precise_qk is True:
        precise_qk = "full"
    if precise_qk not in (False,) + tuple(PRECISE_QK_PLANS):
        raise ValueError(f"precise_qk must be None, False, True or one of {sorted(PRECISE_QK_PLANS)}")
    if precise_qk and dtype not in ("f16", "bf16"):
        raise ValueError("precise_qk applies to dtype 'f16' / 'bf16'")
    # one arithmetic per operand format for a family that says so in its row (include/sgpt_hip.h): refused here, loudly
    if not fam.sgpt_modes and dtype in ("fp8", "fp8mfma"):
        raise ValueError(f"dtype {dtype!r} is not available for {fam.name} models: use {fam.dtype_advice}")
    if not fam.sgpt_modes and (precision != "plain" or precise_qk):
        raise ValueError(f"split-precision operands (precision='x3' / 'auto' / 'auto-class', precise_qk) are not available for {fam.name} models")
    if fam.grouped_kv and cfg.num_heads % cfg.num_kv_heads:
        raise ValueError("num_heads must be a multiple of num_kv_heads")
    if dtype not in ("f16", "bf16", "fp32", "fp8", "fp8mfma"):
        raise ValueError("dtype must be 'f16' (IEEE-half MFMA operands, range-guarded: the 1e-3-parity mode), "
                         "'bf16' (bf16 MFMA operands), 'fp32' (exact fp32 MFMA), "
                         "'fp8' (e4m3fn weight storage, bf16 arithmetic) or 'fp8mfma' (fp8 storage + fp8 MFMA on the MLP)")
    return dtype, precise_qk, precision


def model_desc(cfg: SGPTConfig, dtype: str, precise_qk, precision: str):
    """The sgpt_model_desc of a model (arguments as check_args returns them) and the layer_is_local array it points to: keep both."""
    fam = family(cfg.model_type)
    local = (C.c_uint8 * cfg.num_layers)(*[1 if a == "local" else 0 for a in cfg.attention_layers])
    dh = head_dim(cfg)
    ln1, _, ctx = PRECISE_QK_PLANS[precise_qk] if precise_qk else (0, 0, 0)
    return ModelDesc(arch=fam.arch, n_layers=cfg.num_layers, d_model=cfg.hidden_size, n_heads=cfg.num_heads, d_ffn=cfg.intermediate_size,
                     vocab=cfg.vocab_size, max_pos=table_rows(cfg), window=cfg.window_size, ln_eps=cfg.layer_norm_epsilon,
                     attn_scale=float(1.0 / np.sqrt(np.float32(dh))) if fam.scaled_logits else 1.0,
                     compute_dtype={"f16": SGPT_F16, "bf16": SGPT_BF16, "fp32": SGPT_F32, "fp8": SGPT_FP8W, "fp8mfma": SGPT_FP8M}[dtype],
                     layer_is_local=C.cast(local, C.POINTER(C.c_uint8)),
                     rotary_dim={"none": 0, "config": cfg.rotary_dim, "head_dim": dh}[fam.rotary_dim],
                     n_kv_heads=cfg.num_kv_heads if fam.grouped_kv else 0, qk_split=1 if ln1 in (1, 3) else 0,
                     split_weights=1 if (precision != "plain" or ln1 == 2 or ctx) else 0), local


def load_tensors(cfg: SGPTConfig, weights) -> List[Tuple[str, torch.Tensor]]:
    """A state dict -> the (name, tensor) list sgpt_model_load takes, in the dict's order and after Family.prepare_weights: the
    `transformer.` prefix stripped, what the library does not load dropped.  Tensors stay on their device and keep their dtype."""
    fam, out = family(cfg.model_type), []
    for k, v in fam.prepare_weights(cfg, weights).items():
        k2 = k[len("transformer."):] if k.startswith("transformer.") else k
        # dropped: the learntmean table riding along with the weights, HF's buffers, an LM head tied to the embedding
        if (k2 == "position_weights" or k2.endswith(("attn.attention.bias", "attn.bias", "masked_bias", "embed_positions"))
                or (k.startswith("lm_head") and not fam.keeps_lm_head)):
            continue
        v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        if (k2 in ("wpe.weight", "embeddings.position_embeddings.weight") and cfg.max_position_embeddings > MAX_SEQ_LEN
                and v.shape[0] == cfg.max_position_embeddings):
            v = v[:MAX_SEQ_LEN]           # a learned position table beyond MAX_SEQ_LEN: the descriptor's max_pos rows are loaded
        out.append((k2, v))
    return out


class SGPTModel:
    """GPT-Neo weights resident on one GPU behind an `sgpt_model*` handle."""

    def __init__(self, cfg: SGPTConfig, weights: Dict[str, "np.ndarray | torch.Tensor"], device=None,
                 dtype: str = "f16", ctx: Optional[Context] = None, max_tokens_per_call: int = 131072,
                 calibrate: bool = True, precise_qk=None, precision: Optional[str] = None, attention: str = "causal",
                 projections: Optional[str] = None):
        """projections: None (default) | 'fp8' -- Llama / Mistral / Qwen models of dtype 'bf16' only, set after load
        (sgpt_model_set_projections): the Q | K | V, gate | up and down projections run on the e4m3 MFMA with one dynamic power-of-two
        scale per token row and one per weight row -- no calibration pass -- and their weights take half the bytes; the out-projection
        stays bf16.  hidden_size, num_heads * head_dim, num_kv_heads * head_dim and intermediate_size must be multiples of 256; layouts
        are padded to 256 token rows.  One-way; refused for EncodeGraph.  Quality and speed as measured: README.
        attention: 'causal' (default) | 'bidirectional' -- Llama / Mistral / Qwen models only, set after load
        (sgpt_model_set_attention): in every layer every token sees every token of its sequence, what GritLM, gte-Qwen2-instruct and the
        LLM2Vec checkpoints were trained with.  Refused for the other families and over an applied (unfolded) sliding window.
        precision (dtype 'f16' / 'bf16'): how operands enter the MFMAs (include/sgpt_hip.h::sgpt_model_set_precision).
          'plain'  16-bit operands everywhere (plus the structural rule below);
          'x3'     every operand class of every block as a hi + lo pair of 16-bit values (the "f16x3" mode: embeddings within
                   ~1e-5 of the fp32 reference on ANY checkpoint the f16 range guard accepts, a third of the 16-bit MFMA
                   rate, ~5x the exact-fp32 mode);
          'auto'   (the default for dtype 'f16': parity first) the split weight copies are kept, and the FIRST encode call
                   probes a bounded sample of its own sequences: the crest factor max|v| / rms(v) of every operand class of
                   every block.  A class above the limits (CREST_LIMIT_*) means an ill-conditioned checkpoint -- outlier
                   channels / hidden units, as real GPT-Neo checkpoints have -- and moves the WHOLE model to 'x3'; a clean
                   checkpoint stays 'plain' (same kernels, same bits, same speed).  The choice is sticky and readable
                   (precision_plan(), precision_report); set_precision_plan() pins it across processes.  MEMORY: until the
                   probe has settled, the model holds [W_hi | W_hi | W_lo] copies of its four matrices per block -- 3 x the
                   16-bit weight bytes on top of the plain copy (SGPT-125M +0.5 GB, SGPT-5.8B +35 GB); a probe that settles
                   on 'plain' frees them (release_split_weights(); precision_report["split_weight_bytes_released"]), and a
                   later plan that needs them is refused loudly.  In a multi-process search the decision is COLLECTIVE
                   (sync_precision(): the union of every rank's flags), so all ranks embed at one precision;
          'auto-class'  as 'auto' but only the flagged classes are split (LayerNorm-1 brings the block's attention along).
        precise_qk: the structural rule for GPT-Neo -- no 1/sqrt(dh) in its attention, so at d >= 2048 the path LayerNorm ->
        Wq / Wk -> q / k -> logits carries 80 % of the 16-bit deviation from the fp32 reference.  None (default)
        = default_precise_qk(): ON for dtype 'f16' GPT-Neo models with hidden_size >= 2048 ('act+logits' at SGPT-1.3B shape,
        'qkv+logits' from SGPT-2.7B shape on -- the cheapest variants that keep two seeds of reference fixtures 25 % inside the bar), off elsewhere; False = off; True / 'full' = the Q / K projection over hi + lo pairs of both operands (+33 % FLOPs);
        'logits' = q / k / v / p as hi + lo pairs inside the attention only (no extra GEMM FLOPs); 'act+logits' = that plus the
        LayerNorm-1 output split against plain weights (+17 % FLOPs); 'full+logits'; 'qkv+logits' (the V projection split as
        well); 'attn' (the whole attention sub-block: Q / K / V projection, attention, out-projection)."""
        dtype, precise_qk, precision = check_args(cfg, dtype, precise_qk, precision)
        attention = check_attention(cfg, attention)
        projections = check_projections(cfg, dtype, projections)
        self.cfg = cfg
        self.ctx = ctx or get_context(device)
        self.device = self.ctx.device
        self.dtype = dtype
        self.row_tile = TOKEN_TILE if (dtype == "fp8mfma" or projections == "fp8") else None      # pack(): rows per layout tile (pad_rows)
        # token rows per sgpt_encode call: 131 072 = 6 / 12 / 24 full rounds of 256x256 tiles on 256 CUs for the 125M
        # projections (measured: 1000 TFLOP/s there, 864-890 at 49 k rows, 754 at 25 k); activations ~2.5 GB (125M) to
        # ~13 GB (bloom-7b1) of the 288 GB
        self.max_tokens_per_call = max_tokens_per_call
        desc, _local = model_desc(cfg, dtype, precise_qk, precision)     # (_local: the array desc.layer_is_local points to)
        self.precise_qk, self.precision = precise_qk, precision
        self.precision_report = None      # filled by the probe: crest factors [num_layers, 4] and what was decided
        self._att_ok = family(cfg.model_type).rotary_dim == "none" and head_dim(cfg) in (64, 128)   # split-precision attention: head_dim 64 / 128, no rotary
        self._plan_pending = precision in ("auto", "auto-class")
        keep = [(n.encode(), t.to(device=self.device, dtype=torch.float32).contiguous()) for n, t in load_tensors(cfg, weights)]   # H2D staging only
        views = (TensorView * len(keep))(*[TensorView(n, t.data_ptr(), t.numel()) for n, t in keep])
        self.handle = C.c_void_p()
        torch.cuda.synchronize(self.device)
        _lib.check(self.ctx.handle, self.ctx.lib.sgpt_model_load(self.ctx.handle, C.byref(desc), views, len(keep), C.byref(self.handle)),
                   "sgpt_model_load")
        del keep  # the library now owns packed copies
        self._attention = family(cfg.model_type).native_attention     # (a family without the switch runs its own mode whatever the default says)
        if family(cfg.model_type).attention_switch and attention != self._attention:
            self.set_attention(attention)
        self._projections, self.projection_bytes_freed = None, 0
        if projections == "fp8":
            freed = C.c_int64(0)
            self._call("set_projections", 1, C.byref(freed))
            self._projections, self.projection_bytes_freed = "fp8", int(freed.value)
        self._staging = _Staging(self.device)
        self.act_scales = None
        if dtype == "fp8mfma" and calibrate:
            self.calibrate()
        self.position_weights = None
        if "position_weights" in weights:
            self.set_position_weights(weights["position_weights"])
        if dtype in ("f16", "bf16"):
            base = self._base_plan()
            if precision == "x3":
                base = self._x3_plan()
            if base.any():
                self.set_precision_plan(base, _keep_pending=True)
            if self._plan_pending:
                S = min(64, cfg.max_position_embeddings)
                self._auto_precision(np.random.default_rng(4321).integers(0, cfg.vocab_size, size=(64, S), dtype=np.int64), None, final=False)

    @property
    def max_seq_len(self) -> int:
        """The longest sequence (tokens, framing included) this model encodes: min(cfg.max_position_embeddings, MAX_SEQ_LEN).  What
        the adapters default and clamp their max_seq_length to."""
        return table_rows(self.cfg)

    @property
    def attention(self) -> str:
        """'causal' | 'bidirectional': what every layer's attention shows a token."""
        return self._attention

    @property
    def projections(self) -> Optional[str]:
        """None | 'fp8': the arithmetic of the Q | K | V, gate | up and down projections (SGPTModel(projections=))."""
        return self._projections

    def set_attention(self, attention: str) -> None:
        """Switch a Llama-family model between causal and bidirectional attention (the library refuses the other families)."""
        if attention not in ("causal", "bidirectional"):
            raise ValueError(f"attention must be 'causal' or 'bidirectional', not {attention!r}")
        self._call("set_attention", 1 if attention == "causal" else 0)
        self._attention = attention

    def _call(self, fn: str, *args) -> None:
        """sgpt_model_<fn>(this model, *args); a failure raises with the library's message."""
        _lib.check(self.ctx.handle, getattr(self.ctx.lib, "sgpt_model_" + fn)(self.handle, *args), "sgpt_model_" + fn)

    # ---- precision plan (split-precision operand classes per block) ----
    def _base_plan(self) -> np.ndarray:
        """The structural part of the plan: precise_qk."""
        plan = np.zeros((self.cfg.num_layers, SGPT_PREC_CLASSES), dtype=np.int32)
        if self.precise_qk:
            ln1, att, ctx = PRECISE_QK_PLANS[self.precise_qk]
            if att and not self._att_ok:
                raise ValueError(f"precise_qk={self.precise_qk!r} needs head_dim 64 / 128 and no rotary embedding")
            plan[:, PC_LN1], plan[:, PC_ATT], plan[:, PC_CTX] = ln1, att, ctx
        return plan

    def _x3_plan(self) -> np.ndarray:
        plan = np.ones((self.cfg.num_layers, SGPT_PREC_CLASSES), dtype=np.int32)
        plan[:, PC_LN1] = 2
        if not self._att_ok:
            plan[:, PC_ATT] = 0        # GPT-J (rotary in place on 16-bit q / k; head_dim 256): q / k / v / p stay 16-bit
        return plan

    def precision_plan(self) -> np.ndarray:
        """int32[num_layers, 5]: per block (LayerNorm-1 -> Q/K/V: 0 | 1 q,k | 2 q,k,v | 3 q,k activation-only; attention; context ->
        out-projection; LayerNorm-2 -> fc1; GELU output -> fc2); non-zero = that operand class enters its MFMAs as hi + lo pairs."""
        out = np.zeros(self.cfg.num_layers * SGPT_PREC_CLASSES, dtype=np.int32)
        self._call("get_precision", out.ctypes.data_as(C.c_void_p), out.size)
        return out.reshape(self.cfg.num_layers, SGPT_PREC_CLASSES)

    def set_precision_plan(self, plan, _keep_pending: bool = False) -> None:
        """Install a plan (e.g. the one an earlier run's probe chose: reproducible embeddings across processes).  Ends the
        'auto' probe: the plan is the caller's now."""
        a = np.ascontiguousarray(np.asarray(plan, dtype=np.int32).reshape(-1))
        self._call("set_precision", a.ctypes.data_as(C.c_void_p), a.size)
        if not _keep_pending:
            self._plan_pending = False

    def probe_precision(self, seqs, pad_left=None) -> np.ndarray:
        """Crest factors float32[num_layers, 4] (LayerNorm-1 output, attention context, LayerNorm-2 output, GELU output) of a
        forward over `seqs` (at most PROBE_MAX_ROWS token rows are used)."""
        if self.dtype not in ("f16", "bf16"):
            raise ValueError("probe_precision applies to dtype 'f16' / 'bf16'")
        lens = np.fromiter(map(len, seqs), dtype=np.int64, count=len(seqs))
        alloc = np.cumsum((lens + ALIGN - 1) // ALIGN * ALIGN)
        n = max(1, int(np.searchsorted(alloc, PROBE_MAX_ROWS, side="right")))
        sub = [seqs[i][:PROBE_MAX_ROWS] for i in range(n)]
        pl = None if pad_left is None else [pad_left[i] for i in range(n)]
        out = (C.c_float * (4 * self.cfg.num_layers))()

        def once():
            self._call("precision_probe_begin")
            try:
                self.encode_packed(self.pack(sub, pl))
            finally:
                self._call("precision_probe_end", out)
        self.guarded(once)          # (an f16 range overflow inside the probe forward: shifts raised, probed again)
        return np.array(list(out), dtype=np.float32).reshape(self.cfg.num_layers, 4)

    def ensure_precision_plan(self, seqs, pad_left=None) -> None:
        """precision 'auto' / 'auto-class': run the probe on `seqs` if it has not run yet (every host entry point that takes
        token lists calls this first: encode_ids, token_embeddings, the cross-encoder, EncodeGraph; a caller that only ever
        uses pack() + encode_packed() calls it itself, or pins a plan with set_precision_plan())."""
        if self._plan_pending:
            self._auto_precision(seqs, pad_left)

    def release_split_weights(self) -> int:
        """Give the [W_hi | W_hi | W_lo] weight copies back to the device (3 x the 16-bit weight bytes on top of the plain copy:
        +0.5 GB at SGPT-125M, +35 GB at GPT-J-6B shape).  precision='auto' does this itself once its probe has settled on plain
        operands; afterwards a plan that needs the copies is refused loudly (load the model again with precision='x3').
        Returns the bytes freed (0 when the installed plan still reads them or nothing was held)."""
        plan = self.precision_plan()
        if plan[:, [PC_CTX, PC_LN2, PC_H]].any():
            return 0                       # (a LayerNorm-1 entry only reads the Q / K / V copy, which then stays)
        freed = C.c_int64(0)
        self._call("release_split_weights", C.byref(freed))
        return int(freed.value)

    def sync_precision(self, seqs, reduce, pad_left=None) -> None:
        """COLLECTIVE form of the first-call probe for multi-process runs: every rank of a sharded search holds
        a different query slice / corpus shard, so a per-process decision could settle rank A on plain operands and rank B on
        f16x3 -- embeddings of one search at two precisions, results depending on world size.  Every rank probes its own
        `seqs` (if its probe is still pending), the per-(block, class) flags go through `reduce` (elementwise max over the
        ranks: sgpt_amd.dist.max_reducer), and every rank installs the plan of the UNION.  Called by
        DenseRetrievalExactSearch.search before anything is encoded; all ranks must call it."""
        if self.precision not in ("auto", "auto-class") or self.dtype not in ("f16", "bf16"):
            return
        L = self.cfg.num_layers
        flags = np.zeros(L * 4 + 3, dtype=np.int32)
        crest = None
        if self._plan_pending:
            crest = self.probe_precision(seqs, pad_left)
            flags[: L * 4] = (crest > self._crest_limits()[None, :]).reshape(-1)
            flags[L * 4] = 1
        rep = self.precision_report or {}
        flags[L * 4 + 1] = 1 if rep.get("decided", "plain") != "plain" else 0   # already escalated here
        # a rank that settled on plain operands in an earlier call has given its [W_hi | W_hi | W_lo] copies back: it cannot follow
        # an escalation any more.  That must fail on EVERY rank: a one-sided exception would leave the others waiting
        # in the query all-gather.
        flags[L * 4 + 2] = 1 if (not self._plan_pending and rep.get("split_weight_bytes_released", 0) > 0) else 0
        tot = np.asarray(reduce(flags.copy()), dtype=np.int32)
        if tot[L * 4] == 0 and tot[L * 4 + 1] == flags[L * 4 + 1]:
            return                                     # nobody was pending, everybody agrees
        hot = tot[: L * 4].reshape(L, 4) > 0
        if tot[L * 4 + 1] and not hot.any():
            hot[:] = True                              # a rank that escalated earlier (its own data): the others follow it
        if hot.any() and tot[L * 4 + 2]:
            raise RuntimeError(
                f"sync_precision: the collective probe asks for split-precision operands ({int(hot.sum())} (block, class) flags over "
                f"the ranks), but {int(tot[L * 4 + 2])} rank(s) already settled on plain operands in an earlier call and released "
                "their split weight copies.  Raised on every rank.  Load the models with precision='x3' (or pin one plan with "
                "set_precision_plan() on every rank) before a multi-process search over this data.")
        self._install_from_flags(hot, crest, probed="first call (collective)")

    def _crest_limits(self) -> np.ndarray:
        return np.array([CREST_LIMIT_LN, CREST_LIMIT_LN, CREST_LIMIT_LN, CREST_LIMIT_H], dtype=np.float32)

    def _install_from_flags(self, hot: np.ndarray, crest, probed: str, final: bool = True) -> None:
        plan = self._base_plan()
        if hot.any():
            if self.precision == "auto":
                plan = self._x3_plan()
            else:
                plan[hot[:, 0], PC_LN1] = 2
                if self._att_ok:
                    plan[hot[:, 0], PC_ATT] = 1
                plan[hot[:, 1], PC_CTX] = 1
                plan[hot[:, 2], PC_LN2] = 1
                plan[hot[:, 3], PC_H] = 1
                if family(self.cfg.model_type).parallel_block:
                    plan[:, PC_LN2] = (plan[:, PC_LN1] != 0).astype(np.int32)
            self.set_precision_plan(plan)          # (ends the probing: an ill-conditioned checkpoint stays escalated)
        freed = 0
        if final:
            self._plan_pending = False
            if not hot.any():
                freed = self.release_split_weights()       # plain it is: the 3x copies go back
        self.precision_report = dict(crest=crest, limits=self._crest_limits().tolist(), flagged=int(hot.sum()), probed=probed,
                                     decided="x3" if (hot.any() and self.precision == "auto") else ("classes" if hot.any() else "plain"),
                                     split_weight_bytes_released=freed)

    def _auto_precision(self, seqs, pad_left, final: bool = True) -> None:
        """precision 'auto' / 'auto-class': probe, decide, install.  Runs twice at most: at load on 64 synthetic random-token
        sequences (outlier channels are a property of the checkpoint -- in real GPT-2 / GPT-Neo checkpoints the massive
        activations sit on the first position and on delimiter tokens, which any sequence has) and, if that found nothing, on
        the first real encode call (final=True: the plan is the caller's data's from then on)."""
        if final:
            self._plan_pending = False
        crest = self.probe_precision(seqs, pad_left)
        hot = crest > self._crest_limits()[None, :]       # [L, 4]: LN1, CTX, LN2, H
        self._install_from_flags(hot, crest, probed="first call" if final else "load (synthetic)", final=final or bool(hot.any()))

    def calibrate(self, seqs: Optional[Sequence[Sequence[int]]] = None, margin: float = 2.0) -> np.ndarray:
        """dtype='fp8mfma': fix the per-block power-of-two scales of the e4m3 codes of the GELU output and of the attention
        context from a calibration forward (run in the fp8-storage / bf16-arithmetic mode while the library records the two
        maxima per block).  Returns the 2 * num_layers scales (GELU outputs, then contexts).
        Default sample: 64 deterministic pseudo-random sequences of 64 tokens (reproducible embeddings); pass
        representative token lists to calibrate on real text.  `margin` = head-room factor over the sample's maximum."""
        if self.dtype != "fp8mfma":
            raise ValueError("calibrate() applies to dtype='fp8mfma'")
        if seqs is None:
            import warnings
            warnings.warn("dtype='fp8mfma': activation scales calibrated on 64 synthetic random-token sequences; pass representative "
                          "token lists to SGPTModel.calibrate() (a later batch that saturates the e4m3 range raises SgptRangeError)",
                          stacklevel=2)
            S = min(64, self.cfg.max_position_embeddings)
            seqs = np.random.default_rng(1234).integers(0, self.cfg.vocab_size, size=(64, S), dtype=np.int64)
        self._call("calibrate_begin")
        try:
            self.encode_ids(seqs)
        finally:
            out = (C.c_float * (2 * self.cfg.num_layers))()
            self._call("calibrate_end", float(margin), out)
        self.act_scales = np.array(list(out), dtype=np.float32)
        return self.act_scales

    def set_act_scales(self, scales) -> None:
        a = np.ascontiguousarray(scales, dtype=np.float32)
        self._call("set_act_scales", a.ctypes.data_as(C.c_void_p), a.size)
        self.act_scales = a

    def set_position_weights(self, w) -> None:
        """Trained `position_weights` of models/WeightedMeanPooling.py:16-19 for method 'learntmean'
        (the reference reads 1_WeightedMeanPooling/pytorch_model.bin, useb_dense_retriever.py:253-257)."""
        t = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w))
        t = t.detach().to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        self._call("set_pool_weights", _p(t), t.numel())
        self.position_weights = t

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.sgpt_model_free(self.handle)
            self.handle = None

    # ---- loading real checkpoints (HF folder / sentence-transformers folder layout) ----
    @classmethod
    def from_pretrained(cls, path: str, attention: Optional[str] = None, projections: Optional[str] = None, **kw) -> "SGPTModel":
        """Reads config.json + model.safetensors / pytorch_model.bin of an SGPT checkpoint folder
        (AutoModel.from_pretrained at beir_dense_retriever.py:123; ST folder layout
        SentenceTransformer.py:903-936 keeps the transformer either at the root or in 0_Transformer/).
        attention=None: 'bidirectional' iff config.json says `is_causal: false`, else 'causal' (families.attention_from_hf_dict)."""
        root = path
        if not os.path.exists(os.path.join(root, "config.json")) and os.path.exists(os.path.join(root, "0_Transformer")):
            root = os.path.join(root, "0_Transformer")
        with open(os.path.join(root, "config.json")) as f:
            raw = json.load(f)
        cfg = SGPTConfig.from_hf_dict(raw)
        model = cls(cfg, load_state_dict(root), attention=attention_from_hf_dict(raw, attention), projections=projections, **kw)
        wmp = os.path.join(path, "1_WeightedMeanPooling", "pytorch_model.bin")
        if os.path.exists(wmp):
            model.set_position_weights(torch.load(wmp, map_location="cpu", weights_only=True)["position_weights"])
        return model

    # ---- packing ----
    def pack(self, seqs: Sequence[Sequence[int]], pad_left: Optional[Sequence[int]] = None,
             bucket: Optional[Tuple[int, int, int]] = None, into: Optional[PackedBatch] = None, pool_from=None) -> PackedBatch:
        """Token lists -> device-resident packed batch: ONE pinned, non-blocking H2D copy of the whole layout.
        bucket: pad the layout to a capacity (pack_layout); into: refill that batch's device arena (same bucket) instead of
        allocating a new one -- the form hipGraph replays use, whose kernels hold the arena's addresses.
        pool_from: one int or one per sequence (pack_layout): the batch is pooled from that token on -- mean and weightedmean over the
        tokens behind it, lasttoken unchanged; it travels in the same arena and is refused with 'cls' / 'learntmean' by the encode calls."""
        lay = pack_layout(seqs, pad_left, bucket, self.row_tile, pool_from)
        # two refusals: the library's limit (SGPT_MAX_SEQ_LEN, include/sgpt_hip.h) and the model's own position range
        if int(lay["lens"][: lay["n_real"]].max()) > MAX_SEQ_LEN:
            raise ValueError(f"sequence longer than {MAX_SEQ_LEN} tokens, the longest the library encodes (SGPT_MAX_SEQ_LEN)")
        if lay["max_pos"] >= self.cfg.max_position_embeddings:
            raise ValueError("sequence longer than max_position_embeddings")
        n_int = arena_ints(lay)
        B, T = lay["B"], lay["T_pad"]
        if into is not None and (into.arena is None or (into.B, into.T_pad, into.max_alloc) != (B, T, lay["max_alloc"])):
            raise ValueError(f"packed layout {(B, T, lay['max_alloc'])} does not match the batch being refilled "
                             f"{(into.B, into.T_pad, into.max_alloc)}")
        if into is not None and (into.pool_lo is None) != (lay["pool_lo"] is None):
            raise ValueError("the batch being refilled was packed " + ("without" if into.pool_lo is None else "with") + " pool_from")
        slot, host = self._staging.acquire(n_int)
        hi, lo = fill_arena(seqs, lay, host.numpy())
        if lo < 0 or hi >= self.cfg.vocab_size:
            raise ValueError(f"token id out of range [0, {self.cfg.vocab_size})")
        dev = into.arena if into is not None else torch.empty(n_int, dtype=torch.int32, device=self.device)
        dev.copy_(host[:n_int], non_blocking=True)
        self._staging.release(slot)
        off_host = np.ascontiguousarray(lay["off"], dtype=np.int32)
        if into is not None:
            into.n_tokens, into.max_pos, into.n_real, into.off_host = lay["n_tokens"], lay["max_pos"], lay["n_real"], off_host
            return into
        o = 2 * T
        return PackedBatch(dev[:T], dev[T:o], dev[o: o + B + 1], dev[o + B + 1: o + 2 * B + 1],
                           dev[o + 2 * B + 1: o + 3 * B + 1], B, T, lay["max_alloc"], lay["n_tokens"], lay["max_pos"],
                           arena=dev, n_real=lay["n_real"], off_host=off_host,
                           pool_lo=None if lay["pool_lo"] is None else dev[o + 3 * B + 1: o + 4 * B + 1])

    # ---- one C call: forward + pool ----
    def encode_packed(self, pb: PackedBatch, mode: str = "weightedmean", normalize: bool = False,
                      layer_idx: int = -1, out: Optional[torch.Tensor] = None,
                      return_hidden: bool = False):
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode}")
        L = self.cfg.num_layers
        # hidden_states has L+1 entries: i<L = input of block i (no ln_f); L (== -1) = post ln_f
        li = layer_idx if layer_idx >= 0 else L + 1 + layer_idx
        if not 0 <= li <= L:
            raise ValueError(f"Layer Idx {layer_idx} is larger than the {L + 1} hidden states")
        n_run, final_ln = (L, 1) if li == L else (li, 0)
        self._check_learnt(mode, pb)
        self._check_pool_from(mode, pb)
        d = self.cfg.hidden_size
        if out is None:
            out = torch.empty((pb.B, d), dtype=torch.float32, device=self.device)
        hidden = torch.empty((pb.T_pad, d), dtype=torch.float32, device=self.device) if return_hidden else None
        off_host = pb.off_host.ctypes.data if pb.off_host is not None and pb.off_host.size == pb.B + 1 else None
        args = (self.handle, _p(pb.ids), _p(pb.pos), _p(pb.seq_off), _p(pb.seq_len), _p(pb.pad_left), pb.B, pb.T_pad, pb.max_alloc,
                POOL_MODES[mode], n_run, final_ln, 1 if normalize else 0, _p(out), _p(hidden), off_host)
        if pb.pool_lo is None:
            st = self.ctx.lib.sgpt_encode_host_layout(*args, _stream_ptr(self.device))
        else:
            st = self.ctx.lib.sgpt_encode_pool_from(*args, _p(pb.pool_lo), _stream_ptr(self.device))
        _lib.check(self.ctx.handle, st, "sgpt_encode")
        return (out, hidden) if return_hidden else out

    @staticmethod
    def _check_pool_from(mode: str, pb: PackedBatch) -> None:
        if pb.pool_lo is not None and mode in ("cls", "learntmean"):
            raise ValueError(f"pool_from (pooling the tokens behind a prompt) serves 'mean', 'weightedmean' and 'lasttoken', not {mode!r}")

    def _check_learnt(self, mode: str, pb: PackedBatch) -> None:
        if mode != "learntmean":
            return
        if not family(self.cfg.model_type).sgpt_modes:
            raise ValueError("method 'learntmean' (trained position weights of the SGPT checkpoints) is not available for BERT / Llama models")
        if self.position_weights is None:
            raise ValueError("method 'learntmean' needs trained position weights (1_WeightedMeanPooling)")
        if pb.max_pos >= self.position_weights.numel():
            raise ValueError("fewer learnt position weights than the longest padded sequence")

    def encode_packed_layers(self, pb: PackedBatch, mode: str = "mean", normalize: bool = False,
                             per_layer: bool = False):
        """All L+1 hidden states pooled in ONE forward (the `meanmean` / `lasttokenmean` loops of
        beir_dense_retriever.py:243-257, 284-301).  -> fp32[B, d] layer average, or with per_layer=True
        (fp32[L+1, B, d], fp32[B, d])."""
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode}")
        self._check_learnt(mode, pb)
        self._check_pool_from(mode, pb)
        d, L1 = self.cfg.hidden_size, self.cfg.num_layers + 1
        layers = torch.empty((L1, pb.B, d), dtype=torch.float32, device=self.device) if per_layer else None
        mean = torch.empty((pb.B, d), dtype=torch.float32, device=self.device)
        args = (self.handle, _p(pb.ids), _p(pb.pos), _p(pb.seq_off), _p(pb.seq_len), _p(pb.pad_left), pb.B, pb.T_pad, pb.max_alloc,
                POOL_MODES[mode], 1 if normalize else 0, _p(layers), _p(mean))
        if pb.pool_lo is None:
            st = self.ctx.lib.sgpt_encode_layers(*args, _stream_ptr(self.device))
        else:
            st = self.ctx.lib.sgpt_encode_layers_pool_from(*args, _p(pb.pool_lo), _stream_ptr(self.device))
        _lib.check(self.ctx.handle, st, "sgpt_encode_layers")
        return (layers, mean) if per_layer else mean

    def lm_logprobs(self, hidden: torch.Tensor, row_idx, targets, return_greedy: bool = False):
        """log P(targets[i] | prefix ending at token row row_idx[i]) from post-ln_f hidden states [T_pad, d]
        (the log_softmax + gather of crossencoder/beir/sgptce.py:233-255) -> fp32[n] on the GPU.
        The arguments are checked here, on the host, before anything is uploaded: the C entry has no row count of `hidden` and
        its gather does not clamp (include/sgpt_hip.h::sgpt_lm_logprobs)."""
        if refusal := family(self.cfg.model_type).no_lm_head:
            raise ValueError(refusal)
        if not isinstance(hidden, torch.Tensor) or hidden.dtype != torch.float32 or hidden.dim() != 2:
            raise ValueError("lm_logprobs: hidden must be an fp32 tensor [T_pad, d_model]")
        if hidden.device != self.device:
            raise ValueError(f"lm_logprobs: hidden is on {hidden.device}, the model on {self.device}")
        if hidden.shape[1] != self.cfg.hidden_size:
            raise ValueError(f"lm_logprobs: hidden has width {hidden.shape[1]}, d_model is {self.cfg.hidden_size}")
        ri_host, tg_host = np.asarray(row_idx, dtype=np.int64).reshape(-1), np.asarray(targets, dtype=np.int64).reshape(-1)
        if ri_host.size == 0:
            raise ValueError("lm_logprobs: row_idx is empty")
        if tg_host.size != ri_host.size:
            raise ValueError(f"lm_logprobs: targets has {tg_host.size} entries, row_idx {ri_host.size}")
        if int(ri_host.min()) < 0 or int(ri_host.max()) >= hidden.shape[0]:
            raise ValueError(f"lm_logprobs: row_idx outside [0, {hidden.shape[0]}), the rows of hidden")
        ri = torch.from_numpy(ri_host.astype(np.int32)).to(self.device)
        tg = torch.from_numpy(tg_host.astype(np.int32)).to(self.device)
        n = int(ri.numel())
        out = torch.empty((n,), dtype=torch.float32, device=self.device)
        greedy = torch.empty((n,), dtype=torch.int32, device=self.device) if return_greedy else None
        hidden = hidden.contiguous()
        st = self.ctx.lib.sgpt_lm_logprobs(self.handle, _p(hidden), _p(ri), _p(tg), n, _p(out), _p(greedy),
                                           _stream_ptr(self.device))
        _lib.check(self.ctx.handle, st, "sgpt_lm_logprobs")
        return (out, greedy) if return_greedy else out

    def _num_cus(self) -> int:
        try:
            return int(torch.cuda.get_device_properties(self.device).multi_processor_count) // 8 * 8 or 256
        except Exception:      # noqa: BLE001 -- host-only callers (tests of the planner)
            return 256

    def call_budgets(self, total_rows: int, ncu: Optional[int] = None) -> List[int]:
        """Token-row budgets of the sgpt_encode calls that cover `total_rows` packed rows (round 5).
        The persistent 256x256 GEMM runs `ceil(MT * NT / CUs)` rounds of tiles per launch (MT = rows / 256, NT = N / 256): a call
        whose tile counts stop just past a multiple of the CU count pays a whole extra round on every launch of every block -- three
        equal calls of 99 k rows (a 4096-document step of U{16..128}-token documents, 298 k rows) run 4.55 / 13.6 / 18.2 rounds:
        9 % / 3 % / 4 % idle.  Budgets are chosen from the sizes whose N = d launches end on a round boundary
        (MT = floor(j * CUs / (d / 256)): 85, 170, 256, 341, 426, 512 row tiles at d = 768 on 256 CUs -- the wider launches are
        multiples of that one) by a small search that minimises the modelled rounds x K of the four projections plus a term linear
        in rows (LayerNorm / attention / epilogue bytes); the call count stays at ceil(total / max_tokens_per_call) or one more.
        The one call whose size is not a round boundary (it takes what the others leave) comes LAST: plan_batches() cuts a call
        at the last whole sequence inside its budget, and what those cuts leave over lands in that call, not in an extra one.
        Pure function of (total_rows, model shape, CU count): every rank computes the same plan."""
        ncu = ncu or self._num_cus()
        d, ffn = self.cfg.hidden_size, self.cfg.intermediate_size
        nt_d = max(1, d // TOKEN_TILE)
        mt_max = max(1, self.max_tokens_per_call // TOKEN_TILE)
        mt_tot = -(-int(total_rows) // TOKEN_TILE)
        if mt_tot <= mt_max:
            return [mt_tot * TOKEN_TILE]
        launches = [(3 * d // TOKEN_TILE, d), (nt_d, d), (max(1, ffn // TOKEN_TILE), d), (nt_d, ffn)]     # (column tiles, K): QKV, out, fc1, fc2
        per_row = 0.35 * sum(nt * k for nt, k in launches) / ncu        # HBM-bound phases: ~35 % of a full call's GEMM time at d = 768

        def cost(mt):
            return sum(-(-mt * nt // ncu) * k for nt, k in launches) + per_row * mt

        good = sorted({min(mt_max, j * ncu // nt_d) for j in range(1, mt_max * nt_d // ncu + 2)} | {mt_max})
        good = [g for g in good if g >= 1]
        n_min = -(-mt_tot // mt_max)
        best, cands = None, []
        # all calls but the last three at the maximum (a whole number of rounds by construction when mt_max is a good size);
        # the last <= 3 (or 4) are searched: good sizes for all but one, which takes what is left
        for n_calls in (n_min, n_min + 1):
            n_free = min(n_calls, 3 if n_calls == n_min else 4)
            fixed = n_calls - n_free
            rem = mt_tot - fixed * mt_max
            if rem <= 0:
                continue
            for combo in itertools.combinations_with_replacement(good, n_free - 1):
                last = rem - sum(combo)
                if last <= 0 or last > mt_max:
                    continue
                c = fixed * cost(mt_max) + sum(cost(g) for g in combo) + cost(last)
                cands.append((c, [mt_max] * fixed + sorted(combo, reverse=True) + [last]))      # the free call goes last
        if cands:
            # plans within 0.3 % of the cheapest are equal as far as the model can tell: take the most balanced one (a short
            # last call runs its few rounds at a lower rate than the model's per-round cost -- ramp and tail of every launch)
            c_min = min(c for c, _ in cands)
            best = max((pl for c, pl in cands if c <= c_min * 1.003), key=lambda pl: (min(pl), -len(pl)))
        if best is None:
            best = [mt_max] * (n_min - 1) + [mt_tot - (n_min - 1) * mt_max]
        return [b * TOKEN_TILE for b in best]

    def plan_batches(self, lens: np.ndarray, max_sentences: Optional[int] = None) -> List[np.ndarray]:
        """Length-sorted (longest first, SentenceTransformer.py:148-149 / exact_search.py:66-71)
        contiguous slices bounded by a token budget instead of a padded [B,S] rectangle."""
        order = np.argsort(-lens, kind="stable")
        alloc = (lens[order] + ALIGN - 1) // ALIGN * ALIGN
        # Budgets per call from call_budgets(): sizes whose GEMM launches end on whole rounds of the chip (round 4 cut equal
        # budgets -- better than 131 k + 131 k + 32 k, but a 99 k-row call idles 3-9 % of every launch in its last round).
        # A call is cut at the last whole sequence inside its budget, so it leaves up to one sequence over: the plan is taken
        # again over the rows still to go at every cut (round 6, ADVICE r05: with one plan for the whole list the leftovers of
        # 4096 documents of U{16..128} tokens ended in an 80-row fourth call -- a whole pass through the layers for 80 rows).
        total = int(alloc.sum())
        round_aware = getattr(self, "round_aware_calls", True)
        if not round_aware:       # round 4's rule (A/B: bench.py --equal-calls): equal budgets, a multiple of the GEMM's token tile
            n_calls = max(1, -(-total // self.max_tokens_per_call))
            equal = min(self.max_tokens_per_call, (-(-total // n_calls) + TOKEN_TILE - 1) // TOKEN_TILE * TOKEN_TILE + int(alloc.max()))

        def budget_for(remaining: int) -> int:
            if not round_aware:
                return equal
            b = self.call_budgets(remaining)
            return self.max_tokens_per_call if len(b) == 1 else min(self.max_tokens_per_call, b[0])
        out, start, tok, done = [], 0, 0, 0
        budget = budget_for(total)
        for i, a in enumerate(alloc):
            full = tok + a > budget or (max_sentences and i - start >= max_sentences)
            if full and i > start:
                out.append(order[start:i])
                done += tok
                start, tok = i, 0
                budget = budget_for(total - done)
            tok += int(a)
        out.append(order[start:])
        return out

    # ---- range guards (per model: a flag raised here is never blamed on another model of the same context) ----
    def range_flags(self, reset: bool = True) -> int:
        """The model's guard word since the last reset (syncs the stream; include/sgpt_hip.h::sgpt_model_range_check):
        bit 0 = an f16 activation reached |v| >= 32768, bit 1 / 2 = an fp8mfma GELU output / attention context saturated."""
        flagged = C.c_int32(0)
        self._call("range_check", C.byref(flagged), 1 if reset else 0, _stream_ptr(self.device))
        return int(flagged.value)

    def range_shifts(self) -> np.ndarray:
        """dtype='f16': the power-of-two down-shifts per block, int32[num_layers, 4] = (LayerNorm-1 output, q | k | v,
        LayerNorm-2 output, GELU output).  All zero for a checkpoint whose activations stay inside the half range."""
        out = np.zeros(self.cfg.num_layers * 4, dtype=np.int32)
        self._call("get_range_shifts", out.ctypes.data_as(C.c_void_p), out.size)
        return out.reshape(self.cfg.num_layers, 4)

    def set_range_shifts(self, shifts) -> None:
        """Pin the shifts found on an earlier run (reproducible embeddings across processes)."""
        a = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32).reshape(-1))
        self._call("set_range_shifts", a.ctypes.data_as(C.c_void_p), a.size)

    def _adapt_range(self) -> bool:
        """dtype='f16', after a flagged call: raise the shifts of the classes that overflowed.  True = re-run the call."""
        n = C.c_int32(0)
        self._call("range_adapt", C.byref(n), _stream_ptr(self.device))
        return n.value > 0

    def check_range(self, adapt: bool = False) -> bool:
        """Fail loudly if a call since the last check left a format's range.  adapt=True (dtype='f16'): instead of raising,
        raise the range shifts of the operand classes that overflowed and return True -- the caller re-runs its calls
        (their results were not trustworthy); encode_ids / token_embeddings / the cross-encoder do exactly that."""
        if self.dtype not in ("f16", "fp8mfma"):
            return False
        flags = self.range_flags(reset=False)
        if not flags:
            return False
        # (BERT models run without range shifts: nothing to adapt, the flag is final)
        if flags & 1 and not flags & 6 and adapt and self.dtype == "f16" and family(self.cfg.model_type).sgpt_modes and self._adapt_range():
            return True                      # (sgpt_model_range_adapt cleared bit 0 and the recorded magnitudes)
        self.range_flags(reset=True)
        if flags & 2:
            raise SgptRangeError("dtype='fp8mfma': a GELU output saturated its e4m3 codes; re-run calibrate() on "
                                 "representative inputs (or with a larger margin)")
        if flags & 4:
            raise SgptRangeError("dtype='fp8mfma': an attention context saturated its e4m3 codes; re-run calibrate() on "
                                 "representative inputs (or with a larger margin)")
        raise SgptRangeError("dtype='f16': an activation reached |v| >= 32768 (IEEE-half range)" +
                             (" and no range shift covers it; this checkpoint needs dtype='bf16'" if adapt else
                              "; re-run the call under SGPTModel.guarded / check_range(adapt=True)"))

    _check_range = check_range      # (name used before ABI v5)

    def guarded(self, fn):
        """Run `fn()` (a function that issues encode calls and returns their result) under the range guard: when an f16
        activation class overflowed, its shift is raised and fn runs again with the new factors (at most a few rounds: a
        round fixes every class that overflowed in it; a class pushed over the limit by an earlier fix is caught next)."""
        for _ in range(8):
            out = fn()
            if not self.check_range(adapt=True):
                return out
        raise SgptRangeError("dtype='f16': the range shifts did not converge; this checkpoint needs dtype='bf16'")

    def _batched(self, seqs, pad_left, run, pool_from=None) -> torch.Tensor:
        """Length-sorted token-budget batches -> `run(pb, out_rows)` per batch -> rows back in input order."""
        n = len(seqs)
        d = self.cfg.hidden_size
        if n == 0:
            return torch.empty((0, d), dtype=torch.float32, device=self.device)
        lens = np.fromiter(map(len, seqs), dtype=np.int64, count=n)
        if (lens <= 0).any():
            raise ValueError("Empty items should be cleaned prior to running")
        self.ensure_precision_plan(seqs, pad_left)
        if pool_from is not None and np.ndim(pool_from) == 1 and len(pool_from) != n:
            raise ValueError("pool_from: one int, or one int per sequence")
        return self.guarded(lambda: self._batched_once(seqs, pad_left, run, lens, pool_from))

    def _batched_once(self, seqs, pad_left, run, lens, pool_from=None) -> torch.Tensor:
        n, d = len(seqs), self.cfg.hidden_size
        # everything fits one call: the packed layout has no padding to the longest sequence, so the length sort of the
        # reference (SentenceTransformer.py:148-149) buys nothing -- pack in input order, no un-sort pass
        alloc_total = int(((lens + ALIGN - 1) // ALIGN * ALIGN).sum())
        if alloc_total <= self.max_tokens_per_call:
            res = torch.empty((n, d), dtype=torch.float32, device=self.device)
            run(self.pack(seqs, pad_left, pool_from=pool_from), res)
            return res
        plan = self.plan_batches(lens)
        sorted_rows = torch.empty((n, d), dtype=torch.float32, device=self.device)
        o = 0
        for sel in plan:
            pb = self.pack([seqs[i] for i in sel], None if pad_left is None else [pad_left[i] for i in sel],
                           pool_from=pool_from if pool_from is None or np.ndim(pool_from) == 0 else [pool_from[i] for i in sel])
            run(pb, sorted_rows[o: o + pb.B])
            o += pb.B
        order = torch.from_numpy(np.concatenate(plan)).pin_memory().to(self.device, non_blocking=True)
        res = torch.empty_like(sorted_rows)
        res[order] = sorted_rows                                   # un-sort (SentenceTransformer.py:205), one pass
        return res

    def encode_ids_all_layers(self, seqs: Sequence[Sequence[int]], mode: str = "mean",
                              pad_left: Optional[Sequence[int]] = None, pool_from=None) -> torch.Tensor:
        """n token lists -> fp32[n,d]: the per-layer pooled vectors of all L+1 hidden states, averaged
        (`meanmean` with mode='mean', `lasttokenmean` with mode='lasttoken'), one forward per batch.  pool_from: as encode_ids."""
        return self._batched(seqs, pad_left, lambda pb, out: out.copy_(self.encode_packed_layers(pb, mode)), pool_from)

    def encode_ids(self, seqs: Sequence[Sequence[int]], mode: str = "weightedmean", normalize: bool = False,
                   layer_idx: int = -1, pad_left: Optional[Sequence[int]] = None,
                   out_dtype=torch.float32, pool_from=None) -> torch.Tensor:
        """n token lists -> fp32[n,d] embeddings on the GPU, row-aligned with the input order.
        pool_from: one int or one per sequence -- pool from that token on (counted from the sequence start, frame included): the tokens
        of an instruction prompt in front are encoded, not pooled (pack())."""
        return self._batched(seqs, pad_left, lambda pb, out: self.encode_packed(pb, mode, normalize, layer_idx, out=out), pool_from)

    def token_embeddings(self, seqs: Sequence[Sequence[int]], layer_idx: int = -1,
                         pad_left: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """output_value='token_embeddings' (SentenceTransformer.py:233-241): per-sentence [len,d].  Batched by the
        same token budget as encode_ids, so the fp32 [T_pad, d] hidden buffer stays bounded."""
        n = len(seqs)
        lens = np.fromiter(map(len, seqs), dtype=np.int64, count=n)
        if n == 0 or (lens <= 0).any():
            raise ValueError("Empty items should be cleaned prior to running")
        self.ensure_precision_plan(seqs, pad_left)

        def once():
            out: List[Optional[torch.Tensor]] = [None] * n
            for sel in self.plan_batches(lens):
                sub = [seqs[i] for i in sel]
                pb = self.pack(sub, None if pad_left is None else [pad_left[i] for i in sel])
                _, hid = self.encode_packed(pb, layer_idx=layer_idx, return_hidden=True)
                off = pb.seq_off.cpu().tolist()
                for j, i in enumerate(sel.tolist()):
                    out[i] = hid[off[j]: off[j] + len(sub[j])].clone()
            return out
        return self.guarded(once)


class EncodeGraph:
    """One sgpt_encode call captured as a hipGraph (via torch.cuda.CUDAGraph: every kernel and memset of the call
    is issued on the capturing stream, nothing else) and replayed for new token ids: of the same packed layout
    (B, T_pad, max_alloc), or -- with bucket=(B_cap, T_cap, A_cap) -- of any batch that fits that capacity (padded with
    one-token filler sequences whose output rows are dropped, pack_layout).  Replay refills the captured token arena with
    one pinned copy.  The workspace is sized by a warm-up call before capture (hipMalloc is not capturable).
    What it buys, measured on MI355X: host time only.  A 12-block forward is 63 launches on the query-sized kernels (round 6;
    ~110 before); eager, the host enqueues them faster than the GPU retires them (one query: 0.42 ms of GPU time, launch gaps
    of 0.04 us in the kernel trace), so GPU time is unchanged by replay (round 3, 32 queries: 1.579 ms eager, 1.586 ms replay).
    Use it when the host thread is the scarce resource (many models / streams driven from one Python thread); the GPU-side
    latency of small batches is addressed in the kernels (csrc/qgemm.hip)."""

    def __init__(self, model: "SGPTModel", seqs: Sequence[Sequence[int]], mode: str = "weightedmean",
                 normalize: bool = False, layer_idx: int = -1, pad_left: Optional[Sequence[int]] = None,
                 bucket: Optional[Tuple[int, int, int]] = None, pool_from=None):
        # (out of scope, refused loudly: a captured graph of the bidirectional mode or of a ranged pool has not been built or tested)
        if family(model.cfg.model_type).attention_switch and getattr(model, "attention", "causal") != "causal":
            raise ValueError("EncodeGraph: a model with attention='bidirectional' is not captured (encode it eagerly: encode_ids / encode_packed)")
        if getattr(model, "projections", None) is not None:
            raise ValueError("EncodeGraph: a model with projections='fp8' is not captured (encode it eagerly: encode_ids / encode_packed)")
        if pool_from is not None:
            raise ValueError("EncodeGraph: pool_from is not captured (encode eagerly: encode_ids(pool_from=) / pack(pool_from=))")
        self.model, self.mode, self.normalize, self.layer_idx = model, mode, normalize, layer_idx
        model.ensure_precision_plan(seqs, pad_left)        # (a later plan change would only force a re-capture)
        self.capacity = bucket               # None: exact layouts only; else batches are padded to this capacity
        self.pb = model.pack(seqs, pad_left, bucket)
        self.out = torch.empty((self.pb.B, model.cfg.hidden_size), dtype=torch.float32, device=model.device)
        self._capture()

    def _capture(self):
        """(Re-)capture.  The captured kernels hold raw pointers into the context's grow-only workspace and the model's
        learnt-pooling table; `generation` moves whenever the library re-allocates one of them (a larger eager call on
        the same context, set_position_weights), and replay() re-captures instead of launching into freed memory."""
        m = self.model
        m.encode_packed(self.pb, self.mode, self.normalize, self.layer_idx, out=self.out)   # sizes the workspace: hipMalloc is not capturable
        torch.cuda.synchronize(m.device)
        self.generation = m.ctx.generation()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            m.encode_packed(self.pb, self.mode, self.normalize, self.layer_idx, out=self.out)

    @property
    def bucket(self):
        return (self.pb.B, self.pb.T_pad, self.pb.max_alloc)

    def replay(self, seqs: Optional[Sequence[Sequence[int]]] = None,
               pad_left: Optional[Sequence[int]] = None, check_range: bool = True) -> torch.Tensor:
        """Re-run on new sentences whose packed layout falls in the same bucket (None: same inputs again).
        The returned tensor is the graph's static output buffer (rows past `pb.n_real` belong to bucket fillers).
        check_range=True (default: never silent) reads the model's 4-byte guard word back after the replay -- one stream
        synchronisation per call; a latency path that needs replay() to stay ASYNCHRONOUS passes check_range=False and owes a
        `model.check_range()` before trusting the rows (dtype 'f16' / 'fp8mfma'; other dtypes never synchronise here)."""
        if seqs is not None:
            try:
                self.model.pack(seqs, pad_left, self.capacity, into=self.pb)   # one pinned copy into the captured arena
            except ValueError as e:
                raise ValueError(f"{e}: not this graph's bucket {self.bucket}") from None
            self.model._check_learnt(self.mode, self.pb)
        for _ in range(8):
            if self.model.ctx.generation() != self.generation:
                self._capture()                  # the workspace / pooling table / range shifts moved since capture
            self.graph.replay()
            # range guard (a 4-byte read-back: syncs).  check_range=False keeps replay() asynchronous; the caller then owes
            # a model.check_range() before trusting the rows.  An f16 overflow raises the shifts (-> generation moves ->
            # re-capture) and the replay runs again.
            if not check_range or not self.model.check_range(adapt=True):
                return self.out
        raise SgptRangeError("dtype='f16': the range shifts did not converge; this checkpoint needs dtype='bf16'")


def load_state_dict(root: str) -> Dict[str, torch.Tensor]:
    """HF checkpoint folder -> state dict: model.safetensors / pytorch_model.bin, or the sharded forms large checkpoints
    (sgpt-bloom-7b1, SGPT-5.8B) are saved in (`*.index.json` + `model-0000x-of-0000N.safetensors` /
    `pytorch_model-0000x-of-0000N.bin`).  Pickle files are read with weights_only=True (no code execution)."""
    def read(path):
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            return load_file(path)
        return torch.load(path, map_location="cpu", weights_only=True)
    for single in ("model.safetensors", "pytorch_model.bin"):
        if os.path.exists(os.path.join(root, single)):
            return read(os.path.join(root, single))
    for index in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
        ip = os.path.join(root, index)
        if os.path.exists(ip):
            with open(ip) as f:
                shards = sorted(set(json.load(f)["weight_map"].values()))
            sd: Dict[str, torch.Tensor] = {}
            for sh in shards:
                sd.update(read(os.path.join(root, sh)))
            return sd
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin (single or sharded) under {root}")
