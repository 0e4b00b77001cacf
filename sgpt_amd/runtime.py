"""Thin Python host over the C ABI: a `Context` per GPU.  PyTorch is used only to own device
memory (torch.empty / .data_ptr()) and to name the current HIP stream -- every computation is
a call into libsgpt_hip.so.  No torch compute op stands in for a kernel here."""
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import SGPT_BF16, SGPT_F16, SGPT_F32, POOL_MODES
from .corpus import CORPUS_KINDS, RESCORE_MODES, BinaryCorpus, CorpusBuilders, IVFCorpus, IVFUint8Corpus, QuantizedCorpus, Uint8Corpus, _no_rescore  # noqa: F401  (re-exported)

# torch dtype <-> element-type code of include/sgpt_hip.h
DT_CODE = {torch.float32: SGPT_F32, torch.bfloat16: SGPT_BF16, torch.float16: SGPT_F16}


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


_contexts = {}


def get_context(device=None) -> "Context":
    """One Context per HIP device per process (one process per GPU in multi-GPU runs)."""
    if not torch.cuda.is_available():
        raise _lib.SgptHipError("no HIP device visible: sgpt_amd runs its hot path only as gfx950 kernels "
                                "(there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SgptHipError(f"sgpt_amd needs a HIP device, got {dev}")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _contexts:
        _contexts[idx] = Context(idx)
    return _contexts[idx]


class Context(CorpusBuilders):
    """(The corpus builders and the row conversions under them -- quantize_corpus, scalar_quantize_corpus, binarize_corpus, ivf_index, u8_*,
    pack_sign_bits, rescore_u8, gather_rows, gather_quantize_rows -- are inherited from corpus.py.)"""

    def __init__(self, device_index: int):
        self.lib = _lib.load()
        self.device = torch.device("cuda", device_index)
        h = C.c_void_p()
        st = self.lib.sgpt_ctx_create(device_index, C.byref(h))
        if st != 0:
            raise _lib.SgptHipError(f"sgpt_ctx_create(device={device_index}) failed with status {st}")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sgpt_ctx_destroy(self.handle)
            self.handle = None

    def _chk(self, st, what):
        _lib.check(self.handle, st, what)

    # ---- helpers ----
    def _dev_f32(self, a) -> torch.Tensor:
        """Tensor / ndarray / list -> contiguous fp32 tensor on this device (the coercions of
        util.cos_sim, sentence_transformers/util.py:29-39)."""
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.asarray(a))
        if a.dim() == 1:
            a = a.unsqueeze(0)
        return a.to(device=self.device, dtype=torch.float32).contiguous()

    def _run_list(self, run, nq: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """The running list of a score + top-k call, (values fp32 [nq, k], indices int64 [nq, k], entries so far): the caller's `run`,
        or a fresh one."""
        if run is not None:
            return run
        return (torch.empty((nq, k), dtype=torch.float32, device=self.device),
                torch.empty((nq, k), dtype=torch.int64, device=self.device), 0)

    def _u8_operands(self, corpus: Uint8Corpus) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(codes, start, step) of a Uint8Corpus as the C entries take them: on this device, contiguous, the ranges fp32."""
        return (corpus.codes.to(self.device).contiguous(), corpus.start.to(device=self.device, dtype=torch.float32).contiguous(),
                corpus.step.to(device=self.device, dtype=torch.float32).contiguous())

    # ---- a4: stand-alone pooling ----
    def pool(self, hidden: torch.Tensor, mask: torch.Tensor, mode: str = "weightedmean",
             position_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mode 'learntmean' takes `position_weights` (WeightedMeanPooling.py:21-39), indexed by the padded position; 'cls' is
        row 0 of every sequence, whatever the mask (Pooling.py:103-105)."""
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode}")
        hidden = hidden.to(self.device)
        if hidden.dtype not in DT_CODE:
            hidden = hidden.float()
        hidden = hidden.contiguous()
        B, S, d = hidden.shape
        m = mask.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty((B, d), dtype=torch.float32, device=self.device)
        dt = DT_CODE[hidden.dtype]
        if mode == "learntmean":
            if position_weights is None or position_weights.numel() < S:
                raise ValueError("learntmean needs position_weights covering the sequence length")
            pw = position_weights.to(device=self.device, dtype=torch.float32).contiguous()
            self._chk(self.lib.sgpt_pool_learnt(self.handle, _p(hidden), dt, _p(m), B, S, d, _p(pw), _p(out),
                                                _stream_ptr(self.device)), "sgpt_pool_learnt")
            return out
        self._chk(self.lib.sgpt_pool(self.handle, _p(hidden), dt, _p(m), B, S, d, POOL_MODES[mode], _p(out),
                                     _stream_ptr(self.device)), "sgpt_pool")
        return out

    # ---- normalise / convert ----
    def l2_normalize(self, x: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
        x = self._dev_f32(x)
        n, d = x.shape
        out = torch.empty((n, d), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_l2_normalize(self.handle, _p(x), n, d, _p(out), DT_CODE[out_dtype],
                                             _stream_ptr(self.device)), "sgpt_l2_normalize")
        return out

    def pairwise_scores(self, a: torch.Tensor, b: torch.Tensor, cosine: bool) -> torch.Tensor:
        """out[i] = dot(a[i], b[i]) (cosine: of the L2-normalised rows): include/sgpt_hip.h::sgpt_pairwise_scores."""
        a, b = self._dev_f32(a), self._dev_f32(b)
        if a.shape != b.shape or a.dim() != 2:
            raise ValueError(f"pairwise scores need two [n, d] matrices of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        n, d = a.shape
        out = torch.empty((n,), dtype=torch.float32, device=self.device)
        if n:
            self._chk(self.lib.sgpt_pairwise_scores(self.handle, _p(a), _p(b), n, d, 1 if cosine else 0, _p(out),
                                                    _stream_ptr(self.device)), "sgpt_pairwise_scores")
        return out

    def to_16(self, x: torch.Tensor, dtype=torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 -> bf16 / f16 (RNE) on the device: the scorer's 16-bit operand format."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty(x.shape, dtype=dtype, device=self.device)
        self._chk(self.lib.sgpt_f32_to_16(self.handle, _p(x), x.numel(), _p(out), DT_CODE[dtype],
                                          _stream_ptr(self.device)), "sgpt_f32_to_16")
        return out

    def row_crest(self, x: torch.Tensor) -> float:
        """max over the rows of max|v| / rms(v) (include/sgpt_hip.h::sgpt_row_crest; fp32 rows are rounded to f16 first).
        ~3.5-5 for well-spread embedding rows, ~sqrt(d / 2) when two channels carry the row.  Syncs the stream."""
        if x.dtype not in (torch.float16, torch.bfloat16):
            x = self.to_16(self._dev_f32(x), torch.float16)
        x = x.to(self.device).contiguous()
        n, d = x.shape
        out = C.c_float(0)
        self._chk(self.lib.sgpt_row_crest(self.handle, _p(x), DT_CODE[x.dtype], n, d, d, C.byref(out),
                                          _stream_ptr(self.device)), "sgpt_row_crest")
        return float(out.value)

    def split16(self, x: torch.Tensor, role: str, dtype=torch.float16) -> torch.Tensor:
        """fp32 rows [n, d] -> split-precision 16-bit rows [n, 3 d] for the scorer (include/sgpt_hip.h::sgpt_split16):
        role 'doc' = [hi | lo | hi], role 'query' = [hi | hi | lo]; `scores` / `score_topk` over the 3 d columns then give
        q_hi.c_hi + q_hi.c_lo + q_lo.c_hi -- cosine scores to ~1e-6 on the 16-bit scorer kernels, for embeddings that a few
        channels dominate (the plain 16-bit corpus format alone costs those up to 4e-4)."""
        if role not in ("doc", "query"):
            raise ValueError("role must be 'doc' or 'query'")
        x = self._dev_f32(x)
        n, d = x.shape
        out = torch.empty((n, 3 * d), dtype=dtype, device=self.device)
        self._chk(self.lib.sgpt_split16(self.handle, _p(x), n, d, 0 if role == "doc" else 1, _p(out), DT_CODE[dtype],
                                        _stream_ptr(self.device)), "sgpt_split16")
        return out

    def to_bf16(self, x: torch.Tensor) -> torch.Tensor:
        return self.to_16(x, torch.bfloat16)

    def range_check(self, reset: bool = True) -> int:
        """Range guard of the ctx-level stand-alone ops (`linear` with f16 output; syncs the stream): bit 0 = an f16 value
        left the half range since the last reset.  Models carry their own guard word (SGPTModel.check_range)."""
        flagged = C.c_int32(0)
        self._chk(self.lib.sgpt_range_check(self.handle, C.byref(flagged), 1 if reset else 0, _stream_ptr(self.device)),
                  "sgpt_range_check")
        return int(flagged.value)

    def generation(self) -> int:
        """Changes when a library-owned buffer captured graphs point into was re-allocated (EncodeGraph)."""
        return int(self.lib.sgpt_ctx_generation(self.handle))

    def set_low_latency(self, on: bool) -> bool:
        """Per context: k-groups for query-sized GEMM launches (include/sgpt_hip.h::sgpt_ctx_set_low_latency): ~1 % off a
        16-query encode since round 3 (16 % before), at the price of bit-identical embeddings across batch sizes.  Returns the previous setting."""
        return bool(self.lib.sgpt_ctx_set_low_latency(self.handle, 1 if on else 0))

    def set_gemm_cu_cap(self, n: int) -> int:
        """Per context: at most n workgroups per launch of the persistent 256x256 projection kernel (0 = one per CU), for two
        contexts pipelined on two streams (include/sgpt_hip.h::sgpt_ctx_set_gemm_cu_cap).  Returns the previous value."""
        return int(self.lib.sgpt_ctx_set_gemm_cu_cap(self.handle, int(n)))

    def set_tile_policy(self, force_256) -> int:
        """Per context: True / 1 = keep the 256x256 LDS-DMA GEMM tiles even where the small-tile rule would apply (kernel tests of
        single-tile shapes); 2 = no query- / mid-sized kernels (csrc/qgemm.hip): the bulk path's small-tile kernels on every layout
        (A/Bs); identical bits whatever the policy.  Returns the previous policy (0 | 1 | 2)."""
        return int(self.lib.sgpt_ctx_set_tile_policy(self.handle, int(force_256)))

    def set_query_tile(self, k: int) -> int:
        """Per context, kernel tests: k > 0 = `linear_query` launches the k-th candidate tile of csrc/qgemm.hip (plain kernels 1 .. 7 =
        32x16, 32x32, 32x64, 64x32, 64x64, 128x64, 128x128; LayerNorm prologue 1 .. 3 = 32x32, 32x64, 64x64) instead of the one the
        cost rule picks; a tile that does not serve the shape raises "not served".  0 = the launcher chooses.  Encode calls never read
        it (include/sgpt_hip.h::sgpt_ctx_set_query_tile).  Returns the previous value; -1 (nothing changed) for k outside 0 .. 7."""
        return int(self.lib.sgpt_ctx_set_query_tile(self.handle, int(k)))

    def set_encode_chains(self, n: int, min_rows: int = 0) -> int:
        """Per context: a bulk encode call as two chains of whole sequences on two streams (include/sgpt_hip.h::
        sgpt_ctx_set_encode_chains): n = 0 the library's default, 1 one chain, 2 two chains wherever the conditions hold;
        min_rows > 0 replaces the row threshold.  Identical bits either way.  Returns the previous n."""
        old = int(self.lib.sgpt_ctx_set_encode_chains(self.handle, int(n), int(min_rows)))
        if old < 0:
            raise ValueError("set_encode_chains: n in (0, 1, 2), min_rows >= 0")
        return old

    def encode_chain_calls(self) -> int:
        """Encode calls on this context that ran as two chains so far."""
        return int(self.lib.sgpt_ctx_encode_chain_calls(self.handle))

    def reserve(self, encode_bytes: int = 0, score_bytes: int = 0) -> None:
        self._chk(self.lib.sgpt_ctx_reserve(self.handle, encode_bytes, score_bytes), "sgpt_ctx_reserve")

    # ---- fp8 (e4m3fn, power-of-two per-row scales) weight storage: building blocks of dtype="fp8" models ----
    def fp8_quantize_rows(self, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        w = w.to(device=self.device, dtype=torch.float32).contiguous()
        rows, cols = w.shape
        codes = torch.empty((rows, cols), dtype=torch.uint8, device=self.device)
        scale = torch.empty((rows,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_fp8_quantize_rows(self.handle, _p(w), rows, cols, _p(codes), _p(scale),
                                                  _stream_ptr(self.device)), "sgpt_fp8_quantize_rows")
        return codes, scale

    def fp8_dequantize_rows(self, codes: torch.Tensor, scale: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
        codes = codes.to(device=self.device, dtype=torch.uint8).contiguous()
        scale = scale.to(device=self.device, dtype=torch.float32).contiguous()
        rows, cols = codes.shape
        out = torch.empty((rows, cols), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_fp8_dequantize_rows(self.handle, _p(codes), _p(scale), rows, cols, _p(out),
                                                    DT_CODE[out_dtype],
                                                    _stream_ptr(self.device)), "sgpt_fp8_dequantize_rows")
        return out

    def score_overflow_count(self) -> Tuple[int, int]:
        """(filtered chunks, chunks whose candidate lists overflowed and took the fallback) of the last score_topk pass on this
        context; synchronises (include/sgpt_hip.h::sgpt_score_overflow_count)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.sgpt_score_overflow_count(self.handle, C.byref(a), C.byref(b), _stream_ptr(self.device)),
                  "sgpt_score_overflow_count")
        return int(a.value), int(b.value)

    def _operand(self, x: torch.Tensor, dtype) -> torch.Tensor:
        if x.dtype == dtype and x.device == self.device and x.is_contiguous():
            return x
        if dtype in (torch.bfloat16, torch.float16):
            return self.to_16(x, dtype)
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    # ---- the projection GEMM with a fused epilogue (kernel-level tests, custom blocks) ----
    def linear(self, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epi: str = "store",
               resid: Optional[torch.Tensor] = None, out_dtype=None) -> torch.Tensor:
        """epi: 'store' | 'gelu' (gelu_new(a.w^T + bias)) | 'gelu_erf' (the BERT family's erf GELU) | 'resid' (resid + a.w^T + bias,
        fp32) | 'vt' (transposed)."""
        code = {"store": 0, "gelu": 1, "resid": 2, "vt": 4, "gelu_erf": 9}[epi]
        M, K = a.shape
        N = w.shape[0]
        if out_dtype is None:
            out_dtype = torch.float32 if epi == "resid" else a.dtype
        out = torch.empty((N, M) if epi == "vt" else (M, N), dtype=out_dtype, device=self.device)
        b = None if bias is None else bias.to(device=self.device, dtype=torch.float32).contiguous()
        r = None if resid is None else resid.to(device=self.device, dtype=torch.float32).contiguous()
        self._chk(self.lib.sgpt_linear(self.handle, DT_CODE[a.dtype], code, DT_CODE[out_dtype], _p(a.contiguous()),
                                       _p(w.contiguous()), _p(b), _p(r), _p(out), M, N, K, _stream_ptr(self.device)),
                  "sgpt_linear")
        return out

    def linear_query(self, w: torch.Tensor, a: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None, ln=None,
                     bias: Optional[torch.Tensor] = None, epi: str = "store", resid: Optional[torch.Tensor] = None, n_split: int = 0):
        """The query- / mid-sized projection kernels stand-alone (include/sgpt_hip.h::sgpt_linear_query).  a: [M, K] 16-bit operand, or
        x: fp32 [M, K] with ln = (gamma, beta, eps) -- the LayerNorm prologue.  epi 'store' | 'gelu' | 'resid' | 'qkv' (returns
        (q|k [M, n_split], V^T [N - n_split, M]))."""
        code = {"store": 0, "gelu": 1, "resid": 2, "qkv": 7}[epi]
        N, K = w.shape
        src = a if a is not None else x
        M = src.shape[0]
        odt = torch.float32 if epi == "resid" else w.dtype
        out = torch.empty((M, n_split if epi == "qkv" else N), dtype=odt, device=self.device)
        vt = torch.empty((N - n_split, M), dtype=odt, device=self.device) if epi == "qkv" else None
        f32 = lambda t_: None if t_ is None else t_.to(device=self.device, dtype=torch.float32).contiguous()  # noqa: E731
        g, b, eps = (f32(ln[0]), f32(ln[1]), float(ln[2])) if ln is not None else (None, None, 0.0)
        b32, r32, x32 = f32(bias), f32(resid), f32(x)
        self._chk(self.lib.sgpt_linear_query(self.handle, DT_CODE[w.dtype], code, _p(None if a is None else a.contiguous()), _p(x32), _p(g), _p(b), eps,
                                             _p(w.contiguous()), _p(b32), _p(r32), _p(out), _p(vt), int(n_split), M, N, K,
                                             _stream_ptr(self.device)), "sgpt_linear_query")
        return (out, vt) if epi == "qkv" else out

    def linear_qkv(self, a: torch.Tensor, w: torch.Tensor, n_split: int):
        """The bulk fused Q | K | V projection stand-alone (include/sgpt_hip.h::sgpt_linear_qkv): one launch of the persistent 256x256
        kernel.  a: [M, K], w: [N, K], 16-bit.  Returns (q|k [M, n_split], V^T [N - n_split, M]); shapes the bulk launch does not
        serve raise."""
        M, K = a.shape
        N = w.shape[0]
        out = torch.empty((M, n_split), dtype=a.dtype, device=self.device)
        vt = torch.empty((N - n_split, M), dtype=a.dtype, device=self.device)
        self._chk(self.lib.sgpt_linear_qkv(self.handle, DT_CODE[a.dtype], _p(a.contiguous()), _p(w.contiguous()), _p(out), _p(vt),
                                           int(n_split), M, N, K, _stream_ptr(self.device)), "sgpt_linear_qkv")
        return out, vt

    def linear_split(self, a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epi: str = "store",
                     triple: bool = False) -> torch.Tensor:
        """The split store epilogues (include/sgpt_hip.h::sgpt_linear_split): epi 'store' | 'gelu' -> [M, 2 N] = [hi | lo], or
        with triple=True [M, 3 N] = [hi | lo | hi] (the row layout a split consumer contracts over); 'vt' -> [2, N, M]
        (hi, lo transposed)."""
        code = {"store": 0, "gelu": 1, "vt": 4}[epi]
        M, K = a.shape
        N = w.shape[0]
        b = None if bias is None else bias.to(device=self.device, dtype=torch.float32).contiguous()
        if epi == "vt":
            out = torch.zeros((2, N, M), dtype=a.dtype, device=self.device)
            ldo, lo, hi2 = M, N * M, 0
        else:
            out = torch.zeros((M, (3 if triple else 2) * N), dtype=a.dtype, device=self.device)
            ldo, lo, hi2 = out.shape[1], N, (2 * N if triple else 0)
        self._chk(self.lib.sgpt_linear_split(self.handle, DT_CODE[a.dtype], code, _p(a.contiguous()), _p(w.contiguous()), _p(b),
                                             _p(out), ldo, lo, hi2, M, N, K, _stream_ptr(self.device)), "sgpt_linear_split")
        return out

    # ---- the attention kernels stand-alone (kernel-level tests) ----
    def attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, seq_off: torch.Tensor,
                  H: int, dh: int, max_alloc_len: int, window: int = 0, scale: float = 1.0, alibi: Optional[torch.Tensor] = None,
                  out_scale: float = 0.0, range_flag: Optional[torch.Tensor] = None, x3: bool = False, qk_lo_delta: int = 0,
                  v_lo_delta: int = 0, ctx_lo_delta: int = 0, ctx_hi2_delta: int = 0, causal: Optional[bool] = None,
                  seq_len: Optional[torch.Tensor] = None, n_kv_heads: Optional[int] = None) -> torch.Tensor:
        """include/sgpt_hip.h::sgpt_attention on caller-laid-out buffers (the over-read contract there is the caller's): q, k
        [T, >= H dh] row views of one leading dimension; v = V^T [H dh, >= T] (16-bit) or [T, ...] with q's leading dimension
        (fp32); out [T, ...] in q's dtype, or uint8 (e4m3 codes of ctx / out_scale, bf16 operands).  Deltas in elements.
        causal None: the sgpt_attention entry.  True / False: sgpt_attention_ex -- False is the bidirectional mode of the BERT family,
        every query of a sequence sees its keys [0, seq_len[b]) (seq_len int32 [B]; None = the whole allocation).
        n_kv_heads: sgpt_attention_gqa -- k and v hold n_kv_heads heads, query head h reads head h // (H // n_kv_heads) (causal;
        attention_gqa_ex below is the entry with both grouped K / V and the bidirectional mode)."""
        T = q.shape[0]
        out_fp8 = out.dtype == torch.uint8
        if q.dtype not in DT_CODE:
            raise ValueError(f"attention: operands are fp32, bf16 or f16, got {q.dtype}")
        if k.stride(0) != q.stride(0) or q.stride(1) != 1 or k.stride(1) != 1 or v.stride(1) != 1 or out.stride(1) != 1:
            raise ValueError("attention: q and k share one leading dimension; unit column strides")
        if k.dtype != q.dtype or v.dtype != q.dtype:
            raise ValueError("attention: q, k and v have one dtype")
        if out.dtype != q.dtype and not (out_fp8 and q.dtype == torch.bfloat16):
            raise ValueError("attention: out has q's dtype (or uint8 e4m3 codes for bf16 operands)")
        if q.dtype == torch.float32 and v.stride(0) != q.stride(0):
            raise ValueError("attention: fp32 v rows share q's leading dimension (the fp32 kernel reads v with ldq)")
        so = seq_off.to(device=self.device, dtype=torch.int32).contiguous()
        al = None if alibi is None else alibi.to(device=self.device, dtype=torch.float32).contiguous()
        if n_kv_heads is not None:
            if causal is False or seq_len is not None:
                raise ValueError("attention: grouped K / V is causal")
            self._chk(self.lib.sgpt_attention_gqa(self.handle, DT_CODE[q.dtype], _p(q), _p(k), _p(v), q.stride(0), v.stride(0), _p(out),
                                                  out.stride(0), _p(so), so.numel() - 1, T, H, int(n_kv_heads), dh, window, scale, _p(al),
                                                  max_alloc_len, 1 if out_fp8 else 0, out_scale, _p(range_flag), 1 if x3 else 0,
                                                  qk_lo_delta, v_lo_delta, ctx_lo_delta, ctx_hi2_delta, _stream_ptr(self.device)),
                      "sgpt_attention_gqa")
            return out
        if causal is not None:
            sl = None if seq_len is None else seq_len.to(device=self.device, dtype=torch.int32).contiguous()
            self._chk(self.lib.sgpt_attention_ex(self.handle, DT_CODE[q.dtype], _p(q), _p(k), _p(v), q.stride(0), v.stride(0), _p(out),
                                                 out.stride(0), _p(so), so.numel() - 1, T, H, dh, window, scale, _p(al), max_alloc_len,
                                                 1 if out_fp8 else 0, out_scale, _p(range_flag), 1 if x3 else 0, qk_lo_delta,
                                                 v_lo_delta, ctx_lo_delta, ctx_hi2_delta, 1 if causal else 0, _p(sl),
                                                 _stream_ptr(self.device)), "sgpt_attention_ex")
            return out
        self._chk(self.lib.sgpt_attention(self.handle, DT_CODE[q.dtype], _p(q), _p(k), _p(v), q.stride(0), v.stride(0), _p(out),
                                          out.stride(0), _p(so), so.numel() - 1, T, H, dh, window, scale, _p(al), max_alloc_len,
                                          1 if out_fp8 else 0, out_scale, _p(range_flag), 1 if x3 else 0, qk_lo_delta,
                                          v_lo_delta, ctx_lo_delta, ctx_hi2_delta, _stream_ptr(self.device)), "sgpt_attention")
        return out

    def attention_gqa_ex(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, seq_off: torch.Tensor, H: int,
                         n_kv_heads: int, dh: int, max_alloc_len: int, causal: bool, seq_len: Optional[torch.Tensor] = None, window: int = 0,
                         scale: float = 1.0, alibi: Optional[torch.Tensor] = None, out_scale: float = 0.0, x3: bool = False,
                         qk_lo_delta: int = 0, v_lo_delta: int = 0, ctx_lo_delta: int = 0, ctx_hi2_delta: int = 0) -> torch.Tensor:
        """include/sgpt_hip.h::sgpt_attention_gqa_ex: grouped K / V (as attention(n_kv_heads=)) with the causal / seq_len arguments of
        sgpt_attention_ex -- causal=False is the bidirectional attention of a Llama-family model, every query of sequence b sees its
        keys [0, seq_len[b]) (None = the whole allocation).  Buffers as attention(); the library checks the rest."""
        if q.dtype not in DT_CODE:
            raise ValueError(f"attention_gqa_ex: operands are fp32, bf16 or f16, got {q.dtype}")
        if k.stride(0) != q.stride(0) or q.stride(1) != 1 or k.stride(1) != 1 or v.stride(1) != 1 or out.stride(1) != 1:
            raise ValueError("attention_gqa_ex: q and k share one leading dimension; unit column strides")
        if k.dtype != q.dtype or v.dtype != q.dtype:
            raise ValueError("attention_gqa_ex: q, k and v have one dtype")
        out_fp8 = out.dtype == torch.uint8
        if out.dtype != q.dtype and not out_fp8:
            raise ValueError("attention_gqa_ex: out has q's dtype")
        if q.dtype == torch.float32 and v.stride(0) != q.stride(0):
            raise ValueError("attention_gqa_ex: fp32 v rows share q's leading dimension (the fp32 kernel reads v with ldq)")
        so = seq_off.to(device=self.device, dtype=torch.int32).contiguous()
        sl = None if seq_len is None else seq_len.to(device=self.device, dtype=torch.int32).contiguous()
        al = None if alibi is None else alibi.to(device=self.device, dtype=torch.float32).contiguous()
        self._chk(self.lib.sgpt_attention_gqa_ex(self.handle, DT_CODE[q.dtype], _p(q), _p(k), _p(v), q.stride(0), v.stride(0), _p(out),
                                                 out.stride(0), _p(so), so.numel() - 1, q.shape[0], H, int(n_kv_heads), dh, window, scale,
                                                 _p(al), max_alloc_len, 1 if out_fp8 else 0, out_scale, None, 1 if x3 else 0, qk_lo_delta,
                                                 v_lo_delta, ctx_lo_delta, ctx_hi2_delta, 1 if causal else 0, _p(sl),
                                                 _stream_ptr(self.device)), "sgpt_attention_gqa_ex")
        return out

    # ---- the encoder's row kernels stand-alone (kernel-level tests): include/sgpt_hip.h::sgpt_embed ... sgpt_logprob_rows ----
    # Tensors are taken as they are (device, dtype, unit column stride are the caller's): a test hands in views of larger
    # buffers and over-allocated outputs, and a silent copy would hide what it set up.
    def _f32c(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        return None if t is None else t.to(device=self.device, dtype=torch.float32).contiguous()

    def embed(self, ids: torch.Tensor, pos: Optional[torch.Tensor], wte: torch.Tensor, wpe: Optional[torch.Tensor] = None,
              vocab: Optional[int] = None, max_pos: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out fp32 [T, d] = wte[ids] + wpe[pos] (wpe None: wte[ids]).  vocab / max_pos: the table sizes the kernel clamps
        into (default: the tables' row counts)."""
        T, d = ids.numel(), wte.shape[1]
        if wte.stride() != (d, 1) or (wpe is not None and wpe.stride() != (d, 1)):
            raise ValueError("embed: tables are row-contiguous [rows, d]")
        if out is None:
            out = torch.empty((T, d), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_embed(self.handle, _p(ids), _p(pos), _p(wte), _p(wpe), T, d,
                                      wte.shape[0] if vocab is None else int(vocab),
                                      (wpe.shape[0] if wpe is not None else 0) if max_pos is None else int(max_pos), _p(out),
                                      _stream_ptr(self.device)), "sgpt_embed")
        return out

    def layernorm(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, out_dtype=torch.float32,
                  out_mul: float = 1.0, split: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nn.LayerNorm over the rows of x fp32 [T, d] -> [T, d] in out_dtype (f16: times out_mul), or with split=True the
        [T, 3 d] = [hi | lo | hi] operand of the split-precision projections.  out: written in place of a new tensor (x itself
        for fp32; a larger buffer keeps its rows past T)."""
        T, d = x.shape
        if out is None:
            out = torch.empty((T, 3 * d if split else d), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_layernorm(self.handle, _p(x), _p(self._f32c(gamma)), _p(self._f32c(beta)), T, d, float(eps), _p(out),
                                          DT_CODE[out_dtype], float(out_mul), 1 if split else 0, _stream_ptr(self.device)),
                  "sgpt_layernorm")
        return out

    def layernorm_writeback(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12,
                            out_dtype=torch.float16) -> torch.Tensor:
        """The LayerNorm of a post-LN block (include/sgpt_hip.h::sgpt_layernorm_writeback): x fp32 [T, d] is normalised IN PLACE and
        the same values, rounded once, are returned as a [T, d] tensor of out_dtype (f16 | bf16)."""
        T, d = x.shape
        out = torch.empty((T, d), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_layernorm_writeback(self.handle, _p(x), _p(self._f32c(gamma)), _p(self._f32c(beta)), T, d, float(eps),
                                                    _p(out), DT_CODE[out_dtype], _stream_ptr(self.device)), "sgpt_layernorm_writeback")
        return out

    def rmsnorm(self, x: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-6, out_dtype=torch.float32,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """RMSNorm over the rows of x fp32 [T, d] (include/sgpt_hip.h::sgpt_rmsnorm): x * rsqrt(mean(x^2) + eps) * gamma -> [T, d] in
        out_dtype, rounded once.  out: written in place of a new tensor (x itself for fp32)."""
        T, d = x.shape
        if out is None:
            out = torch.empty((T, d), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_rmsnorm(self.handle, _p(x), _p(self._f32c(gamma)), T, d, float(eps), _p(out), DT_CODE[out_dtype],
                                        _stream_ptr(self.device)), "sgpt_rmsnorm")
        return out

    def swiglu(self, gu: torch.Tensor) -> torch.Tensor:
        """silu(gu[:, :ffn]) * gu[:, ffn:] for gu [T, 2 ffn] (fp32, bf16 or f16, contiguous) -> [T, ffn] of the same dtype
        (include/sgpt_hip.h::sgpt_swiglu)."""
        if gu.dtype not in DT_CODE or not gu.is_contiguous() or gu.shape[1] % 2:
            raise ValueError("swiglu: gu is a contiguous fp32 / bf16 / f16 [T, 2 ffn] tensor")
        T, ffn = gu.shape[0], gu.shape[1] // 2
        out = torch.empty((T, ffn), dtype=gu.dtype, device=self.device)
        self._chk(self.lib.sgpt_swiglu(self.handle, _p(gu), DT_CODE[gu.dtype], T, ffn, _p(out), _stream_ptr(self.device)), "sgpt_swiglu")
        return out

    def rope_half(self, buf: torch.Tensor, pos: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor, H: int, H_kv: int, head_dim: int,
                  k_off: int, T: Optional[int] = None, max_pos: Optional[int] = None) -> torch.Tensor:
        """HF rotate_half rotary embedding in place on the H query heads (column 0) and the H_kv key heads (column k_off) of the
        first T rows of buf [rows, ld]; sin / cos fp32 [max_pos, head_dim / 2] (include/sgpt_hip.h::sgpt_rope_half)."""
        if buf.dtype not in DT_CODE or buf.stride(1) != 1:
            raise ValueError("rope_half: buf is fp32, bf16 or f16 with a unit column stride")
        if sin.stride() != (head_dim // 2, 1) or cos.stride() != (head_dim // 2, 1):
            raise ValueError("rope_half: sin / cos are row-contiguous [max_pos, head_dim / 2]")
        self._chk(self.lib.sgpt_rope_half(self.handle, _p(buf), DT_CODE[buf.dtype], buf.stride(0), int(k_off), _p(pos), _p(sin), _p(cos),
                                          buf.shape[0] if T is None else int(T), H, H_kv, head_dim,
                                          sin.shape[0] if max_pos is None else int(max_pos), _stream_ptr(self.device)), "sgpt_rope_half")
        return buf

    def qknorm_rope_half(self, buf: torch.Tensor, pos: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor, q_gamma: torch.Tensor,
                         k_gamma: torch.Tensor, H: int, H_kv: int, head_dim: int, k_off: int, eps: float = 1e-6, T: Optional[int] = None,
                         max_pos: Optional[int] = None) -> torch.Tensor:
        """The per-head RMSNorm of q and k (gains q_gamma / k_gamma fp32 [head_dim], shared by the heads) fused with rope_half, in place
        on the first T rows of buf [rows, ld]; head_dim 64 | 128 (include/sgpt_hip.h::sgpt_qknorm_rope_half)."""
        if buf.dtype not in DT_CODE or buf.stride(1) != 1:
            raise ValueError("qknorm_rope_half: buf is fp32, bf16 or f16 with a unit column stride")
        if sin.stride() != (head_dim // 2, 1) or cos.stride() != (head_dim // 2, 1):
            raise ValueError("qknorm_rope_half: sin / cos are row-contiguous [max_pos, head_dim / 2]")
        if q_gamma.shape != (head_dim,) or k_gamma.shape != (head_dim,):
            raise ValueError("qknorm_rope_half: q_gamma / k_gamma are [head_dim]")
        self._chk(self.lib.sgpt_qknorm_rope_half(self.handle, _p(buf), DT_CODE[buf.dtype], buf.stride(0), int(k_off), _p(pos), _p(sin),
                                                 _p(cos), buf.shape[0] if T is None else int(T), H, H_kv, head_dim,
                                                 sin.shape[0] if max_pos is None else int(max_pos), _p(self._f32c(q_gamma)),
                                                 _p(self._f32c(k_gamma)), float(eps), _stream_ptr(self.device)), "sgpt_qknorm_rope_half")
        return buf

    def lnf_pool(self, x: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor, pad_left: Optional[torch.Tensor] = None,
                 ln=None, mode: str = "weightedmean", normalize: bool = False, position_weights: Optional[torch.Tensor] = None,
                 n_weights: Optional[int] = None, nonfinite_flag: Optional[torch.Tensor] = None, rms=None) -> torch.Tensor:
        """The fused final LayerNorm + pooling of a packed batch (include/sgpt_hip.h::sgpt_lnf_pool): x fp32 [T_pad, d], int32
        seq_off / seq_len / pad_left on the device; ln = (gamma, beta, eps) or None (pool x as it is) -> fp32 [B, d].
        rms = (gamma, eps): the final RMSNorm of the Llama family instead (sgpt_lnf_pool_ex, norm_kind 1)."""
        if rms is not None:
            if ln is not None:
                raise ValueError("lnf_pool: ln or rms, not both")
            if mode not in POOL_MODES:
                raise ValueError(f"unknown pooling mode {mode}")
            B, d = seq_len.numel(), x.shape[1]
            pw = self._f32c(position_weights)
            n_w = (0 if pw is None else pw.numel()) if n_weights is None else int(n_weights)
            out = torch.empty((B, d), dtype=torch.float32, device=self.device)
            self._chk(self.lib.sgpt_lnf_pool_ex(self.handle, _p(x), _p(self._f32c(rms[0])), None, _p(seq_off), _p(seq_len), _p(pad_left), B, d,
                                                float(rms[1]), 1, POOL_MODES[mode], 1 if normalize else 0, _p(pw), n_w, _p(out),
                                                _p(nonfinite_flag), 1, _stream_ptr(self.device)), "sgpt_lnf_pool_ex")
            return out
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode}")
        B, d = seq_len.numel(), x.shape[1]
        g, b, eps = (self._f32c(ln[0]), self._f32c(ln[1]), float(ln[2])) if ln is not None else (None, None, 0.0)
        pw = self._f32c(position_weights)
        n_w = (0 if pw is None else pw.numel()) if n_weights is None else int(n_weights)
        out = torch.empty((B, d), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_lnf_pool(self.handle, _p(x), _p(g), _p(b), _p(seq_off), _p(seq_len), _p(pad_left), B, d, eps,
                                         0 if ln is None else 1, POOL_MODES[mode], 1 if normalize else 0, _p(pw), n_w, _p(out),
                                         _p(nonfinite_flag), _stream_ptr(self.device)), "sgpt_lnf_pool")
        return out

    def lnf_pool_range(self, x: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor, pool_lo: Optional[torch.Tensor],
                       pad_left: Optional[torch.Tensor] = None, ln=None, rms=None, mode: str = "weightedmean",
                       normalize: bool = False) -> torch.Tensor:
        """lnf_pool over the rows [pool_lo[b], seq_len[b]) of every sequence (include/sgpt_hip.h::sgpt_lnf_pool_range): pool_lo int32 [B]
        on the device, clamped by the kernel; None = every row.  ln = (gamma, beta, eps) | rms = (gamma, eps) | neither (pool x as it is)."""
        if ln is not None and rms is not None:
            raise ValueError("lnf_pool_range: ln or rms, not both")
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode}")
        B, d = seq_len.numel(), x.shape[1]
        g, b, eps = (self._f32c(ln[0]), self._f32c(ln[1]), float(ln[2])) if ln is not None else (
            (self._f32c(rms[0]), None, float(rms[1])) if rms is not None else (None, None, 0.0))
        out = torch.empty((B, d), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_lnf_pool_range(self.handle, _p(x), _p(g), _p(b), _p(seq_off), _p(seq_len), _p(pad_left), B, d, eps,
                                               0 if (ln is None and rms is None) else 1, POOL_MODES[mode], 1 if normalize else 0, None, 0,
                                               _p(out), None, 1 if rms is not None else 0, _p(pool_lo), _stream_ptr(self.device)),
                  "sgpt_lnf_pool_range")
        return out

    def rope(self, buf: torch.Tensor, pos: torch.Tensor, sin: torch.Tensor, cos: torch.Tensor, H: int, head_dim: int,
             rotary_dim: int, k_off: int, T: Optional[int] = None, max_pos: Optional[int] = None) -> torch.Tensor:
        """GPT-J rotary embedding in place on q (column 0) and k (column k_off) of the first T rows of buf [rows, ld]; sin / cos
        fp32 [max_pos, rotary_dim / 2] (include/sgpt_hip.h::sgpt_rope)."""
        if buf.dtype not in DT_CODE or buf.stride(1) != 1:
            raise ValueError("rope: buf is fp32, bf16 or f16 with a unit column stride")
        if sin.stride() != (rotary_dim // 2, 1) or cos.stride() != (rotary_dim // 2, 1):
            raise ValueError("rope: sin / cos are row-contiguous [max_pos, rotary_dim / 2]")
        self._chk(self.lib.sgpt_rope(self.handle, _p(buf), DT_CODE[buf.dtype], buf.stride(0), int(k_off), _p(pos), _p(sin), _p(cos),
                                     buf.shape[0] if T is None else int(T), H, head_dim, rotary_dim,
                                     sin.shape[0] if max_pos is None else int(max_pos), _stream_ptr(self.device)), "sgpt_rope")
        return buf

    def logprob_rows(self, logits: torch.Tensor, targets: torch.Tensor, V: Optional[int] = None, greedy: bool = True):
        """-> (log_softmax(logits[r, :V])[targets[r]] fp32 [n], argmax int32 [n] or None); logits fp32 [n, ld >= V] with a unit
        column stride (include/sgpt_hip.h::sgpt_logprob_rows)."""
        if logits.dtype != torch.float32 or logits.stride(1) != 1:
            raise ValueError("logprob_rows: logits are fp32 rows with a unit column stride")
        n = logits.shape[0]
        lp = torch.empty((n,), dtype=torch.float32, device=self.device)
        am = torch.empty((n,), dtype=torch.int32, device=self.device) if greedy else None
        self._chk(self.lib.sgpt_logprob_rows(self.handle, _p(logits), logits.stride(0), logits.shape[1] if V is None else int(V),
                                             _p(targets), n, _p(lp), _p(am), _stream_ptr(self.device)), "sgpt_logprob_rows")
        return lp, am

    # ---- fp8-MFMA building blocks (dtype='fp8mfma'): quantising LayerNorm, e4m3 x e4m3 projection ----
    def layernorm_fp8(self, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        T, d = x.shape
        codes = torch.empty((T, d), dtype=torch.uint8, device=self.device)
        scale = torch.empty((T,), dtype=torch.float32, device=self.device)
        g = gamma.to(device=self.device, dtype=torch.float32).contiguous()
        b = beta.to(device=self.device, dtype=torch.float32).contiguous()
        self._chk(self.lib.sgpt_layernorm_fp8(self.handle, _p(x), _p(g), _p(b), T, d, eps, _p(codes), _p(scale),
                                              _stream_ptr(self.device)), "sgpt_layernorm_fp8")
        return codes, scale

    # ---- the quantising row kernels of the fp8 projections of the Llama family (SGPTModel(projections='fp8')) ----
    def rmsnorm_fp8(self, x: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-6):
        """RMSNorm rows of x fp32 [T, d] -> (e4m3fn codes uint8 [T, d], power-of-two scale fp32 [T]); value = code * scale
        (include/sgpt_hip.h::sgpt_rmsnorm_fp8)."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        T, d = x.shape
        codes = torch.empty((T, d), dtype=torch.uint8, device=self.device)
        scale = torch.empty((T,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_rmsnorm_fp8(self.handle, _p(x), _p(self._f32c(gamma)), T, d, float(eps), _p(codes), _p(scale),
                                            _stream_ptr(self.device)), "sgpt_rmsnorm_fp8")
        return codes, scale

    def swiglu_fp8(self, gu: torch.Tensor):
        """silu(gu[:, :ffn]) * gu[:, ffn:] of gu [T, 2 ffn] (bf16 or f16, contiguous), in fp32, -> (e4m3fn codes uint8 [T, ffn],
        power-of-two scale fp32 [T]) (include/sgpt_hip.h::sgpt_swiglu_fp8)."""
        if gu.dtype not in (torch.bfloat16, torch.float16) or not gu.is_contiguous() or gu.shape[1] % 2:
            raise ValueError("swiglu_fp8: gu is a contiguous bf16 / f16 [T, 2 ffn] tensor")
        T, ffn = gu.shape[0], gu.shape[1] // 2
        codes = torch.empty((T, ffn), dtype=torch.uint8, device=self.device)
        scale = torch.empty((T,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_swiglu_fp8(self.handle, _p(gu), DT_CODE[gu.dtype], T, ffn, _p(codes), _p(scale),
                                           _stream_ptr(self.device)), "sgpt_swiglu_fp8")
        return codes, scale

    def linear_fp8(self, a8: torch.Tensor, w8: torch.Tensor, w_scale: torch.Tensor, bias: torch.Tensor, epi: str,
                   a_scale: Optional[torch.Tensor] = None, a_scalar: float = 1.0, resid: Optional[torch.Tensor] = None,
                   out_scale: float = 1.0, out_dtype=None) -> torch.Tensor:
        """epi 'gelu': u8 codes of gelu_new(acc + bias) / out_scale;  'resid': fp32 resid + acc + bias;
        'store' / 'vt': 16-bit (out_dtype) acc (+ bias), row-major / transposed."""
        M, K = a8.shape
        N = w8.shape[0]
        code = {"store": 0, "gelu": 1, "resid": 2, "vt": 4}[epi]
        odt = {"gelu": torch.uint8, "resid": torch.float32}.get(epi, out_dtype if out_dtype is not None else torch.bfloat16)
        out = torch.empty((N, M) if epi == "vt" else (M, N), dtype=odt, device=self.device)
        r = None if resid is None else resid.to(device=self.device, dtype=torch.float32).contiguous()
        b = None if bias is None else bias.contiguous()
        self._chk(self.lib.sgpt_linear_fp8(self.handle, code, DT_CODE.get(odt, 0), _p(a8.contiguous()), _p(a_scale), a_scalar,
                                           _p(w8.contiguous()), _p(w_scale.contiguous()), _p(b), _p(r), _p(out),
                                           out_scale, M, N, K, _stream_ptr(self.device)), "sgpt_linear_fp8")
        return out

    # ---- a7: dense score matrix (cos_sim / dot_score) ----
    def scores(self, a: torch.Tensor, b: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        a, b = self._operand(a, dtype), self._operand(b, dtype)
        na, d = a.shape
        nb, d2 = b.shape
        if d != d2:
            raise ValueError(f"embedding dims differ: {d} vs {d2}")
        ldo = (nb + 3) // 4 * 4
        out = torch.empty((na, ldo), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_scores(self.handle, _p(a), _p(b), DT_CODE[dtype],
                                       na, nb, d, _p(out), ldo, _stream_ptr(self.device)), "sgpt_scores")
        return out[:, :nb]

    # ---- a7+a8: fused chunked score + running top-k ----
    def score_topk(self, q: torch.Tensor, corpus: torch.Tensor, k: int, idx_base: int = 0,
                   run: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                   dtype=None, rescore: str = "sign", rescore_multiplier=4) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """-> (values fp32[nq,k], indices int64[nq,k], n_valid); rows sorted by descending score.  `corpus` may be a QuantizedCorpus
        (fp8 codes + per-document scales): the queries are then f16 (dtype None / torch.float16 only) and the result equals the f16
        scorer's on corpus.dequantize(torch.float16), sgpt_score_topk_q8.  Over a Uint8Corpus (sgpt_score_topk_u8): q of any float
        dtype, upcast to fp32, `dtype` None; queries run in groups of 64, each re-streaming the codes.  Over a BinaryCorpus (sgpt_score_topk_bits): q fp32, normalised
        and UNcentred; stage 1 takes the kp = min(1024, max(k, k * rescore_multiplier)) best by Hamming distance, `rescore` orders
        them -- "sign" (<q, signs> / sqrt(d), no extra memory), "fp8" (the corpus's fp8 copy), "uint8" (the corpus's uint8 copy,
        sgpt_score_topk_bits_u8), or "none" (Hamming only, kp = k, values
        agreement / d); a running list must come from calls with the same `rescore`.  corpus.center is subtracted from q here, for the
        bits and for "sign"; rescore="fp8" on a centred corpus is refused (ValueError: the C call takes one query matrix, and the fp8
        rows need the raw q); rescore="uint8" serves a centred corpus too (its entry takes the raw q and the centre: the bits come from
        q - center, the values from q).  1 <= k <= 1024.  `rescore` / `rescore_multiplier` belong to a BinaryCorpus: any other corpus with
        non-default values of them raises ValueError."""
        if isinstance(corpus, CORPUS_KINDS):
            return corpus.score_topk(self, q, k, idx_base, run, dtype, rescore, rescore_multiplier)
        _no_rescore(rescore, rescore_multiplier)
        if dtype is None:
            dtype = corpus.dtype if corpus.dtype in DT_CODE else torch.float32
        q, corpus = self._operand(q, dtype), self._operand(corpus, dtype)
        nq, d = q.shape
        N, d2 = corpus.shape
        if d != d2:
            raise ValueError(f"embedding dims differ: {d} vs {d2}")
        val, idx, n_run = self._run_list(run, nq, k)
        n_out = C.c_int32(0)
        self._chk(self.lib.sgpt_score_topk(self.handle, _p(q), _p(corpus), DT_CODE[dtype], nq, N, d, k,
                                           idx_base, _p(val), _p(idx), n_run, C.byref(n_out),
                                           _stream_ptr(self.device)), "sgpt_score_topk")
        return val, idx, int(n_out.value)

    REFINE_MARGIN_UNIT_F16 = 2.5e-3      # 2 eps for L2-normalised rows with IEEE-half stage-1 copies (include/sgpt_hip.h)

    def score_topk_refined(self, q: torch.Tensor, corpus32: torch.Tensor, corpus16: Optional[torch.Tensor], k: int,
                           idx_base: int = 0, run: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                           margin: Optional[float] = None, report: bool = False):
        """The fp32 top-k (fp32 scores, the fp32 set) at the 16-bit scorer's speed: sgpt_score_topk_refined.  q, corpus32: fp32
        rows (L2-normalised for the default margin); corpus16: their f16 rounding (None: made here).  report=True synchronises
        and returns a fourth value: 1 if the exact fallback pass ran, 0 if not, -1 if the call was the exact pass outright."""
        q = q.to(device=self.device, dtype=torch.float32).contiguous()
        corpus32 = corpus32.to(device=self.device, dtype=torch.float32).contiguous()
        if corpus16 is None:
            corpus16 = self.to_16(corpus32, torch.float16)
        if corpus16.dtype not in (torch.float16, torch.bfloat16) or corpus16.shape != corpus32.shape or not corpus16.is_contiguous():
            raise ValueError("corpus16 must be the contiguous 16-bit rounding of corpus32")
        if margin is None:
            if corpus16.dtype != torch.float16:
                raise ValueError("the default margin is the bound for IEEE-half copies of unit rows: pass margin= for bf16 copies")
            margin = self.REFINE_MARGIN_UNIT_F16
        nq, d = q.shape
        N = corpus32.shape[0]
        val, idx, n_run = self._run_list(run, nq, k)
        n_out, fb = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.sgpt_score_topk_refined(self.handle, _p(q), _p(corpus32), _p(corpus16), DT_CODE[corpus16.dtype], nq, N, d, k,
                                                   idx_base, float(margin), _p(val), _p(idx), n_run, C.byref(n_out),
                                                   C.byref(fb) if report else None, _stream_ptr(self.device)), "sgpt_score_topk_refined")
        return (val, idx, int(n_out.value), int(fb.value)) if report else (val, idx, int(n_out.value))

    def topk_merge(self, val: torch.Tensor, idx: torch.Tensor, k: int,
                   exclude_idx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        val = val.to(device=self.device, dtype=torch.float32).contiguous()
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        nq, m = val.shape
        ov = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        ex = None if exclude_idx is None else exclude_idx.to(device=self.device, dtype=torch.int64).contiguous()
        self._chk(self.lib.sgpt_topk_merge(self.handle, _p(val), _p(idx), nq, m, k, _p(ex), _p(ov), _p(oi),
                                           _stream_ptr(self.device)), "sgpt_topk_merge")
        return ov, oi

    def fold_gathered_topk(self, gathered_val: torch.Tensor, gathered_idx: torch.Tensor, k_out: int,
                           exclude_idx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """[world, nq, k] all-gathered per-rank lists (rank order) -> the k_out best per query: the rank-local half of
        sgpt_exchange_topk (include/sgpt_hip.h::sgpt_fold_gathered_topk), no communicator involved."""
        gv = gathered_val.to(device=self.device, dtype=torch.float32).contiguous()
        gi = gathered_idx.to(device=self.device, dtype=torch.int64).contiguous()
        world, nq, k = gv.shape
        ov = torch.empty((nq, k_out), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k_out), dtype=torch.int64, device=self.device)
        ex = None if exclude_idx is None else exclude_idx.to(device=self.device, dtype=torch.int64).contiguous()
        self._chk(self.lib.sgpt_fold_gathered_topk(self.handle, _p(gv), _p(gi), world, nq, k, k_out, _p(ex), _p(ov), _p(oi),
                                                   _stream_ptr(self.device)), "sgpt_fold_gathered_topk")
        return ov, oi

    def topk(self, scores: torch.Tensor, k: int, idx_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """torch.topk(scores, k, dim=1) with NaN -> -1 first (exact_search.py:99-108); sorted descending."""
        scores = scores.to(device=self.device, dtype=torch.float32)
        if scores.stride(1) != 1:
            scores = scores.contiguous()
        nq, n = scores.shape
        ov = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        self._chk(self.lib.sgpt_topk(self.handle, _p(scores), nq, n, scores.stride(0), k, idx_base, _p(ov), _p(oi),
                                     _stream_ptr(self.device)), "sgpt_topk")
        return ov, oi

    # ---- evaluation: per-query, per-cut metric sums from device-resident ranked lists ----
    def eval_ranked(self, idx: torch.Tensor, val: Optional[torch.Tensor], qrel_off, qrel_pos, qrel_rel, ideal_rel, k_values,
                    check_order: bool = True) -> dict:
        """include/sgpt_hip.h::sgpt_eval_ranked.  idx int64 [nq, K] (position < 0 = padding, ends the list), val fp32 [nq, K];
        the qrels as a CSR in the same position space (sgpt_amd.evaluation.pack_qrels builds it); k_values ascending, <= K.
        -> {"hits", "first" int32 [nq, nk]; "dcg", "idcg", "sp" fp32 [nq, nk]; "R" int32 [nq]} on the device.
        check_order=True synchronises the stream and raises ValueError (SGPT_ERR_INVALID) when a row is not sorted by
        descending score."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        nq, K = idx.shape
        if val is not None:
            val = val.to(device=self.device, dtype=torch.float32).contiguous()
            if val.shape != idx.shape:
                raise ValueError(f"eval_ranked: val {tuple(val.shape)} and idx {tuple(idx.shape)} differ in shape")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device) if not isinstance(a, torch.Tensor) \
            else a.to(device=self.device, dtype=torch.int32).contiguous()  # noqa: E731
        off, rel, ideal = i32(qrel_off), i32(qrel_rel), i32(ideal_rel)
        pos = (qrel_pos if isinstance(qrel_pos, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(qrel_pos, dtype=np.int64)))
        pos = pos.to(device=self.device, dtype=torch.int64).contiguous()
        if off.numel() != nq + 1 or not (pos.numel() == rel.numel() == ideal.numel()):
            raise ValueError("eval_ranked: qrel_off has nq + 1 entries; qrel_pos, qrel_rel and ideal_rel have one length")
        if pos.numel() == 0:        # no judgement at all: the kernel reads none, the C entry still wants addressable arrays
            pos, rel, ideal = (torch.zeros((1,), dtype=t.dtype, device=self.device) for t in (pos, rel, ideal))
        ks = [int(k) for k in k_values]
        nk = len(ks)
        kv = (C.c_int32 * max(nk, 1))(*ks)
        out = {n: torch.zeros((nq, nk), dtype=torch.int32, device=self.device) for n in ("hits", "first")}
        out.update({n: torch.zeros((nq, nk), dtype=torch.float32, device=self.device) for n in ("dcg", "idcg", "sp")})
        out["R"] = torch.zeros((nq,), dtype=torch.int32, device=self.device)
        self._chk(self.lib.sgpt_eval_ranked(self.handle, _p(idx), _p(val), nq, K, _p(off), _p(pos), _p(rel), _p(ideal), kv, nk,
                                            1 if check_order else 0, _p(out["hits"]), _p(out["first"]), _p(out["dcg"]),
                                            _p(out["idcg"]), _p(out["sp"]), _p(out["R"]), _stream_ptr(self.device)),
                  "sgpt_eval_ranked")
        return out

    # ---- evaluation, USEB: grouped re-ranking and pair statistics ----
    def _i32(self, a) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.int32).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def eval_groups(self, grp_off, cand_rel, emb: Optional[torch.Tensor] = None, q_row=None, cand_row=None, mode: str = "cos",
                    scores_in: Optional[torch.Tensor] = None, R_extra=None, ideal_off=None, ideal_rel=None) -> dict:
        """include/sgpt_hip.h::sgpt_eval_groups.  grp_off: HOST int array [G + 1] (the CSR the caller built; its largest group and
        its total are read here); cand_rel [grp_off[G]]; either emb fp32 [n, d] with q_row [G], cand_row and mode "cos" | "dot" |
        "neg_l2", or scores_in fp32 [grp_off[G]].  -> {"scores" fp32, "order" int32 (per candidate); "hits1", "hits5", "first",
        "R" int32 [G]; "sp", "dcg", "idcg" fp32 [G]} on the device.  Asynchronous."""
        off_h = np.ascontiguousarray(grp_off.cpu().numpy() if isinstance(grp_off, torch.Tensor) else grp_off, dtype=np.int64)
        if off_h.ndim != 1 or off_h.size < 1 or off_h[0] != 0 or (np.diff(off_h) < 0).any() or off_h[-1] >= 2 ** 31:
            raise ValueError("eval_groups: grp_off must be a CSR offset array: G + 1 ascending entries starting at 0")
        G, n_cand = off_h.size - 1, int(off_h[-1])
        max_group = int(np.diff(off_h).max()) if G else 0
        rel = self._i32(cand_rel)
        if rel.numel() != n_cand:
            raise ValueError(f"eval_groups: cand_rel has {rel.numel()} entries, the groups hold {n_cand}")
        if scores_in is not None:
            scores_in = scores_in.to(device=self.device, dtype=torch.float32).contiguous()
            if scores_in.numel() != n_cand:
                raise ValueError(f"eval_groups: scores_in has {scores_in.numel()} entries, the groups hold {n_cand}")
            if n_cand == 0:                         # the C entry tells "scores given" by the pointer: keep it addressable
                scores_in = torch.zeros((1,), dtype=torch.float32, device=self.device)
            emb_t, qr, cr, n_rows, d, mode_code = None, None, None, 0, 1, _lib.SGPT_COS
        else:
            modes = {"cos": _lib.SGPT_COS, "dot": _lib.SGPT_DOT, "neg_l2": _lib.SGPT_NEG_L2}
            if mode not in modes:
                raise ValueError(f"eval_groups: mode {mode!r} is not one of {sorted(modes)}")
            if emb is None or q_row is None or cand_row is None:
                raise ValueError("eval_groups: emb, q_row and cand_row are needed when scores_in is not given")
            emb_t = emb.to(device=self.device, dtype=torch.float32).contiguous()
            if emb_t.dim() != 2:
                raise ValueError("eval_groups: emb must be [n, d]")
            n_rows, d = emb_t.shape
            qr, cr, mode_code = self._i32(q_row), self._i32(cand_row), modes[mode]
            if qr.numel() != G or cr.numel() != n_cand:
                raise ValueError("eval_groups: q_row has one entry per group, cand_row one per candidate")
        rx = None if R_extra is None else self._i32(R_extra)
        if rx is not None and rx.numel() != G:
            raise ValueError("eval_groups: R_extra has one entry per group")
        if (ideal_off is None) != (ideal_rel is None):
            raise ValueError("eval_groups: ideal_off and ideal_rel go together")
        io = ir = None
        n_ideal = 0
        if ideal_off is not None:
            io_h = np.ascontiguousarray(ideal_off.cpu().numpy() if isinstance(ideal_off, torch.Tensor) else ideal_off, dtype=np.int64)
            ir = self._i32(ideal_rel)
            if io_h.size != G + 1 or io_h[0] != 0 or (np.diff(io_h) < 0).any() or io_h[-1] != ir.numel():
                raise ValueError("eval_groups: ideal_off must be a CSR offset array over ideal_rel with G + 1 entries")
            io, n_ideal = self._i32(io_h), int(ir.numel())
            if ir.numel() == 0:
                ir = torch.zeros((1,), dtype=torch.int32, device=self.device)
        off = self._i32(off_h)
        out = {"scores": torch.zeros((n_cand,), dtype=torch.float32, device=self.device),
               "order": torch.zeros((n_cand,), dtype=torch.int32, device=self.device)}
        out.update({n: torch.zeros((G,), dtype=torch.int32, device=self.device) for n in ("hits1", "hits5", "first", "R")})
        out.update({n: torch.zeros((G,), dtype=torch.float32, device=self.device) for n in ("sp", "dcg", "idcg")})
        self._chk(self.lib.sgpt_eval_groups(self.handle, _p(emb_t), n_rows, d, mode_code, _p(scores_in), G, _p(off), n_cand, max_group,
                                            _p(qr), _p(cr), _p(rel), _p(rx), _p(io), _p(ir), n_ideal, _p(out["scores"]), _p(out["order"]),
                                            _p(out["hits1"]), _p(out["hits5"]), _p(out["first"]), _p(out["R"]), _p(out["sp"]),
                                            _p(out["dcg"]), _p(out["idcg"]), _stream_ptr(self.device)), "sgpt_eval_groups")
        return out

    def eval_pairs(self, score: torch.Tensor, label, check_nan: bool = True) -> dict:
        """include/sgpt_hip.h::sgpt_eval_pairs.  score fp32 [n]; label int [n] (> 0 positive, 0 negative, < 0 ranked but left out
        of the average precision).  -> {"rank2" int32 [n]: twice the tie-averaged ascending rank; "n_pos", "n_used" int64 [1];
        "ap_num" float64 [1]} on the device.  check_nan=True synchronises and raises ValueError on a NaN score."""
        score = score.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        lab = self._i32(label).reshape(-1)
        n = score.numel()
        if lab.numel() != n:
            raise ValueError(f"eval_pairs: {n} scores and {lab.numel()} labels")
        out = {"rank2": torch.zeros((n,), dtype=torch.int32, device=self.device),
               "n_pos": torch.zeros((1,), dtype=torch.int64, device=self.device),
               "n_used": torch.zeros((1,), dtype=torch.int64, device=self.device),
               "ap_num": torch.zeros((1,), dtype=torch.float64, device=self.device)}
        self._chk(self.lib.sgpt_eval_pairs(self.handle, _p(score), _p(lab), n, 1 if check_nan else 0, _p(out["rank2"]),
                                           _p(out["n_pos"]), _p(out["n_used"]), _p(out["ap_num"]), _stream_ptr(self.device)),
                  "sgpt_eval_pairs")
        return out

    # ---- measurement hooks (bench.py) ----
    def prof_enable(self, on: bool):
        self._chk(self.lib.sgpt_prof_enable(self.handle, 1 if on else 0), "sgpt_prof_enable")

    def prof_read(self, reset=True):
        n, ms, fl = C.c_int64(0), C.c_double(0), C.c_double(0)
        self._chk(self.lib.sgpt_prof_read(self.handle, C.byref(n), C.byref(ms), C.byref(fl), 1 if reset else 0),
                  "sgpt_prof_read")
        return int(n.value), float(ms.value), float(fl.value)
