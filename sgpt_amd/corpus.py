"""The corpus kinds a search can run against besides plain rows -- QuantizedCorpus (fp8), Uint8Corpus, BinaryCorpus, IVFCorpus, IVFUint8Corpus -- in one place:
what each holds, what a search over it may ask (`check_search`, device-free), how it is scored (`score_topk`, the C entry of its
format) and how it is built from embeddings (`CorpusBuilders`, the methods Context inherits).  util.semantic_search and
Context.score_topk dispatch on CORPUS_KINDS once and know no kind by name.
`_rt` is sgpt_amd.runtime, looked up at call time: get_context and _stream_ptr are what tests replace to keep a call off the device."""
import copy
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch


def _p(t):
    return _rt._p(t)


def _stream_ptr(device):
    return _rt._stream_ptr(device)


def _score_kind(score_function) -> Optional[bool]:
    """True: cos_sim, False: dot_score, None: an arbitrary callable."""
    from . import util
    if score_function in (util.cos_sim, util.pytorch_cos_sim):
        return True
    return False if score_function is util.dot_score else None


class _CodesCorpus:
    """What the two kinds that keep the rows' norms share (fp8, uint8): `codes` [N, ...] and `normalized`."""
    default_rescore = "sign"         # (score_topk's default: re-scoring belongs to a BinaryCorpus)

    def __len__(self) -> int:
        return int(self.codes.shape[0])

    @property
    def data(self) -> torch.Tensor:
        """The tensor that says where the corpus lives."""
        return self.codes

    def check_search(self, score_function, top_k: int) -> bool:
        """What semantic_search may ask of this corpus, before anything reaches for the device -> are the queries to be normalised:
        cos_sim over normalised rows, dot_score over raw ones."""
        cosine = _score_kind(score_function)
        if cosine is None:
            raise ValueError(f"semantic_search over a {type(self).__name__} scores with cos_sim or dot_score; an arbitrary score function needs "
                             "the de-quantised rows (corpus.dequantize())")
        if cosine != bool(self.normalized):
            raise ValueError("semantic_search: cos_sim needs a corpus quantised with normalize=True, dot_score one with normalize=False "
                             f"(this one has normalize={bool(self.normalized)})")
        return cosine


def _no_rescore(rescore, rescore_multiplier):
    if rescore != "sign" or rescore_multiplier != 4:
        raise ValueError("score_topk: rescore / rescore_multiplier apply to a BinaryCorpus only")


@dataclass
class QuantizedCorpus(_CodesCorpus):
    """A corpus held as fp8: `codes` uint8 [N, d] (OCP e4m3fn) and `scale` fp32 [N], one power of two per document (the format of
    include/sgpt_hip.h::sgpt_score_topk_q8; document n = codes[n] * scale[n]).  `normalized`: the rows were L2-normalised before
    quantisation (cosine scores) or not (dot scores).  Built by Context.quantize_corpus / util.quantize_embeddings."""
    codes: torch.Tensor
    scale: torch.Tensor
    normalized: bool = True
    dim: Optional[int] = None        # width of the embeddings; codes carry zero columns up to the next multiple of 8 (None: no padding)

    @property
    def nbytes(self) -> int:
        return self.codes.numel() * self.codes.element_size() + self.scale.numel() * self.scale.element_size()

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        """The rows the scorer sees, codes * scale, on the device: exact in fp32, and in f16 / bf16 while codes * scale is a value
        of that format (unit rows are).  As wide as `codes` (zero columns behind `dim` included)."""
        return _rt.get_context(self.codes.device).fp8_dequantize_rows(self.codes, self.scale, out_dtype=dtype)

    def score_topk(self, ctx, q, k, idx_base, run, dtype, rescore, rescore_multiplier):
        _no_rescore(rescore, rescore_multiplier)
        if dtype not in (None, torch.float16):
            raise ValueError(f"a QuantizedCorpus is scored with f16 queries: dtype must be None or torch.float16, got {dtype}")
        if q.shape[1] != self.codes.shape[1] and q.shape[1] == self.dim:
            q = torch.nn.functional.pad(q, (0, self.codes.shape[1] - q.shape[1]))
        q = ctx._operand(q, torch.float16)
        codes = self.codes.to(ctx.device).contiguous()
        scale = self.scale.to(device=ctx.device, dtype=torch.float32).contiguous()
        nq, d = q.shape
        N, d2 = codes.shape
        if d != d2:
            raise ValueError(f"embedding dims differ: {d} vs {d2}")
        val, idx, n_run = ctx._run_list(run, nq, k)
        n_out = C.c_int32(0)
        ctx._chk(ctx.lib.sgpt_score_topk_q8(ctx.handle, _p(q), _p(codes), _p(scale), nq, N, d, k, idx_base, _p(val), _p(idx),
                                            n_run, C.byref(n_out), _stream_ptr(ctx.device)), "sgpt_score_topk_q8")
        return val, idx, int(n_out.value)


class Uint8Corpus(_CodesCorpus):
    """A corpus held as uint8 codes with one range per dimension (include/sgpt_hip.h::sgpt_score_topk_u8; sentence-transformers'
    precision="uint8"): `codes` uint8 [N, ld], ld = ceil(dim / 128) * 128, pad columns 128; `start`, `step` fp32 [ld], pad columns 0;
    document n = start + codes[n] * step.  `normalized`: the rows were L2-normalised before quantisation (cosine scores) or not (dot
    scores).  Built by Context.scalar_quantize_corpus / util.quantize_embeddings(precision="uint8")."""

    def __init__(self, codes: torch.Tensor, start: torch.Tensor, step: torch.Tensor, normalized: bool = True, dim: Optional[int] = None):
        if codes.dim() != 2 or codes.dtype != torch.uint8 or codes.shape[1] == 0 or codes.shape[1] % 128:
            raise ValueError(f"Uint8Corpus: codes are uint8 [N, ld] with ld % 128 == 0, got {codes.dtype} {tuple(codes.shape)}")
        ld = int(codes.shape[1])
        dim = ld if dim is None else int(dim)
        if dim < 1 or dim > ld or (dim + 127) // 128 * 128 != ld:
            raise ValueError(f"Uint8Corpus: {ld} bytes per row do not hold dim = {dim} (ld = ceil(dim / 128) * 128)")
        if tuple(start.shape) != (ld,) or tuple(step.shape) != (ld,):
            raise ValueError(f"Uint8Corpus: start and step must be [{ld}], got {tuple(start.shape)} and {tuple(step.shape)}")
        self.codes, self.start, self.step, self.normalized, self.dim = codes, start, step, bool(normalized), dim

    @property
    def nbytes(self) -> int:
        return self.codes.numel() + self.start.numel() * self.start.element_size() + self.step.numel() * self.step.element_size()

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        """The rows the scorer stands for, start + codes * step (product and sum each rounded once in fp32, then to `dtype`), on the
        device.  As wide as `codes` (zero columns behind `dim` included)."""
        return _rt.get_context(self.codes.device).u8_dequantize_rows(self.codes, self.start, self.step, out_dtype=dtype)

    def codes_int8(self) -> torch.Tensor:
        """sentence-transformers' "int8" view of the same levels: codes - 128 as int8 [N, dim]."""
        return (self.codes[:, :self.dim].to(torch.int16) - 128).to(torch.int8)

    def score_topk(self, ctx, q, k, idx_base, run, dtype, rescore, rescore_multiplier):
        _no_rescore(rescore, rescore_multiplier)
        if dtype is not None:
            raise ValueError(f"a Uint8Corpus is scored from fp32 queries (the kernel pre-scales them itself): dtype must be None, got {dtype}")
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"embedding dims differ: {tuple(q.shape)[-1]} vs {self.dim}")
        q = ctx._dev_f32(q)
        codes, start, step = ctx._u8_operands(self)
        nq, d = q.shape
        N, ld = codes.shape
        val, idx, n_run = ctx._run_list(run, nq, k)
        n_out = C.c_int32(0)
        # groups of 64 queries, each re-streaming the codes (the pass is HBM-bound there); the running list is chained per group
        for g0 in range(0, nq, 64):
            gn = min(64, nq - g0)
            ctx._chk(ctx.lib.sgpt_score_topk_u8(ctx.handle, _p(q[g0:g0 + gn]), _p(codes), _p(start), _p(step), gn, N, d, ld, k,
                                                idx_base, _p(val[g0:g0 + gn]), _p(idx[g0:g0 + gn]), n_run, C.byref(n_out),
                                                _stream_ptr(ctx.device)), "sgpt_score_topk_u8")
        return val, idx, int(n_out.value)


RESCORE_MODES = {"none": 0, "sign": 1, "fp8": 2}      # the modes of sgpt_score_topk_bits; "uint8" is an entry of its own (_bits_u8)


class BinaryCorpus:
    """A corpus held as packed sign bits: `bits` uint8 [N, ldb], ldb = 4 * ceil(dim / 32) (include/sgpt_hip.h::sgpt_score_topk_bits;
    dimension i of a document is bit 7 - i % 8 of byte i / 8, set when the element is > 0 -- numpy.packbits order, "ubinary" in
    sentence-transformers).  `center` fp32 [dim] or None: what was subtracted from the normalised rows before the signs were taken, and
    is subtracted from the queries; `fp8`: an optional QuantizedCorpus of the same (uncentred, normalised) rows for re-scoring; `u8`: an
    optional Uint8Corpus of the same rows for re-scoring (rescore="uint8": binary retrieval + int8 re-scoring, with or without a
    centre).  Built by Context.binarize_corpus / util.quantize_embeddings(precision="ubinary")."""

    def __init__(self, bits: torch.Tensor, dim: int, center: Optional[torch.Tensor] = None, fp8: Optional[QuantizedCorpus] = None,
                 u8: Optional[Uint8Corpus] = None):
        dim = int(dim)
        if bits.dim() != 2 or bits.dtype != torch.uint8:
            raise ValueError(f"BinaryCorpus: bits are uint8 [N, ldb], got {bits.dtype} {tuple(bits.shape)}")
        if dim < 1 or bits.shape[1] % 4 or bits.shape[1] < 4 * ((dim + 31) // 32):
            raise ValueError(f"BinaryCorpus: {bits.shape[1]} bytes per row do not hold dim = {dim} (ldb % 4 == 0, ldb >= 4 * ceil(dim / 32))")
        if center is not None and tuple(center.shape) != (dim,):
            raise ValueError(f"BinaryCorpus: center must be [{dim}], got {tuple(center.shape)}")
        if fp8 is not None and (not isinstance(fp8, QuantizedCorpus) or len(fp8) != bits.shape[0] or
                                fp8.codes.shape[1] != (dim + 7) // 8 * 8):
            raise ValueError("BinaryCorpus: fp8 must be a QuantizedCorpus of the same rows (codes [N, ceil(dim / 8) * 8])")
        if u8 is not None and (not isinstance(u8, Uint8Corpus) or len(u8) != bits.shape[0] or u8.dim != dim):
            raise ValueError(f"BinaryCorpus: u8 must be a Uint8Corpus of the same rows (N = {bits.shape[0]}, dim = {dim})")
        self.bits, self.dim, self.center, self.fp8, self.u8 = bits, dim, center, fp8, u8

    def __len__(self) -> int:
        return int(self.bits.shape[0])

    @property
    def nbytes(self) -> int:
        n = self.bits.numel()
        if self.center is not None:
            n += self.center.numel() * self.center.element_size()
        if self.fp8 is not None:
            n += self.fp8.nbytes
        if self.u8 is not None:
            n += self.u8.nbytes
        return n

    @property
    def data(self) -> torch.Tensor:
        return self.bits

    @property
    def default_rescore(self) -> str:
        """What semantic_search re-scores with: the uint8 copy where there is one (centred or not); else the fp8 copy where there is one
        and no centre (a centred corpus needs q - center for the bits and the raw q for the fp8 rows; that search call takes one
        matrix); the sign bits otherwise."""
        if self.u8 is not None:
            return "uint8"
        return "fp8" if self.fp8 is not None and self.center is None else "sign"

    def check_search(self, score_function, top_k: int) -> bool:
        """As _CodesCorpus.check_search: cos_sim only, and no deeper than the candidate lists of the Hamming stage."""
        if not _score_kind(score_function):
            raise ValueError("semantic_search over a BinaryCorpus scores with cos_sim only: sign bits carry no norms, so dot_score and "
                             "arbitrary score functions cannot be computed from them")
        if min(top_k, len(self)) > 1024:
            raise ValueError(f"semantic_search over a BinaryCorpus takes top_k <= 1024 (the candidate lists of the Hamming stage), got {top_k}")
        return True

    def score_topk(self, ctx, q, k, idx_base, run, dtype, rescore, rescore_multiplier):
        if rescore not in RESCORE_MODES and rescore != "uint8":
            raise ValueError(f"score_topk: rescore must be 'sign', 'none', 'fp8' or 'uint8', got {rescore!r}")
        if rescore == "fp8" and self.fp8 is None:
            raise ValueError("score_topk: rescore='fp8' needs a BinaryCorpus built with keep_fp8=True (corpus.fp8 is None)")
        if rescore == "uint8" and self.u8 is None:
            raise ValueError("score_topk: rescore='uint8' needs a BinaryCorpus built with keep_uint8=True (corpus.u8 is None)")
        if k < 1 or k > 1024:
            raise ValueError(f"score_topk over a BinaryCorpus takes 1 <= k <= 1024, got {k}")
        mode = RESCORE_MODES.get(rescore)
        kp = k if mode == 0 else min(1024, max(k, int(round(k * rescore_multiplier))))
        q = ctx._dev_f32(q)
        nq, d = q.shape
        if d != self.dim:
            raise ValueError(f"embedding dims differ: {d} vs {self.dim}")
        # sgpt_score_topk_bits takes ONE query matrix: it packs the stage-1 bits from it and re-scores with it.  A centred corpus needs the
        # bits of q - center, its fp8 copy the raw q: no single matrix serves both, and the raw one would search sign(q) against sign(x - center).
        if self.center is not None and mode == 2:
            raise ValueError("score_topk: rescore='fp8' is refused on a centred BinaryCorpus -- the stage-1 bits need q - center, the fp8 "
                             "rows the raw q, and sgpt_score_topk_bits takes one query matrix; use rescore='sign', or an uncentred corpus")
        f32 = dict(device=ctx.device, dtype=torch.float32)
        bits = self.bits.to(ctx.device).contiguous()
        N, ldb = bits.shape
        val, idx, n_run = ctx._run_list(run, nq, k)
        n_out = C.c_int32(0)
        tail = (idx_base, _p(val), _p(idx), n_run, C.byref(n_out), _stream_ptr(ctx.device))
        if rescore == "uint8":
            # an entry of its own: it takes the RAW q and the centre, packs the stage-1 bits of q - center and re-scores with q
            codes, start, step = ctx._u8_operands(self.u8)
            center = None if self.center is None else self.center.to(**f32).contiguous()
            ctx._chk(ctx.lib.sgpt_score_topk_bits_u8(ctx.handle, _p(q), _p(center), _p(bits), ldb, _p(codes), _p(start), _p(step), codes.shape[1],
                                                     nq, N, d, k, kp, *tail), "sgpt_score_topk_bits_u8")
        else:
            if self.center is not None:
                q = q - self.center.to(ctx.device)
            codes = scale = None
            if mode == 2:
                codes, scale = self.fp8.codes.to(ctx.device).contiguous(), self.fp8.scale.to(**f32).contiguous()
            ctx._chk(ctx.lib.sgpt_score_topk_bits(ctx.handle, _p(q), _p(bits), ldb, nq, N, d, k, kp, mode, _p(codes), _p(scale), *tail),
                     "sgpt_score_topk_bits")
        return val, idx, int(n_out.value)


IVF_CHUNK, IVF_MAX_DIM, IVF_MAX_LISTS = 256, 4096, 65536      # SGPT_IVF_CHUNK, SGPT_IVF_MAX_DIM, SGPT_IVF_MAX_LISTS of include/sgpt_hip.h


class _IVFLists:
    """What the two IVF kinds share (f16 lists, uint8 lists): `centroids` [nlist, d], `nprobe` and its range, and what a search over
    lists may ask."""
    default_rescore = "sign"         # (score_topk's default: re-scoring belongs to a BinaryCorpus)

    @property
    def nlist(self) -> int:
        return int(self.centroids.shape[0])

    def _check_nprobe(self, nprobe) -> int:
        top = min(self.nlist, 1024)
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or nprobe < 1 or nprobe > top:
            raise ValueError(f"{type(self).__name__}: nprobe must be an integer in [1, {top}] (min(nlist, 1024)), got {nprobe!r}")
        return int(nprobe)

    def with_nprobe(self, nprobe: int):
        """The same index (shared tensors) probing `nprobe` lists per query."""
        view = copy.copy(self)
        view.nprobe = self._check_nprobe(nprobe)
        return view

    def check_search(self, score_function, top_k: int) -> bool:
        """As _CodesCorpus.check_search: cos_sim only (the rows are normalised, k-means is spherical), top_k <= 1024, nprobe in range."""
        name = type(self).__name__
        if not _score_kind(score_function):
            raise ValueError(f"semantic_search over an {name} scores with cos_sim only: the lists come from spherical k-means over "
                             "L2-normalised rows, so dot_score and arbitrary score functions are not served")
        if top_k > 1024:
            raise ValueError(f"semantic_search over an {name} takes top_k <= 1024, got {top_k}")
        self._check_nprobe(self.nprobe)
        return True

    def _search_operands(self, ctx, q, k: int, run, return_probes: bool):
        """The checks and buffers of a search call: (q fp32 on the device, nprobe, values, indices, n_run, probes or None)."""
        nprobe = self._check_nprobe(self.nprobe)
        if k < 1 or k > 1024:
            raise ValueError(f"score_topk over an {type(self).__name__} takes 1 <= k <= 1024, got {k}")
        q = ctx._dev_f32(q)
        if q.shape[1] != self.dim:
            raise ValueError(f"embedding dims differ: {q.shape[1]} vs {self.dim}")
        val, idx, n_run = ctx._run_list(run, q.shape[0], k)
        probes = torch.empty((q.shape[0], nprobe), dtype=torch.int64, device=ctx.device) if return_probes else None
        return q, nprobe, val, idx, n_run, probes

    def score_topk(self, ctx, q, k, idx_base, run, dtype, rescore, rescore_multiplier):
        _no_rescore(rescore, rescore_multiplier)
        if dtype is not None:
            raise ValueError(f"an {type(self).__name__} is scored from fp32 queries (the call rounds them to f16 for the centroids itself): dtype "
                             f"must be None, got {dtype}")
        return self.search(ctx, q, k, idx_base, run)


def _check_lists(name: str, centroids, N: int, ids, offsets, centroids16, max_list) -> Tuple[torch.Tensor, int]:
    """What the constructors of the two IVF kinds ask of the parts they share -> (centroids16, max_list)."""
    nlist, d = (int(v) for v in centroids.shape)
    if ids.dtype != torch.int64 or tuple(ids.shape) != (N,):
        raise ValueError(f"{name}: ids must be int64 [{N}], got {ids.dtype} {tuple(ids.shape)}")
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (nlist + 1,):
        raise ValueError(f"{name}: offsets must be int64 [{nlist + 1}], got {offsets.dtype} {tuple(offsets.shape)}")
    if centroids16 is None:
        centroids16 = centroids.to(torch.float16)      # (a conversion: round-to-nearest-even, as sgpt_f32_to_16)
    if centroids16.dtype != torch.float16 or tuple(centroids16.shape) != (nlist, d):
        raise ValueError(f"{name}: centroids16 must be f16 [{nlist}, {d}], got {centroids16.dtype} {tuple(centroids16.shape)}")
    max_list = int(max_list)
    if max_list < 0 or max_list > N:
        raise ValueError(f"{name}: max_list (the longest list) must lie in [0, {N}], got {max_list}")
    return centroids16, max_list


def _check_centroids(name: str, centroids) -> Tuple[int, int]:
    if centroids.dim() != 2 or centroids.dtype != torch.float32 or centroids.shape[0] == 0:
        raise ValueError(f"{name}: centroids are fp32 [nlist, d], got {centroids.dtype} {tuple(centroids.shape)}")
    nlist, d = (int(v) for v in centroids.shape)
    if d == 0 or d % 8 or d > IVF_MAX_DIM or nlist > IVF_MAX_LISTS:
        raise ValueError(f"{name}: d % 8 == 0, d <= {IVF_MAX_DIM} and nlist <= {IVF_MAX_LISTS} are required, got d = {d}, nlist = {nlist}")
    return nlist, d


class IVFCorpus(_IVFLists):
    """A corpus held as inverted lists over spherical k-means centroids (include/sgpt_hip.h::sgpt_ivf_search): `centroids` fp32 [nlist, d]
    unit rows and `centroids16`, their f16 rounding; `rows` f16 [N, d] in list-major order, list c = rows[offsets[c]:offsets[c + 1]];
    `ids` int64 [N], the original row number of every stored row, ascending inside every list; `offsets` int64 [nlist + 1]; `max_list`, a
    host int: the longest list (the launch geometry, so a search never synchronises); `nprobe`: how many lists a query scans.  A search
    scores the centroids with the f16 scorer and scans the nprobe best lists with fp32 accumulation: cosine only, approximate -- a hit
    outside the probed lists is missed, and slots that found no row come back as (-inf, -1).  Built by Context.ivf_index /
    util.build_ivf_index."""
    def __init__(self, centroids: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, max_list: int,
                 nprobe: Optional[int] = None, centroids16: Optional[torch.Tensor] = None):
        nlist, d = _check_centroids("IVFCorpus", centroids)
        if rows.dim() != 2 or rows.dtype != torch.float16 or rows.shape[0] == 0 or rows.shape[1] != d:
            raise ValueError(f"IVFCorpus: rows are f16 [N, {d}] with N >= 1, got {rows.dtype} {tuple(rows.shape)}")
        centroids16, max_list = _check_lists("IVFCorpus", centroids, int(rows.shape[0]), ids, offsets, centroids16, max_list)
        self.centroids, self.centroids16, self.rows, self.ids, self.offsets, self.max_list = centroids, centroids16, rows, ids, offsets, max_list
        self.nprobe = self._check_nprobe(min(nlist, 32) if nprobe is None else nprobe)

    @property
    def dim(self) -> int:
        return int(self.centroids.shape[1])

    def __len__(self) -> int:
        return int(self.rows.shape[0])

    @property
    def data(self) -> torch.Tensor:
        return self.rows

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.centroids, self.centroids16, self.rows, self.ids, self.offsets))

    def search(self, ctx, q, k: int, idx_base: int = 0, run=None, return_probes: bool = False):
        """sgpt_ivf_search: q [nq, d] L2-normalised (upcast to fp32) -> (values fp32 [nq, k], indices int64 [nq, k], n_valid[, the probe
        sets int64 [nq, nprobe]]); slots that found no row are (-inf, -1) inside n_valid."""
        q, nprobe, val, idx, n_run, probes = self._search_operands(ctx, q, k, run, return_probes)
        dev = dict(device=ctx.device)
        c16, rows = self.centroids16.to(**dev).contiguous(), self.rows.to(**dev).contiguous()
        ids, offsets = self.ids.to(**dev).contiguous(), self.offsets.to(**dev).contiguous()
        n_out = C.c_int32(0)
        ctx._chk(ctx.lib.sgpt_ivf_search(ctx.handle, _p(q), _p(c16), _p(rows), _p(ids), _p(offsets), q.shape[0], len(self), self.dim, self.nlist,
                                         self.max_list, nprobe, k, idx_base, _p(val), _p(idx), n_run, C.byref(n_out), _p(probes),
                                         _stream_ptr(ctx.device)), "sgpt_ivf_search")
        return (val, idx, int(n_out.value), probes) if return_probes else (val, idx, int(n_out.value))


class IVFUint8Corpus(_IVFLists):
    """An IVFCorpus whose lists hold uint8 codes with one range per dimension instead of f16 rows (include/sgpt_hip.h::sgpt_ivf_search_u8;
    IVF-SQ8): `centroids`, `centroids16`, `ids`, `offsets`, `max_list`, `nprobe` as there; `codes` uint8 [N, ld] in list-major order,
    ld = ceil(dim / 128) * 128, pad columns 128; `start`, `step` fp32 [ld], pad columns 0 -- stored row n stands for start + codes[n] *
    step, the format of a Uint8Corpus.  ld bytes per row instead of 2 dim.  The probe sets are the f16 index's; the values are those of
    the de-quantised rows.  Built by Context.ivf_index(precision="uint8") / util.build_ivf_index(precision="uint8")."""

    def __init__(self, centroids: torch.Tensor, codes: torch.Tensor, start: torch.Tensor, step: torch.Tensor, ids: torch.Tensor,
                 offsets: torch.Tensor, max_list: int, nprobe: Optional[int] = None, centroids16: Optional[torch.Tensor] = None,
                 dim: Optional[int] = None):
        nlist, d = _check_centroids("IVFUint8Corpus", centroids)
        if codes.dim() != 2 or codes.dtype != torch.uint8 or codes.shape[0] == 0 or codes.shape[1] == 0 or codes.shape[1] % 128:
            raise ValueError(f"IVFUint8Corpus: codes are uint8 [N, ld] with N >= 1 and ld % 128 == 0, got {codes.dtype} {tuple(codes.shape)}")
        N, ld = (int(v) for v in codes.shape)
        dim = d if dim is None else int(dim)
        if dim != d or (dim + 127) // 128 * 128 != ld:
            raise ValueError(f"IVFUint8Corpus: {ld} bytes per row do not hold dim = {dim} of centroids [{nlist}, {d}] (ld = ceil(dim / 128) * 128)")
        for name, t in (("start", start), ("step", step)):
            if t.dtype != torch.float32 or tuple(t.shape) != (ld,):
                raise ValueError(f"IVFUint8Corpus: {name} must be fp32 [{ld}], got {t.dtype} {tuple(t.shape)}")
        centroids16, max_list = _check_lists("IVFUint8Corpus", centroids, N, ids, offsets, centroids16, max_list)
        self.centroids, self.centroids16, self.codes, self.start, self.step = centroids, centroids16, codes, start, step
        self.ids, self.offsets, self.max_list, self.dim = ids, offsets, max_list, dim
        self.nprobe = self._check_nprobe(min(nlist, 32) if nprobe is None else nprobe)

    def __len__(self) -> int:
        return int(self.codes.shape[0])

    @property
    def data(self) -> torch.Tensor:
        return self.codes

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.centroids, self.centroids16, self.codes, self.start, self.step, self.ids,
                                                          self.offsets))

    def as_uint8_corpus(self) -> Uint8Corpus:
        """The same codes (no copy) as a Uint8Corpus in LIST-MAJOR order: document p of it is row ids[p] of the embeddings.  What
        Context.rescore_u8 and the full uint8 scan take."""
        return Uint8Corpus(self.codes, self.start, self.step, True, self.dim)

    def dequantize(self, dtype=torch.float32) -> torch.Tensor:
        """The rows the scan stands for, start + codes * step, in list-major order (Uint8Corpus.dequantize)."""
        return self.as_uint8_corpus().dequantize(dtype)

    def search(self, ctx, q, k: int, idx_base: int = 0, run=None, return_probes: bool = False):
        """sgpt_ivf_search_u8: as IVFCorpus.search; a running list must hold values of this kind."""
        q, nprobe, val, idx, n_run, probes = self._search_operands(ctx, q, k, run, return_probes)
        dev = dict(device=ctx.device)
        c16 = self.centroids16.to(**dev).contiguous()
        codes, start, step = ctx._u8_operands(self)
        ids, offsets = self.ids.to(**dev).contiguous(), self.offsets.to(**dev).contiguous()
        n_out = C.c_int32(0)
        ctx._chk(ctx.lib.sgpt_ivf_search_u8(ctx.handle, _p(q), _p(c16), _p(codes), _p(start), _p(step), _p(ids), _p(offsets), q.shape[0],
                                            len(self), self.dim, codes.shape[1], self.nlist, self.max_list, nprobe, k, idx_base, _p(val),
                                            _p(idx), n_run, C.byref(n_out), _p(probes), _stream_ptr(ctx.device)), "sgpt_ivf_search_u8")
        return (val, idx, int(n_out.value), probes) if return_probes else (val, idx, int(n_out.value))


CORPUS_KINDS = (QuantizedCorpus, Uint8Corpus, BinaryCorpus, IVFCorpus, IVFUint8Corpus)


def check_ivf_precision(who: str, precision, ranges, calibration_embeddings) -> None:
    """What an IVF build may be asked to hold in its lists (device-free): "f16" rows or "uint8" codes with their ranges."""
    if precision == "int8":
        raise ValueError(f"{who}: precision 'int8' is not built -- the same scalar quantisation is precision=\"uint8\" (its codes are the "
                         "int8 codes + 128)")
    if precision not in ("f16", "uint8"):
        raise ValueError(f"{who}: unknown precision {precision!r} (only 'f16' and 'uint8' lists are built)")
    if precision == "f16" and (ranges is not None or calibration_embeddings is not None):
        raise ValueError(f"{who}: ranges / calibration_embeddings belong to precision='uint8'")
    if ranges is not None and calibration_embeddings is not None:
        raise ValueError(f"{who}: give ranges or calibration_embeddings, not both")


def _matrix(emb, who: str) -> torch.Tensor:
    if not isinstance(emb, torch.Tensor):
        emb = torch.as_tensor(np.asarray(emb))
    if emb.dim() != 2 or emb.shape[0] == 0 or emb.shape[1] == 0:
        raise ValueError(f"{who} needs a non-empty [N, d] matrix, got {tuple(emb.shape)}")
    return emb


class CorpusBuilders:
    """The methods of Context that build a corpus kind from embeddings, and the row conversions they are made of."""

    def _row_blocks(self, emb: torch.Tensor, normalize: bool, block_rows: int):
        """(r0, fp32 rows [r0, r0 + block_rows) of emb on the device, L2-normalised or as they are): the fp32 copy of a large corpus never
        exists whole on the device, and `emb` may live on the host."""
        for r0 in range(0, emb.shape[0], block_rows):
            rows = self._dev_f32(emb[r0:r0 + block_rows])
            yield r0, self.l2_normalize(rows) if normalize else rows

    # ---- fp8 corpus ----
    def _fp8_quantize_block(self, rows: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor):
        """fp32 rows [n, d0] -> codes [n, d], scale [n] (row views of a corpus's): sgpt_fp8_quantize_rows behind zero columns up to d."""
        n, d = codes.shape
        if d != rows.shape[1]:
            rows = torch.nn.functional.pad(rows, (0, d - rows.shape[1]))
        self._chk(self.lib.sgpt_fp8_quantize_rows(self.handle, _p(rows), n, d, _p(codes), _p(scale),
                                                  _stream_ptr(self.device)), "sgpt_fp8_quantize_rows")

    def _fp8_empty(self, N: int, d0: int) -> Tuple[torch.Tensor, torch.Tensor]:
        d = (d0 + 7) // 8 * 8          # the scorer takes d % 8 == 0: zero columns (zero codes) change no score
        return torch.empty((N, d), dtype=torch.uint8, device=self.device), torch.empty((N,), dtype=torch.float32, device=self.device)

    def quantize_corpus(self, emb, normalize: bool = True, block_rows: int = 65536) -> QuantizedCorpus:
        """Embeddings [N, d] -> QuantizedCorpus (d padded with zero columns to a multiple of 8): rows L2-normalised (normalize=True, cosine search) or taken as they are
        (dot scores), then sgpt_fp8_quantize_rows.  Works in blocks of `block_rows` rows, so the fp32 (normalised) copy of a large
        corpus never exists whole on the device; `emb` may live on the host."""
        emb = _matrix(emb, "quantize_corpus")
        N, d0 = emb.shape
        codes, scale = self._fp8_empty(N, d0)
        for r0, rows in self._row_blocks(emb, normalize, block_rows):
            self._fp8_quantize_block(rows, codes[r0:r0 + block_rows], scale[r0:r0 + block_rows])
        return QuantizedCorpus(codes, scale, bool(normalize), d0)

    # ---- uint8 corpus: scalar quantisation with one range per dimension ----
    def u8_col_minmax(self, x, run: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Column min / max of fp32 rows [n, d] (NaN-propagating); run = (min, max) of earlier blocks of rows, updated in place."""
        x = self._dev_f32(x)
        n, d = x.shape
        if n == 0 or d == 0:
            raise ValueError(f"u8_col_minmax needs a non-empty [n, d] matrix, got {tuple(x.shape)}")
        if run is None:
            mn = torch.empty((d,), dtype=torch.float32, device=self.device)
            mx = torch.empty((d,), dtype=torch.float32, device=self.device)
        else:
            mn, mx = run
        self._chk(self.lib.sgpt_u8_col_minmax(self.handle, _p(x), n, d, 0 if run is None else 1, _p(mn), _p(mx),
                                              _stream_ptr(self.device)), "sgpt_u8_col_minmax")
        return mn, mx

    def u8_quantize_rows(self, x, start: torch.Tensor, step: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 rows [n, d] -> uint8 [n, ld] by the rule of include/sgpt_hip.h; start / step fp32 [ld], ld = ceil(d / 128) * 128."""
        x = self._dev_f32(x)
        n, d = x.shape
        ld = int(start.shape[0])
        if out is None:
            out = torch.empty((n, ld), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.sgpt_u8_quantize_rows(self.handle, _p(x), n, d, ld, _p(start), _p(step), _p(out),
                                                 _stream_ptr(self.device)), "sgpt_u8_quantize_rows")
        return out

    def u8_dequantize_rows(self, codes: torch.Tensor, start: torch.Tensor, step: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
        codes = codes.to(device=self.device, dtype=torch.uint8).contiguous()
        start = start.to(device=self.device, dtype=torch.float32).contiguous()
        step = step.to(device=self.device, dtype=torch.float32).contiguous()
        n, ld = codes.shape
        out = torch.empty((n, ld), dtype=out_dtype, device=self.device)
        self._chk(self.lib.sgpt_u8_dequantize_rows(self.handle, _p(codes), n, ld, _p(start), _p(step), _p(out), _rt.DT_CODE[out_dtype],
                                                   _stream_ptr(self.device)), "sgpt_u8_dequantize_rows")
        return out

    def u8_prepare_queries(self, q, start: torch.Tensor, step: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The scorer's query prologue on its own (tests): q fp32 [nq <= 64, d] -> (q'' f16 [64, ld], qscale fp32 [64], qbias fp32 [64])."""
        q = self._dev_f32(q)
        nq, d = q.shape
        ld = int(start.shape[0])
        qpad = torch.empty((64, ld), dtype=torch.float16, device=self.device)
        qscale = torch.empty((64,), dtype=torch.float32, device=self.device)
        qbias = torch.empty((64,), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_u8_prepare_queries(self.handle, _p(q), _p(start), _p(step), nq, d, ld, _p(qpad), _p(qscale), _p(qbias),
                                                   _stream_ptr(self.device)), "sgpt_u8_prepare_queries")
        return qpad, qscale, qbias

    def scalar_quantize_corpus(self, emb, normalize: bool = True, ranges=None, calibration_embeddings=None,
                               block_rows: int = 65536) -> Uint8Corpus:
        """Embeddings [N, d] -> Uint8Corpus: rows L2-normalised (normalize=True, cosine search) or taken as they are (dot scores), then
        quantised to 256 levels between each column's min and max.  The ranges are `ranges` ([2, d]: min row, max row -- the layout of
        sentence-transformers), or those of `calibration_embeddings` (normalised like the corpus), or the corpus's own; elements outside
        them clamp.  Non-finite ranges (a NaN or inf in the rows they come from) raise ValueError.  Works in blocks of `block_rows` rows,
        as quantize_corpus does; `emb` may live on the host."""
        emb = _matrix(emb, "scalar_quantize_corpus")
        N, d = emb.shape
        start, step = self._u8_ranges(emb, normalize, ranges, calibration_embeddings, block_rows)
        codes = torch.empty((N, start.shape[0]), dtype=torch.uint8, device=self.device)
        for r0, rows in self._row_blocks(emb, normalize, block_rows):
            self.u8_quantize_rows(rows, start, step, out=codes[r0:r0 + block_rows])
        return Uint8Corpus(codes, start, step, bool(normalize), d)

    def _u8_ranges(self, emb: torch.Tensor, normalize: bool, ranges, calibration_embeddings, block_rows: int,
                   who: str = "scalar_quantize_corpus", blocks=None):
        """(start, step) fp32 [ld] of scalar_quantize_corpus's rule for the rows of emb [N, d]: from `ranges`, from
        `calibration_embeddings`, or from emb itself.  blocks(src): the fp32 row blocks of a source as they are quantised (default: _row_blocks
        under `normalize`)."""
        if blocks is None:
            def blocks(src):
                return (rows for _, rows in self._row_blocks(src, normalize, block_rows))
        if ranges is not None and calibration_embeddings is not None:
            raise ValueError(f"{who}: give ranges or calibration_embeddings, not both")
        N, d = emb.shape
        ld = (d + 127) // 128 * 128
        if ranges is not None:
            ranges = torch.as_tensor(np.asarray(ranges.cpu() if isinstance(ranges, torch.Tensor) else ranges)).to(torch.float32)
            if tuple(ranges.shape) != (2, d):
                raise ValueError(f"{who}: ranges must be [2, {d}] (min row, max row), got {tuple(ranges.shape)}")
            mn, mx = ranges[0].to(self.device).contiguous(), ranges[1].to(self.device).contiguous()
        else:
            src = emb if calibration_embeddings is None else calibration_embeddings
            if not isinstance(src, torch.Tensor):
                src = torch.as_tensor(np.asarray(src))
            if src.dim() != 2 or src.shape[0] == 0 or src.shape[1] != d:
                raise ValueError(f"{who}: calibration_embeddings must be a non-empty [n, {d}] matrix, got {tuple(src.shape)}")
            run = None
            for rows in blocks(src):
                run = self.u8_col_minmax(rows, run)
            mn, mx = run
        if not bool(torch.isfinite(mn).all()) or not bool(torch.isfinite(mx).all()) or bool((mx < mn).any()):
            raise ValueError(f"{who}: the ranges are not finite, or a max lies below its min (a NaN or inf in the rows they "
                             "come from)")
        start = torch.zeros((ld,), dtype=torch.float32, device=self.device)
        step = torch.zeros((ld,), dtype=torch.float32, device=self.device)
        start[:d] = mn
        step[:d] = (mx - mn) / torch.full_like(mx, 255.0)      # (a tensor divisor: one IEEE division per column, not a multiplication by 1 / 255)
        if not bool(torch.isfinite(step).all()):
            raise ValueError(f"{who}: max - min overflows fp32")
        return start, step

    def rescore_u8(self, q, corpus_u8: Uint8Corpus, idx: torch.Tensor, idx_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """The values <q_i, document idx[i][j]> of candidate lists against a Uint8Corpus (include/sgpt_hip.h::sgpt_u8_rescore): q [nq, dim]
        (upcast to fp32), idx int64 [nq, m] of document indices idx_base + n -> (values fp32 [nq, m], indices int64 [nq, m]), slot for
        slot and unsorted; a slot with idx < 0 or idx - idx_base outside [0, N) gives (-inf, -1).  The candidates may come from any
        first stage."""
        q = self._dev_f32(q)
        if q.dim() != 2 or q.shape[1] != corpus_u8.dim:
            raise ValueError(f"embedding dims differ: {tuple(q.shape)[-1]} vs {corpus_u8.dim}")
        if idx.dim() != 2 or idx.shape[0] != q.shape[0] or idx.shape[1] == 0 or idx.dtype != torch.int64:
            raise ValueError(f"rescore_u8: idx must be int64 [{q.shape[0]}, m], got {idx.dtype} {tuple(idx.shape)}")
        idx = idx.to(self.device).contiguous()
        codes, start, step = self._u8_operands(corpus_u8)
        nq, d = q.shape
        m = int(idx.shape[1])
        val = torch.empty((nq, m), dtype=torch.float32, device=self.device)
        out = torch.empty((nq, m), dtype=torch.int64, device=self.device)
        self._chk(self.lib.sgpt_u8_rescore(self.handle, _p(q), _p(codes), _p(start), _p(step), nq, codes.shape[0], d, codes.shape[1], _p(idx), m,
                                           m, idx_base, _p(val), _p(out), _stream_ptr(self.device)), "sgpt_u8_rescore")
        return val, out

    # ---- binary (1-bit) corpus: packed sign bits ----
    def pack_sign_bits(self, x, center: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 rows [n, d] -> uint8 [n, 4 * ceil(d / 32)]: the sign bits of x - center (center None: of x) in numpy.packbits order, pad
        bits zero (include/sgpt_hip.h::sgpt_pack_sign_bits)."""
        x = self._dev_f32(x)
        n, d = x.shape
        if n == 0 or d == 0:
            raise ValueError(f"pack_sign_bits needs a non-empty [n, d] matrix, got {tuple(x.shape)}")
        ldb = 4 * ((d + 31) // 32)
        if center is not None:
            center = center.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(center.shape) != (d,):
                raise ValueError(f"pack_sign_bits: center must be [{d}], got {tuple(center.shape)}")
        if out is None:
            out = torch.empty((n, ldb), dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != (n, ldb) or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"pack_sign_bits: out must be a contiguous uint8 [{n}, {ldb}] tensor on {self.device}, got {out.dtype} "
                             f"{tuple(out.shape)} on {out.device}")
        self._chk(self.lib.sgpt_pack_sign_bits(self.handle, _p(x), n, d, _p(center), _p(out), ldb, _stream_ptr(self.device)),
                  "sgpt_pack_sign_bits")
        return out

    def binarize_corpus(self, emb, normalize: bool = True, center=None, keep_fp8: bool = False,
                        block_rows: int = 65536, keep_uint8: bool = False, ranges=None, calibration_embeddings=None) -> BinaryCorpus:
        """Embeddings [N, d] -> BinaryCorpus: rows L2-normalised, the centre subtracted, signs packed.  center: None | "mean" (the mean of
        the normalised rows, kept on the corpus so that queries get the same shift) | a [d] tensor.  keep_fp8: the same normalised,
        uncentred rows are also quantised as quantize_corpus does, block by block beside the bits (re-scoring with rescore="fp8").
        keep_uint8: they are also quantised by scalar_quantize_corpus's rule (its `ranges` / `calibration_embeddings`), likewise
        (re-scoring with rescore="uint8", with or without a centre).  Works in blocks of `block_rows` rows, as
        quantize_corpus does; `emb` may live on the host.  Sign bits carry no norms: normalize=False is refused."""
        if not keep_uint8 and (ranges is not None or calibration_embeddings is not None):
            raise ValueError("binarize_corpus: ranges / calibration_embeddings belong to keep_uint8=True")
        if keep_fp8 and center is not None:
            raise ValueError("binarize_corpus: keep_fp8 with a centre is refused -- fp8 re-scoring needs the raw query, the centred bits "
                             "q - center, and the search call takes one query matrix (score_topk)")
        if not normalize:
            raise ValueError("binarize_corpus: normalize=False is refused -- sign bits carry no norms, the search is a cosine search")
        emb = _matrix(emb, "binarize_corpus")
        N, d = emb.shape
        if isinstance(center, str):
            if center != "mean":
                raise ValueError(f"binarize_corpus: center must be None, 'mean' or a [d] tensor, got {center!r}")
            acc = torch.zeros((d,), dtype=torch.float64, device=self.device)
            for _, rows in self._row_blocks(emb, True, block_rows):
                acc += rows.sum(dim=0, dtype=torch.float64)
            center = (acc / N).to(torch.float32)
        elif center is not None:
            center = torch.as_tensor(center).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(center.shape) != (d,):
                raise ValueError(f"binarize_corpus: center must be [{d}], got {tuple(center.shape)}")
        bits = torch.empty((N, 4 * ((d + 31) // 32)), dtype=torch.uint8, device=self.device)
        fp8 = QuantizedCorpus(*self._fp8_empty(N, d), True, d) if keep_fp8 else None
        u8 = None
        if keep_uint8:
            start, step = self._u8_ranges(emb, True, ranges, calibration_embeddings, block_rows)
            u8 = Uint8Corpus(torch.empty((N, start.shape[0]), dtype=torch.uint8, device=self.device), start, step, True, d)
        for r0, rows in self._row_blocks(emb, True, block_rows):
            r1 = r0 + rows.shape[0]
            self.pack_sign_bits(rows, center, out=bits[r0:r1])
            if keep_uint8:
                self.u8_quantize_rows(rows, u8.start, u8.step, out=u8.codes[r0:r1])
            if keep_fp8:
                self._fp8_quantize_block(rows, fp8.codes[r0:r1], fp8.scale[r0:r1])
        return BinaryCorpus(bits, d, center, fp8, u8)


    # ---- IVF corpus: spherical k-means lists (sgpt_ivf_lists, sgpt_ivf_centroids, sgpt_gather_rows) ----
    def _ivf_rows(self, x: torch.Tensor, who: str) -> torch.Tensor:
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.to(self.device).contiguous()
        if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 8 or x.shape[1] > IVF_MAX_DIM:
            raise ValueError(f"{who}: rows are [n, d] with d % 8 == 0 and d <= {IVF_MAX_DIM}, got {tuple(x.shape)}")
        return x

    def ivf_lists(self, assign: torch.Tensor, nlist: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """assign int64 [N] -> (offsets int64 [nlist + 1], perm int64 [N]): perm is the stable argsort of assign, offsets the exclusive
        prefix of the list sizes; assignments outside [0, nlist) are clamped (include/sgpt_hip.h::sgpt_ivf_lists)."""
        assign = assign.to(device=self.device, dtype=torch.int64).contiguous()
        if assign.dim() != 1 or assign.shape[0] == 0:
            raise ValueError(f"ivf_lists needs a non-empty [N] assignment, got {tuple(assign.shape)}")
        N = int(assign.shape[0])
        offsets = torch.empty((nlist + 1,), dtype=torch.int64, device=self.device)
        perm = torch.empty((N,), dtype=torch.int64, device=self.device)
        self._chk(self.lib.sgpt_ivf_lists(self.handle, _p(assign), N, nlist, _p(offsets), _p(perm), _stream_ptr(self.device)), "sgpt_ivf_lists")
        return offsets, perm

    def ivf_centroids(self, x: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor, prev: Optional[torch.Tensor] = None,
                      normalize: bool = True) -> torch.Tensor:
        """out[c] = sum of x[perm[p]] over list c (divided by its L2 norm with normalize), in the fixed order of
        include/sgpt_hip.h::sgpt_ivf_centroids; x fp32 or f16 [n_x, d]; an empty list (or a zero / non-finite sum) gives prev[c] or zeros."""
        x = self._ivf_rows(x, "ivf_centroids")
        perm = perm.to(device=self.device, dtype=torch.int64).contiguous()
        offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
        nlist, d = int(offsets.shape[0]) - 1, int(x.shape[1])
        if prev is not None:
            prev = prev.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(prev.shape) != (nlist, d):
                raise ValueError(f"ivf_centroids: prev must be [{nlist}, {d}], got {tuple(prev.shape)}")
        out = torch.empty((nlist, d), dtype=torch.float32, device=self.device)
        self._chk(self.lib.sgpt_ivf_centroids(self.handle, _p(x), _rt.DT_CODE[x.dtype], x.shape[0], d, _p(perm), perm.shape[0], _p(offsets), nlist,
                                              _p(prev), 1 if normalize else 0, _p(out), _stream_ptr(self.device)), "sgpt_ivf_centroids")
        return out

    def gather_rows(self, x: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        """out[p] = RNE_f16(x[perm[p]]): x fp32 or f16 [n_x, d] -> f16 [len(perm), d] (include/sgpt_hip.h::sgpt_gather_rows)."""
        x = self._ivf_rows(x, "gather_rows")
        perm = perm.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty((perm.shape[0], x.shape[1]), dtype=torch.float16, device=self.device)
        self._chk(self.lib.sgpt_gather_rows(self.handle, _p(x), _rt.DT_CODE[x.dtype], x.shape[0], _p(perm), perm.shape[0], x.shape[1], _p(out),
                                            _stream_ptr(self.device)), "sgpt_gather_rows")
        return out

    def gather_quantize_rows(self, x: torch.Tensor, perm: torch.Tensor, start: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
        """codes[p] = the uint8 rule of u8_quantize_rows applied to x[perm[p]]: x fp32 or f16 [n_x, d], start / step fp32 [ld],
        ld = ceil(d / 128) * 128 -> uint8 [len(perm), ld], pad columns 128; a perm entry outside [0, n_x) gives a row of 128s
        (include/sgpt_hip.h::sgpt_u8_gather_quantize_rows)."""
        x = self._ivf_rows(x, "gather_quantize_rows")
        perm = perm.to(device=self.device, dtype=torch.int64).contiguous()
        start = start.to(device=self.device, dtype=torch.float32).contiguous()
        step = step.to(device=self.device, dtype=torch.float32).contiguous()
        ld = int(start.shape[0])
        if tuple(step.shape) != (ld,):
            raise ValueError(f"gather_quantize_rows: start and step must be [ld], got {tuple(start.shape)} and {tuple(step.shape)}")
        out = torch.empty((perm.shape[0], ld), dtype=torch.uint8, device=self.device)
        self._chk(self.lib.sgpt_u8_gather_quantize_rows(self.handle, _p(x), _rt.DT_CODE[x.dtype], x.shape[0], _p(perm), perm.shape[0], x.shape[1],
                                                        ld, _p(start), _p(step), _p(out), _stream_ptr(self.device)),
                  "sgpt_u8_gather_quantize_rows")
        return out

    def ivf_assign(self, x16: torch.Tensor, centroids16: torch.Tensor, block_rows: int = 65536) -> torch.Tensor:
        """The list of every row: the k = 1 result of the f16 scorer with the rows as queries against the centroids (ties to the lowest
        list), in blocks of `block_rows` queries -> int64 [n]."""
        assign = torch.empty((x16.shape[0],), dtype=torch.int64, device=self.device)
        for r0 in range(0, x16.shape[0], block_rows):
            _, idx, _ = self.score_topk(x16[r0:r0 + block_rows], centroids16, 1, dtype=torch.float16)
            assign[r0:r0 + block_rows] = idx[:, 0]
        return assign

    def spherical_kmeans(self, x16: torch.Tensor, k: int, n_iter: int = 10, seed: int = 0, block_rows: int = 65536) -> torch.Tensor:
        """Lloyd iterations over unit f16 rows [n, d] -> unit fp32 centroids [k, d], deterministic: the first centroids are the rows at a
        seeded CPU randperm (sorted); every iteration assigns with the f16 scorer (ivf_assign), builds the lists (ivf_lists) and takes the
        normalised list sums (ivf_centroids; an empty list keeps its centroid)."""
        n = int(x16.shape[0])
        if k < 1 or k > min(n, IVF_MAX_LISTS):
            raise ValueError(f"spherical_kmeans: 1 <= k <= min(n, {IVF_MAX_LISTS}) is required, got k = {k}, n = {n}")
        pick = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:k].sort().values.to(self.device)
        centroids = self.ivf_centroids(x16, pick, torch.arange(k + 1, dtype=torch.int64, device=self.device))
        for _ in range(int(n_iter)):
            assign = self.ivf_assign(x16, self.to_16(centroids), block_rows)
            offsets, perm = self.ivf_lists(assign, k)
            centroids = self.ivf_centroids(x16, perm, offsets, prev=centroids)
        return centroids

    def ivf_index(self, emb, nlist: Optional[int] = None, n_iter: int = 10, train_size: Optional[int] = None, seed: int = 0,
                  block_rows: int = 65536, nprobe: Optional[int] = None, precision: str = "f16", ranges=None, calibration_embeddings=None):
        """Embeddings [N, d] (d % 8 == 0) -> IVFCorpus: rows L2-normalised and rounded to f16, spherical k-means (spherical_kmeans) on a
        strided sample of `train_size` rows (default min(N, 256 nlist)), a final assignment of all N rows, the lists, the rows gathered in
        list-major order.  nlist None: the power of two nearest 4 sqrt(N).  Works in blocks of `block_rows` rows: the fp32 copy of a large
        corpus never exists whole on the device (its f16 copy does, twice while the rows are gathered); `emb` may live on the host.  torch
        allocates and copies; every sum, score and sort is a kernel of this library.
        precision="uint8" -> IVFUint8Corpus: the same clustering and lists (same seed: the same centroids, ids and offsets, bit for bit),
        the lists holding uint8 codes of the f16-rounded unit rows by scalar_quantize_corpus's rule (gather_quantize_rows: the f16 rows
        exist once, beside the codes).  The ranges are `ranges` ([2, d]: min row, max row), or those of `calibration_embeddings`
        (normalised and rounded to f16 like the corpus), or the corpus's own; elements outside them clamp."""
        check_ivf_precision("ivf_index", precision, ranges, calibration_embeddings)
        emb = _matrix(emb, "ivf_index")
        N, d = emb.shape
        if d % 8 or d > IVF_MAX_DIM:
            raise ValueError(f"ivf_index: d % 8 == 0 and d <= {IVF_MAX_DIM} are required, got d = {d}")
        if nlist is None:
            nlist = 2 ** int(round(math.log2(4.0 * math.sqrt(N))))
            nlist = max(1, min(nlist, N, IVF_MAX_LISTS))
        if nlist < 1 or nlist > min(N, IVF_MAX_LISTS):
            raise ValueError(f"ivf_index: 1 <= nlist <= min(N, {IVF_MAX_LISTS}) is required, got nlist = {nlist}, N = {N}")
        x16 = torch.empty((N, d), dtype=torch.float16, device=self.device)
        for r0 in range(0, N, block_rows):
            x16[r0:r0 + block_rows] = self.l2_normalize(emb[r0:r0 + block_rows], out_dtype=torch.float16)
        T = min(N, 256 * nlist) if train_size is None else int(train_size)
        if T < nlist or T > N:
            raise ValueError(f"ivf_index: nlist <= train_size <= N is required, got train_size = {T}")
        step = N // T
        train = x16 if step == 1 and T == N else x16[0:step * T:step].contiguous()
        centroids = self.spherical_kmeans(train, nlist, n_iter, seed, block_rows)
        centroids16 = self.to_16(centroids)
        offsets, perm = self.ivf_lists(self.ivf_assign(x16, centroids16, block_rows), nlist)
        sizes = offsets.cpu().numpy()
        max_list = int((sizes[1:] - sizes[:-1]).max())
        if precision == "f16":
            return IVFCorpus(centroids, self.gather_rows(x16, perm), perm, offsets, max_list, nprobe, centroids16)

        def blocks(src):      # the rows as they are quantised: unit rows rounded to f16 (the corpus's are x16 already), widened exactly
            for r0 in range(0, src.shape[0], block_rows):
                b = src[r0:r0 + block_rows]
                yield (b if src is x16 else self.l2_normalize(b, out_dtype=torch.float16)).to(torch.float32)
        start, qstep = self._u8_ranges(x16, True, ranges, calibration_embeddings, block_rows, "ivf_index", blocks)
        codes = self.gather_quantize_rows(x16, perm, start, qstep)
        return IVFUint8Corpus(centroids, codes, start, qstep, perm, offsets, max_list, nprobe, centroids16, d)


from . import runtime as _rt  # noqa: E402  (last: runtime.py imports the names above, whichever of the two modules is loaded first)
