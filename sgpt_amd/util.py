"""Drop-in for the scoring helpers the reference imports
(sentence_transformers/util.py:24-91,197-258 == beir.util.cos_sim/dot_score used at
biencoder/beir/custommodels/exact_search.py:9,27,96-98), computed by the HIP scorer."""
from typing import Callable, List

import numpy as np
import torch

from .corpus import CORPUS_KINDS, BinaryCorpus, check_ivf_precision
from .runtime import get_context


def _ctx_for(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return get_context(x.device), x.device
    return get_context(), torch.device("cpu")


def _wrap(a):
    if not isinstance(a, torch.Tensor):
        a = torch.tensor(np.asarray(a))
    if a.dim() == 1:
        a = a.unsqueeze(0)
    return a


def _as_tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a))


def normalize_embeddings(embeddings: torch.Tensor) -> torch.Tensor:
    """util.normalize_embeddings (util.py:66-70): rows scaled to unit L2 norm."""
    ctx, home = _ctx_for(embeddings)
    out = ctx.l2_normalize(_wrap(embeddings))
    return out if home.type == "cuda" else out.cpu()


def cos_sim(a, b) -> torch.Tensor:
    """util.cos_sim (util.py:24-43): res[i][j] = cos(a[i], b[j]); exact-fp32 MFMA."""
    ctx, home = _ctx_for(a, b)
    out = ctx.scores(ctx.l2_normalize(_wrap(a)), ctx.l2_normalize(_wrap(b)))
    return out if home.type == "cuda" else out.cpu()


pytorch_cos_sim = cos_sim


def dot_score(a, b) -> torch.Tensor:
    """util.dot_score (util.py:46-63)."""
    ctx, home = _ctx_for(a, b)
    out = ctx.scores(ctx._dev_f32(_wrap(a)), ctx._dev_f32(_wrap(b)))
    return out if home.type == "cuda" else out.cpu()


def pairwise_dot_score(a, b) -> torch.Tensor:
    """util.pairwise_dot_score (util.py:66-76): res[i] = dot(a[i], b[i])."""
    ctx, home = _ctx_for(a, b)
    a, b = _as_tensor(a), _as_tensor(b)
    lead = a.shape[:-1]
    out = ctx.pairwise_scores(a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), cosine=False).reshape(lead)
    return out if home.type == "cuda" else out.cpu()


def pairwise_cos_sim(a, b) -> torch.Tensor:
    """util.pairwise_cos_sim (util.py:79-91): res[i] = cos_sim(a[i], b[i]) -- the product sum of the normalised rows."""
    ctx, home = _ctx_for(a, b)
    a, b = _as_tensor(a), _as_tensor(b)
    out = ctx.pairwise_scores(a, b, cosine=True)         # (normalize_embeddings is dim=1: matrices, as in the reference)
    return out if home.type == "cuda" else out.cpu()


def quantize_embeddings(embeddings, precision: str = "fp8", normalize: bool = True, center=None, keep_fp8: bool = False,
                        ranges=None, calibration_embeddings=None, keep_uint8: bool = False):
    """Corpus embeddings -> a corpus object for semantic_search / Context.score_topk.  Named after sentence-transformers' later
    `quantize_embeddings`.
    precision="fp8": QuantizedCorpus (e4m3fn codes + one power-of-two scale per row), one byte per element on the device and per
    search pass.  normalize=True L2-normalises the rows first (search with cos_sim), normalize=False keeps them (dot_score).
    precision="ubinary" (sentence-transformers' name for packed unsigned bits): BinaryCorpus, one BIT per element -- Hamming search
    plus re-scoring of an over-fetched candidate list.  center: None | "mean" | a [d] tensor, subtracted from the normalised rows (and
    later from the queries) before the signs are taken; keep_fp8=True also keeps an fp8 copy to re-score with (uncentred corpora
    only); keep_uint8=True also keeps a uint8 copy of the same rows (its ranges from `ranges` / `calibration_embeddings` as below) to
    re-score with, centred or not -- binary retrieval plus int8 re-scoring.  normalize=False is refused: sign bits carry no norms.
    precision="uint8" (sentence-transformers' scalar quantisation): Uint8Corpus, one byte per element with one range per DIMENSION --
    256 uniform levels between each column's min and max.  ranges: None | a [2, d] matrix of (min, max) per column, as
    sentence-transformers takes it; calibration_embeddings: rows to take the ranges from instead of the corpus itself (elements outside
    them clamp).  The ranges are those of the rows as they are quantised: the normalised rows with normalize=True.  Its signed
    spelling 'int8' (the same levels, code - 128) stays refused: Uint8Corpus.codes_int8() gives that view."""
    if precision == "int8":
        raise ValueError("quantize_embeddings: precision 'int8' is not built -- the same scalar quantisation is precision=\"uint8\" "
                         "(its codes are the int8 codes + 128; Uint8Corpus.codes_int8() gives the signed view)")
    if precision not in ("fp8", "ubinary", "uint8"):
        raise ValueError(f"quantize_embeddings: unknown precision {precision!r} (only 'fp8', 'ubinary' and 'uint8' are built)")
    if keep_uint8 and precision != "ubinary":
        raise ValueError("quantize_embeddings: keep_uint8 belongs to precision='ubinary'")
    takes_ranges = precision == "uint8" or (precision == "ubinary" and keep_uint8)
    if not takes_ranges and (ranges is not None or calibration_embeddings is not None):
        raise ValueError("quantize_embeddings: ranges / calibration_embeddings belong to precision='uint8' (and to precision='ubinary' "
                         "with keep_uint8=True)")
    if precision == "uint8" and (center is not None or keep_fp8):
        raise ValueError("quantize_embeddings: center / keep_fp8 belong to precision='ubinary'")
    if takes_ranges and ranges is not None and calibration_embeddings is not None:
        raise ValueError("quantize_embeddings: give ranges or calibration_embeddings, not both")
    if precision == "ubinary" and not normalize:
        raise ValueError("quantize_embeddings: precision='ubinary' with normalize=False is refused -- sign bits carry no norms")
    if precision == "ubinary" and keep_fp8 and center is not None:
        raise ValueError("quantize_embeddings: keep_fp8 with a centre is refused -- fp8 re-scoring needs the raw query, the centred bits "
                         "q - center, and the search call takes one query matrix")
    if precision == "fp8" and (center is not None or keep_fp8):
        raise ValueError("quantize_embeddings: center / keep_fp8 belong to precision='ubinary'")
    if isinstance(embeddings, list):
        embeddings = torch.stack(embeddings)
    e = _wrap(embeddings)
    ctx, _ = _ctx_for(e)
    if isinstance(calibration_embeddings, list):
        calibration_embeddings = torch.stack(calibration_embeddings)
    cal = None if calibration_embeddings is None else _wrap(calibration_embeddings)
    if precision == "ubinary":
        return ctx.binarize_corpus(e, normalize=True, center=center, keep_fp8=keep_fp8, keep_uint8=keep_uint8, ranges=ranges,
                                   calibration_embeddings=cal)
    if precision == "uint8":
        return ctx.scalar_quantize_corpus(e, normalize=normalize, ranges=ranges, calibration_embeddings=cal)
    return ctx.quantize_corpus(e, normalize=normalize)


def build_ivf_index(embeddings, nlist=None, n_iter: int = 10, train_size=None, seed: int = 0, nprobe=None, precision: str = "f16",
                    ranges=None, calibration_embeddings=None):
    """Corpus embeddings [N, d] (d % 8 == 0) -> an IVFCorpus for semantic_search / Context.score_topk (Context.ivf_index): the rows
    L2-normalised, cut into `nlist` lists by spherical k-means on the device (nlist None: the power of two nearest 4 sqrt(N)); a query
    then scans its `nprobe` best lists only (corpus.with_nprobe(p) changes that).  Cosine only.  Deterministic for a given seed.
    precision="uint8": an IVFUint8Corpus -- the same lists holding uint8 codes with one range per dimension instead of f16 rows, half
    the bytes per row; `ranges` / `calibration_embeddings` as quantize_embeddings(precision="uint8") takes them.  Its signed spelling
    'int8' stays refused."""
    check_ivf_precision("build_ivf_index", precision, ranges, calibration_embeddings)
    if isinstance(embeddings, list):
        embeddings = torch.stack(embeddings)
    e = _wrap(embeddings)
    ctx, _ = _ctx_for(e)
    if isinstance(calibration_embeddings, list):
        calibration_embeddings = torch.stack(calibration_embeddings)
    cal = None if calibration_embeddings is None else _wrap(calibration_embeddings)
    return ctx.ivf_index(e, nlist=nlist, n_iter=n_iter, train_size=train_size, seed=seed, nprobe=nprobe, precision=precision,
                         ranges=ranges, calibration_embeddings=cal)


def kmeans(embeddings, k: int, n_iter: int = 10, seed: int = 0):
    """Spherical k-means of the L2-normalised rows on the device, the steps an IVF build takes (Context.spherical_kmeans) ->
    (centroids fp32 [k, d] unit rows, labels int64 [N]: every row's best centroid by the f16 scorer, ties to the lowest)."""
    if isinstance(embeddings, list):
        embeddings = torch.stack(embeddings)
    e = _wrap(embeddings)
    ctx, home = _ctx_for(e)
    x16 = ctx.l2_normalize(e, out_dtype=torch.float16)
    centroids = ctx.spherical_kmeans(x16, int(k), n_iter, seed)
    labels = ctx.ivf_assign(x16, ctx.to_16(centroids))
    return (centroids, labels) if home.type == "cuda" else (centroids.cpu(), labels.cpu())


def _binary_rescore(corpus: BinaryCorpus) -> str:
    return corpus.default_rescore


def _hits(val: torch.Tensor, idx: torch.Tensor, n: int) -> List[List[dict]]:
    val, idx = val.cpu().tolist(), idx.cpu().tolist()
    # (index -1: a slot that found no document -- an IVFCorpus whose probed lists hold fewer than top_k rows; no other list has one before n)
    return [[{"corpus_id": j, "score": s} for j, s in zip(ii[:n], vv[:n]) if j >= 0] for vv, ii in zip(val, idx)]


def semantic_search(query_embeddings, corpus_embeddings, query_chunk_size: int = 100,
                    corpus_chunk_size: int = 500000, top_k: int = 10,
                    score_function: Callable = cos_sim) -> List[List[dict]]:
    """util.semantic_search (util.py:197-258).  Same result contract (per query a list of
    {'corpus_id','score'} sorted by decreasing score); the chunk loops collapse into one fused
    score + running-top-k pass on the GPU when score_function is cos_sim / dot_score (query_chunk_size / corpus_chunk_size are then
    not used).  Over a BinaryCorpus: cos_sim only, top_k <= 1024, re-scored with the corpus's uint8 copy when it has one, else with its
    fp8 copy when it has one and is not centred, with its sign bits otherwise."""
    if isinstance(query_embeddings, list):
        query_embeddings = torch.stack(query_embeddings)
    if isinstance(corpus_embeddings, CORPUS_KINDS):        # fp8 codes, uint8 codes, packed sign bits or IVF lists of f16 rows / uint8 codes (corpus.py)
        corpus, q = corpus_embeddings, _wrap(query_embeddings)
        cosine = corpus.check_search(score_function, top_k)           # (refusals come before anything reaches for the device)
        ctx, _ = _ctx_for(corpus.data, q)
        qd = ctx.l2_normalize(q) if cosine else ctx._dev_f32(q)
        return _hits(*ctx.score_topk(qd, corpus, min(top_k, len(corpus)), rescore=corpus.default_rescore))
    if isinstance(corpus_embeddings, list):
        corpus_embeddings = torch.stack(corpus_embeddings)
    q, c = _wrap(query_embeddings), _wrap(corpus_embeddings)
    ctx, _ = _ctx_for(c, q)
    if score_function in (cos_sim, pytorch_cos_sim):
        qd, cd = ctx.l2_normalize(q), ctx.l2_normalize(c)
    elif score_function is dot_score:
        qd, cd = ctx._dev_f32(q), ctx._dev_f32(c)
    else:  # arbitrary callable: materialise its scores chunk by chunk, top-k on the GPU
        out = [[] for _ in range(len(q))]
        for qs in range(0, len(q), query_chunk_size):
            for cs in range(0, len(c), corpus_chunk_size):
                sc = score_function(q[qs:qs + query_chunk_size], c[cs:cs + corpus_chunk_size])
                v, i = ctx.topk(sc, min(top_k, sc.shape[1]), idx_base=cs)
                for r, (vv, ii) in enumerate(zip(v.cpu().tolist(), i.cpu().tolist())):
                    out[qs + r] += [{"corpus_id": j, "score": s} for j, s in zip(ii, vv)]
        return [sorted(o, key=lambda x: x["score"], reverse=True)[:top_k] for o in out]
    return _hits(*ctx.score_topk(qd, cd, min(top_k, len(c))))
