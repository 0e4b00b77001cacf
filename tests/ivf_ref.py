"""numpy restatement of the IVF corpus (include/sgpt_hip.h: sgpt_ivf_lists, sgpt_ivf_centroids, sgpt_gather_rows, sgpt_ivf_search;
sgpt_amd/corpus.py::IVFCorpus, CorpusBuilders.ivf_index), in float64, with the fp32 bounds the kernels are held to.

Bounds are the standard ones: a sum that passes n roundings of unit roundoff u = 2^-24 is within gamma_n = n u / (1 - n u) times the
sum of the terms' magnitudes of the exact value."""
import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 256                      # SGPT_IVF_CHUNK: rows of one work item of the search
SUM_ROWS = 256                   # rows of one partial of the centroid sums


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- lists ----
def lists(assign, nlist):
    """assign int [N] -> (offsets int64 [nlist + 1], perm int64 [N]): the stable argsort and the exclusive prefix of the list sizes;
    assignments outside [0, nlist) are clamped."""
    a = np.clip(np.asarray(assign, dtype=np.int64), 0, nlist - 1)
    perm = np.argsort(a, kind="stable").astype(np.int64)
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(a, minlength=nlist))
    return offsets, perm


# ---- centroids ----
def list_sums(x, perm, offsets):
    """(sums float64 [nlist, d], sums of magnitudes float64 [nlist, d], list lengths)."""
    x = np.asarray(x).astype(np.float64)
    nlist = len(offsets) - 1
    s = np.zeros((nlist, x.shape[1]))
    a = np.zeros((nlist, x.shape[1]))
    for c in range(nlist):
        rows = x[perm[offsets[c]:offsets[c + 1]]]
        s[c], a[c] = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    return s, a, np.diff(offsets)


def centroids(x, perm, offsets, prev=None, normalize=True):
    """float64 [nlist, d]: the list sums, divided by their L2 norms under `normalize`; an empty list -- and under `normalize` a zero or
    non-finite sum -- gives prev[c] (zeros without prev)."""
    s, _, n = list_sums(x, perm, offsets)
    out = np.zeros_like(s) if prev is None else np.asarray(prev).astype(np.float64).copy()
    for c in range(len(n)):
        if n[c] == 0:
            continue
        if not normalize:
            out[c] = s[c]
            continue
        with np.errstate(all="ignore"):
            t = float((s[c] * s[c]).sum())
        if t > 0 and np.isfinite(t):
            out[c] = s[c] / np.sqrt(t)
    return out


def centroid_bound(x, perm, offsets):
    """|fp32 normalised centroid - float64 one| per element, [nlist, d].  A column's sum passes at most min(len, 256) - 1 additions inside a
    chunk and ceil(len / 256) - 1 across chunks: |s^_j - s_j| <= e_j = gamma_n sum |x_j|.  The squared norm is d rounded products under at
    most ceil(d / 256) + 8 additions, the square root and the division round once each: a relative gamma_m, m = ceil(d / 256) + 13, on
    s^_j / |s^|.  |s^ / |s^| - s / |s|| <= e_j / |s| + |s^_j| |e| / (|s^| |s|)."""
    s, a, n = list_sums(x, perm, offsets)
    d = s.shape[1]
    out = np.zeros_like(s)
    for c in range(len(n)):
        if n[c] == 0:
            continue
        n_add = min(int(n[c]), SUM_ROWS) - 1 + (int(n[c]) + SUM_ROWS - 1) // SUM_ROWS - 1
        e = gamma(max(n_add, 1)) * a[c]
        ns, ne = np.linalg.norm(s[c]), np.linalg.norm(e)
        hat = np.abs(s[c]) + e
        if not ns > ne:                                  # (a sum the errors may cancel: no bound)
            out[c] = np.inf
            continue
        out[c] = e / ns + hat * ne / ((ns - ne) * ns) + gamma((d + 255) // 256 + 13) * hat / (ns - ne)
    return out


# ---- search ----
def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def scores64(q, rows):
    """<q_i, float(row_n)> in float64: q fp32 [nq, d], rows f16 [n, d]."""
    return np.asarray(q, dtype=np.float32).astype(np.float64) @ np.asarray(rows).astype(np.float64).T


def score_terms(q, rows):
    """sum_j |q_j row_j|, [nq, n]."""
    return np.abs(np.asarray(q, dtype=np.float32).astype(np.float64)) @ np.abs(np.asarray(rows).astype(np.float64)).T


def score_roundings(d):
    """Roundings on the longest path of the search kernel's value: 2 fmas per 512-column round, 2 joining additions, 6 butterfly steps."""
    return 2 * ((d + 511) // 512) + 8


def score_bound(q, rows):
    return gamma(score_roundings(np.asarray(q).shape[1])) * score_terms(q, rows)


def library_order(val, idx):
    """Positions of (val, idx) pairs in the library order: score descending (-0 == +0), then index ascending."""
    return np.lexsort((idx, -(np.asarray(val, dtype=np.float64) + 0.0)))


def probe_sets(q, centroids16, nprobe):
    """The nprobe best lists per query by <RNE_f16(q), centroids16> in float64, ties to the lowest list: what the f16 scorer returns
    wherever its fp32 sums are exact or the scores are apart."""
    s = f16(q).astype(np.float64) @ np.asarray(centroids16).astype(np.float64).T
    return np.stack([library_order(r, np.arange(len(r)))[:nprobe] for r in s]).astype(np.int64)


def search(q, rows, ids, offsets, probes, k, idx_base=0, run=None):
    """The restricted top-k: every row of the probed lists scored in float64 (NaN -> -1), merged with the running list
    (run = (val [nq, k], idx [nq, k], n_run)), the k best in the library order; unused slots (-inf, -1).  -> (val float64 [nq, k], idx int64 [nq, k],
    the candidate rows' positions per query)."""
    q = np.asarray(q, dtype=np.float32)
    nq = q.shape[0]
    val = np.full((nq, k), -np.inf)
    idx = np.full((nq, k), -1, dtype=np.int64)
    cands = []
    for i in range(nq):
        pos = np.concatenate([np.arange(offsets[c], offsets[c + 1]) for c in probes[i]] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        cands.append(pos)
        with np.errstate(invalid="ignore", over="ignore"):
            v = scores64(q[i:i + 1], rows[pos])[0] if len(pos) else np.zeros(0)
        v = np.where(np.isnan(v), -1.0, v)
        j = np.asarray(ids)[pos] + idx_base
        if run is not None and run[2] > 0:
            v = np.concatenate([v, np.asarray(run[0][i, :run[2]], dtype=np.float64)])
            j = np.concatenate([j, np.asarray(run[1][i, :run[2]], dtype=np.int64)])
        keep = (v > -np.inf) & (j >= 0)
        v, j = v[keep], j[keep]
        o = library_order(v, j)[:k]
        val[i, :len(o)], idx[i, :len(o)] = v[o], j[o]
    return val, idx, cands


# ---- spherical k-means, the steps of CorpusBuilders.spherical_kmeans / ivf_index ----
def normalize_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


def kmeans_init(n, k, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:k].sort().values.numpy().astype(np.int64)


def assign(x16, centroids32):
    """Every row's best centroid by <row, RNE_f16(centroid)> in float64, ties to the lowest."""
    s = np.asarray(x16).astype(np.float64) @ f16(centroids32).astype(np.float64).T
    return np.argmax(s, axis=1).astype(np.int64)


def kmeans(x16, k, n_iter, seed):
    """x16 f16 unit rows [n, d] -> fp32 centroids [k, d] (float64 arithmetic, rounded to fp32 after every update, as the device keeps them)."""
    pick = kmeans_init(len(x16), k, seed)
    c = centroids(x16, pick, np.arange(k + 1)).astype(np.float32)
    for _ in range(n_iter):
        offsets, perm = lists(assign(x16, c), k)
        c = centroids(x16, perm, offsets, prev=c).astype(np.float32)
    return c


def build(x, nlist, n_iter, seed):
    """Unit rows -> (centroids fp32, rows f16 list-major, ids, offsets): ivf_index with the whole corpus as the training sample."""
    x16 = f16(normalize_rows(x))
    c = kmeans(x16, nlist, n_iter, seed)
    offsets, perm = lists(assign(x16, c), nlist)
    return c, x16[perm], perm, offsets


def clustered_fixture(n=4096, d=128, clusters=40, noise=0.7, nq=32, seed=0):
    """Unit rows drawn from `clusters` Gaussian clusters (unit-variance centres, per-element noise `noise`) that share three strong
    directions (every row carries a random multiple of each, standard deviation 4), and `nq` queries: perturbed corpus rows."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, d))
    shared = rng.standard_normal((3, d))
    x = centres[rng.integers(0, clusters, n)] + noise * rng.standard_normal((n, d)) + 4.0 * rng.standard_normal((n, 3)) @ shared / np.sqrt(d)
    x = normalize_rows(x).astype(np.float32)
    q = x[rng.choice(n, nq, replace=False)] + 0.05 * rng.standard_normal((nq, d)).astype(np.float32) / np.sqrt(d) * 4
    return x, normalize_rows(q).astype(np.float32)


def recall_at(found_idx, exact_idx):
    """Mean fraction of each exact list found."""
    return float(np.mean([len(set(f.tolist()) & set(e.tolist())) / len(e) for f, e in zip(found_idx, exact_idx)]))
