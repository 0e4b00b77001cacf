// C ABI (include/sgpt_hip.h): the scorer -- score tiles, the filtered score + top-k schedule and its exact-fp32 refinement.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
// A score + top-k pass is three parts: the schedule (score_plan.h: plan_score_topk, pure arithmetic on the shape), the corpus (Corpus /
// corpus_gemm below: the one place that knows what the document rows are) and the executor (score_topk_impl: the launches of a plan).
#include "host.h"
#include "score_plan.h"

extern "C" {

sgpt_status sgpt_l2_normalize(sgpt_ctx* c, const float* in, int64_t n, int32_t d, void* out, int32_t out_dtype,
                              void* stream) {
    if (!c || !in || !out || n <= 0 || d <= 0 || (out_dtype != SGPT_F32 && out_dtype != SGPT_BF16 && out_dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_l2_normalize: bad arguments (out fp32, bf16 or f16)");
    HIPC(c, hipSetDevice(c->device));
    launch_l2norm(in, n, d, out, out_dtype, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_pairwise_scores(sgpt_ctx* c, const float* a, const float* b, int64_t n, int32_t d, int32_t cosine, float* out,
                                 void* stream) {
    if (!c || !a || !b || !out || n <= 0 || d <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_pairwise_scores: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    launch_pairwise(a, b, n, d, cosine != 0, out, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

static sgpt_status check_score_dims(sgpt_ctx* c, int dtype, int d) {
    if (dtype != SGPT_F32 && dtype != SGPT_BF16 && dtype != SGPT_F16) return fail(c, SGPT_ERR_INVALID, "score: bad dtype");
    const int mult = dtype == SGPT_F32 ? 4 : 8;
    if (d <= 0 || d % mult) return fail(c, SGPT_ERR_INVALID, "score: d must be a multiple of 4 (fp32) / 8 (bf16, f16)");
    return SGPT_OK;
}

sgpt_status sgpt_scores(sgpt_ctx* c, const void* a, const void* b, int32_t dtype, int64_t na, int64_t nb, int32_t d,
                        float* out, int64_t ldo, void* stream) {
    if (!c || !a || !b || !out || na <= 0 || nb <= 0 || ldo < nb || ldo % 4 || na > INT32_MAX || nb > INT32_MAX)
        return fail(c, SGPT_ERR_INVALID, "sgpt_scores: bad arguments");
    sgpt_status st = check_score_dims(c, dtype, d);
    if (st != SGPT_OK) return st;
    HIPC(c, hipSetDevice(c->device));
    GemmArgs g{};
    g.A = a; g.lda = d; g.W = b; g.ldw = d; g.M = (int)na; g.m_valid = (int)na; g.N = (int)nb; g.K = d;
    g.out = out; g.ldo = ldo;
    gemm(c, dtype, EPI_STORE, SGPT_F32, g, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

// What a score + top-k pass reads its documents from.  The kinds share one schedule; only the launches that read the corpus differ:
//   rows (fp32 / bf16 / f16, `dtype`): the GEMM kernels;
//   fp8 (sgpt_score_topk_q8, short query batches): `base` holds e4m3fn codes [N][d] bytes, `scale` one power-of-two scale per document,
//     q is f16 (dtype SGPT_F16).  Whole 256-document tiles go through launch_score64q8 (score8.hip), a ragged tail is de-quantised
//     into f16 scratch (ws6) for the register-staged kernel;
//   bits (sgpt_score_topk_bits, at most 64 queries per call): `base` holds packed sign bits [N][ldb] bytes, q the packed query rows of
//     qw dwords; the score is the agreement d - 2 * hamming, an integer in fp32.  Every launch that reads the corpus is the Hamming
//     tile (scorebits.hip), which takes any number of documents, so no launch is split for a ragged tail;
//   uint8 (sgpt_score_topk_u8, at most 64 queries per call): `base` holds uint8 codes [N][ld] bytes, `start` / `step` the range of every
//     dimension, q the caller's fp32 rows of width d0; `d` is ld, the k extent of the tile.  The pass prologue turns q into the 64-row
//     tile of pre-scaled f16 rows with qscale / qbias (ws2); every launch that reads the corpus is launch_score64u8 (scoreu8.hip),
//     which takes any number of documents.
struct Corpus {
    ScoreCorpusKind kind = SCORE_CORPUS_F32;
    const void* base = nullptr;
    int dtype = SGPT_F16, d = 0;    // (dtype: of the query rows the GEMM kernels take; rows: of the corpus too)
    size_t rowb = 0;                // bytes of a corpus row
    long ldw1 = 0;                  // GemmArgs.ldw of consecutive rows (the Hamming tile counts bytes)
    const float* scale = nullptr;   // fp8: [N]
    long ldb = 0; int qw = 0;       // bits
    size_t ws6_bytes = 0;           // scratch the launches need (fp8: the f16 rows of a ragged tail, < 256 documents)
    const float *start = nullptr, *step = nullptr; int d0 = 0;        // uint8: ranges [ld], width of the caller's query rows
    const float *qscale = nullptr, *qbias = nullptr;                  // uint8: [64] in ws2, set by the executor
};
// every kind: its tag, its rows and their extent; then the fields of its kind by name
static Corpus corpus_of(ScoreCorpusKind kind, const void* base, int d, size_t rowb, long ldw1) {
    Corpus cp;
    cp.kind = kind; cp.base = base; cp.d = d; cp.rowb = rowb; cp.ldw1 = ldw1;
    return cp;
}
static Corpus corpus_rows(const void* rows, int dtype, int d) {
    Corpus cp = corpus_of(dtype == SGPT_F32 ? SCORE_CORPUS_F32 : SCORE_CORPUS_16, rows, d, (size_t)d * (dtype == SGPT_F32 ? 4 : 2), d);
    cp.dtype = dtype;
    return cp;
}
static Corpus corpus_fp8(const uint8_t* codes, const float* scale, int d) {
    Corpus cp = corpus_of(SCORE_CORPUS_FP8, codes, d, (size_t)d, d);
    cp.scale = scale; cp.ws6_bytes = (size_t)256 * d * 2;
    return cp;
}
static Corpus corpus_bits(const uint8_t* bits, long ldb, int qw, int d) {
    Corpus cp = corpus_of(SCORE_CORPUS_BITS, bits, d, (size_t)ldb, ldb);
    cp.ldb = ldb; cp.qw = qw;
    return cp;
}
static Corpus corpus_u8(const uint8_t* codes, const float* start, const float* step, int d0, int ld) {
    Corpus cp = corpus_of(SCORE_CORPUS_U8, codes, ld, (size_t)ld, ld);
    cp.start = start; cp.step = step; cp.d0 = d0;
    return cp;
}

// The row layouts the entries check, once each.  `align`: what the entry's kernels load or store the rows with, in bytes.
//   uint8: codes [N][ld] bytes, ld whole 128-byte pieces that hold the d columns
static inline bool u8_layout_ok(const void* codes, int64_t d, int64_t ld, size_t align) { return codes && d > 0 && d <= ld && ld >= 128 && ld % 128 == 0 && !((size_t)codes & (align - 1)); }
//   bits: [N][ldb] bytes, ldb whole dwords that hold the d bits
static inline bool bits_layout_ok(const void* bits, int64_t d, int64_t ldb, size_t align) { return bits && d > 0 && ldb % 4 == 0 && ldb >= 4 * ((d + 31) / 32) && !((size_t)bits & (align - 1)); }

// one launch that reads documents [doc0, doc0 + h.N) (at row_stride): h.W / h.ldw are set for them already
static void corpus_gemm(sgpt_ctx* c, const Corpus& cp, int epi, GemmArgs h, long doc0, long row_stride, bool sample, hipStream_t s) {
    switch (cp.kind) {
    case SCORE_CORPUS_BITS:
        launch_scorebits(epi, h, cp.d, cp.qw, cp.ldb, s, sample);
        return;
    case SCORE_CORPUS_U8:
        launch_score64u8(epi, ScoreU8Args{h, cp.qscale, cp.qbias}, s);
        return;
    case SCORE_CORPUS_FP8:
        if (h.N % 256 == 0) {
            Score8Args a8{h, cp.scale + doc0, row_stride};
            launch_score64q8(epi, a8, s);
        } else {        // (the tail is never strided)
            launch_fp8_dequant_rows(h.W, cp.scale + doc0, h.N, cp.d, c->ws6, SGPT_F16, s);
            h.W = c->ws6; h.ldw = cp.d;
            gemm(c, SGPT_F16, epi, SGPT_F32, h, s);
        }
        return;
    default:
        gemm(c, cp.dtype, epi, SGPT_F32, h, s);
    }
}

// what the launches of one pass share
struct ScoreRun {
    sgpt_ctx* c; hipStream_t s;
    const ScorePlan& p; const Corpus& cp;
    const void *q, *qpad;          // the caller's query rows | what the 256-document tile kernels read (their zero-padded copy)
    int nq, d, k; long idx_base;
    float* sc;                     // the score tile
    float* tv[2]; int64_t* ti[2];  // ping-pong running lists
    float* sav_v; int64_t* sav_i;  // third list: ping-pong partner of a recomputation
};

// fp32 scores of documents [c0, c0 + nc) for every query -> sc[nq][ld]
static void score_tile(const ScoreRun& r, long c0, long nc, long ld, const int* pred, long row_stride = 1, bool sample = false) {
    GemmArgs g{};
    g.A = r.q; g.lda = r.d; g.M = r.nq; g.m_valid = r.nq; g.K = r.d; g.pred = pred;
    g.W = (const char*)r.cp.base + (size_t)c0 * r.cp.rowb; g.ldw = r.cp.ldw1 * row_stride; g.N = (int)nc;   // row_stride > 1: a strided sample
    g.out = r.sc; g.ldo = ld;
    if (r.p.any_n && r.p.pad_queries) { g.A = r.qpad; g.M = r.p.nq_pad; }      // (uint8: the prologue's tile, not the caller's rows)
    if (r.p.any_n) { corpus_gemm(r.c, r.cp, EPI_SCORE, g, c0, row_stride, sample, r.s); return; }
    const long na = r.p.fast ? nc / 256 * 256 : 0;      // documents the 256-document tile kernels take
    // (round 5, measured and reverted: handing a predicated fallback piece to the register-staged kernel whole -- one no-op launch
    //  instead of two -- made the shard pass 12 % SLOWER: a no-op launch of the persistent 256x256 kernel is 256 workgroups that
    //  exit, one of the small-tile kernel for 125 k documents x 1000 queries is ~8 000.)
    // the < 256 trailing documents ride in the 256x256 launch (clamped rows, GemmArgs.n_valid; their missing columns land in the
    // padding of the score row, which the select does not read): one launch less per piece -- a no-op one in the predicated
    // fallback of every filtered chunk
    const bool fold = r.p.tile_folds(na, nc, ld, row_stride, r.d);
    if (na > 0) {
        GemmArgs h = g;
        h.A = r.qpad; h.M = r.p.nq_pad; h.N = (int)(fold ? na + 256 : na); h.n_valid = fold ? (int)nc : 0;
        corpus_gemm(r.c, r.cp, EPI_SCORE, h, c0, row_stride, false, r.s);
    }
    if (na < nc && !fold) {                         // fp32, or the ragged tail (< 256 documents): register-staged kernel
        g.W = (const char*)r.cp.base + (size_t)(c0 + na) * r.cp.rowb; g.N = (int)(nc - na); g.out = r.sc + na;
        corpus_gemm(r.c, r.cp, EPI_SCORE, g, c0 + na, 1, false, r.s);
    }
}

// Materialise-and-select over documents [lo, hi): the reference's chunk loop (exact_search.py:96-132).
// (pv, pi, have) = running best going in; the last chunk writes (fin_v, fin_i), earlier ones ping-pong.
static sgpt_status classic(const ScoreRun& r, long lo, long hi, const float* pv, const int64_t* pi, int have, float* fin_v, int64_t* fin_i,
                           const int* pred) {
    sgpt_ctx* c = r.c;
    const long chunk = r.p.chunk;
    const int nq = r.nq, k = r.k;
    int cur = (pv == r.tv[0]) ? 1 : 0;
    for (long c0 = lo; c0 < hi; c0 += chunk) {
        const long nc = (hi - c0) < chunk ? (hi - c0) : chunk;
        score_tile(r, c0, nc, chunk, pred);
        const bool last = c0 + nc >= hi;
        if (last && pv == fin_v) {  // in/out alias on a single-chunk call: stage through the ping-pong buffer
            launch_topk_select(r.sc, chunk, nc, r.idx_base + c0, pv, pi, have, k, nq, k, 0, nullptr, r.tv[cur], r.ti[cur], r.s, pred);
            HIPC(c, hipMemcpyAsync(fin_v, r.tv[cur], (size_t)nq * k * 4, hipMemcpyDeviceToDevice, r.s));
            HIPC(c, hipMemcpyAsync(fin_i, r.ti[cur], (size_t)nq * k * 8, hipMemcpyDeviceToDevice, r.s));
        } else {
            launch_topk_select(r.sc, chunk, nc, r.idx_base + c0, pv, pi, have, k, nq, k, 0, nullptr,
                               last ? fin_v : r.tv[cur], last ? fin_i : r.ti[cur], r.s, pred);
        }
        pv = r.tv[cur]; pi = r.ti[cur];
        have = k;  // unused tail slots carry idx = -1 and are ignored by the next merge
        cur ^= 1;
    }
    return SGPT_OK;
}

// The same over [lo, hi) with every launch predicated on *pred (a filtered chunk's overflow flag): (pv, pi) = the
// k-slot running best before the chunk, result in (fin_v, fin_i); pieces of fchunk documents ping-pong through the
// third list so that nothing is copied (a copy could not be predicated).
static void recompute(const ScoreRun& r, long lo, long hi, const float* pv, const int64_t* pi, float* fin_v, int64_t* fin_i, const int* pred) {
    const long fchunk = r.p.fchunk;
    const long P = (hi - lo + fchunk - 1) / fchunk;
    for (long pc = 0; pc < P; ++pc) {
        const long c0 = lo + pc * fchunk, nc = (hi - c0) < fchunk ? (hi - c0) : fchunk;
        const bool to_fin = (P - 1 - pc) % 2 == 0;
        float* dv = to_fin ? fin_v : r.sav_v;
        int64_t* di = to_fin ? fin_i : r.sav_i;
        score_tile(r, c0, nc, fchunk, pred);
        launch_topk_select(r.sc, fchunk, nc, r.idx_base + c0, pv, pi, r.k, r.k, r.nq, r.k, 0, nullptr, dv, di, r.s, pred);
        pv = dv; pi = di;
    }
}

// entries of a k-slot running list after N more documents
static inline int32_t list_fill(int32_t n_run, int64_t N, int32_t k) { const int64_t tot = (int64_t)n_run + N; return (int32_t)(tot < k ? tot : k); }

// A/B switches of the schedule (score_plan.h takes them as input); the product build has the defaults
#ifndef SGPT_SAMPLE_MULT
#define SGPT_SAMPLE_MULT 1.0    // the sample as a multiple of the size the list capacity asks for (A/B builds: the sample is cheap since
#endif                          // its scores stay in the GEMM -- more sampled documents, tighter thresholds, fewer appended survivors)
#ifndef SGPT_FOLD_TAIL_SCORE
#define SGPT_FOLD_TAIL_SCORE 1  // 0: A/B builds -- the materialise-and-select pieces keep their small-tile tail launch
#endif
#ifndef SGPT_FOLD_TAIL
#define SGPT_FOLD_TAIL 1        // 0: the trailing < 256 documents of a shard in a small-tile launch of their own (A/B builds)
#endif
#ifndef SGPT_SAMPLE_TOP2
#define SGPT_SAMPLE_TOP2 1      // 0: the materialised sample tile + select of round 4 (A/B builds)
#endif
#ifndef SGPT_CAP_SHORT
#define SGPT_CAP_SHORT 512
#endif

// in_val / in_idx: the running list going in (n_run entries per row, row stride k); run_val / run_idx: the list coming out (they
// may be the same buffers -- the public entry point).  pred_all (device flag or null): every launch of the call is predicated on
// it and the call takes the materialise-and-select path -- the sync-free fallback of sgpt_score_topk_refined.
static sgpt_status score_topk_impl(sgpt_ctx* c, const void* q, const Corpus& cp_in, int32_t nq, int64_t N, int32_t k, int64_t idx_base,
                                   const float* in_val, const int64_t* in_idx, float* run_val, int64_t* run_idx, int32_t n_run,
                                   int32_t* n_out, void* stream, const int* pred_all) {
    Corpus cp = cp_in;
    const int d = cp.d;
    if (!c || !q || !cp.base || !run_val || !run_idx || nq <= 0 || N <= 0 || k <= 0 || n_run < 0 || n_run > k)
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk: bad arguments");
    sgpt_status st = cp.kind == SCORE_CORPUS_BITS ? SGPT_OK : check_score_dims(c, cp.dtype, d);
    if (st != SGPT_OK) return st;
    if (cp.kind == SCORE_CORPUS_BITS && (nq > 64 || d <= 0)) return fail(c, SGPT_ERR_INVALID, "score (binary corpus): at most 64 queries per pass");
    if (cp.kind == SCORE_CORPUS_U8 && !(nq <= 64 && N <= ((int64_t)1 << 30) && cp.d0 > 0 && cp.d0 <= d && score64u8_shape_ok(64, N, d, cp.base, d)))
        return fail(c, SGPT_ERR_INVALID, "score (uint8 corpus): shape not served by the streaming tile");
    if (cp.kind == SCORE_CORPUS_FP8 && !(nq <= 64 && score64q8_shape_ok(64, 256, d, cp.base, d)))
        return fail(c, SGPT_ERR_INVALID, "score (fp8 corpus): shape not served by the streaming tile");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // (SGPT_SCORE_NO64, SGPT_SCORE_CLASSIC, SGPT_GEMM128: A/B switches of the experiment build only)
    static const ScoreSwitches sw{exp_env("SGPT_SCORE_NO64") != nullptr, exp_env("SGPT_SCORE_CLASSIC") != nullptr, exp_env("SGPT_GEMM128") != nullptr,
                                  SGPT_SAMPLE_MULT, SGPT_FOLD_TAIL != 0, SGPT_FOLD_TAIL_SCORE != 0, SGPT_SAMPLE_TOP2 != 0, SGPT_CAP_SHORT};
    ScorePlan p;
    plan_score_topk(ScorePlanIn{nq, (long)N, d, k, n_run, cp.kind, pred_all != nullptr, sw}, p);

    st = ensure(c, &c->ws2, &c->ws2_bytes, p.total);
    if (st != SGPT_OK) return st;
    if (cp.ws6_bytes) {
        st = ensure(c, &c->ws6, &c->ws6_bytes, cp.ws6_bytes);
        if (st != SGPT_OK) return st;
    }
    char* base = (char*)c->ws2;
    auto at = [&](const ScorePlan::Region& r) { return r.bytes ? base + r.off : nullptr; };
    void* qpad = p.pad_queries ? at(p.qpad) : (p.fast ? const_cast<void*>(q) : nullptr);   // (packed query rows are read where they are)
    const ScoreRun r{c, s, p, cp, q, qpad, nq, d, k, (long)idx_base, (float*)at(p.sc), {(float*)at(p.tv[0]), (float*)at(p.tv[1])},
                     {(int64_t*)at(p.ti[0]), (int64_t*)at(p.ti[1])}, (float*)at(p.sav_v), (int64_t*)at(p.sav_i)};
    float* const* tv = r.tv; int64_t* const* ti = r.ti;
    float* cand_v = (float*)at(p.cand_v);
    long long* cand_i = (long long*)at(p.cand_i);
    int* cand_cnt = (int*)at(p.cand_cnt);                   // counters + per-chunk overflow flags
    int* flag = p.filt ? cand_cnt + p.nq_pad : nullptr;
    float* th_v = (float*)at(p.th_v); int64_t* th_i = (int64_t*)at(p.th_i);   // sample's list + dense thresholds
    float* thr_dense = (float*)at(p.thr);
    const int nq_pad = p.nq_pad;
    const long n_clear = p.filt ? (long)(nq_pad + p.n_flags) : 0;
    // prologue: one launch (query rows into their zero-padded tile, counters and flags cleared, an empty running list marked)
    if (cp.kind == SCORE_CORPUS_U8) {      // the tile is computed, not copied: q'' = q * step / qscale, with qscale and qbias beside it
        cp.qscale = (const float*)at(p.qscale); cp.qbias = (const float*)at(p.qbias);
        launch_u8_prepare_queries((const float*)q, cp.start, cp.step, nq, cp.d0, d, qpad, (float*)at(p.qscale), (float*)at(p.qbias), s);
        if (n_clear > 0 || p.fresh_list)
            launch_score_prep(nullptr, nullptr, 0, 0, cand_cnt, n_clear, p.fresh_list ? (long long*)ti[0] : nullptr, p.fresh_list ? (long)nq * k : 0, s);
    } else if (p.fast && (!p.pad_queries || (d % 8 == 0 && ((size_t)q & 15) == 0))) {
        launch_score_prep(q, qpad, p.pad_queries ? (long)nq * d * 2 : 0, p.pad_queries ? (long)nq_pad * d * 2 : 0, cand_cnt, n_clear,
                          p.fresh_list ? (long long*)ti[0] : nullptr, p.fresh_list ? (long)nq * k : 0, s);
    } else {
        if (p.pad_queries) {
            if (nq_pad > nq) HIPC(c, hipMemsetAsync((char*)qpad + (size_t)nq * d * 2, 0, (size_t)(nq_pad - nq) * d * 2, s));   // the pad rows only
            HIPC(c, hipMemcpyAsync(qpad, q, (size_t)nq * d * 2, hipMemcpyDeviceToDevice, s));
        }
        if (p.filt) HIPC(c, hipMemsetAsync(cand_cnt, 0, (size_t)n_clear * 4, s));
        if (p.fresh_list) HIPC(c, hipMemsetAsync(ti[0], 0xff, (size_t)nq * k * 8, s));
    }

    // the running best going into the trailing materialise-and-select: the caller's list, or what the filtered chunks leave
    const float* bv = n_run > 0 ? in_val : nullptr;
    const int64_t* bi = n_run > 0 ? in_idx : nullptr;
    int have = n_run;
    c->filt_chunks = 0;
    if (p.filt) {
        static const bool no_fallback = exp_env("SGPT_SCORE_NOFALLBACK") != nullptr;   // timing experiments ONLY: unsafe
        int cur = 0, chunk_i = 0;
        if (p.sampled) {
            // running best going in: tv[0] / ti[0] = the caller's list padded to k columns, or empty (idx -1 everywhere)
            if (n_run > 0) {
                launch_topk_select(in_val, k, 0, 0, in_val, in_idx, n_run, k, nq, k, 0, nullptr, tv[0], ti[0], s);
            }   // (n_run == 0: the prologue marked tv[0] / ti[0] empty -- idx -1, whatever the values say)
            // thresholds: the k-th best of {running best} U {S documents at stride s_stride across the shard}; only the VALUES
            // of this selection are used (its indices are sample positions) -- the filtered chunks below re-score the sampled
            // documents like any other and find them again
            if (p.sample_top2) {
                // the sample's scores never leave the GEMM: 8 floats per query row and 256-document tile (the two best of each
                // wave's 64 documents, EPI_SCORE_TOP2); the k-th best of those and the running list is the threshold
                const long ld2 = 8 * (p.S / 256);
                GemmArgs h{};
                h.A = qpad; h.lda = d; h.M = nq_pad; h.m_valid = nq; h.K = d;
                h.W = cp.base; h.ldw = cp.ldw1 * p.s_stride; h.N = (int)p.S; h.out = r.sc; h.ldo = ld2;
                corpus_gemm(c, cp, EPI_SCORE_TOP2, h, 0, p.s_stride, true, s);
                launch_topk_select(r.sc, ld2, ld2, 0, tv[0], ti[0], k, k, nq, k, 0, nullptr, th_v, th_i, s, nullptr, thr_dense);
            } else {
                score_tile(r, 0, p.S, p.S, nullptr, p.s_stride, true);      // (binary corpus: the sample's ties spread, launch_scorebits)
                launch_topk_select(r.sc, p.S, p.S, 0, tv[0], ti[0], k, k, nq, k, 0, nullptr, th_v, th_i, s, nullptr, thr_dense);   // (+ the inclusive threshold)
            }
        } else {
            // first chunk: materialise + select -> the initial thresholds
            st = classic(r, 0, p.first, bv, bi, n_run, tv[0], ti[0], nullptr);
            if (st != SGPT_OK) return st;
        }
        for (const ScoreChunk& ch : p.chunks) {
            GemmArgs g{};
            g.A = qpad; g.lda = d; g.M = nq_pad; g.m_valid = nq; g.K = d;
            g.W = (const char*)cp.base + (size_t)ch.doc0 * cp.rowb; g.ldw = cp.ldw1;
            // the < 256 trailing documents ride in the last chunk's launch (the 256x256 kernel clamps their rows and masks their
            // columns, GemmArgs.n_valid)
            g.N = (int)(ch.fold_tail ? (p.any_n ? ch.n_valid : ch.len + 256) : ch.len); g.n_valid = (int)ch.n_valid;
            // sampled schedule: the dense thresholds -- the sample's k-th best, raised by every merge to the running k-th best
            if (p.sampled) { g.thr = thr_dense; g.thr_ld = 1; }
            else { g.thr = tv[cur] + (k - 1); g.thr_ld = k; }
            g.cand_val = cand_v; g.cand_idx = cand_i; g.cand_cnt = cand_cnt; g.cand_cap = p.cap; g.idx_base = idx_base + ch.doc0;
            corpus_gemm(c, cp, EPI_SCORE_FILTER, g, ch.doc0, 1, false, s);
            g.n_valid = 0;
            long seen = ch.fold_tail ? (long)N : ch.doc0 + ch.len;
            if (ch.tail_launch) {
                // ragged tail (< 256 documents): filtered against the same thresholds by the small-tile kernel, its
                // survivors join this chunk's candidate lists -- one merge, no materialise + select round for 72 documents
                g.W = (const char*)cp.base + (size_t)seen * cp.rowb; g.N = (int)(N - seen); g.idx_base = idx_base + seen;
                corpus_gemm(c, cp, EPI_SCORE_FILTER, g, seen, 1, false, s);
                seen = N;
            }
            const bool fin = seen >= N;
            int* cflag = flag + (chunk_i < p.n_flags ? chunk_i : p.n_flags - 1);
            float* ov = fin ? run_val : tv[cur ^ 1];
            int64_t* oi = fin ? run_idx : ti[cur ^ 1];
            launch_cand_merge(tv[cur], ti[cur], cand_v, (const int64_t*)cand_i, cand_cnt, p.cap, nq, k, ov, oi, cflag, s,
                              p.sampled ? thr_dense : nullptr);
            // A candidate list of this chunk overflowed (document order with a drifting score distribution, a mass of
            // equal scores): the merge result is incomplete -- redo THIS chunk from the pre-chunk best by materialise +
            // select.  Sync-free: predicated on the chunk's device flag.  The thresholds of the next chunk come from the
            // corrected list, so a drift costs one or two recomputed chunks, not the whole call.
            // (Deferring the fallback to ONE predicated whole-shard recomputation per pass for short query batches saves 8 no-op
            // launches = 2 % at nq = 16, and costs 12.9 ms instead of 0.55 when a drift does overflow: a select over 1 M columns
            // has 16 rows of parallelism.  Measured and dropped, profiles/r03_score_defer_ab.txt.)
            if (!no_fallback) recompute(r, ch.doc0, seen, tv[cur], ti[cur], ov, oi, cflag);
            cur ^= 1;
            ++chunk_i;
        }
        c->filt_flag_off = (size_t)((char*)flag - base); c->filt_chunks = (int)(chunk_i < p.n_flags ? (long)chunk_i : p.n_flags);
        bv = tv[cur]; bi = ti[cur]; have = k;
    }
    if (p.rest > 0) {   // (filtered: only when no filtered chunk ran, N - first < 256 -- the ragged tail)
        st = classic(r, N - p.rest, N, bv, bi, have, run_val, run_idx, pred_all);
        if (st != SGPT_OK) return st;
    }
    if (n_out) *n_out = list_fill(n_run, N, k);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_score_topk(sgpt_ctx* c, const void* q, const void* corpus, int32_t dtype, int32_t nq, int64_t N,
                            int32_t d, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run,
                            int32_t* n_out, void* stream) {
    return score_topk_impl(c, q, corpus_rows(corpus, dtype, d), nq, N, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr);
}

// Documents [0, N) in blocks of at most `blk`, the running list chained from block to block: corpus_at(b0, nb) is the corpus of documents
// [b0, b0 + nb) (and may launch what makes it).
extern "C++" {     // (a template cannot have the C linkage this file is wrapped in)
template <class CorpusAt>
static sgpt_status score_topk_blocks(sgpt_ctx* c, const void* q, CorpusAt corpus_at, int64_t blk, int32_t nq, int64_t N, int32_t k,
                                     int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream) {
    int32_t have = n_run;
    for (int64_t b0 = 0; b0 < N; b0 += blk) {
        const int64_t nb = N - b0 < blk ? N - b0 : blk;
        sgpt_status st = score_topk_impl(c, q, corpus_at(b0, nb), nq, nb, k, idx_base + b0, run_val, run_idx, run_val, run_idx, have, &have, stream, nullptr);
        if (st != SGPT_OK) return st;
    }
    if (n_out) *n_out = have;
    return SGPT_OK;
}
}  // extern "C++"

// The same over a corpus of e4m3fn codes + one power-of-two scale per document (include/sgpt_hip.h).
sgpt_status sgpt_score_topk_q8(sgpt_ctx* c, const void* q, const uint8_t* codes, const float* scale, int32_t nq, int64_t N, int32_t d,
                               int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream) {
    if (!c || !q || !codes || !scale || !run_val || !run_idx || nq <= 0 || N <= 0 || d <= 0 || d % 8 || k <= 0 || n_run < 0 || n_run > k ||
        ((size_t)q & 15) || ((size_t)codes & 3))
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk_q8: bad arguments (d % 8 == 0, 0 <= n_run <= k, q 16-byte aligned)");
    // short query batches on a served width: the streaming tile reads the codes themselves
    if (nq <= 64 && score64q8_shape_ok(64, 256, d, codes, d))
        return score_topk_impl(c, q, corpus_fp8(codes, scale, d), nq, N, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr);
    // everything else (MFMA-bound, or a width the tile does not serve): blocks of at most 131 072 documents de-quantised to f16 rows
    // and scored by the f16 path, the running list chained from block to block -- the corpus stays one byte per element in memory
    const int64_t blk = 131072;
    HIPC(c, hipSetDevice(c->device));
    sgpt_status st = ensure(c, &c->ws6, &c->ws6_bytes, (size_t)(N < blk ? N : blk) * d * 2);
    if (st != SGPT_OK) return st;
    auto f16_block = [&](int64_t b0, int64_t nb) {
        launch_fp8_dequant_rows(codes + (size_t)b0 * d, scale + b0, nb, d, c->ws6, SGPT_F16, (hipStream_t)stream);
        return corpus_rows(c->ws6, SGPT_F16, d);
    };
    return score_topk_blocks(c, q, f16_block, blk, nq, N, k, idx_base, run_val, run_idx, n_run, n_out, stream);
}

// The same over a corpus of uint8 codes with one range per dimension (include/sgpt_hip.h): at most 64 fp32 query rows per call, every
// launch that reads the corpus is the streaming tile of scoreu8.hip.  Documents in blocks the launches index with 32 bits, the running
// list chained from block to block.
sgpt_status sgpt_score_topk_u8(sgpt_ctx* c, const float* q, const uint8_t* codes, const float* start, const float* step, int32_t nq,
                               int64_t N, int32_t d, int32_t ld, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run,
                               int32_t* n_out, void* stream) {
    if (!c || !q || !start || !step || !run_val || !run_idx || nq <= 0 || nq > 64 || N <= 0 || !u8_layout_ok(codes, d, ld, 16) ||
        k <= 0 || n_run < 0 || n_run > k)
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk_u8: bad arguments (1 <= nq <= 64, ld % 128 == 0, 0 < d <= ld, 0 <= n_run <= k, codes "
                                         "16-byte aligned)");
    auto block = [&](int64_t b0, int64_t) { return corpus_u8(codes + (size_t)b0 * ld, start, step, d, ld); };
    return score_topk_blocks(c, q, block, (int64_t)1 << 30, nq, N, k, idx_base, run_val, run_idx, n_run, n_out, stream);
}

sgpt_status sgpt_u8_col_minmax(sgpt_ctx* c, const float* x, int64_t n, int32_t d, int32_t accumulate, float* col_min, float* col_max,
                               void* stream) {
    if (!c || !x || !col_min || !col_max || n <= 0 || d <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_u8_col_minmax: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    launch_u8_col_minmax(x, n, d, accumulate != 0, col_min, col_max, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_u8_quantize_rows(sgpt_ctx* c, const float* x, int64_t n, int32_t d, int32_t ld, const float* start, const float* step,
                                  uint8_t* codes, void* stream) {
    if (!c || !x || !start || !step || n <= 0 || !u8_layout_ok(codes, d, ld, 4))
        return fail(c, SGPT_ERR_INVALID, "sgpt_u8_quantize_rows: bad arguments (ld % 128 == 0, 0 < d <= ld)");
    HIPC(c, hipSetDevice(c->device));
    launch_u8_quant_rows(x, n, d, ld, start, step, codes, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_u8_dequantize_rows(sgpt_ctx* c, const uint8_t* codes, int64_t n, int32_t ld, const float* start, const float* step, void* out,
                                    int32_t out_dtype, void* stream) {
    if (!c || !start || !step || !out || n <= 0 || !u8_layout_ok(codes, ld, ld, 4) || ((size_t)out & 15) ||
        (out_dtype != SGPT_F32 && out_dtype != SGPT_BF16 && out_dtype != SGPT_F16))
        return fail(c, SGPT_ERR_INVALID, "sgpt_u8_dequantize_rows: bad arguments (ld % 128 == 0, out 16-byte aligned)");
    HIPC(c, hipSetDevice(c->device));
    launch_u8_dequant_rows(codes, n, ld, start, step, out, out_dtype, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

// The second stage shared by sgpt_score_topk_bits and sgpt_score_topk_refined: stage 1 leaves the kp best per query in (lv, li), the
// caller re-scores them into the candidate list (cv, ci; row stride ldc = kp + k), and finish() appends the running list and selects.
// ws4 = [head bytes of the caller] | lv | li | cv | ci | [tail bytes of the caller]
struct TwoStage {
    char *head, *tail;
    float* lv; int64_t* li;
    float* cv; int64_t* ci;
    int ldc;
};
static sgpt_status two_stage_carve(sgpt_ctx* c, size_t head_b, size_t tail_b, int nq, int kp, int k, TwoStage& t) {
    t.ldc = kp + k;
    const size_t lv_b = align_up((size_t)nq * kp * 4, 256), li_b = align_up((size_t)nq * kp * 8, 256);
    const size_t cv_b = align_up((size_t)nq * t.ldc * 4, 256), ci_b = align_up((size_t)nq * t.ldc * 8, 256);
    sgpt_status st = ensure(c, &c->ws4, &c->ws4_bytes, head_b + lv_b + li_b + cv_b + ci_b + tail_b);
    if (st != SGPT_OK) return st;
    char* b = (char*)c->ws4;
    t.head = b; b += head_b;
    t.lv = (float*)b; b += lv_b;
    t.li = (int64_t*)b; b += li_b;
    t.cv = (float*)b; b += cv_b;
    t.ci = (int64_t*)b; b += ci_b;
    t.tail = b;
    return SGPT_OK;
}
// the re-scored candidates | the running list -> top-k
static void two_stage_finish(const TwoStage& t, float* run_val, int64_t* run_idx, int k, int n_run, int nq, int kp, hipStream_t s) {
    launch_list_append(run_val, run_idx, k, n_run, nq, t.cv, t.ci, t.ldc, kp, s);
    launch_topk_select(t.cv, t.ldc, 0, 0, t.cv, t.ci, kp + n_run, t.ldc, nq, k, 0, nullptr, run_val, run_idx, s);
}

static inline int bits_query_words(int d) { return (d + 127) / 128 * 4; }     // dwords of a packed query row: whole 16-byte pieces

// The two-stage search over packed sign bits that sgpt_score_topk_bits and sgpt_score_topk_bits_u8 are: the bits of q - center (center
// null: of q) packed, stage 1, the caller's second stage, the running list appended and selected.  ws4 head = [packed query bits | head_b
// bytes of the caller].  rescore(t, head, s) launches what values the candidates (t.lv, t.li) into (t.cv, t.ci); `head` is the caller's
// part of the head.  entry_ok: the caller's own argument checks; `bad`: its message for them and for the shared ones.
// Stage 1: the kp best by agreement (a descending, index ascending) of every packed query row, a fresh list per call, into (t.lv, t.li).
// Queries in groups of 64 (re-streaming 96-byte rows is cheap), documents in blocks the launches index with 32 bits, chained through the
// stage-1 list.
extern "C++" {
template <class Rescore>
static sgpt_status bits_two_stage(sgpt_ctx* c, const char* bad, bool entry_ok, const float* q, const float* center, const uint8_t* bits,
                                  int64_t ldb, int32_t nq, int64_t N, int32_t d, int32_t k, int32_t kp, int64_t idx_base, float* run_val,
                                  int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream, size_t head_b, Rescore rescore) {
    if (!entry_ok || !c || !q || !run_val || !run_idx || nq <= 0 || N <= 0 || !bits_layout_ok(bits, d, ldb, 4) || k <= 0 || kp < k || kp > 1024 ||
        n_run < 0 || n_run > k)
        return fail(c, SGPT_ERR_INVALID, bad);
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int qw = bits_query_words(d);
    const size_t qbits_b = align_up((size_t)nq * qw * 4, 256);
    TwoStage t;
    sgpt_status st = two_stage_carve(c, qbits_b + head_b, 0, nq, kp, k, t);
    if (st != SGPT_OK) return st;
    uint32_t* qbits = (uint32_t*)t.head;
    launch_pack_sign_bits(q, nq, d, center, (uint8_t*)qbits, (long)qw * 4, s);
    auto block = [&](int64_t b0, int64_t) { return corpus_bits(bits + (size_t)b0 * ldb, (long)ldb, qw, d); };
    for (int32_t g0 = 0; g0 < nq; g0 += 64) {
        st = score_topk_blocks(c, qbits + (size_t)g0 * qw, block, (int64_t)1 << 30, nq - g0 < 64 ? nq - g0 : 64, N, kp, idx_base,
                               t.lv + (size_t)g0 * kp, t.li + (size_t)g0 * kp, 0, nullptr, stream);
        if (st != SGPT_OK) return st;
    }
    rescore(t, t.head + qbits_b, s);
    two_stage_finish(t, run_val, run_idx, k, n_run, nq, kp, s);
    if (n_out) *n_out = list_fill(n_run, N, k);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}
}  // extern "C++"

// Hamming search over packed sign bits with optional re-scoring of the over-fetched candidates (include/sgpt_hip.h).
sgpt_status sgpt_score_topk_bits(sgpt_ctx* c, const float* q, const uint8_t* bits, int64_t ldb, int32_t nq, int64_t N, int32_t d, int32_t k,
                                 int32_t kp, int32_t mode, const uint8_t* codes, const float* scale, int64_t idx_base, float* run_val,
                                 int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream) {
    const bool ok = mode >= 0 && mode <= 2 && !(mode == 0 && kp != k) && !(mode == 2 && (!codes || !scale));
    // stage 2: the candidates' values by `mode` (as sgpt_score_topk_refined)
    auto rescore = [&](const TwoStage& t, char*, hipStream_t s) {
        launch_rescore_bits(mode, q, bits, (long)ldb, codes, ((long)d + 7) / 8 * 8, scale, t.lv, t.li, kp, nq, kp, d, idx_base, N, t.cv, t.ci, t.ldc, s);
    };
    return bits_two_stage(c, "sgpt_score_topk_bits: bad arguments (ldb % 4 == 0, ldb >= 4 ceil(d / 32), 0 < k <= kp <= 1024, "
                             "mode 0 with kp == k, mode 2 with codes and scale, 0 <= n_run <= k)",
                          ok, q, nullptr, bits, ldb, nq, N, d, k, kp, idx_base, run_val, run_idx, n_run, n_out, stream, 0, rescore);
}

// What launch_u8_rescore reads of the queries, carved from `b` and made there: [qs fp32 [nq][ld] | qbias fp32 [nq]].
struct U8RescoreQueries { const float *qs, *qbias; };
static inline size_t u8_rescore_queries_bytes(int nq, int ld) { return align_up((size_t)nq * ld * 4, 256) + align_up((size_t)nq * 4, 256); }
static U8RescoreQueries u8_rescore_queries(char* b, const float* q, const float* start, const float* step, int nq, int d, int ld, hipStream_t s) {
    float* qs = (float*)b;
    float* qbias = (float*)(b + align_up((size_t)nq * ld * 4, 256));
    launch_u8_rescore_prepare(q, start, step, nq, d, ld, qs, qbias, s);
    return {qs, qbias};
}

// The same first stage with a uint8 second stage (include/sgpt_hip.h): the bits are searched with q - center, the candidates re-scored
// from the codes with the raw q.
sgpt_status sgpt_score_topk_bits_u8(sgpt_ctx* c, const float* q, const float* center, const uint8_t* bits, int64_t ldb, const uint8_t* codes,
                                    const float* start, const float* step, int32_t ld, int32_t nq, int64_t N, int32_t d, int32_t k,
                                    int32_t kp, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out,
                                    void* stream) {
    const bool ok = start && step && u8_layout_ok(codes, d, ld, 16);
    // stage 2: <q, x^_n> of the candidates from the codes
    auto rescore = [&](const TwoStage& t, char* head, hipStream_t s) {
        const U8RescoreQueries u = u8_rescore_queries(head, q, start, step, nq, d, ld, s);
        launch_u8_rescore(u.qs, u.qbias, codes, ld, t.li, kp, nq, kp, idx_base, N, t.cv, t.ci, t.ldc, s);
    };
    return bits_two_stage(c, "sgpt_score_topk_bits_u8: bad arguments (ldb % 4 == 0, ldb >= 4 ceil(d / 32), ld % 128 == 0, 0 < d <= ld, "
                             "codes 16-byte aligned, 0 < k <= kp <= 1024, 0 <= n_run <= k)",
                          ok, q, center, bits, ldb, nq, N, d, k, kp, idx_base, run_val, run_idx, n_run, n_out, stream,
                          u8_rescore_queries_bytes(nq, ld), rescore);
}

// The second stage of the above alone: the values of the caller's candidate lists (include/sgpt_hip.h).  ws4 = [qs | qbias].
sgpt_status sgpt_u8_rescore(sgpt_ctx* c, const float* q, const uint8_t* codes, const float* start, const float* step, int32_t nq, int64_t N,
                            int32_t d, int32_t ld, const int64_t* idx, int64_t ld_idx, int32_t m, int64_t idx_base, float* out_val,
                            int64_t* out_idx, void* stream) {
    if (!c || !q || !start || !step || !idx || !out_val || !out_idx || nq <= 0 || N <= 0 || !u8_layout_ok(codes, d, ld, 16) || m <= 0 || ld_idx < m)
        return fail(c, SGPT_ERR_INVALID, "sgpt_u8_rescore: bad arguments (ld % 128 == 0, 0 < d <= ld, codes 16-byte aligned, 0 < m <= ld_idx)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    sgpt_status st = ensure(c, &c->ws4, &c->ws4_bytes, u8_rescore_queries_bytes(nq, ld));
    if (st != SGPT_OK) return st;
    const U8RescoreQueries u = u8_rescore_queries((char*)c->ws4, q, start, step, nq, d, ld, s);
    launch_u8_rescore(u.qs, u.qbias, codes, ld, idx, (long)ld_idx, nq, m, idx_base, N, out_val, out_idx, m, s);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_pack_sign_bits(sgpt_ctx* c, const float* x, int64_t n, int32_t d, const float* center, uint8_t* bits, int64_t ldb,
                                void* stream) {
    if (!c || !x || n <= 0 || !bits_layout_ok(bits, d, ldb, 1))
        return fail(c, SGPT_ERR_INVALID, "sgpt_pack_sign_bits: bad arguments (ldb % 4 == 0, ldb >= 4 ceil(d / 32))");
    HIPC(c, hipSetDevice(c->device));
    launch_pack_sign_bits(x, n, d, center, bits, ldb, (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

// How many filtered chunks of the last score + top-k pass on this context overflowed their candidate lists and were recomputed by
// the predicated fallback (diagnostics of the measurement scripts; synchronises `stream`).
sgpt_status sgpt_score_overflow_count(sgpt_ctx* c, int32_t* n_chunks, int32_t* n_overflowed, void* stream) {
    if (!c || !n_chunks || !n_overflowed) return fail(c, SGPT_ERR_INVALID, "sgpt_score_overflow_count: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    *n_chunks = c->filt_chunks; *n_overflowed = 0;
    if (c->ws2 && c->filt_chunks > 0) {
        std::vector<int> f(c->filt_chunks);
        HIPC(c, hipMemcpyAsync(f.data(), (const char*)c->ws2 + c->filt_flag_off, (size_t)c->filt_chunks * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPC(c, hipStreamSynchronize((hipStream_t)stream));
        for (int v : f) *n_overflowed += v != 0;
    }
    return SGPT_OK;
}

// The exact-fp32 top-k at the 16-bit scorer's speed (round 5): what `torch.mm(q, c.T)` + `torch.topk` of the reference compute in
// fp32 (util.py:41-43, exact_search.py:96-108), found in two stages.
//   1. the 16-bit filtered scorer over f16 copies of the rows takes the k' = k + M best per query (M: head-room, k' <= 64 keeps
//      the sampled schedule);
//   2. every candidate is re-scored in exact fp32 from the fp32 rows (rescore_kernel), merged with the running list, top-k.
// Guarantee: rows L2-normalised (or any rows with |q| |d| <= 1): |s16 - s32| <= eps = 2^-10 (two roundings of relative 2^-11,
// Cauchy-Schwarz) + 2^-25 (|q|_1 + |d|_1) (subnormal flushes) + the two fp32 accumulations ~ 1.1e-3.  A document outside the k'
// candidates has s16 <= u = the k'-th best; if u < t - 2 eps (t = the k-th best s16) its fp32 score is below t - eps, which k
// candidates reach or exceed: it cannot be in the fp32 top-k.  `margin` >= 2 eps is the caller's statement of that bound for its
// rows (2.5e-3 for unit rows; scale by max |q| max |d| for raw dot products).  Queries for which the check fails (masses of
// near-equal scores: duplicated documents) raise a device flag, and the chunk is redone by the exact-fp32 materialise-and-select
// pass, every launch predicated on that flag -- sync-free, exact either way; `refined_fallbacks` counts nothing on the host.
sgpt_status sgpt_score_topk_refined(sgpt_ctx* c, const float* q, const float* corpus32, const void* corpus16, int32_t dtype16,
                                    int32_t nq, int64_t N, int32_t d, int32_t k, int64_t idx_base, float margin,
                                    float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, int32_t* fallback_flag_out,
                                    void* stream) {
    if (!c || !q || !corpus32 || !corpus16 || !run_val || !run_idx || nq <= 0 || N <= 0 || k <= 0 || n_run < 0 || n_run > k ||
        !(margin > 0.f) || (dtype16 != SGPT_F16 && dtype16 != SGPT_BF16) || d % 8)
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk_refined: bad arguments (16-bit stage-1 rows, d % 8 == 0, margin > 0)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const Corpus rows32 = corpus_rows(corpus32, SGPT_F32, d);
    // head-room: as many extra candidates as the sampled schedule allows (k' <= 64), at least 8; deep lists (k > 56) take k / 8
    int kp = k <= 56 ? 64 : k + (k / 8 > 8 ? k / 8 : 8);
    if (kp > 1024 && k <= 1024) kp = 1024;
    if ((int64_t)kp > N) kp = (int)N;
    if (kp <= k || kp > 1024) {       // nothing to filter with (k >= N) or lists beyond the filtered scorer: the exact pass itself
        if (fallback_flag_out) *fallback_flag_out = -1;
        return score_topk_impl(c, q, rows32, nq, N, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr);
    }
    // ws4: the 16-bit query rows in front; behind the lists the running list as it was (for the fallback) and the flag
    const size_t sv_b = align_up((size_t)nq * k * 4, 256), si_b = align_up((size_t)nq * k * 8, 256);
    TwoStage t;
    sgpt_status st = two_stage_carve(c, align_up((size_t)nq * d * 2, 256), sv_b + si_b + 256, nq, kp, k, t);
    if (st != SGPT_OK) return st;
    void* q16 = t.head;
    float* sv = (float*)t.tail;
    int64_t* si = (int64_t*)(t.tail + sv_b);
    int* flag = (int*)(t.tail + sv_b + si_b);
    HIPC(c, hipMemsetAsync(flag, 0, 4, s));
    launch_f32_to_16(q, (int64_t)nq * d, q16, dtype16, s);
    // stage 1: the k' best by 16-bit score (fresh list)
    int32_t n1 = 0;
    st = score_topk_impl(c, q16, corpus_rows(corpus16, dtype16, d), nq, N, kp, idx_base, t.lv, t.li, t.lv, t.li, 0, &n1, stream, nullptr);
    if (st != SGPT_OK) return st;
    launch_refine_check(t.lv, k, kp, margin, nq, flag, s);
    // stage 2: exact fp32 scores of the candidates | the running list -> top-k
    if (n_run > 0) {      // (kept for the fallback: it starts from the list as it was before this chunk)
        HIPC(c, hipMemcpy2DAsync(sv, (size_t)k * 4, run_val, (size_t)k * 4, (size_t)n_run * 4, nq, hipMemcpyDeviceToDevice, s));
        HIPC(c, hipMemcpy2DAsync(si, (size_t)k * 8, run_idx, (size_t)k * 8, (size_t)n_run * 8, nq, hipMemcpyDeviceToDevice, s));
    }
    launch_rescore(q, corpus32, t.li, kp, nq, kp, d, idx_base, N, t.cv, t.ci, t.ldc, s);
    two_stage_finish(t, run_val, run_idx, k, n_run, nq, kp, s);
    // the predicated exact pass (no-op launches unless a query failed the check)
    st = score_topk_impl(c, q, rows32, nq, N, k, idx_base, sv, si, run_val, run_idx, n_run, nullptr, stream, flag);
    if (st != SGPT_OK) return st;
    if (fallback_flag_out) {     // optional, host-synchronising: did the exact pass run? (tests / diagnostics; pass NULL to stay asynchronous)
        HIPC(c, hipMemcpyAsync(fallback_flag_out, flag, 4, hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
    }
    if (n_out) *n_out = list_fill(n_run, N, k);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_topk_merge(sgpt_ctx* c, const float* val, const int64_t* idx, int32_t nq, int32_t mcand, int32_t k,
                            const int64_t* exclude_idx, float* out_val, int64_t* out_idx, void* stream) {
    if (!c || !val || !idx || !out_val || !out_idx || nq <= 0 || mcand <= 0 || k <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_topk_merge: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    // all candidates ride in the "previous best" leg of the virtual row (n = 0 fresh scores)
    launch_topk_select(val, mcand, 0, 0, val, idx, mcand, mcand, nq, k, 0, exclude_idx, out_val, out_idx,
                       (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_topk(sgpt_ctx* c, const float* scores, int32_t nq, int64_t n, int64_t ld, int32_t k, int64_t idx_base,
                      float* out_val, int64_t* out_idx, void* stream) {
    if (!c || !scores || !out_val || !out_idx || nq <= 0 || n <= 0 || ld < n || k <= 0)
        return fail(c, SGPT_ERR_INVALID, "sgpt_topk: bad arguments");
    HIPC(c, hipSetDevice(c->device));
    launch_topk_select(scores, ld, n, idx_base, nullptr, nullptr, 0, 0, nq, k, 1, nullptr, out_val, out_idx,
                       (hipStream_t)stream);
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

}  // extern "C"
