// C ABI (include/sgpt_hip.h): the scorer -- score tiles, the filtered score + top-k schedule and its exact-fp32 refinement.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
#include "host.h"

extern "C" {

sgpt_status sgpt_l2_normalize(sgpt_ctx* c, const float* in, int64_t n, int32_t d, void* out, int32_t out_dtype,
                              void* stream) {
    if (!c || !in || !out || n <= 0 || d <= 0) return fail(c, SGPT_ERR_INVALID, "sgpt_l2_normalize: bad arguments");
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

// in_val / in_idx: the running list going in (n_run entries per row, row stride k); run_val / run_idx: the list coming out (they
// may be the same buffers -- the public entry point).  pred_all (device flag or null): every launch of the call is predicated on
// it and the call takes the materialise-and-select path -- the sync-free fallback of sgpt_score_topk_refined.
// A corpus of packed sign bits (sgpt_score_topk_bits): rows of ldb bytes, queries packed alike in rows of qw dwords
struct BitRows { long ldb; int qw; };

static sgpt_status score_topk_impl(sgpt_ctx* c, const void* q, const void* corpus, int32_t dtype, int32_t nq, int64_t N,
                                   int32_t d, int32_t k, int64_t idx_base, const float* in_val, const int64_t* in_idx,
                                   float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream, const int* pred_all,
                                   const float* q8_scale = nullptr, const BitRows* bits = nullptr) {
    // q8_scale (sgpt_score_topk_q8, short query batches): `corpus` holds e4m3fn codes [N][d] bytes, q8_scale one power-of-two scale per
    // document, q is f16 (dtype SGPT_F16).  Same schedule; only the launches that read the corpus change: whole 256-document tiles go
    // through score64q8_kernel (score8.hip), a ragged tail is de-quantised into f16 scratch for the register-staged kernel.
    // bits (sgpt_score_topk_bits, at most 64 queries per call): `corpus` holds packed sign bits [N][bits->ldb] bytes, q the packed
    // query rows; the score is the agreement d - 2 * hamming, an integer in fp32.  Same schedule again; every launch that reads the
    // corpus is the Hamming tile (scorebits.hip), which takes any number of documents, so no launch is split for a ragged tail.
    const bool q8 = q8_scale != nullptr;
    if (!c || !q || !corpus || !run_val || !run_idx || nq <= 0 || N <= 0 || k <= 0 || n_run < 0 || n_run > k)
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk: bad arguments");
    sgpt_status st = bits ? SGPT_OK : check_score_dims(c, dtype, d);
    if (st != SGPT_OK) return st;
    if (bits && (nq > 64 || d <= 0 || q8)) return fail(c, SGPT_ERR_INVALID, "score (binary corpus): at most 64 queries per pass");
    if (q8 && !(dtype == SGPT_F16 && nq <= 64 && score64q8_shape_ok(64, 256, d, corpus, d)))
        return fail(c, SGPT_ERR_INVALID, "score (fp8 corpus): shape not served by the streaming tile");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // chunk the corpus so the fp32 score tile [nq, chunk] stays resident in the 256 MiB Infinity Cache, and so
    // that the score GEMM has a whole number of 256-CU waves of 256x256 tiles (query tiles x document tiles)
    const size_t budget = (size_t)160 << 20;
    const int mtq = (nq + 255) / 256;                 // (short query batches, nq <= 64: one 64-row tile, see below)
    long unit = 256;                                  // documents per chunk granule
    { int g = mtq, h = 256; while (h) { int r = g % h; g = h; h = r; } unit = 256L * (256 / g); }
    long chunk = (long)(budget / ((size_t)nq * 4));
    if (chunk >= unit) chunk = chunk / unit * unit;
    else { chunk = chunk / 256 * 256; if (chunk < 256) chunk = 256; }
    if (chunk > 131072) chunk = 131072;
    if (chunk > N) chunk = (long)align_up((size_t)N, 4);
    // bf16 fast path: the 256x256 LDS-DMA GEMM needs the query rows padded to a multiple of 256 (zero rows,
    // never stored) and d % 64 == 0; chunks that are multiples of 256 documents take it, the ragged tail and
    // fp32 go through the 128^2 kernel.
    const bool fast = bits || (dtype != SGPT_F32 && d % 64 == 0 && d >= 128);
    // nq <= 64: the 64-query-row scorer tile (score64_kernel) instead of 256 padded rows -- the pass is HBM-bound there
    static const bool no_small_q = exp_env("SGPT_SCORE_NO64") != nullptr;      // A/B switch (experiment build only)
    const int nq_pad = (fast && nq <= 64 && !no_small_q) ? 64 : (nq + 255) / 256 * 256;
    // Threshold-filtered chunks (after the first): see EPI_SCORE_FILTER.  Candidate capacity per query and chunk;
    // the doubling schedule below keeps the expected count at ~k.
    static const bool classic_only = exp_env("SGPT_SCORE_CLASSIC") != nullptr;
    // Capacity and growth: a filtered chunk of len = growth * seen documents expects ~k * growth survivors per query
    // (the threshold is the k-th best of `seen` documents); the merge sorts the candidates in 2048 LDS slots.
    // k <= 64 ("sampled" schedule, round 4): the first thresholds come from a STRIDED SAMPLE of the whole shard instead of its
    // first documents, so (a) nothing is materialised but the sample's own score tile, (b) the expected number of survivors of
    // a chunk, k * len / S, holds whatever the document order does to the score distribution (the reference sorts the corpus
    // by length: a drift along the index used to overflow the lists and pay the materialised recomputation of the chunk), and
    // (c) chunks can therefore be as long as the lists allow instead of doubling: a 125 k-document shard is ONE filtered
    // launch, 1 M documents three (1 + 6 before).  The rank of a sample's k-th best in the population is Gamma(k)-distributed
    // (relative spread 1 / sqrt(k)): lists of `cap` entries take R = cap / (k (1 + 6 / sqrt(k))) times the documents the
    // thresholds were drawn from with ~6 sigma of head-room.
    const bool sampled_k = k <= 64;
    // list capacity of the sampled schedule: the sample is N / ratio documents and ratio grows with cap, so long shards take
    // long lists (1 M documents, k = 11: 2048 entries -> a 15 k-document sample instead of 60 k); short shards keep short
    // ones, because the expected survivors per row and 256-document tile, cap / (2.8 N / 256), is what the filtered GEMM's
    // append path pays for (0.37 at 125 k documents with 512 entries: 236 us per launch against ~190 without appends)
    // nq <= 64 (the HBM-bound 64-row tile): same-box A/B of 512 / 1024 / 2048 entries at 1 M documents (profiles/r04_cap64_ab.txt):
    // nq = 16 0.39 / 0.36 / 0.365 ms, nq = 64 0.41 / 0.375 / 0.39 ms -- the sample is 6 % / 3 % / 1.5 % of the corpus stream, and
    // past 1024 entries the appends cost the streaming tile more than the smaller sample returns
    // (re-measured with the LDS-staged appends, nq = 1000: 125 k documents 0.28 / 0.36 / 0.40 ms with 512 / 1024 / 2048 entries,
    //  250 k documents 0.51 / 0.50 / 0.58 -- the short lists stay)
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
    const int cap_n = nq <= 64 ? (N >= 400000 ? 1024 : 512) : (N >= 800000 ? 2048 : (N >= 400000 ? 1024 : SGPT_CAP_SHORT));
    const int cap_s = cap_n * (k <= 32 ? 1 : 2) > 2048 ? 2048 : cap_n * (k <= 32 ? 1 : 2);
    const int cap = sampled_k ? cap_s : ((4 * k < 2048 - k) ? 4 * k : 2048 - k);
    const bool half_growth = 2 * cap < 5 * k;          // k > ~340: cap < 2.5 k -> grow by half, expect ~k/2 per chunk
    // k > 64 keeps the first-chunk + doubling schedule.  Two other schedules were measured against doubling and rejected:
    //   round 2: 4x growth with 256-entry lists -- overflowed on corpora whose score distribution drifts along the index and
    //            paid the materialised recomputation;
    //   round 3: 2048-entry lists with growth cap / 6k (k = 11: first chunk + two filtered chunks per 1 M documents) -- ~330
    //            survivors per query and chunk through the epilogue's append path: the filtered GEMM went from 1.45 to 1.58 ms
    //            per pass (nq = 1000), and a drift at 10 % of the corpus from 2.2 to 3.5 ms (profiles/r03_score_schedule.txt).
    const int growth = 1;
    const bool filt = fast && !classic_only && k <= 1024 && chunk % 256 == 0 && N >= 2 * chunk && pred_all == nullptr;
    const bool sampled = filt && sampled_k;
    // (binary corpus: half the ratio.  Integer agreements tie at the threshold, and the inclusive threshold lets the whole tie class of
    //  the k-th best through -- up to ~2x the survivors at d = 768.)
    const double ratio = (double)cap / ((double)k * (1.0 + 6.0 / std::sqrt((double)k))) * (bits ? 0.5 : 1.0);   // documents per threshold document
    const long n256_all = N / 256 * 256;
    long S = 0, s_stride = 1;                           // sample size (documents) and row stride
    if (sampled) {
        // S = N / ratio: the survivors of the WHOLE shard fit the lists even if no chunk ever raises the thresholds (a corpus
        // whose best documents all come last).  Bounded by a 512 MiB score tile (131 072 documents at nq = 1000; 1 M documents
        // need 60 k): behind that the schedule relies on the merges raising the thresholds, like the doubling one did.
        S = ((long)((double)N / ratio * SGPT_SAMPLE_MULT) + 255) / 256 * 256;     // rounded UP: ratio * S covers the shard
        if (S < 2048) S = 2048;
        const long s_max = (long)(((size_t)512 << 20) / ((size_t)nq * 4)) / 256 * 256;
        if (S > s_max) S = s_max > 2048 ? s_max : 2048;
        // binary corpus: a sample the select takes in ONE pass -- its LDS candidate list (2048 slots) expects k * S / 1024 entries, and
        // past it the radix passes over a million columns on one workgroup per query cost more than the whole bit stream
        // (profiles/score_bits_corpus.txt, variant B: 16 M x 768, nq = 1, 10.8 ms without this bound and the spread sample scores, 0.38 ms with both).  The filtered chunks then grow from S * ratio documents as the merges raise the
        // thresholds: two launches for 16 M documents instead of one.
        if (bits) { const long s_one = 1000L * 1024 / k / 256 * 256; if (S > s_one) S = s_one > 2048 ? s_one : 2048; }
        if (S > n256_all / 2) S = n256_all / 2 / 256 * 256;
        s_stride = n256_all / S;
        if (s_stride < 1) s_stride = 1;
        // an ODD stride: a corpus with a power-of-two period (bench.py's 1 M shard is perturbed copies of a 40 960-document
        // block: stride 16 met the SAME source documents in every copy -- a third of the effective sample, and lists that
        // overflowed for a few queries in a thousand) is the structure a sample must not resonate with
        if (s_stride > 1 && s_stride % 2 == 0) s_stride -= 1;
        // equally spaced rows have an integer stride: stretch the sample to the END of the shard at that stride (a tail the
        // sample never visits is invisible to the thresholds -- 33 k of 1 M documents at stride 16: a corpus whose best
        // documents sit at the end overflowed the lists of ~3 queries in 1000)
        S = n256_all / s_stride / 256 * 256;
    }

    // A filtered chunk whose candidate lists overflow is recomputed by materialise + select in pieces whose fp32 score tile
    // stays in the Infinity Cache (measured: 1 GiB tiles made the recomputation 6x slower than the plain materialised
    // loop).  Its launches are predicated and exit at once otherwise -- for short query batches one piece covers a whole
    // chunk (nq = 16: 2.6 M documents per 160 MiB tile), so a pass carries 2 predicated launches per chunk, not 2 per 131 072
    // documents.
    long fchunk = (long)(budget / ((size_t)nq * 4)) / 256 * 256;
    // sampled schedule: an overflow needs an adversarial mass of near-equal scores now, so the fallback is sized for few
    // no-op launches (a predicated 256x256 launch that exits at once still costs ~4.4 us, two per piece: ~60 of them were
    // 0.05-0.08 ms of a 1 M-document pass) rather than for the cache: pieces of up to 131 072 documents
    // -- but never beyond a byte budget: the tile is allocated whether or not a fallback ever runs (nq = 10 000 x 131 072 x 4 B
    // would be 5 GB of workspace for launches that exit at once)
    if (sampled && fchunk < 131072) {
        const long by_bytes = (long)(((size_t)512 << 20) / ((size_t)nq * 4)) / 256 * 256;
        const long want = by_bytes < 131072 ? by_bytes : 131072;
        if (fchunk < want) fchunk = want;
    }
    if (fchunk > (long)align_up((size_t)N, 256)) fchunk = (long)align_up((size_t)N, 256);
    if (fchunk < chunk) fchunk = chunk;
    const long n_flags = 64 + N / (1L << 19) + 1;      // one overflow flag per filtered chunk
    const size_t sc_bytes = align_up((size_t)nq * (fchunk > S ? fchunk : S) * 4, 256);
    const size_t tv_bytes = align_up((size_t)nq * k * 4, 256), ti_bytes = align_up((size_t)nq * k * 8, 256);
    const size_t qp_bytes = fast && !bits ? align_up((size_t)nq_pad * d * 2, 256) : 0;     // (packed query rows are read where they are)
    const size_t cv_bytes = filt ? align_up((size_t)nq * cap * 4, 256) : 0, ci_bytes = filt ? align_up((size_t)nq * cap * 8, 256) : 0;
    const size_t cc_bytes = filt ? align_up((size_t)(nq_pad + n_flags) * 4, 256) : 0;  // counters + per-chunk overflow flags
    const size_t th_bytes = sampled ? tv_bytes + ti_bytes + align_up((size_t)nq * 4, 256) : 0;   // sample's list + dense thresholds
    st = ensure(c, &c->ws2, &c->ws2_bytes,
                sc_bytes + 3 * (tv_bytes + ti_bytes) + qp_bytes + cv_bytes + ci_bytes + cc_bytes + th_bytes);
    if (st != SGPT_OK) return st;
    if (q8) {       // f16 rows of a ragged tail (< 256 documents)
        st = ensure(c, &c->ws6, &c->ws6_bytes, (size_t)256 * d * 2);
        if (st != SGPT_OK) return st;
    }
    char* base = (char*)c->ws2;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p_ = base + off; off += bytes; return p_; };
    float* sc = (float*)take(sc_bytes);
    float* tv[2]; int64_t* ti[2];
    tv[0] = (float*)take(tv_bytes); tv[1] = (float*)take(tv_bytes);
    ti[0] = (int64_t*)take(ti_bytes); ti[1] = (int64_t*)take(ti_bytes);
    float* sav_v = (float*)take(tv_bytes); int64_t* sav_i = (int64_t*)take(ti_bytes);   // third list: ping-pong partner of a recomputation
    void* qpad = bits ? const_cast<void*>(q) : (fast ? take(qp_bytes) : nullptr);
    float* cand_v = filt ? (float*)take(cv_bytes) : nullptr;
    long long* cand_i = filt ? (long long*)take(ci_bytes) : nullptr;
    int* cand_cnt = filt ? (int*)take(cc_bytes) : nullptr;
    int* flag = filt ? cand_cnt + nq_pad : nullptr;
    float* th_v = sampled ? (float*)take(tv_bytes) : nullptr;
    int64_t* th_i = sampled ? (int64_t*)take(ti_bytes) : nullptr;
    float* thr_dense = sampled ? (float*)take(align_up((size_t)nq * 4, 256)) : nullptr;
    // prologue: one launch (query rows into their zero-padded tile, counters and flags cleared, an empty running list marked)
    const bool fresh_list = sampled && n_run == 0;
    if (bits || (fast && d % 8 == 0 && ((size_t)q & 15) == 0)) {
        launch_score_prep(q, qpad, bits ? 0 : (long)nq * d * 2, bits ? 0 : (long)nq_pad * d * 2, filt ? cand_cnt : nullptr, filt ? (long)(nq_pad + n_flags) : 0,
                          fresh_list ? (long long*)ti[0] : nullptr, fresh_list ? (long)nq * k : 0, s);
    } else {
        if (fast) {
            if (nq_pad > nq) HIPC(c, hipMemsetAsync((char*)qpad + (size_t)nq * d * 2, 0, (size_t)(nq_pad - nq) * d * 2, s));   // the pad rows only
            HIPC(c, hipMemcpyAsync(qpad, q, (size_t)nq * d * 2, hipMemcpyDeviceToDevice, s));
        }
        if (filt) HIPC(c, hipMemsetAsync(cand_cnt, 0, (size_t)(nq_pad + n_flags) * 4, s));
        if (fresh_list) HIPC(c, hipMemsetAsync(ti[0], 0xff, (size_t)nq * k * 8, s));
    }
    const size_t esz = q8 ? 1 : (dtype == SGPT_F32 ? 4 : 2);
    const size_t rowb = bits ? (size_t)bits->ldb : (size_t)d * esz;     // bytes of a corpus row
    const long ldw1 = bits ? bits->ldb : d;                             // GemmArgs.ldw of consecutive rows (the Hamming tile counts bytes)
    // one launch that reads documents [doc0, doc0 + h.N) (at row_stride): h.W / h.ldw are set for them already
    auto docs_gemm = [&](int epi, GemmArgs h, long doc0, long row_stride, bool sample = false) {
        if (bits) { h.A = q; h.m_valid = nq; launch_scorebits(epi, h, d, bits->qw, bits->ldb, s, sample); return; }
        if (!q8) { gemm(c, dtype, epi, SGPT_F32, h, s); return; }
        if (h.N % 256 == 0) {
            Score8Args a8{h, q8_scale + doc0, row_stride};
            launch_score64q8(epi, a8, s);
        } else {        // (the tail is never strided)
            launch_fp8_dequant_rows(h.W, q8_scale + doc0, h.N, d, c->ws6, SGPT_F16, s);
            h.W = c->ws6; h.ldw = d;
            gemm(c, SGPT_F16, epi, SGPT_F32, h, s);
        }
    };

    // fp32 scores of documents [c0, c0 + nc) for every query -> sc[nq][ld]
    auto score_tile = [&](long c0, long nc, long ld, const int* pred, long row_stride = 1, bool sample = false) {
        GemmArgs g{};
        g.A = q; g.lda = d; g.M = nq; g.m_valid = nq; g.K = d; g.pred = pred;
        g.W = (const char*)corpus + (size_t)c0 * rowb; g.ldw = ldw1 * row_stride; g.N = (int)nc;   // row_stride > 1: a strided sample
        g.out = sc; g.ldo = ld;
        if (bits) { docs_gemm(EPI_SCORE, g, c0, row_stride, sample); return; }
        const long na = fast ? nc / 256 * 256 : 0;      // documents the 256-document tile kernels take
        // (round 5, measured and reverted: handing a predicated fallback piece to the register-staged kernel whole -- one no-op launch
        //  instead of two -- made the shard pass 12 % SLOWER: a no-op launch of the persistent 256x256 kernel is 256 workgroups that
        //  exit, one of the small-tile kernel for 125 k documents x 1000 queries is ~8 000.)
        // the < 256 trailing documents ride in the 256x256 launch (clamped rows, GemmArgs.n_valid; their missing columns land in the
        // padding of the score row, which the select does not read): one launch less per piece -- a no-op one in the predicated
        // fallback of every filtered chunk
        const bool fold = SGPT_FOLD_TAIL && SGPT_FOLD_TAIL_SCORE && na > 0 && na < nc && row_stride == 1 && na + 256 <= ld &&
                          gemm_score_tail_foldable(nq_pad, na + 256, d);
        if (na > 0) {
            GemmArgs h = g;
            h.A = qpad; h.M = nq_pad; h.N = (int)(fold ? na + 256 : na); h.n_valid = fold ? (int)nc : 0;
            docs_gemm(EPI_SCORE, h, c0, row_stride);
        }
        if (na < nc && !fold) {                         // fp32, or the ragged tail (< 256 documents): register-staged kernel
            g.W = (const char*)corpus + (size_t)(c0 + na) * rowb; g.N = (int)(nc - na); g.out = sc + na;
            docs_gemm(EPI_SCORE, g, c0 + na, 1);
        }
    };
    // Materialise-and-select over documents [lo, hi): the reference's chunk loop (exact_search.py:96-132).
    // (pv, pi, have) = running best going in; the last chunk writes (fin_v, fin_i), earlier ones ping-pong.
    auto classic = [&](long lo, long hi, const float* pv, const int64_t* pi, int have, float* fin_v, int64_t* fin_i,
                       const int* pred, long chunk) -> sgpt_status {
        int cur = (pv == tv[0]) ? 1 : 0;
        for (long c0 = lo; c0 < hi; c0 += chunk) {
            const long nc = (hi - c0) < chunk ? (hi - c0) : chunk;
            score_tile(c0, nc, chunk, pred);
            const bool last = c0 + nc >= hi;
            if (last && pv == fin_v) {  // in/out alias on a single-chunk call: stage through the ping-pong buffer
                launch_topk_select(sc, chunk, nc, idx_base + c0, pv, pi, have, k, nq, k, 0, nullptr, tv[cur], ti[cur], s, pred);
                HIPC(c, hipMemcpyAsync(fin_v, tv[cur], (size_t)nq * k * 4, hipMemcpyDeviceToDevice, s));
                HIPC(c, hipMemcpyAsync(fin_i, ti[cur], (size_t)nq * k * 8, hipMemcpyDeviceToDevice, s));
            } else {
                launch_topk_select(sc, chunk, nc, idx_base + c0, pv, pi, have, k, nq, k, 0, nullptr,
                                   last ? fin_v : tv[cur], last ? fin_i : ti[cur], s, pred);
            }
            pv = tv[cur]; pi = ti[cur];
            have = k;  // unused tail slots carry idx = -1 and are ignored by the next merge
            cur ^= 1;
        }
        return SGPT_OK;
    };

    // The same over [lo, hi) with every launch predicated on *pred (a filtered chunk's overflow flag): (pv, pi) = the
    // k-slot running best before the chunk, result in (fin_v, fin_i); pieces of fchunk documents ping-pong through the
    // third list so that nothing is copied (a copy could not be predicated).
    auto recompute = [&](long lo, long hi, const float* pv, const int64_t* pi, float* fin_v, int64_t* fin_i, const int* pred) {
        const long P = (hi - lo + fchunk - 1) / fchunk;
        for (long pc = 0; pc < P; ++pc) {
            const long c0 = lo + pc * fchunk, nc = (hi - c0) < fchunk ? (hi - c0) : fchunk;
            const bool to_fin = (P - 1 - pc) % 2 == 0;
            float* dv = to_fin ? fin_v : sav_v;
            int64_t* di = to_fin ? fin_i : sav_i;
            score_tile(c0, nc, fchunk, pred);
            launch_topk_select(sc, fchunk, nc, idx_base + c0, pv, pi, k, k, nq, k, 0, nullptr, dv, di, s, pred);
            pv = dv; pi = di;
        }
    };

    const float* pv0 = n_run > 0 ? in_val : nullptr;
    const int64_t* pi0 = n_run > 0 ? in_idx : nullptr;
    c->filt_chunks = 0;
    if (!filt) {
        st = classic(0, N, pv0, pi0, n_run, run_val, run_idx, pred_all, chunk);
        if (st != SGPT_OK) return st;
    } else {
        static const bool no_fallback = exp_env("SGPT_SCORE_NOFALLBACK") != nullptr;   // timing experiments ONLY: unsafe
        int cur = 0, chunk_i = 0;
        long seen = 0;                 // documents behind which the filtered chunks continue
        long eff = 0;                  // documents the current thresholds are the k-th best of
        const long n256 = n256_all;
        if (sampled) {
            // running best going in: tv[0] / ti[0] = the caller's list padded to k columns, or empty (idx -1 everywhere)
            if (n_run > 0) {
                launch_topk_select(in_val, k, 0, 0, in_val, in_idx, n_run, k, nq, k, 0, nullptr, tv[0], ti[0], s);
            }   // (n_run == 0: the prologue marked tv[0] / ti[0] empty -- idx -1, whatever the values say)
            // thresholds: the k-th best of {running best} U {S documents at stride s_stride across the shard}; only the VALUES
            // of this selection are used (its indices are sample positions) -- the filtered chunks below re-score the sampled
            // documents like any other and find them again
            if (SGPT_SAMPLE_TOP2 && nq_pad >= 256 && S % 256 == 0) {
                // the sample's scores never leave the GEMM: 8 floats per query row and 256-document tile (the two best of each
                // wave's 64 documents, EPI_SCORE_TOP2); the k-th best of those and the running list is the threshold
                const long ld2 = 8 * (S / 256);
                GemmArgs h{};
                h.A = qpad; h.lda = d; h.M = nq_pad; h.m_valid = nq; h.K = d;
                h.W = corpus; h.ldw = (long)d * s_stride; h.N = (int)S; h.out = sc; h.ldo = ld2;
                gemm(c, dtype, EPI_SCORE_TOP2, SGPT_F32, h, s);
                launch_topk_select(sc, ld2, ld2, 0, tv[0], ti[0], k, k, nq, k, 0, nullptr, th_v, th_i, s, nullptr, thr_dense);
            } else {
                score_tile(0, S, S, nullptr, s_stride, true);      // (binary corpus: the sample's ties spread, launch_scorebits)
                launch_topk_select(sc, S, S, 0, tv[0], ti[0], k, k, nq, k, 0, nullptr, th_v, th_i, s, nullptr, thr_dense);   // (+ the inclusive threshold)
            }
            eff = S;
        } else {
            // first chunk: materialise + select -> the initial thresholds.  One whole wave of tiles is enough (the
            // doubling schedule takes over from there): 16 384 documents for nq = 1000 instead of 32 768
            const long first = unit < chunk ? unit : chunk;
            st = classic(0, first, pv0, pi0, n_run, tv[0], ti[0], nullptr, chunk);
            if (st != SGPT_OK) return st;
            seen = first; eff = first;
        }
        // k > 64, doubling schedule: a filtered chunk is as long as everything seen before it, so a query expects ~k
        // survivors per chunk (k * len / seen) whatever N is; 1 M documents = 1 + 5 launches instead of 31.
        // k <= 64, sampled schedule: `ratio` times the documents the thresholds stand for (see above).
        while (n256 - seen >= 256) {
            long len;
            if (sampled) len = (long)((double)eff * ratio) / 256 * 256;
            else len = half_growth ? (eff / 2 / 256 * 256 > 256 ? eff / 2 / 256 * 256 : 256) : eff * growth;
            if (len < 256) len = 256;
            // chunks of at most 2^19 documents: a merge half-way through a 1 M-document pass tightens the thresholds of the
            // second half (nq = 1000: 380 + 10 appended candidates per query instead of 730; measured 1.62-1.64 against
            // 1.65-1.69 ms, nq = 128 0.51 against 0.54).  Short query batches (the HBM-bound 64-row tile) take the whole shard
            // in ONE launch instead: a merge, three no-op fallback launches and a pipeline ramp less (nq = 16: 0.36 -> 0.35 ms)
            if (len > (1L << 19) && !(sampled && nq <= 64)) len = 1L << 19;
            if (len >= n256 - seen) len = n256 - seen;          // the last chunk takes what is left (no whole-wave rounding: that
            else if (len >= unit) len = len / unit * unit;      //  left a 17 k-document sixth launch behind 1 M documents at nq = 16)
            GemmArgs g{};
            g.A = qpad; g.lda = d; g.M = nq_pad; g.m_valid = nq; g.K = d;
            g.W = (const char*)corpus + (size_t)seen * rowb; g.ldw = ldw1; g.N = (int)len;
            // sampled schedule: the dense thresholds -- the sample's k-th best, raised by every merge to the running k-th best
            if (sampled) { g.thr = thr_dense; g.thr_ld = 1; }
            else { g.thr = tv[cur] + (k - 1); g.thr_ld = k; }
            g.cand_val = cand_v; g.cand_idx = cand_i; g.cand_cnt = cand_cnt; g.cand_cap = cap; g.idx_base = idx_base + seen;
            // the < 256 trailing documents ride in the last chunk's launch (the 256x256 kernel clamps their rows and masks their
            // columns, GemmArgs.n_valid) when documents are its streamed operand; the 64-row tile keeps its own tail launch
            const bool fold_tail = seen + len == n256 && N > n256 && (bits || (SGPT_FOLD_TAIL && gemm_score_tail_foldable(nq_pad, len + 256, d)));
            if (fold_tail) { g.N = (int)(bits ? len + (N - n256) : len + 256); g.n_valid = (int)(len + (N - n256)); }
            docs_gemm(EPI_SCORE_FILTER, g, seen, 1);
            g.n_valid = 0;
            const long c_lo = seen;
            seen += len;
            if (fold_tail) seen = N;
            eff = seen;                                         // the thresholds now stand for every document of [0, seen)
            if (seen == n256 && seen < N) {
                // ragged tail (< 256 documents): filtered against the same thresholds by the small-tile kernel, its
                // survivors join this chunk's candidate lists -- one merge, no materialise + select round for 72 documents
                g.W = (const char*)corpus + (size_t)seen * rowb; g.N = (int)(N - seen); g.idx_base = idx_base + seen;
                docs_gemm(EPI_SCORE_FILTER, g, seen, 1);
                seen = N;
            }
            const bool fin = seen >= N;
            int* cflag = flag + (chunk_i < n_flags ? chunk_i : n_flags - 1);
            float* ov = fin ? run_val : tv[cur ^ 1];
            int64_t* oi = fin ? run_idx : ti[cur ^ 1];
            launch_cand_merge(tv[cur], ti[cur], cand_v, (const int64_t*)cand_i, cand_cnt, cap, nq, k, ov, oi, cflag, s,
                              sampled ? thr_dense : nullptr);
            // A candidate list of this chunk overflowed (document order with a drifting score distribution, a mass of
            // equal scores): the merge result is incomplete -- redo THIS chunk from the pre-chunk best by materialise +
            // select.  Sync-free: predicated on the chunk's device flag.  The thresholds of the next chunk come from the
            // corrected list, so a drift costs one or two recomputed chunks, not the whole call.
            // (Deferring the fallback to ONE predicated whole-shard recomputation per pass for short query batches saves 8 no-op
            // launches = 2 % at nq = 16, and costs 12.9 ms instead of 0.55 when a drift does overflow: a select over 1 M columns
            // has 16 rows of parallelism.  Measured and dropped, profiles/r03_score_defer_ab.txt.)
            if (!no_fallback) recompute(c_lo, seen, tv[cur], ti[cur], ov, oi, cflag);
            cur ^= 1;
            ++chunk_i;
        }
        c->filt_flag_off = (size_t)((char*)flag - base); c->filt_chunks = (int)(chunk_i < n_flags ? (long)chunk_i : n_flags);
        if (seen < N) {   // (only when no filtered chunk ran: N - first < 256) ragged tail: materialise + select
            st = classic(seen, N, tv[cur], ti[cur], k, run_val, run_idx, nullptr, chunk);
            if (st != SGPT_OK) return st;
        }
    }
    if (n_out) { const int64_t tot = (int64_t)n_run + N; *n_out = (int32_t)(tot < k ? tot : k); }
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_score_topk(sgpt_ctx* c, const void* q, const void* corpus, int32_t dtype, int32_t nq, int64_t N,
                            int32_t d, int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run,
                            int32_t* n_out, void* stream) {
    return score_topk_impl(c, q, corpus, dtype, nq, N, d, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr);
}

// The same over a corpus of e4m3fn codes + one power-of-two scale per document (include/sgpt_hip.h).
sgpt_status sgpt_score_topk_q8(sgpt_ctx* c, const void* q, const uint8_t* codes, const float* scale, int32_t nq, int64_t N, int32_t d,
                               int32_t k, int64_t idx_base, float* run_val, int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream) {
    if (!c || !q || !codes || !scale || !run_val || !run_idx || nq <= 0 || N <= 0 || d <= 0 || d % 8 || k <= 0 || n_run < 0 || n_run > k ||
        ((size_t)q & 15) || ((size_t)codes & 3))
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk_q8: bad arguments (d % 8 == 0, 0 <= n_run <= k, q 16-byte aligned)");
    // short query batches on a served width: the streaming tile reads the codes themselves
    if (nq <= 64 && score64q8_shape_ok(64, 256, d, codes, d))
        return score_topk_impl(c, q, codes, SGPT_F16, nq, N, d, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr, scale);
    // everything else (MFMA-bound, or a width the tile does not serve): blocks of at most 131 072 documents de-quantised to f16 rows
    // and scored by the f16 path, the running list chained from block to block -- the corpus stays one byte per element in memory
    const int64_t blk = 131072;
    HIPC(c, hipSetDevice(c->device));
    sgpt_status st = ensure(c, &c->ws6, &c->ws6_bytes, (size_t)(N < blk ? N : blk) * d * 2);
    if (st != SGPT_OK) return st;
    int32_t have = n_run;
    for (int64_t b0 = 0; b0 < N; b0 += blk) {
        const int64_t nb = N - b0 < blk ? N - b0 : blk;
        launch_fp8_dequant_rows(codes + (size_t)b0 * d, scale + b0, nb, d, c->ws6, SGPT_F16, (hipStream_t)stream);
        st = score_topk_impl(c, q, c->ws6, SGPT_F16, nq, nb, d, k, idx_base + b0, run_val, run_idx, run_val, run_idx, have, &have, stream, nullptr);
        if (st != SGPT_OK) return st;
    }
    if (n_out) *n_out = have;
    return SGPT_OK;
}

// Hamming search over packed sign bits with optional re-scoring of the over-fetched candidates (include/sgpt_hip.h).
sgpt_status sgpt_score_topk_bits(sgpt_ctx* c, const float* q, const uint8_t* bits, int64_t ldb, int32_t nq, int64_t N, int32_t d, int32_t k,
                                 int32_t kp, int32_t mode, const uint8_t* codes, const float* scale, int64_t idx_base, float* run_val,
                                 int64_t* run_idx, int32_t n_run, int32_t* n_out, void* stream) {
    if (!c || !q || !bits || !run_val || !run_idx || nq <= 0 || N <= 0 || d <= 0 || ldb % 4 || ldb < 4 * (((int64_t)d + 31) / 32) ||
        k <= 0 || kp < k || kp > 1024 || mode < 0 || mode > 2 || (mode == 0 && kp != k) || (mode == 2 && (!codes || !scale)) ||
        n_run < 0 || n_run > k || ((size_t)bits & 3))
        return fail(c, SGPT_ERR_INVALID, "sgpt_score_topk_bits: bad arguments (ldb % 4 == 0, ldb >= 4 ceil(d / 32), 0 < k <= kp <= 1024, "
                                         "mode 0 with kp == k, mode 2 with codes and scale, 0 <= n_run <= k)");
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int qw = (d + 127) / 128 * 4;                 // dwords of a packed query row: whole 16-byte pieces
    const int ldc = kp + k;
    const size_t qb_b = align_up((size_t)nq * qw * 4, 256), lv_b = align_up((size_t)nq * kp * 4, 256), li_b = align_up((size_t)nq * kp * 8, 256);
    const size_t cv_b = align_up((size_t)nq * ldc * 4, 256), ci_b = align_up((size_t)nq * ldc * 8, 256);
    sgpt_status st = ensure(c, &c->ws4, &c->ws4_bytes, qb_b + lv_b + li_b + cv_b + ci_b);
    if (st != SGPT_OK) return st;
    char* b = (char*)c->ws4;
    uint32_t* qbits = (uint32_t*)b; b += qb_b;
    float* lv = (float*)b; b += lv_b;
    int64_t* li = (int64_t*)b; b += li_b;
    float* cv = (float*)b; b += cv_b;
    int64_t* ci = (int64_t*)b; b += ci_b;
    launch_pack_sign_bits(q, nq, d, nullptr, (uint8_t*)qbits, (long)qw * 4, s);
    // stage 1: the kp best by agreement (a descending, index ascending), a fresh list per call.  Queries in groups of 64 (re-streaming
    // 96-byte rows is cheap), documents in blocks the launches index with 32 bits, chained through the stage-1 list.
    const BitRows br{(long)ldb, qw};
    const int64_t blk = (int64_t)1 << 30;
    for (int32_t g0 = 0; g0 < nq; g0 += 64) {
        const int32_t gn = nq - g0 < 64 ? nq - g0 : 64;
        float* gv = lv + (size_t)g0 * kp;
        int64_t* gi = li + (size_t)g0 * kp;
        int32_t have = 0;
        for (int64_t b0 = 0; b0 < N; b0 += blk) {
            const int64_t nb = N - b0 < blk ? N - b0 : blk;
            st = score_topk_impl(c, qbits + (size_t)g0 * qw, bits + (size_t)b0 * ldb, SGPT_F16, gn, nb, d, kp, idx_base + b0, gv, gi, gv, gi,
                                 have, &have, stream, nullptr, nullptr, &br);
            if (st != SGPT_OK) return st;
        }
    }
    // stage 2: the candidates' values by `mode` | the running list -> top-k (as sgpt_score_topk_refined)
    launch_rescore_bits(mode, q, bits, (long)ldb, codes, ((long)d + 7) / 8 * 8, scale, lv, li, kp, nq, kp, d, idx_base, N, cv, ci, ldc, s);
    launch_list_append(run_val, run_idx, k, n_run, nq, cv, ci, ldc, kp, s);
    launch_topk_select(cv, ldc, 0, 0, cv, ci, kp + n_run, ldc, nq, k, 0, nullptr, run_val, run_idx, s);
    if (n_out) { const int64_t tot = (int64_t)n_run + N; *n_out = (int32_t)(tot < k ? tot : k); }
    HIPC(c, hipGetLastError());
    return SGPT_OK;
}

sgpt_status sgpt_pack_sign_bits(sgpt_ctx* c, const float* x, int64_t n, int32_t d, const float* center, uint8_t* bits, int64_t ldb,
                                void* stream) {
    if (!c || !x || !bits || n <= 0 || d <= 0 || ldb % 4 || ldb < 4 * (((int64_t)d + 31) / 32))
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
    // head-room: as many extra candidates as the sampled schedule allows (k' <= 64), at least 8; deep lists (k > 56) take k / 8
    int kp = k <= 56 ? 64 : k + (k / 8 > 8 ? k / 8 : 8);
    if (kp > 1024 && k <= 1024) kp = 1024;
    if ((int64_t)kp > N) kp = (int)N;
    if (kp <= k || kp > 1024) {       // nothing to filter with (k >= N) or lists beyond the filtered scorer: the exact pass itself
        if (fallback_flag_out) *fallback_flag_out = -1;
        return score_topk_impl(c, q, corpus32, SGPT_F32, nq, N, d, k, idx_base, run_val, run_idx, run_val, run_idx, n_run, n_out, stream, nullptr);
    }
    const int ldc = kp + k;
    const size_t q16_b = align_up((size_t)nq * d * 2, 256), lv_b = align_up((size_t)nq * kp * 4, 256), li_b = align_up((size_t)nq * kp * 8, 256);
    const size_t cv_b = align_up((size_t)nq * ldc * 4, 256), ci_b = align_up((size_t)nq * ldc * 8, 256);
    const size_t sv_b = align_up((size_t)nq * k * 4, 256), si_b = align_up((size_t)nq * k * 8, 256);
    sgpt_status st = ensure(c, &c->ws4, &c->ws4_bytes, q16_b + lv_b + li_b + cv_b + ci_b + sv_b + si_b + 256);
    if (st != SGPT_OK) return st;
    char* b = (char*)c->ws4;
    void* q16 = b; b += q16_b;
    float* lv = (float*)b; b += lv_b;
    int64_t* li = (int64_t*)b; b += li_b;
    float* cv = (float*)b; b += cv_b;
    int64_t* ci = (int64_t*)b; b += ci_b;
    float* sv = (float*)b; b += sv_b;
    int64_t* si = (int64_t*)b; b += si_b;
    int* flag = (int*)b;
    HIPC(c, hipMemsetAsync(flag, 0, 4, s));
    launch_f32_to_16(q, (int64_t)nq * d, q16, dtype16, s);
    // stage 1: the k' best by 16-bit score (fresh list)
    int32_t n1 = 0;
    st = score_topk_impl(c, q16, corpus16, dtype16, nq, N, d, kp, idx_base, lv, li, lv, li, 0, &n1, stream, nullptr);
    if (st != SGPT_OK) return st;
    launch_refine_check(lv, k, kp, margin, nq, flag, s);
    // stage 2: exact fp32 scores of the candidates | the running list -> top-k
    if (n_run > 0) {      // (kept for the fallback: it starts from the list as it was before this chunk)
        HIPC(c, hipMemcpy2DAsync(sv, (size_t)k * 4, run_val, (size_t)k * 4, (size_t)n_run * 4, nq, hipMemcpyDeviceToDevice, s));
        HIPC(c, hipMemcpy2DAsync(si, (size_t)k * 8, run_idx, (size_t)k * 8, (size_t)n_run * 8, nq, hipMemcpyDeviceToDevice, s));
    }
    launch_rescore(q, corpus32, li, kp, nq, kp, d, idx_base, N, cv, ci, ldc, s);
    launch_list_append(run_val, run_idx, k, n_run, nq, cv, ci, ldc, kp, s);
    launch_topk_select(cv, ldc, 0, 0, cv, ci, kp + n_run, ldc, nq, k, 0, nullptr, run_val, run_idx, s);
    // the predicated exact pass (no-op launches unless a query failed the check)
    st = score_topk_impl(c, q, corpus32, SGPT_F32, nq, N, d, k, idx_base, sv, si, run_val, run_idx, n_run, nullptr, stream, flag);
    if (st != SGPT_OK) return st;
    if (fallback_flag_out) {     // optional, host-synchronising: did the exact pass run? (tests / diagnostics; pass NULL to stay asynchronous)
        HIPC(c, hipMemcpyAsync(fallback_flag_out, flag, 4, hipMemcpyDeviceToHost, s));
        HIPC(c, hipStreamSynchronize(s));
    }
    if (n_out) { const int64_t tot = (int64_t)n_run + N; *n_out = (int32_t)(tot < k ? tot : k); }
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
