// The schedule of a score + top-k pass (score.hip) as a pure function of its shape: chunk sizes, list capacity, the threshold sample,
// the filtered chunks with their fold / tail decisions and the ws2 layout.  Plain C++17 -- no HIP, no device state -- so a host
// compiler builds it alone (tests/score_plan_dump.cpp, tests/test_score_plan.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

// what the corpus rows are: fp32 | bf16 / f16 | e4m3fn codes + one scale per document (sgpt_score_topk_q8, queries f16) | packed sign
// bits (sgpt_score_topk_bits, at most 64 packed query rows) | uint8 codes with one range per dimension (sgpt_score_topk_u8, at most 64
// fp32 query rows, d = the padded row width ld): planned like fp8, with the any-N launches and tail folding of the binary corpus
enum ScoreCorpusKind { SCORE_CORPUS_F32, SCORE_CORPUS_16, SCORE_CORPUS_FP8, SCORE_CORPUS_BITS, SCORE_CORPUS_U8 };

// A/B switches of the schedule, filled once by score.hip: the exp_env() results (experiment build only) and the build-time macros
struct ScoreSwitches {
    bool no64, classic, gemm128;            // SGPT_SCORE_NO64, SGPT_SCORE_CLASSIC, SGPT_GEMM128
    double sample_mult;                     // SGPT_SAMPLE_MULT
    bool fold_tail, fold_tail_score, sample_top2;   // SGPT_FOLD_TAIL, SGPT_FOLD_TAIL_SCORE, SGPT_SAMPLE_TOP2
    int cap_short;                          // SGPT_CAP_SHORT
};

struct ScorePlanIn {
    int nq; long N; int d, k, n_run;
    ScoreCorpusKind kind;
    bool predicated;                        // every launch predicated on one device flag: the materialise-and-select path
    ScoreSwitches sw;
};

// one filtered launch over documents [doc0, doc0 + len) (+ the < 256 trailing documents of the shard: fold_tail, in the same launch with
// n_valid = len + tail documents that exist; tail_launch, in a small-tile launch of their own), then one merge
struct ScoreChunk { long doc0, len; bool fold_tail; long n_valid; bool tail_launch; };

struct ScorePlan {
    long chunk, unit, fchunk, S, s_stride, n_flags;
    int nq_pad, cap;
    double ratio;
    bool fast, filt, sampled;
    bool pad_queries;       // the query rows are copied into a zero-padded tile of nq_pad rows (else read where they are)
    bool any_n;             // every corpus launch takes any number of documents: none is split for a ragged tail, and a folded one
                            // counts the documents that exist (else whole tiles + 256, masked by GemmArgs.n_valid)
    bool fold_score;        // materialise-and-select pieces may fold their tail (tile_folds)
    bool fresh_list;        // the prologue marks the running list empty
    bool sample_top2;       // the sample runs as EPI_SCORE_TOP2
    long first;             // k > 64: documents of the materialised first chunk
    long rest;              // documents [N - rest, N) left for a trailing materialise-and-select (!filt: all of them)
    std::vector<ScoreChunk> chunks;   // the filtered chunks in order
    // ws2: byte offsets of the regions (a region of 0 bytes is not there), in this order
    struct Region { size_t off, bytes; };
    Region sc, tv[2], ti[2], sav_v, sav_i, qpad, cand_v, cand_i, cand_cnt, th_v, th_i, thr;
    Region qscale, qbias;   // uint8 corpus: the two fp32 values per padded query row of the scorer's fma (0 bytes for every other kind)
    size_t total;

    // May the < 256 trailing documents of a materialised tile ride in its 256x256 launch (na whole-tile documents of nc, score rows of ld)?
    bool tile_folds(long na, long nc, long ld, long row_stride, int d) const;
};

static inline size_t score_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The shape arithmetic of THE predicate of the folded ragged tail (gemm.hip: gemm_score_tail_foldable adds the SGPT_GEMM128 switch): a
// scorer launch of M padded query rows against N = (whole 256-document tiles + 256) documents of width K takes the 256x256 kernel with
// the documents as its streamed operand -- the only kernel that honours GemmArgs.n_valid.
static inline bool score_tail_foldable_shape(int M, long N, int K) {
    return M >= 256 && M != 64 && M % 256 == 0 && N % 256 == 0 && N >= 512 && K % 64 == 0 && K >= 128 && (long)M < N;
}

inline bool ScorePlan::tile_folds(long na, long nc, long ld, long row_stride, int d) const {
    return fold_score && na > 0 && na < nc && row_stride == 1 && na + 256 <= ld && score_tail_foldable_shape(nq_pad, na + 256, d);
}

static inline void plan_score_topk(const ScorePlanIn& in, ScorePlan& p) {
    const int nq = in.nq, d = in.d, k = in.k;
    const long N = in.N;
    const bool bits = in.kind == SCORE_CORPUS_BITS, u8 = in.kind == SCORE_CORPUS_U8;
    const bool any_n = bits || u8;                    // the corpus launches take any number of documents
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
    if (chunk > N) chunk = (long)score_align_up((size_t)N, 4);
    // bf16 fast path: the 256x256 LDS-DMA GEMM needs the query rows padded to a multiple of 256 (zero rows,
    // never stored) and d % 64 == 0; chunks that are multiples of 256 documents take it, the ragged tail and
    // fp32 go through the 128^2 kernel.
    const bool fast = bits || (in.kind != SCORE_CORPUS_F32 && d % 64 == 0 && d >= 128);
    // nq <= 64: the 64-query-row scorer tile (score64_kernel) instead of 256 padded rows -- the pass is HBM-bound there
    const int nq_pad = (fast && nq <= 64 && !in.sw.no64) ? 64 : (nq + 255) / 256 * 256;
    // Threshold-filtered chunks (after the first): see EPI_SCORE_FILTER.  Candidate capacity per query and chunk;
    // the doubling schedule below keeps the expected count at ~k.
    // Capacity and growth: a filtered chunk of as many documents as were seen before it expects ~k survivors per query
    // (the threshold is the k-th best of `seen` documents); the merge sorts the candidates in 2048 LDS slots.
    // k <= 64 ("sampled" schedule, round 4): the first thresholds come from a STRIDED SAMPLE of the whole shard instead of its
    // first documents, so (a) nothing is materialised but the sample's own score tile, (b) the expected number of survivors of
    // a chunk, k * len / S, holds whatever the document order does to the score distribution (the reference sorts the corpus
    // by length: a drift along the index used to overflow the lists and pay the materialised recomputation of the chunk), and
    // (c) chunks can therefore be as long as the lists allow instead of doubling: a 125 k-document shard is ONE filtered
    // launch, 1 M documents two (1 + 6 before; tests/golden/score_plans.json).  The rank of a sample's k-th best in the population
    // is Gamma(k)-distributed (relative spread 1 / sqrt(k)): lists of `cap` entries take R = cap / (k (1 + 6 / sqrt(k))) times the
    // documents the thresholds were drawn from with ~6 sigma of head-room.
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
    const int cap_n = nq <= 64 ? (N >= 400000 ? 1024 : 512) : (N >= 800000 ? 2048 : (N >= 400000 ? 1024 : in.sw.cap_short));
    const int cap_s = cap_n * (k <= 32 ? 1 : 2) > 2048 ? 2048 : cap_n * (k <= 32 ? 1 : 2);
    const int cap = sampled_k ? cap_s : ((4 * k < 2048 - k) ? 4 * k : 2048 - k);
    const bool half_growth = 2 * cap < 5 * k;          // k > ~340: cap < 2.5 k -> grow by half, expect ~k/2 per chunk
    // k > 64 keeps the first-chunk + doubling schedule.  Two other schedules were measured against doubling and rejected:
    //   round 2: 4x growth with 256-entry lists -- overflowed on corpora whose score distribution drifts along the index and
    //            paid the materialised recomputation;
    //   round 3: 2048-entry lists with growth cap / 6k (k = 11: first chunk + two filtered chunks per 1 M documents) -- ~330
    //            survivors per query and chunk through the epilogue's append path: the filtered GEMM went from 1.45 to 1.58 ms
    //            per pass (nq = 1000), and a drift at 10 % of the corpus from 2.2 to 3.5 ms (profiles/r03_score_schedule.txt).
    const bool filt = fast && !in.sw.classic && k <= 1024 && chunk % 256 == 0 && N >= 2 * chunk && !in.predicated;
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
        S = ((long)((double)N / ratio * in.sw.sample_mult) + 255) / 256 * 256;     // rounded UP: ratio * S covers the shard
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
    if (fchunk > (long)score_align_up((size_t)N, 256)) fchunk = (long)score_align_up((size_t)N, 256);
    if (fchunk < chunk) fchunk = chunk;
    const long n_flags = 64 + N / (1L << 19) + 1;      // one overflow flag per filtered chunk
    const size_t sc_bytes = score_align_up((size_t)nq * (fchunk > S ? fchunk : S) * 4, 256);
    const size_t tv_bytes = score_align_up((size_t)nq * k * 4, 256), ti_bytes = score_align_up((size_t)nq * k * 8, 256);
    const size_t qp_bytes = fast && !bits ? score_align_up((size_t)nq_pad * d * 2, 256) : 0;     // (packed query rows are read where they are)
    const size_t cv_bytes = filt ? score_align_up((size_t)nq * cap * 4, 256) : 0, ci_bytes = filt ? score_align_up((size_t)nq * cap * 8, 256) : 0;
    const size_t cc_bytes = filt ? score_align_up((size_t)(nq_pad + n_flags) * 4, 256) : 0;  // counters + per-chunk overflow flags
    const size_t td_bytes = score_align_up((size_t)nq * 4, 256);
    const size_t th_bytes = sampled ? tv_bytes + ti_bytes + td_bytes : 0;   // sample's list + dense thresholds
    const size_t qs_bytes = u8 ? score_align_up((size_t)nq_pad * 4, 256) : 0;
    p.total = sc_bytes + 3 * (tv_bytes + ti_bytes) + qp_bytes + cv_bytes + ci_bytes + cc_bytes + th_bytes + 2 * qs_bytes;
    size_t off = 0;
    auto take = [&](size_t bytes) { ScorePlan::Region r{off, bytes}; off += bytes; return r; };
    p.sc = take(sc_bytes);
    p.tv[0] = take(tv_bytes); p.tv[1] = take(tv_bytes);
    p.ti[0] = take(ti_bytes); p.ti[1] = take(ti_bytes);
    p.sav_v = take(tv_bytes); p.sav_i = take(ti_bytes);   // third list: ping-pong partner of a recomputation
    p.qpad = take(qp_bytes);
    p.cand_v = take(cv_bytes); p.cand_i = take(ci_bytes); p.cand_cnt = take(cc_bytes);
    p.th_v = take(sampled ? tv_bytes : 0); p.th_i = take(sampled ? ti_bytes : 0); p.thr = take(sampled ? td_bytes : 0);
    p.qscale = take(qs_bytes); p.qbias = take(qs_bytes);

    p.chunk = chunk; p.unit = unit; p.fchunk = fchunk; p.S = S; p.s_stride = s_stride; p.n_flags = n_flags;
    p.nq_pad = nq_pad; p.cap = cap; p.ratio = ratio;
    p.fast = fast; p.filt = filt; p.sampled = sampled;
    p.pad_queries = fast && !bits;
    p.any_n = any_n;
    p.fold_score = in.sw.fold_tail && in.sw.fold_tail_score && !in.sw.gemm128;
    p.fresh_list = sampled && in.n_run == 0;
    p.sample_top2 = sampled && in.sw.sample_top2 && nq_pad >= 256 && S % 256 == 0;
    p.first = 0; p.chunks.clear();
    long seen = 0;                 // documents behind which the filtered chunks continue
    if (filt) {
        long eff = 0;              // documents the current thresholds are the k-th best of
        const long n256 = n256_all;
        if (sampled) eff = S;
        else {
            // first chunk: materialise + select -> the initial thresholds.  One whole wave of tiles is enough (the
            // doubling schedule takes over from there): 16 384 documents for nq = 1000 instead of 32 768
            p.first = unit < chunk ? unit : chunk;
            seen = p.first; eff = p.first;
        }
        // k > 64, doubling schedule: a filtered chunk is as long as everything seen before it, so a query expects ~k
        // survivors per chunk (k * len / seen) whatever N is; 1 M documents = 1 + 5 launches instead of 31.
        // k <= 64, sampled schedule: `ratio` times the documents the thresholds stand for (see above).
        while (n256 - seen >= 256) {
            long len;
            if (sampled) len = (long)((double)eff * ratio) / 256 * 256;
            else len = half_growth ? (eff / 2 / 256 * 256 > 256 ? eff / 2 / 256 * 256 : 256) : eff;
            if (len < 256) len = 256;
            // chunks of at most 2^19 documents: a merge half-way through a 1 M-document pass tightens the thresholds of the
            // second half (nq = 1000: 380 + 10 appended candidates per query instead of 730; measured 1.62-1.64 against
            // 1.65-1.69 ms, nq = 128 0.51 against 0.54).  Short query batches (the HBM-bound 64-row tile) take the whole shard
            // in ONE launch instead: a merge, three no-op fallback launches and a pipeline ramp less (nq = 16: 0.36 -> 0.35 ms)
            if (len > (1L << 19) && !(sampled && nq <= 64)) len = 1L << 19;
            if (len >= n256 - seen) len = n256 - seen;          // the last chunk takes what is left (no whole-wave rounding: that
            else if (len >= unit) len = len / unit * unit;      //  left a 17 k-document sixth launch behind 1 M documents at nq = 16)
            // the < 256 trailing documents ride in the last chunk's launch (the 256x256 kernel clamps their rows and masks their
            // columns, GemmArgs.n_valid) when documents are its streamed operand; the 64-row tile keeps its own tail launch
            const bool fold_tail = seen + len == n256 && N > n256 &&
                                   (any_n || (in.sw.fold_tail && !in.sw.gemm128 && score_tail_foldable_shape(nq_pad, len + 256, d)));
            ScoreChunk c{seen, len, fold_tail, fold_tail ? len + (N - n256) : 0, false};
            seen += len;
            if (fold_tail) seen = N;
            eff = seen;                                         // the thresholds now stand for every document of [0, seen)
            // ragged tail (< 256 documents): filtered against the same thresholds by the small-tile kernel, its
            // survivors join this chunk's candidate lists -- one merge, no materialise + select round for 72 documents
            c.tail_launch = seen == n256 && seen < N;
            if (c.tail_launch) seen = N;
            p.chunks.push_back(c);
        }
    }
    p.rest = N - seen;   // (filt: only when no filtered chunk ran, N - first < 256)
}
