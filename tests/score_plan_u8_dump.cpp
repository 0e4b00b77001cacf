// Prints the score + top-k plans (sgpt_amd/csrc/score_plan.h) of the uint8 corpus as JSON lines over the grid of
// tests/test_score_plan_u8.py, and -- behind them, with "u8":0 -- the same shapes for the other corpus kinds (their qscale / qbias regions
// must be empty).  Includes nothing of the library but the planner.
#include <cstdio>

#include "../sgpt_amd/csrc/score_plan.h"

static void reg(const char* name, const ScorePlan::Region& r, const char* end) { printf("\"%s\":[%zu,%zu]%s", name, r.off, r.bytes, end); }

static void one(int nq, long N, int d, int k, int kind, int n_run) {
    // the switches at their defaults (score.hip: the product build)
    const ScorePlanIn in{nq, N, d, k, n_run, (ScoreCorpusKind)kind, false, {false, false, false, 1.0, true, true, true, 512}};
    ScorePlan p;
    plan_score_topk(in, p);
    printf("{\"u8\":%d,\"kind\":%d,\"nq\":%d,\"N\":%ld,\"d\":%d,\"k\":%d,\"n_run\":%d,", (int)(kind == SCORE_CORPUS_U8), kind, nq, N, d, k, n_run);
    printf("\"chunk\":%ld,\"fast\":%d,\"nq_pad\":%d,\"filt\":%d,\"sampled\":%d,\"cap\":%d,\"S\":%ld,\"s_stride\":%ld,\"fchunk\":%ld,\"n_flags\":%ld,"
           "\"fresh_list\":%d,\"any_n\":%d,\"pad_queries\":%d,\"top2\":%d,\"first\":%ld,\"chunks\":[",
           p.chunk, (int)p.fast, p.nq_pad, (int)p.filt, (int)p.sampled, p.cap, p.S, p.s_stride, p.fchunk, p.n_flags, (int)p.fresh_list, (int)p.any_n,
           (int)p.pad_queries, (int)p.sample_top2, p.first);
    for (size_t i = 0; i < p.chunks.size(); ++i) {
        const ScoreChunk& c = p.chunks[i];
        printf("%s[%ld,%ld,%d,%ld,%d]", i ? "," : "", c.doc0, c.len, (int)c.fold_tail, c.n_valid, (int)c.tail_launch);
    }
    printf("],\"rest\":%ld,\"ws\":{", p.rest);
    reg("sc", p.sc, ","); reg("tv0", p.tv[0], ","); reg("tv1", p.tv[1], ","); reg("ti0", p.ti[0], ","); reg("ti1", p.ti[1], ",");
    reg("sav_v", p.sav_v, ","); reg("sav_i", p.sav_i, ","); reg("qpad", p.qpad, ","); reg("cand_v", p.cand_v, ","); reg("cand_i", p.cand_i, ",");
    reg("cand_cnt", p.cand_cnt, ","); reg("th_v", p.th_v, ","); reg("th_i", p.th_i, ","); reg("thr", p.thr, ",");
    reg("qscale", p.qscale, ","); reg("qbias", p.qbias, "},");
    printf("\"total\":%zu}\n", p.total);
}

int main() {
    static const int nqs[] = {1, 16, 64};
    static const long Ns[] = {1, 255, 256, 257, 1000, 262221, 1000000};
    static const int ds[] = {128, 768};
    static const int ks[] = {1, 11, 100, 1001};
    for (int kind = SCORE_CORPUS_U8; kind >= 0; --kind)
        for (int nq : nqs) for (long N : Ns) for (int d : ds) for (int k : ks) for (int r = 0; r < 2; ++r) {
            if (kind == SCORE_CORPUS_BITS && k > 1024) continue;      // (refused by its entry point)
            one(nq, N, d, k, kind, r ? k : 0);
        }
    return 0;
}
