// Prints the score + top-k plans (sgpt_amd/csrc/score_plan.h) as JSON lines: `--grid` walks the whole grid of tests/test_score_plan.py,
// otherwise shapes are read from stdin as "nq N d k kind predicated n_run" lines.  Includes nothing of the library but the planner.
#include <cstdio>
#include <cstring>

#include "../sgpt_amd/csrc/score_plan.h"

static const char* const KINDS[] = {"f32", "16", "fp8", "bits"};

static void reg(const char* name, const ScorePlan::Region& r, const char* end) { printf("\"%s\":[%zu,%zu]%s", name, r.off, r.bytes, end); }

static void one(int nq, long N, int d, int k, int kind, int predicated, int n_run) {
    // the switches at their defaults (score.hip: the product build)
    const ScorePlanIn in{nq, N, d, k, n_run, (ScoreCorpusKind)kind, predicated != 0, {false, false, false, 1.0, true, true, true, 512}};
    ScorePlan p;
    plan_score_topk(in, p);
    printf("{\"nq\":%d,\"N\":%ld,\"d\":%d,\"k\":%d,\"kind\":\"%s\",\"pred\":%d,\"n_run\":%d,", nq, N, d, k, KINDS[kind], predicated, n_run);
    printf("\"chunk\":%ld,\"unit\":%ld,\"fast\":%d,\"nq_pad\":%d,\"filt\":%d,\"sampled\":%d,\"cap\":%d,\"ratio\":\"%.17g\",\"S\":%ld,\"s_stride\":%ld,"
           "\"fchunk\":%ld,\"n_flags\":%ld,\"fresh_list\":%d,", p.chunk, p.unit, (int)p.fast, p.nq_pad, (int)p.filt, (int)p.sampled, p.cap, p.ratio, p.S,
           p.s_stride, p.fchunk, p.n_flags, (int)p.fresh_list);
    printf("\"top2\":%d,\"first\":%ld,\"chunks\":[", (int)p.sample_top2, p.first);
    for (size_t i = 0; i < p.chunks.size(); ++i) {
        const ScoreChunk& c = p.chunks[i];
        printf("%s[%ld,%ld,%d,%ld,%d]", i ? "," : "", c.doc0, c.len, (int)c.fold_tail, c.n_valid, (int)c.tail_launch);
    }
    printf("],\"rest\":%ld,\"ws\":{", p.rest);
    reg("sc", p.sc, ","); reg("tv0", p.tv[0], ","); reg("tv1", p.tv[1], ","); reg("ti0", p.ti[0], ","); reg("ti1", p.ti[1], ",");
    reg("sav_v", p.sav_v, ","); reg("sav_i", p.sav_i, ","); reg("qpad", p.qpad, ","); reg("cand_v", p.cand_v, ","); reg("cand_i", p.cand_i, ",");
    reg("cand_cnt", p.cand_cnt, ","); reg("th_v", p.th_v, ","); reg("th_i", p.th_i, ","); reg("thr", p.thr, "},");
    printf("\"total\":%zu}\n", p.total);
}

int main(int argc, char** argv) {
    static const int nqs[] = {1, 16, 64, 65, 200, 1000, 2048, 10000};
    static const long Ns[] = {255, 256, 5000, 65536, 70000, 100003, 200037, 262144, 262216, 300005, 1000000, 1000072, 16000000, 1L << 30};
    static const int ds[] = {64, 128, 192, 768};
    static const int ks[] = {1, 10, 11, 33, 64, 65, 100, 300, 1001, 1024, 1025};
    if (argc > 1 && !strcmp(argv[1], "--grid")) {
        for (int nq : nqs) for (long N : Ns) for (int d : ds) for (int k : ks) for (int kind = 0; kind < 4; ++kind) {
            // what the entry points refuse: an fp8 corpus on the streaming tile is nq <= 64 at d % 128 == 0, a binary one nq <= 64, k <= 1024
            if (kind == SCORE_CORPUS_FP8 && (nq > 64 || d % 128)) continue;
            if (kind == SCORE_CORPUS_BITS && (nq > 64 || k > 1024)) continue;
            for (int pred = 0; pred < 2; ++pred) for (int r = 0; r < 2; ++r) one(nq, N, d, k, kind, pred, r ? k : 0);
        }
        return 0;
    }
    int nq, d, k, pred, n_run; long N; char kind[16];
    while (scanf("%d %ld %d %d %15s %d %d", &nq, &N, &d, &k, kind, &pred, &n_run) == 7) {
        int ki = -1;
        for (int i = 0; i < 4; ++i) if (!strcmp(kind, KINDS[i])) ki = i;
        if (ki < 0 || nq <= 0 || N <= 0 || d <= 0 || k <= 0 || n_run < 0 || n_run > k) { fprintf(stderr, "bad shape line\n"); return 2; }
        one(nq, N, d, k, ki, pred, n_run);
    }
    return 0;
}
