// C ABI (include/sgpt_hip.h): the context, its workspaces, profiling and per-ctx policies; the shared launch helpers of host.h.
// Host-side C++ only -- every device op is one of the hand-written kernels in this directory.
#include "host.h"

namespace sgpt_host {

sgpt_status ensure(sgpt_ctx* c, void** p, size_t* have, size_t need) {
    if (*have >= need) return SGPT_OK;
    if (*p) { HIPC(c, hipDeviceSynchronize()); HIPC(c, hipFree(*p)); *p = nullptr; *have = 0; }
    need = align_up(need + (need >> 3), 1 << 20);
    if (hipMalloc(p, need) != hipSuccess) { *p = nullptr; return fail(c, SGPT_ERR_OOM, "hipMalloc workspace failed"); }
    HIPC(c, hipMemset(*p, 0, need));
    *have = need;
    c->generation++;
    return SGPT_OK;
}

void gemm(sgpt_ctx* c, int dtype, int epi, int out_dtype, const GemmArgs& a0, hipStream_t s) {
    Prof p(c, s, 2.0 * (double)a0.m_valid * a0.N * (a0.k_algo > 0 ? a0.k_algo : a0.K));   // algorithmic FLOPs (split blocks not counted)
    GemmArgs a = a0;
    a.kgroups = c->kgroups; a.force256 = c->force256; a.cu_cap = c->cu_cap;     // per-ctx policies (no process-global state)
    launch_gemm(dtype, epi, out_dtype, a, s);
}

// query-sized projection (qgemm.hip); false = not served, the caller launches gemm()
bool qgemm(sgpt_ctx* c, int dtype, int epi, int out_dtype, const QGemmArgs& a, hipStream_t s) {
    Prof p(c, s, 2.0 * (double)a.g.m_valid * a.g.N * a.g.K);
    return launch_qgemm(dtype, epi, out_dtype, a, s);
}

}  // namespace sgpt_host

extern "C" {

int sgpt_abi_version(void) { return SGPT_ABI_VERSION; }

sgpt_status sgpt_ctx_create(int hip_device, sgpt_ctx** out) {
    if (!out) return SGPT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || hip_device < 0 || hip_device >= n) return SGPT_ERR_HIP;
    if (hipSetDevice(hip_device) != hipSuccess) return SGPT_ERR_HIP;
    sgpt_ctx* c = new sgpt_ctx();
    c->device = hip_device;
    if (hipMalloc((void**)&c->range_flag, 256) != hipSuccess || hipMemset(c->range_flag, 0, 256) != hipSuccess) {
        delete c;
        return SGPT_ERR_OOM;
    }
    *out = c;
    return SGPT_OK;
}

void sgpt_ctx_destroy(sgpt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->ws) (void)hipFree(c->ws);
    if (c->ws2) (void)hipFree(c->ws2);
    (void)sgpt_comm_destroy(c);
    if (c->ws3) (void)hipFree(c->ws3);
    if (c->ws4) (void)hipFree(c->ws4);
    if (c->ws5) (void)hipFree(c->ws5);
    if (c->ws6) (void)hipFree(c->ws6);
    if (c->ws7) (void)hipFree(c->ws7);
    if (c->range_flag) (void)hipFree(c->range_flag);
    for (auto& e : c->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (hipEvent_t e : c->chain_ev) if (e) (void)hipEventDestroy(e);
    if (c->chain_stream) (void)hipStreamDestroy(c->chain_stream);
    delete c;
}

const char* sgpt_last_error(const sgpt_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

uint64_t sgpt_ctx_generation(const sgpt_ctx* c) { return c ? c->generation : 0; }

sgpt_status sgpt_ctx_reserve(sgpt_ctx* c, size_t encode_bytes, size_t score_bytes) {
    if (!c) return SGPT_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    sgpt_status st = ensure(c, &c->ws, &c->ws_bytes, encode_bytes);
    if (st != SGPT_OK) return st;
    return ensure(c, &c->ws2, &c->ws2_bytes, score_bytes);
}

sgpt_status sgpt_range_check(sgpt_ctx* c, int32_t* flagged, int32_t reset, void* stream) {
    if (!c || !flagged) return SGPT_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int h = 0;
    HIPC(c, hipMemcpyAsync(&h, c->range_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(c, hipStreamSynchronize(s));
    if (reset && h) HIPC(c, hipMemsetAsync(c->range_flag, 0, sizeof(int), s));
    *flagged = h;
    return SGPT_OK;
}

sgpt_status sgpt_prof_enable(sgpt_ctx* c, int32_t on) {
    if (!c) return SGPT_ERR_INVALID;
    c->prof = on != 0;
    return SGPT_OK;
}

sgpt_status sgpt_prof_read(sgpt_ctx* c, int64_t* launches, double* ms, double* flops, int32_t reset) {
    if (!c) return SGPT_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipDeviceSynchronize());
    for (size_t i = 0; i < c->ev_used; ++i) {
        float t = 0;
        HIPC(c, hipEventElapsedTime(&t, c->ev_pool[i].first, c->ev_pool[i].second));
        c->prof_ms += t;
        c->prof_flops += c->ev_flops[i];
        c->prof_launches++;
    }
    c->ev_used = 0;
    if (launches) *launches = c->prof_launches;
    if (ms) *ms = c->prof_ms;
    if (flops) *flops = c->prof_flops;
    if (reset) { c->prof_launches = 0; c->prof_ms = 0; c->prof_flops = 0; }
    return SGPT_OK;
}

int32_t sgpt_ctx_set_low_latency(sgpt_ctx* c, int32_t on) {
    if (!c) return 0;
    const int old = c->kgroups > 1 ? 1 : 0;
    c->kgroups = on ? 2 : 1;
    return old;
}
int32_t sgpt_ctx_set_gemm_cu_cap(sgpt_ctx* c, int32_t n) {
    if (!c) return 0;
    const int old = c->cu_cap;
    c->cu_cap = n > 0 ? n : 0;
    return old;
}
int32_t sgpt_ctx_set_tile_policy(sgpt_ctx* c, int32_t policy) {
    if (!c) return 0;
    const int old = c->force256 ? 1 : c->no_qpath ? 2 : 0;
    c->force256 = policy == 1 ? 1 : 0;
    c->no_qpath = policy == 2 ? 1 : 0;
    return old;
}
int32_t sgpt_ctx_set_encode_chains(sgpt_ctx* c, int32_t n, int32_t min_rows) {
    if (!c || n < 0 || n > 2 || min_rows < 0) return -1;
    const int old = c->chains;
    c->chains = n;
    c->chain_min_rows = min_rows;
    return old;
}
int64_t sgpt_ctx_encode_chain_calls(const sgpt_ctx* c) { return c ? c->chain_calls : 0; }
int32_t sgpt_ctx_set_query_tile(sgpt_ctx* c, int32_t k) {
    if (!c || k < 0 || k > 7) return -1;           // (7 plain candidates, 3 with the LayerNorm prologue: a k the kernel family lacks is "not served")
    const int old = c->qtile;
    c->qtile = k;
    return old;
}
#ifdef SGPT_EXPERIMENTS
int32_t sgpt_exp_set_gemm_skew(int32_t cycles) { return set_gemm_skew(cycles); }
int32_t sgpt_exp_set_gemm_w(int32_t on) { return set_gemm_use_w(on); }
#endif

}  // extern "C"
