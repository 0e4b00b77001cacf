// Ascending sort of unique 64-bit keys on the device, shared by useb_eval.hip (sgpt_eval_pairs) and ivf.hip (sgpt_ivf_lists): a bitonic
// network, tiles of S64_TILE keys in LDS for the strides below S64_TILE, one global compare-exchange launch per stride above.  The keys
// are unique wherever this is used ((score key | list) << 32 | index), so the result is the one sorted order.  Integer compares only.
// Every translation unit that includes this gets its own copy of the kernels (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef unsigned long long u64;

constexpr int S64_TILE = 2048;           // keys sorted in LDS by one workgroup (16 KiB)
constexpr int S64_THREADS = 256;

__device__ __forceinline__ uint32_t f2key(float f) {  // ascending uint order == ascending float order
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {  // the inverse of f2key
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// one compare-exchange step of the ascending bitonic network on a tile in LDS whose first key is key `base` of the array
__device__ __forceinline__ void s64_tile_step(u64* s, int base, int size, int stride, int t) {
    for (int p = t; p < S64_TILE / 2; p += S64_THREADS) {
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
        const bool up = ((base + i) & size) == 0;
        const u64 x = s[i], y = s[j];
        if ((x > y) == up && x != y) { s[i] = y; s[j] = x; }
    }
    __syncthreads();
}

// FULL: every size 2 .. S64_TILE of the network (the first launch); else the strides below S64_TILE of one size > S64_TILE
template <bool FULL>
__global__ __launch_bounds__(S64_THREADS) void s64_sort_tile_kernel(u64* __restrict__ keys, int size_outer) {
    __shared__ u64 s[S64_TILE];
    const int t = threadIdx.x;
    const int base = blockIdx.x * S64_TILE;
    for (int k = t; k < S64_TILE; k += S64_THREADS) s[k] = keys[base + k];
    __syncthreads();
    if (FULL) {
        for (int size = 2; size <= S64_TILE; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) s64_tile_step(s, base, size, stride, t);
    } else {
        for (int stride = S64_TILE >> 1; stride > 0; stride >>= 1) s64_tile_step(s, base, size_outer, stride, t);
    }
    for (int k = t; k < S64_TILE; k += S64_THREADS) keys[base + k] = s[k];
}

__global__ __launch_bounds__(S64_THREADS) void s64_sort_global_kernel(u64* __restrict__ keys, int np2, int size, int stride) {
    const int p = blockIdx.x * S64_THREADS + threadIdx.x;
    if (p >= (np2 >> 1)) return;
    const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
    const bool up = (i & size) == 0;
    const u64 x = keys[i], y = keys[j];
    if ((x > y) == up && x != y) { keys[i] = y; keys[j] = x; }
}

// the smallest power of two >= n that the network serves (at least one tile)
inline int s64_padded(long n) {
    int np2 = S64_TILE;
    while (np2 < n) np2 <<= 1;
    return np2;
}

// keys[0 .. np2) ascending; np2 = s64_padded(n) <= 2^30, the padding keys ~0 sort behind everything
inline void launch_sort_u64(u64* keys, int np2, hipStream_t s) {
    hipLaunchKernelGGL(s64_sort_tile_kernel<true>, dim3(np2 / S64_TILE), dim3(S64_THREADS), 0, s, keys, 0);
    for (long size = (long)S64_TILE * 2; size <= np2; size <<= 1) {
        for (int stride = (int)(size >> 1); stride >= S64_TILE; stride >>= 1)
            hipLaunchKernelGGL(s64_sort_global_kernel, dim3(np2 / 2 / S64_THREADS), dim3(S64_THREADS), 0, s, keys, np2, (int)size, stride);
        hipLaunchKernelGGL(s64_sort_tile_kernel<false>, dim3(np2 / S64_TILE), dim3(S64_THREADS), 0, s, keys, (int)size);
    }
}

// first p in [0, n) with keys[p] >= key (n if none)
__device__ __forceinline__ int lower_bound_key(const u64* __restrict__ keys, int n, u64 key) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = keys[lo + half] < key;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

}  // namespace
