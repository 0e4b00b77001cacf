// The fp8 codec of the one-byte scorer tile (score64c.h): a corpus held as OCP e4m3fn codes [N][d] bytes with one power-of-two fp32
// scale per document (the format of sgpt_fp8_quantize_rows).
//
// Arithmetic.  Every e4m3 value is an f16 value (4 exponent bits, 3 mantissa bits, |v| <= 448, smallest subnormal 2^-9 -- a NORMAL
// f16), so codes are converted in registers by the hardware conversions e4m3 -> f32 -> f16 (v_cvt_pk_f32_fp8, v_cvt_pkrtz_f16_f32:
// both exact here) and feed the same v_mfma_f32_16x16x32_f16 as the f16 scorer, in the same k order.  The arithmetic conversion
// rather than the bit move (b & 0x80) << 8 | (b & 0x7f) << 7: it is two instructions per code pair where the bit move is four or
// five, it keeps the operands clear of f16 subnormals, and the NaN codes 0x7f / 0xff become NaN without a test (NaN score -> -1 in
// the epilogue, as the f16 scorer).  The document's scale multiplies the fp32 accumulators once per tile: a power of two, so the
// product is exactly the accumulator the f16 scorer reaches on the de-quantised row (code * scale in f16) as long as nothing under-
// or overflows -- scores are comparable bit for bit.
#include "score64c.h"

namespace {

struct Fp8Codec {
    typedef Score8Args Args;
    static constexpr bool kRagged = false;         // whole 256-document tiles (score64q8_shape_ok); the planner routes a tail elsewhere
    // 8 e4m3fn codes (k ascending from the low byte of c.x) -> 8 f16, exact; NaN codes -> NaN
    static __device__ __forceinline__ uint4 cvt(const uint2 c) {
        const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
        const f32x2_t e = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), f = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
        uint4 r;
        r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a[0], a[1]));
        r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(b[0], b[1]));
        r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(e[0], e[1]));
        r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f[0], f[1]));
        return r;
    }
    struct Lane {
        float sc[2][4];                            // this lane's 8 documents' scales
        __device__ __forceinline__ void before_loop(const Args&, int) {}
        __device__ __forceinline__ void tile_begin(const Args& a, long n0, int g) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[j][r] = a.scale[(n0 + j * 16 + 4 * g + r) * a.scale_stride];
        }
        __device__ __forceinline__ float finish(float acc, int, int j, int r) const { return acc * sc[j][r]; }
    };
};

}  // namespace

// 64 padded f16 query rows, whole 256-document tiles, d a multiple of the 128-element k-step, 8-byte aligned code rows
bool score64q8_shape_ok(int M, long N, int K, const void* codes, long ldw) {
    return M == 64 && N > 0 && N % 256 == 0 && K >= 128 && K % 128 == 0 && ((size_t)codes & 7) == 0 && ldw % 8 == 0;
}

void launch_score64q8(int epi, const Score8Args& a, hipStream_t s) {
    if (!score64q8_shape_ok(a.g.M, a.g.N, a.g.K, a.g.W, a.g.ldw) || (epi != EPI_SCORE && epi != EPI_SCORE_FILTER)) abort();
    launch_score64c<Fp8Codec>(epi, a, s);
}
