// The opt-in FP8 decoder weights (DESIGN.md 2 "FP8 weight storage", include/crab_hip.h "FP8 decoder weights"): the quantiser.  The kernel
// that streams the codes is gemm_skinny_dma_w8_kernel (skinny.hip).  Nothing here is reached unless a caller asks for
// weight_dtype = "fp8_e4m3"; the bf16 weights stay where they are (prefill, M > 16 and lm_head keep reading them).
//
// STORAGE FORMAT.  W [N, K] bf16 -> codes [N, K] uint8 (OCP e4m3fn, row stride ld_codes bytes) + scale [N] fp32, one scale per OUTPUT row:
// the row format of the FP8 KV cache (fp8_common.h) applied to the rows of W as stored - the interleaved gate|up rows of a packed group
// each get their own scale.  W[n, k] reads back as float(code[n, k]) * scale[n]: the scale factors out of the K sum, so the GEMM applies
// it once per output column in its epilogue.
#include "common.h"
#include "crab_internal.h"
#include "fp8_common.h"

namespace {

// One wave per row (4 rows per block): pass 1 takes the row's amax (16-byte loads, 64 lanes x 8 elements per trip), pass 2 re-reads the row
// (L2 hits: a row is at most 37 KiB) and stores 8 codes per lane and trip.  Bytes K .. ld_codes - 1 of a code row are not written.
__global__ __launch_bounds__(256) void weight_quant_fp8_kernel(const bf16_t* __restrict__ W, long ldw, int N, int K, uint8_t* __restrict__ codes,
                                                              long ldc, float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                           // wave-uniform
    const bf16_t* src = W + n * ldw;
    float amax = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(src + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fmaxf(fabsf(lo_bf(w[i])), fabsf(hi_bf(w[i]))));
    }
    amax = wave_max(amax);
    const float sc = kv8_scale(amax);
    const float inv = __fdiv_rn(1.0f, sc);
    uint8_t* dst = codes + n * ldc;
    for (int k = lane * 8; k < K; k += 512) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(src + k);
        u32x2 c;
        c[0] = pack_fp8x4(__fmul_rn(lo_bf(w[0]), inv), __fmul_rn(hi_bf(w[0]), inv), __fmul_rn(lo_bf(w[1]), inv), __fmul_rn(hi_bf(w[1]), inv));
        c[1] = pack_fp8x4(__fmul_rn(lo_bf(w[2]), inv), __fmul_rn(hi_bf(w[2]), inv), __fmul_rn(lo_bf(w[3]), inv), __fmul_rn(hi_bf(w[3]), inv));
        *reinterpret_cast<u32x2*>(dst + k) = c;
    }
    if (lane == 0) scale[n] = sc;
}

}  // namespace

extern "C" int crab_weight_quant_fp8(crab_ctx* ctx, void* stream, const void* W, int64_t ldw, int N, int K, void* codes, int64_t ld_codes,
                                     float* scale) {
    if (!ctx) return CRAB_E_INVALID;
    if (!W || !codes || !scale || N <= 0 || K <= 0) return crab_fail(ctx, CRAB_E_INVALID, "weight_quant_fp8: bad argument");
    if ((K & 7) || (ldw & 7) || ldw < K || ((uintptr_t)W & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "weight_quant_fp8: K and ldw must be multiples of 8, ldw >= K, W 16-byte aligned");
    if ((ld_codes & 15) || ld_codes < K || ((uintptr_t)codes & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "weight_quant_fp8: ld_codes must be a multiple of 16 and >= K, codes 16-byte aligned (the GEMM streams code rows in 16-byte pieces)");
    hipLaunchKernelGGL(weight_quant_fp8_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, (long)ldw, N, K,
                       (uint8_t*)codes, (long)ld_codes, scale);
    return crab_check_launch(ctx, "weight_quant_fp8_kernel");
}
