// OCP e4m3fn helpers shared by the FP8 KV cache (kv_fp8.hip) and the FP8 decoder weights (w8.hip, skinny.hip): ONE statement of the row
// format - scale = amax / 448 (1.0 for an all-zero row, floored at FLT_MIN), code = e4m3fn_rne(x * (1 / scale)) - and of the conversions
// (v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8: two values per instruction, round to nearest even, word select for the upper half).
#pragma once
#include "common.h"
#include <float.h>

typedef float f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float kv8_scale(float amax) {
    if (amax == 0.f) return 1.0f;
    return fmaxf(__fdiv_rn(amax, 448.0f), FLT_MIN);
}
// four fp32 -> one word of four e4m3fn codes (element 0 in the low byte)
__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}
// two words of eight e4m3fn codes -> four words of eight bf16, an MFMA fragment (element 0 in the low half of word 0).  Exact: every e4m3fn
// value, subnormals included, is a bf16 value (4 exponent bits, 3 mantissa bits), so the fp32 the hardware conversion returns has 16 zero low
// bits and the byte permute that keeps the high halves loses nothing.
__device__ __forceinline__ u32x4 fp8x8_to_bf16x8(uint32_t w0, uint32_t w1) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
    const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
    u32x4 r;
    r[0] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
    r[1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
    r[2] = __builtin_amdgcn_perm(__float_as_uint(c[1]), __float_as_uint(c[0]), 0x07060302u);
    r[3] = __builtin_amdgcn_perm(__float_as_uint(d[1]), __float_as_uint(d[0]), 0x07060302u);
    return r;
}
