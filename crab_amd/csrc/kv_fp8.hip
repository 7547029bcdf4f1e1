// The opt-in FP8 KV cache (DESIGN.md 2 "FP8 storage mode", include/crab_hip.h "FP8 KV cache"): the quantiser that moves a prefilled
// bf16 block into it and the decode attention that appends to it and streams it.  Nothing here is reached unless a caller asks for
// kv_cache_dtype = "fp8_e4m3"; the bf16 kernels (attn.hip) are untouched.
//
// STORAGE FORMAT.  K (after RoPE) and V: one byte per element, OCP e4m3fn (gfx950's native fp8; NOT the fnuz encoding of gfx942), layout
// [L, B, Hk, Tmax, d] like the bf16 cache.  One fp32 scale per cached row and KV head, for K and for V: two arrays [L, B, Hk, Tmax].
//     amax  = max |x| over the row's d elements (x = the bf16 values the bf16 cache would hold)
//     scale = amax / 448.0f  (fp32 division);  scale = 1.0f when amax == 0;  scale = FLT_MIN when the quotient is below FLT_MIN (*)
//     inv   = 1.0f / scale;   code = e4m3fn_rne(x * inv);   value read back = float(code) * scale
// |x * inv| exceeds 448 only by the rounding of the product, which still rounds to 448 (the next e4m3fn step would be 480; the tie is at
// 464): no saturation mode is relied on.  (*) amax below 448 * 2^-126 (bf16 subnormals and the smallest normals) would make `inv` overflow
// to infinity and every code NaN; with the floor, inv = 2^126 and the codes are finite (such a row is all noise: |x| < 6e-36).
// A cached row costs d + 4 bytes instead of 2 d (132 / 256 = 0.516 at d = 128).
// Prefill attends bf16 K / V (it runs into a bf16 staging block that crab_kv_quant_fp8 then moves here).  Decode attends the fp8 cache
// for EVERY key, the one appended in the same step included: a decode step's output is a function of the cache contents and the raw
// q|k|v row alone.
//
// Conversions: __builtin_amdgcn_cvt_pk_fp8_f32 / __builtin_amdgcn_cvt_pk_f32_fp8 (v_cvt_pk_fp8_f32, v_cvt_pk_f32_fp8: two values per
// instruction, round to nearest even, word select for the upper half).  Everything written to memory is a plain vector store.
#include "common.h"
#include "crab_internal.h"
#include "attn_decode_core.h"
#include "fp8_common.h"                     // kv8_scale, pack_fp8x4: the row format, shared with the FP8 decoder weights

namespace {

// max over the 8 lanes (lane ^ 1, ^ 2, ^ 4) / the 16 lanes of a DPP row
__device__ __forceinline__ float row8_max(float v) {
    v = fmaxf(v, row_xor4(v));
    v = fmaxf(v, row_xor2(v));
    v = fmaxf(v, row_xor1(v));
    return v;
}
__device__ __forceinline__ float row8_sum(float v) {
    v += row_xor4(v);
    v += row_xor2(v);
    v += row_xor1(v);
    return v;
}
// ---------------------------------------------------------------------------------------------- bf16 block -> fp8 cache
// One 16-byte load (8 bf16) per lane; LPR = HD / 8 lanes share a row (16 at d = 128: a DPP row, 8 at d = 64: half of one), amax by DPP,
// 8 codes = one 8-byte store per lane, one scale store per row.  blockIdx.y: 0 = K, 1 = V.  Rows below row_off[b] of a front-padded
// sequence are neither read nor written.
template <int HD>
__global__ __launch_bounds__(256) void kv_quant_fp8_kernel(const bf16_t* __restrict__ ksrc, const bf16_t* __restrict__ vsrc, long src_ls, int Tsrc,
                                                           int t0, uint8_t* __restrict__ kdst, uint8_t* __restrict__ vdst, long dst_ls,
                                                           float* __restrict__ kscale, float* __restrict__ vscale, long sc_ls, int L, int Bc,
                                                           int Hk, int Tmax, int b0, int t_dst, int S, const int* __restrict__ row_off) {
    constexpr int LPR = HD / 8, RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const long r = (long)blockIdx.x * RPB + threadIdx.x / LPR;        // row id over [L, Bc, Hk, S]
    const long total = (long)L * Bc * Hk * S;
    const bool isv = blockIdx.y != 0;
    bool live = r < total;
    const long rr = live ? r : 0;
    const int s = (int)(rr % S);
    const long t1 = rr / S;
    const int hk = (int)(t1 % Hk);
    const long t2 = t1 / Hk;
    const int b = (int)(t2 % Bc), l = (int)(t2 / Bc);
    if (row_off && s < row_off[b]) live = false;
    const bf16_t* src = (isv ? vsrc : ksrc) + (long)l * src_ls + (((long)b * Hk + hk) * Tsrc + t0 + s) * HD + sub * 8;
    u32x4 w = {0u, 0u, 0u, 0u};
    if (live) w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
    float x[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = lo_bf(w[i]); x[2 * i + 1] = hi_bf(w[i]); }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
    amax = row8_max(amax);
    if (LPR == 16) amax = fmaxf(amax, row_xor8(amax));
    const float scale = kv8_scale(amax);
    const float inv = __fdiv_rn(1.0f, scale);
    u32x2 c;
    c[0] = pack_fp8x4(__fmul_rn(x[0], inv), __fmul_rn(x[1], inv), __fmul_rn(x[2], inv), __fmul_rn(x[3], inv));
    c[1] = pack_fp8x4(__fmul_rn(x[4], inv), __fmul_rn(x[5], inv), __fmul_rn(x[6], inv), __fmul_rn(x[7], inv));
    if (live) {
        const long drow = ((long)(b0 + b) * Hk + hk) * Tmax + t_dst + s;
        uint8_t* dst = (isv ? vdst : kdst) + (long)l * dst_ls + drow * HD + sub * 8;
        *reinterpret_cast<u32x2*>(dst) = c;
        if (sub == 0) ((isv ? vscale : kscale) + (long)l * sc_ls)[drow] = scale;
    }
}

// ---------------------------------------------------------------------------------------------- decode attention over the fp8 cache
// One block per (b, h), 256 threads = NG = 32 groups of 8 lanes; group g streams the cached rows kv_start + g, + g + 32, ...; a lane owns
// EPL = HD / 8 consecutive head-dim elements = EPL bytes of a row (HD = 128: one 16-byte load per lane and row, as many bytes in flight
// per wave as attn_decode_kernel keeps).  The row scales are folded in as scalars: score = (q . codes) * k_scale, and v_scale rides on
// the softmax weight - nothing is scaled element-wise.  Two keys per trip with the next pair requested before the current one is
// consumed, non-temporal loads (every row is read once per step by one block; the G blocks of a grouped-query KV head meet in L2): the
// schedule of dec_stream (attn_decode_core.h) over codes and row scales instead of bf16 words, so the loop is this kernel's own; the merge
// of the 32 groups is dec_group_merge of that header.
// From the RAW q|k|v row (the projection ran without RoPE): q and the new k rotate here at position pos - kv_start (lane sub's partner
// dim +- d/2 is lane sub ^ 4), are rounded to bf16 like the stored form, the new k / v rows are quantised exactly like the quantiser
// above; the block with h % G == 0 appends codes and scales at slot pos, and EVERY block attends the dequantised new row (group 0 seeds
// its running softmax with it).
template <int WPL> struct CodeVec;
template <> struct CodeVec<4> { typedef u32x4 type; };
template <> struct CodeVec<2> { typedef u32x2 type; };

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_fp8_kernel(const bf16_t* __restrict__ qkv, long ldq, const float* __restrict__ tab,
                                                              uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, float* __restrict__ ksc,
                                                              float* __restrict__ vsc, bf16_t* __restrict__ o, long ldo, int H, int Hk, int Tmax,
                                                              int pos0, const int* __restrict__ pos_dev, float scale,
                                                              const int* __restrict__ kv_start) {
    constexpr int NG = 32, EPL = HD / 8, WPL = EPL / 4;                   // elements, fp8 words per lane
    typedef typename CodeVec<WPL>::type cvec;
    __shared__ float snew[3][HD];                               // q | new k | new v of this head, fp32 of the bf16-rounded values
    const int tid = threadIdx.x;
    const int grp = tid >> 3, sub = tid & 7;
    const int h = blockIdx.x, b = blockIdx.y;
    const int G = H / Hk, hk = h / G;
    const int pos = pos0 + (pos_dev ? pos_dev[0] : 0);          // slot of the token being decoded
    const int ks0 = kv_start ? kv_start[b] : 0;                 // first slot of this sequence (right-aligned ragged batch)
    if (pos >= Tmax || pos < ks0 || ks0 < 0) return;            // never index outside the cache (a caller error; the host checks what it can see)
    const int nc = pos - ks0;                                   // cached keys: slots ks0 .. pos - 1
    const long crow = ((long)b * Hk + hk) * (long)Tmax;
    const uint8_t* kb = kc + (crow + ks0) * HD + sub * EPL;
    const uint8_t* vb = vc + (crow + ks0) * HD + sub * EPL;
    const float* ksb = ksc + crow + ks0;
    const float* vsb = vsc + crow + ks0;
    // ---- the first two keys of this group are requested before anything else
    cvec k0 = {}, v0 = {}, k1 = {}, v1 = {};
    float ks_0 = 0.f, vs_0 = 0.f, ks_1 = 0.f, vs_1 = 0.f;
    if (grp < nc) {
        k0 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(kb + (long)grp * HD));
        v0 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(vb + (long)grp * HD));
        ks_0 = ksb[grp]; vs_0 = vsb[grp];
    }
    if (grp + NG < nc) {
        k1 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(kb + (long)(grp + NG) * HD));
        v1 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(vb + (long)(grp + NG) * HD));
        ks_1 = ksb[grp + NG]; vs_1 = vsb[grp + NG];
    }
    // ---- q, new k (rotated, rounded like the stored bf16 form) and new v of this head, once per block through LDS: thread i of wave 0 / 1 owns
    // the rotation pair (i, i + d/2) of q / k, wave 2 copies v (rotating per 8-lane group instead kept the whole table row, three packed rows
    // and their results live beside the K / V rows in flight: 146 VGPRs)
    {
        const int part = tid >> 6, i = tid & 63;                 // 0: q, 1: k, 2: v
        if (part < 3 && i < HD / 2) {
            const bf16_t* src = qkv + (long)b * ldq + (long)(part == 0 ? h : part == 1 ? H + hk : H + Hk + hk) * HD;
            const float x1 = bf2f(src[i]), x2 = bf2f(src[i + HD / 2]);
            float y1 = x1, y2 = x2;
            if (part < 2) {
                const float* cs = tab + ((long)(pos - ks0) * (HD / 2) + i) * 2;
                const uint32_t w = pack_bf2(rope_lo(x1, x2, cs[0], cs[1]), rope_hi(x1, x2, cs[0], cs[1]));
                y1 = lo_bf(w); y2 = hi_bf(w);
            }
            snew[part][i] = y1; snew[part][i + HD / 2] = y2;
        }
    }
    __syncthreads();
    float qv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) qv[e] = snew[0][sub * EPL + e] * scale;
    float m = -1e30f, l = 0.f;
    f32x2_t acc[EPL / 2];
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) acc[e] = f32x2_t{0.f, 0.f};
    // dot of this lane's q elements with the codes of one row / accumulate a weighted row of codes
#define KV8_DOT(cv, out)                                                                                         \
    {                                                                                                            \
        f32x2_t d2 = {0.f, 0.f};                                                                                 \
        _Pragma("unroll") for (int i = 0; i < WPL; ++i) {                                                        \
            const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)cv[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)cv[i], true); \
            d2 += f32x2_t{qv[4 * i], qv[4 * i + 1]} * lo;                                                        \
            d2 += f32x2_t{qv[4 * i + 2], qv[4 * i + 3]} * hi;                                                    \
        }                                                                                                        \
        out = row8_sum(d2[0] + d2[1]);                                                                           \
    }
#define KV8_ACC(cv, w)                                                                                           \
    _Pragma("unroll") for (int i = 0; i < WPL; ++i) {                                                            \
        const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)cv[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)cv[i], true); \
        acc[2 * i] += f32x2_t{w, w} * lo;                                                                        \
        acc[2 * i + 1] += f32x2_t{w, w} * hi;                                                                    \
    }
    if (grp == 0) {
        // ---- the new rows: quantised exactly like kv_quant_fp8_kernel (8 lanes hold a row), appended by the block of the KV head's first
        // query head, and attended from registers in their DEQUANTISED form (this group's running softmax starts with them)
        float kn[EPL], vn[EPL], ka = 0.f, va = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            kn[e] = snew[1][sub * EPL + e]; vn[e] = snew[2][sub * EPL + e];
            ka = fmaxf(ka, fabsf(kn[e])); va = fmaxf(va, fabsf(vn[e]));
        }
        const float ksn = kv8_scale(row8_max(ka)), vsn = kv8_scale(row8_max(va));
        const float kin = __fdiv_rn(1.0f, ksn), vin = __fdiv_rn(1.0f, vsn);
        cvec kq, vq;
#pragma unroll
        for (int i = 0; i < WPL; ++i) {
            kq[i] = pack_fp8x4(__fmul_rn(kn[4 * i], kin), __fmul_rn(kn[4 * i + 1], kin), __fmul_rn(kn[4 * i + 2], kin), __fmul_rn(kn[4 * i + 3], kin));
            vq[i] = pack_fp8x4(__fmul_rn(vn[4 * i], vin), __fmul_rn(vn[4 * i + 1], vin), __fmul_rn(vn[4 * i + 2], vin), __fmul_rn(vn[4 * i + 3], vin));
        }
        if (h % G == 0) {                                       // append for the following steps
            *reinterpret_cast<cvec*>(kc + (crow + pos) * HD + sub * EPL) = kq;
            *reinterpret_cast<cvec*>(vc + (crow + pos) * HD + sub * EPL) = vq;
            if (sub == 0) { ksc[crow + pos] = ksn; vsc[crow + pos] = vsn; }
        }
        float s;
        KV8_DOT(kq, s);
        m = s * ksn; l = 1.f;
        KV8_ACC(vq, vsn);
    }
    for (int j = grp; j < nc; j += 2 * NG) {
        cvec kn0 = {}, vn0 = {}, kn1 = {}, vn1 = {};
        float ksn0 = 0.f, vsn0 = 0.f, ksn1 = 0.f, vsn1 = 0.f;
        if (j + 2 * NG < nc) {
            kn0 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(kb + (long)(j + 2 * NG) * HD));
            vn0 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(vb + (long)(j + 2 * NG) * HD));
            ksn0 = ksb[j + 2 * NG]; vsn0 = vsb[j + 2 * NG];
        }
        if (j + 3 * NG < nc) {
            kn1 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(kb + (long)(j + 3 * NG) * HD));
            vn1 = __builtin_nontemporal_load(reinterpret_cast<const cvec*>(vb + (long)(j + 3 * NG) * HD));
            ksn1 = ksb[j + 3 * NG]; vsn1 = vsb[j + 3 * NG];
        }
        float s0, s1;
        KV8_DOT(k0, s0);
        KV8_DOT(k1, s1);
        s0 *= ks_0; s1 *= ks_1;
        const bool has1 = j + NG < nc;                          // group-uniform
        const float mn = fmaxf(m, has1 ? fmaxf(s0, s1) : s0);
        const float a = __expf(m - mn), p0 = __expf(s0 - mn), p1 = has1 ? __expf(s1 - mn) : 0.f;
        l = l * a + (p0 + p1);
#pragma unroll
        for (int e = 0; e < EPL / 2; ++e) acc[e] *= f32x2_t{a, a};
        const float w0 = p0 * vs_0, w1 = p1 * vs_1;
        KV8_ACC(v0, w0);
        KV8_ACC(v1, w1);
        m = mn;
        k0 = kn0; v0 = vn0; k1 = kn1; v1 = vn1;
        ks_0 = ksn0; vs_0 = vsn0; ks_1 = ksn1; vs_1 = vsn1;
    }
#undef KV8_DOT
#undef KV8_ACC
    // (one VGPR fewer than with the merge written here, 98 / 66 at HD = 128 / 64; LDS and occupancy as before)
    float accf[EPL], M, L, O;
#pragma unroll
    for (int e = 0; e < EPL / 2; ++e) { accf[2 * e] = acc[e][0]; accf[2 * e + 1] = acc[e][1]; }
    dec_group_merge<HD, NG, EPL, 4>(grp, sub, m, l, accf, M, L, O);
    if (tid < HD) o[(long)b * ldo + (long)h * HD + tid] = f2bf(O / L);
}

}  // namespace

extern "C" int crab_kv_quant_fp8(crab_ctx* ctx, void* stream, const void* k_src, const void* v_src, int64_t src_layer_stride, int T_src, int t0,
                                 void* k_codes, void* v_codes, int64_t code_layer_stride, float* k_scale, float* v_scale,
                                 int64_t scale_layer_stride, int L, int Bc, int Hk, int d, int Tmax, int b0, int t_dst, int S,
                                 const int32_t* row_off) {
    if (!ctx) return CRAB_E_INVALID;
    if (!k_src || !v_src || !k_codes || !v_codes || !k_scale || !v_scale || L <= 0 || Bc <= 0 || Hk <= 0 || S <= 0)
        return crab_fail(ctx, CRAB_E_INVALID, "kv_quant_fp8: bad argument");
    if (d != 64 && d != 128) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "kv_quant_fp8: head_dim must be 64 or 128");
    if (t0 < 0 || t0 + S > T_src || t_dst < 0 || t_dst + S > Tmax || b0 < 0)
        return crab_fail(ctx, CRAB_E_INVALID, "kv_quant_fp8: rows t0 .. t0 + S - 1 must lie in the source block and slots t_dst .. t_dst + S - 1 in the cache");
    if (((uintptr_t)k_src & 15) || ((uintptr_t)v_src & 15) || ((uintptr_t)k_codes & 7) || ((uintptr_t)v_codes & 7) || (src_layer_stride & 7) ||
        (code_layer_stride & 7))
        return crab_fail(ctx, CRAB_E_INVALID, "kv_quant_fp8: alignment (16-byte source rows, 8-byte code rows)");
    const long rows = (long)L * Bc * Hk * S;
    const int rpb = 256 / (d / 8);
    const long blocks = (rows + rpb - 1) / rpb;
    if (blocks > 0x7fffffffL) return crab_fail(ctx, CRAB_E_INVALID, "kv_quant_fp8: too many rows for one launch");
    dim3 grid((unsigned)blocks, 2), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d == 128)
        hipLaunchKernelGGL((kv_quant_fp8_kernel<128>), grid, block, 0, s, (const bf16_t*)k_src, (const bf16_t*)v_src, (long)src_layer_stride, T_src, t0,
                           (uint8_t*)k_codes, (uint8_t*)v_codes, (long)code_layer_stride, k_scale, v_scale, (long)scale_layer_stride, L, Bc, Hk, Tmax,
                           b0, t_dst, S, row_off);
    else
        hipLaunchKernelGGL((kv_quant_fp8_kernel<64>), grid, block, 0, s, (const bf16_t*)k_src, (const bf16_t*)v_src, (long)src_layer_stride, T_src, t0,
                           (uint8_t*)k_codes, (uint8_t*)v_codes, (long)code_layer_stride, k_scale, v_scale, (long)scale_layer_stride, L, Bc, Hk, Tmax,
                           b0, t_dst, S, row_off);
    return crab_check_launch(ctx, d == 128 ? "kv_quant_fp8_kernel<128>" : "kv_quant_fp8_kernel<64>");
}

extern "C" int crab_attn_decode_fp8(crab_ctx* ctx, void* stream, const void* qkv, int64_t ldqkv, const float* rope_tab, void* k_codes,
                                    void* v_codes, float* k_scale, float* v_scale, void* o, int64_t ldo, int B, int H, int Hk, int d, int Tmax,
                                    int pos0, const int32_t* pos_dev, float scale, const int32_t* kv_start) {
    if (!ctx) return CRAB_E_INVALID;
    if (!qkv || !rope_tab || !k_codes || !v_codes || !k_scale || !v_scale || !o || B <= 0 || H <= 0 || Hk <= 0 || H % Hk)
        return crab_fail(ctx, CRAB_E_INVALID, "attn_decode_fp8: bad argument");
    if (d != 64 && d != 128) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_decode_fp8: head_dim must be 64 or 128");
    if ((ldqkv & 1) || ((uintptr_t)qkv & 3) || ((uintptr_t)k_codes & 15) || ((uintptr_t)v_codes & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "attn_decode_fp8: alignment");
    if (!pos_dev && (pos0 < 0 || pos0 >= Tmax)) return crab_fail(ctx, CRAB_E_INVALID, "attn_decode_fp8: position outside the KV cache");
    dim3 grid(H, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d == 128)
        hipLaunchKernelGGL((attn_decode_fp8_kernel<128>), grid, block, 0, s, (const bf16_t*)qkv, (long)ldqkv, rope_tab, (uint8_t*)k_codes,
                           (uint8_t*)v_codes, k_scale, v_scale, (bf16_t*)o, (long)ldo, H, Hk, Tmax, pos0, pos_dev, scale, kv_start);
    else
        hipLaunchKernelGGL((attn_decode_fp8_kernel<64>), grid, block, 0, s, (const bf16_t*)qkv, (long)ldqkv, rope_tab, (uint8_t*)k_codes,
                           (uint8_t*)v_codes, k_scale, v_scale, (bf16_t*)o, (long)ldo, H, Hk, Tmax, pos0, pos_dev, scale, kv_start);
    return crab_check_launch(ctx, d == 128 ? "attn_decode_fp8_kernel<128>" : "attn_decode_fp8_kernel<64>");
}
