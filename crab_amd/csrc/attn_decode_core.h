// What the one-query-per-row decode attention kernels share: key groups of LPG lanes stream K / V rows, each group keeps an online softmax
// (m, l, acc) over its keys, and the NG groups of a block are merged through LDS with the log-sum-exp rule in group order.
//   dec_group_merge   attn_decode_kernel, attn_decode_keymask_kernel, attn_decode_rope_kernel (attn.hip), attn_own_merge_row_kernel (attn_prefix.hip),
//                     attn_decode_fp8_kernel (kv_fp8.hip)
//   dec_stream        attn_decode_kernel<128>, attn_own_merge_row_kernel<128>
// The one-key online-softmax steps of these kernels stay at their sites: shared, the compiler fused other products and output bits moved
// ("One decode-attention core").  attn_decode_gqa_kernel and px_attend (the MFMA score path) are another algorithm.
// Device inline templates only.
#pragma once
#include "common.h"

// A lane's partial q . k over WPL packed bf16 words (an u32x4: HD = 128), in the pair order of every HD = 128 site.
template <int WPL, typename W>
__device__ __forceinline__ float dec_dot(const float* qv, W w) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < WPL; ++i) s += qv[2 * i] * lo_bf(w[i]) + qv[2 * i + 1] * hi_bf(w[i]);
    return s;
}

// 16 groups of 16 lanes over the keys 0 .. ctx - 1 of the rows at kb / vb (this lane's HD / 16 elements of row 0): group grp takes keys grp,
// grp + 16, ...  Every K / V row is read exactly once per step by exactly one block, so the loads carry the non-temporal hint
// (global_load ... nt): measured 562 -> 537 us per launch in the benchmark (6.2 -> 6.5 TB/s; 6.8 TB/s in isolation) - the stream no longer
// displaces the weights and activations the neighbouring GEMMs keep in L2 / MALL.
// HD = 128 only: at HD = 64 the two kernels keep their one-key loop (through this function its bits moved).
__device__ __forceinline__ void dec_stream(const float* qv, const bf16_t* kb, const bf16_t* vb, int ctx, int grp,
                                           float& m, float& l, float* acc) {
    constexpr int HD = 128;
    {
        // TWO keys per trip (j and j + 16) with the next pair requested before the current one is consumed: every lane keeps four
        // 16-byte K and four 16-byte V loads in flight, and the loop-carried online-softmax chain (max, two exps, rescale of the
        // accumulators) is paid once per two keys
        const u32x4 z4 = {0u, 0u, 0u, 0u};
        u32x4 k0 = z4, v0 = z4, k1 = z4, v1 = z4;
        if (grp < ctx) {
            k0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (long)grp * HD));
            v0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (long)grp * HD));
        }
        if (grp + 16 < ctx) {
            k1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (long)(grp + 16) * HD));
            v1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (long)(grp + 16) * HD));
        }
        for (int j = grp; j < ctx; j += 32) {
            u32x4 kn0 = z4, vn0 = z4, kn1 = z4, vn1 = z4;
            if (j + 32 < ctx) {
                kn0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (long)(j + 32) * HD));
                vn0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (long)(j + 32) * HD));
            }
            if (j + 48 < ctx) {
                kn1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + (long)(j + 48) * HD));
                vn1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + (long)(j + 48) * HD));
            }
            const float s0 = row16_sum(dec_dot<4>(qv, k0)), s1 = row16_sum(dec_dot<4>(qv, k1));
            const bool has1 = j + 16 < ctx;                      // group-uniform
            const float mn = fmaxf(m, has1 ? fmaxf(s0, s1) : s0);
            const float a = __expf(m - mn), p0 = __expf(s0 - mn), p1 = has1 ? __expf(s1 - mn) : 0.f;
            l = l * a + (p0 + p1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] = acc[2 * e] * a + (p0 * lo_bf(v0[e]) + p1 * lo_bf(v1[e]));
                acc[2 * e + 1] = acc[2 * e + 1] * a + (p0 * hi_bf(v0[e]) + p1 * hi_bf(v1[e]));
            }
            m = mn;
            k0 = kn0; v0 = vn0; k1 = kn1; v1 = vn1;
        }
    }
}

// Merge of the NG key groups of a block (lane sub of group grp holds elements sub * EPL .. + EPL - 1 of its group's acc): through LDS, then
// thread tid < HD reduces element tid over the groups in group order - a group without keys (m = -1e30, l = 0) adds nothing.  (M, L, O) is the
// block's max, sum and unnormalised output element; threads tid >= HD get (-1e30, 0, 0).  The caller owns the final store.  UNR: unroll
// factor of the weighted sum.
template <int HD, int NG, int EPL, int UNR = NG>
__device__ __forceinline__ void dec_group_merge(int grp, int sub, float m, float l, const float* acc, float& M, float& L, float& O) {
    __shared__ float sm[NG], sl[NG];
    __shared__ float so[NG][HD];
    const int tid = threadIdx.x;
    if (sub == 0) { sm[grp] = m; sl[grp] = l; }
#pragma unroll
    for (int e = 0; e < EPL; ++e) so[grp][sub * EPL + e] = acc[e];
    __syncthreads();
    M = -1e30f; L = 0.f; O = 0.f;
    if (tid < HD) {
#pragma unroll
        for (int g = 0; g < NG; ++g) M = fmaxf(M, sm[g]);
#pragma unroll UNR
        for (int g = 0; g < NG; ++g) {
            const float w = __expf(sm[g] - M);
            L += sl[g] * w;
            O += so[g][tid] * w;
        }
    }
}
