// Verify-step attention of prompt-lookup speculative decoding (HF generation/utils.py _assisted_decoding: one forward over [current token ; k draft
// tokens] of ONE sequence; modeling_llama.py:394-445 with the causal mask of the k + 1 new positions): Sq <= 16 queries of a sequence over its cache,
// query i seeing the slots kv_start .. ctx - 1 + i.  The queries are MFMA A-operand rows, as the sibling rows of a clip are in
// attn_prefix_partial_kernel (attn_prefix.hip): one block per (sequence, kv head, group of 16 / (H / Hk) queries), every K / V row up to the group's
// last visible slot read ONCE per block - crab_attn_decode launched Sq times, or attn_own_merge_kernel with its block per query, read the cache Sq
// times.  The causal tail is a per-row key limit: a score at or past the row's limit takes no part in the row's maximum and its probability is an
// exact 0 (not exp of a masked score), so whatever a later query's slot holds cannot reach an earlier query; slots past the group's last visible one
// are never read.  No atomics, fixed reduction order: the output is a function of the inputs alone.
//
// vf_attend is a COPY of px_attend (attn_prefix.hip) with the per-row limit added in phase B.  It lives here, not as a parameter of px_attend,
// because px_attend is instantiated by the shared-prefix and beam kernels, whose bits are pinned (scripts/ab_bits.py attn): a moved loop has cost
// those kernels their last bit before (see attn_own_merge_row_kernel).  Built with -mllvm -amdgpu-mfma-vgpr-form like attn_prefix.hip (build.sh).
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

constexpr int VF_CH = 512;                                      // keys per chunk (scores of a chunk live in LDS), PX_CH of attn_prefix.hip

template <int HD, int ROWS>
struct VfShared {
    static constexpr int SMEM_F = (4 * ROWS * HD > VF_CH * ROWS) ? 4 * ROWS * HD : VF_CH * ROWS;
    __attribute__((aligned(16))) float sbuf[SMEM_F];
    float red[4][ROWS];
    float m_run[ROWS], l_run[ROWS], alpha_s[ROWS];
    int lim[ROWS];                                              // keys (from kbase on) visible to the row; 0 for a row without a query
};

template <int EPL> struct VfVec;
template <> struct VfVec<8> { typedef u32x4 T; };
template <> struct VfVec<4> { typedef u32x2 T; };

// ROWS query rows against nkeys K / V rows at kbase / vbase; row r sees the keys [0, sh.lim[r]) only (sh.lim written by the caller before the
// call, lim[r] <= nkeys).  On return sh.m_run / sh.l_run hold the running max and sum of every row and sh.sbuf[(w * ROWS + r) * HD + dd],
// w = 0 .. 3, the four per-wave partial sums of the unnormalised output; a __syncthreads() has been passed.  A row with lim 0: m = -1e30, l = 0, o = 0.
template <int HD, int ROWS>
__device__ __forceinline__ void vf_attend(VfShared<HD, ROWS>& sh, const bf16_t* __restrict__ qrow, const bf16_t* __restrict__ kbase,
                                          const bf16_t* __restrict__ vbase, int nkeys, float scale) {
    static_assert((HD == 64 || HD == 128) && (ROWS == 8 || ROWS == 16), "head_dim 64 / 128, 8 or 16 operand rows");
    constexpr int EPL = (HD == 128 && ROWS == 8) ? 8 : 4, KS = HD / 32;
    constexpr int LPG = HD / EPL, NG = 256 / LPG;               // lanes per key group (16 / 32), key groups per block (16 / 8)
    typedef typename VfVec<EPL>::T vrow_t;
    float* sbuf = sh.sbuf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = tid / LPG, sub = tid % LPG;
    const int fr = lane & 15, fg = lane >> 4;
    // A operand: row fr, k index 8 fg + e <-> d = 32 ks + 8 fg + e
    bf16x8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (qrow) w = *reinterpret_cast<const u32x4*>(qrow + ks * 32 + fg * 8);
        qf[ks] = __builtin_bit_cast(bf16x8_t, w);
    }
    const bf16_t* kfr = kbase + fg * 8;                         // + key * HD + 32 ks
    const bf16_t* vb = vbase + sub * EPL;
    float acc[ROWS][EPL];
#pragma unroll
    for (int g = 0; g < ROWS; ++g)
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[g][e] = 0.f;
    if (tid < ROWS) { sh.m_run[tid] = -1e30f; sh.l_run[tid] = 0.f; }

#pragma unroll 1
    for (int c0 = 0; c0 < nkeys; c0 += VF_CH) {
        const int cn = min(VF_CH, nkeys - c0);
        __syncthreads();                                  // previous chunk's probabilities consumed, m_run / l_run / lim visible
        // ---- A: scores on the matrix pipe.  Wave w takes the 16-key tiles w, w + 4, ...; keys beyond the chunk are clamped and not stored
        const int ntile = (cn + 15) >> 4;
        constexpr int TPT = 2;
#pragma unroll 1
        for (int t0 = wave; t0 < ntile; t0 += 4 * TPT) {
            u32x4 kw[TPT][KS];
#pragma unroll
            for (int u = 0; u < TPT; ++u) {
                const int jc = min((t0 + 4 * u) * 16 + fr, cn - 1);
                const bf16_t* kr = kfr + (long)(c0 + jc) * HD;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) kw[u][ks] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kr + ks * 32));
            }
#pragma unroll
            for (int u = 0; u < TPT; ++u) {
                if (t0 + 4 * u < ntile) {                       // wave-uniform
                    f32x4_t sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[ks], __builtin_bit_cast(bf16x8_t, kw[u][ks]), sc, 0, 0, 0);
                    // D: lane (key = l & 15) holds rows 4 (l >> 4) .. + 3 of its key
                    const int j = (t0 + 4 * u) * 16 + fr;
                    if (fg < ROWS / 4 && j < cn) *reinterpret_cast<f32x4_t*>(sbuf + j * ROWS + fg * 4) = sc * scale;
                }
            }
        }
        __syncthreads();
        // the first trip of V rows of phase C is requested here: it flies under phase B
        constexpr int RPT = 4;
        const int rounds = (cn + NG - 1) / NG;
        vrow_t vw[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int jc = min(u * NG + grp, cn - 1);
            vw[u] = __builtin_nontemporal_load(reinterpret_cast<const vrow_t*>(vb + (long)(c0 + jc) * HD));
        }
        // ---- B: per-row chunk max over the row's VISIBLE keys -> running max, p = exp(s - m) in place (0 for a key the row may not see), running sum
        {
            const int g = tid & (ROWS - 1);
            constexpr int KSTEP = 256 / ROWS;
            const int vis = min(sh.lim[g] - c0, cn);             // visible keys of row g inside this chunk (<= 0: none)
            float mx = -1e30f;
#pragma unroll 1
            for (int j = tid / ROWS; j < vis; j += KSTEP) mx = fmaxf(mx, sbuf[j * ROWS + g]);
            if (ROWS == 8) mx = fmaxf(mx, row_xor8(mx));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (lane < ROWS) sh.red[wave][lane] = mx;
            __syncthreads();
            const float m_old = sh.m_run[g];
            const float m_new = fmaxf(fmaxf(fmaxf(sh.red[0][g], sh.red[1][g]), fmaxf(sh.red[2][g], sh.red[3][g])), m_old);
            float sum = 0.f;
#pragma unroll 1
            for (int j = tid / ROWS; j < cn; j += KSTEP) {
                const float pv = j < vis ? __expf(sbuf[j * ROWS + g] - m_new) : 0.f;
                sbuf[j * ROWS + g] = pv;
                sum += pv;
            }
            if (ROWS == 8) sum += row_xor8(sum);
            sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
            __syncthreads();                                             // red[] max values consumed
            if (lane < ROWS) sh.red[wave][lane] = sum;
            __syncthreads();
            if (tid < ROWS) {
                const float a = __expf(m_old - m_new);
                sh.alpha_s[tid] = a;
                sh.l_run[tid] = sh.l_run[tid] * a + ((sh.red[0][tid] + sh.red[1][tid]) + (sh.red[2][tid] + sh.red[3][tid]));
                sh.m_run[tid] = m_new;
            }
            __syncthreads();
        }
        // ---- C: rescale (once per chunk) and accumulate P.V
#pragma unroll
        for (int g = 0; g < ROWS; ++g) {
            const float a = sh.alpha_s[g];
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[g][e] *= a;
        }
#pragma unroll 1
        for (int r0 = 0; r0 < rounds; r0 += RPT) {
            if (r0 > 0) {
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    const int jc = min((r0 + u) * NG + grp, cn - 1);
                    vw[u] = __builtin_nontemporal_load(reinterpret_cast<const vrow_t*>(vb + (long)(c0 + jc) * HD));
                }
            }
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int j = (r0 + u) * NG + grp, jc = min(j, cn - 1);
                float vx[EPL];
#pragma unroll
                for (int e = 0; e < EPL / 2; ++e) { vx[2 * e] = lo_bf(vw[u][e]); vx[2 * e + 1] = hi_bf(vw[u][e]); }
#pragma unroll
                for (int g4 = 0; g4 < ROWS / 4; ++g4) {
                    f32x4_t p = *reinterpret_cast<const f32x4_t*>(sbuf + jc * ROWS + g4 * 4);
                    if (j >= cn) p = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int e = 0; e < EPL; ++e) acc[g4 * 4 + r][e] += p[r] * vx[e];
                }
                // the scheduler otherwise hoists the probability reads of ALL rows of the trip above the first product (spills)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __syncthreads();
    // ---- the key groups share the running max: the groups of a wave are summed by shuffles, the 4 waves are left side by side in LDS
#pragma unroll
    for (int g = 0; g < ROWS; ++g)
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            float v = acc[g][e];
            if (LPG == 16) v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            acc[g][e] = v;
        }
    if (lane < LPG) {
#pragma unroll
        for (int g = 0; g < ROWS; ++g)
#pragma unroll
            for (int e = 0; e < EPL; ++e) sbuf[(wave * ROWS + g) * HD + sub * EPL + e] = acc[g][e];
    }
    __syncthreads();
}

// grid (Hk, B, query groups).  Group z holds the queries z * per .. of sequence b, per = 16 / (H / Hk) (ROWS == 8: the launcher found all Sq
// queries' heads in 8 operand rows, one group).  Operand row r = query (r / GH) of the group, head hk * GH + r % GH.
template <int HD, int ROWS>
__global__ __launch_bounds__(256, 2) void attn_verify_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, bf16_t* __restrict__ o, long ldo, int H, int Hk, int Tmax,
                                                          int Sq, int per, int ctx_host, const int* __restrict__ ctx_dev, float scale,
                                                          const int* __restrict__ kv_start) {
    __shared__ VfShared<HD, ROWS> sh;
    const int GH = H / Hk;
    const int hk = blockIdx.x, b = blockIdx.y, i0 = blockIdx.z * per;
    const int nq = min(per, Sq - i0);                            // >= 1 by the grid
    const int ks0 = min(max(kv_start ? kv_start[b] : 0, 0), Tmax);
    const int ctx = ctx_host + (ctx_dev ? ctx_dev[0] : 0);
    // one past the last slot query i0 + s may see, never past the cache (and never below ks0: an empty range)
    if (threadIdx.x < ROWS) {
        const int s = threadIdx.x / GH;
        const long last = (long)ctx + i0 + s;
        sh.lim[threadIdx.x] = s < nq ? (int)max(min(last, (long)Tmax) - ks0, 0L) : 0;
    }
    const long lastg = (long)ctx + i0 + nq - 1;
    const int nkeys = (int)max(min(lastg, (long)Tmax) - ks0, 0L);
    const int fr = threadIdx.x & 15;
    const int sib = fr / GH, hd = fr - sib * GH;
    const bf16_t* qrow = (fr < ROWS && sib < nq) ? q + ((long)b * Sq + i0 + sib) * ldq + (long)(hk * GH + hd) * HD : nullptr;
    const long kv0 = (((long)b * Hk + hk) * (long)Tmax + ks0) * HD;
    __syncthreads();                                             // lim visible also when the chunk loop runs zero times
    vf_attend<HD, ROWS>(sh, qrow, kc + kv0, vc + kv0, nkeys, scale);
    const int nvalid = nq * GH;
    for (int idx = threadIdx.x; idx < nvalid * HD; idx += 256) {
        const int r = idx / HD, dd = idx - r * HD;
        const int s2 = r / GH, h2 = hk * GH + (r - s2 * GH);
        const float L = sh.l_run[r];
        const float O = (sh.sbuf[idx] + sh.sbuf[ROWS * HD + idx]) + (sh.sbuf[2 * ROWS * HD + idx] + sh.sbuf[3 * ROWS * HD + idx]);
        o[((long)b * Sq + i0 + s2) * ldo + (long)h2 * HD + dd] = f2bf(L > 0.f ? O / L : 0.f);      // an empty range gives 0, as attn_decode_kernel
    }
}

bool vf_supported(int H, int Hk, int d) {                       // px_supported of attn_prefix.hip
    if (Hk <= 0 || H <= 0 || H % Hk) return false;
    const int g = H / Hk;
    return (d == 64 || d == 128) && (g == 1 || g == 2 || g == 4 || g == 7 || g == 8);
}

}  // namespace

extern "C" int crab_attn_verify(crab_ctx* ctx, void* stream, const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, void* o,
                                int64_t ldo, int B, int Sq, int H, int Hk, int d, int Tmax, int ctx_len_host, const int32_t* ctx_dev, float scale,
                                const int32_t* kv_start) {
    if (!ctx) return CRAB_E_INVALID;
    if (!vf_supported(H, Hk, d)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_verify: head_dim 64 / 128 with H / Hk in {1, 2, 4, 7, 8}");
    if (Sq < 1 || Sq > 16) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_verify: 1 <= Sq <= 16 queries per sequence");
    if (!qkv || !k_cache || !v_cache || !o || B <= 0 || B > 65535 || Tmax <= 0) return crab_fail(ctx, CRAB_E_INVALID, "attn_verify: bad argument");
    if (!ctx_dev && (ctx_len_host < 0 || ctx_len_host + Sq - 1 > Tmax)) return crab_fail(ctx, CRAB_E_INVALID, "attn_verify: ctx_len out of range");
    if (ldqkv < (int64_t)H * d || ldo < (int64_t)H * d || (ldqkv & 7) || ((uintptr_t)qkv & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "attn_verify: alignment (ldqkv % 8, 16-byte pointers) and ldqkv, ldo >= H * d");
    const int G = H / Hk, per = 16 / G;
    const bool small = Sq * G <= 8;                             // all queries' heads fit 8 operand rows: half the accumulators, one group
    dim3 grid(Hk, B, small ? 1 : (Sq + per - 1) / per), block(256);
    hipStream_t s = (hipStream_t)stream;
#define VF_LAUNCH(HD_, ROWS_)                                                                                                                          \
    hipLaunchKernelGGL((attn_verify_kernel<HD_, ROWS_>), grid, block, 0, s, (const bf16_t*)qkv, (long)ldqkv, (const bf16_t*)k_cache,                   \
                       (const bf16_t*)v_cache, (bf16_t*)o, (long)ldo, H, Hk, Tmax, Sq, small ? 8 / G : per, ctx_len_host, ctx_dev, scale, kv_start)
    if (d == 128) { if (small) VF_LAUNCH(128, 8); else VF_LAUNCH(128, 16); }
    else          { if (small) VF_LAUNCH(64, 8); else VF_LAUNCH(64, 16); }
#undef VF_LAUNCH
    return crab_check_launch(ctx, d == 128 ? "attn_verify_kernel<128>" : "attn_verify_kernel<64>");
}
