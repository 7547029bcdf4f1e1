// The streaming attend loop of the kernels that put several query rows on the MFMA A operand: the shared-prefix pair and the beam kernels
// (attn_prefix.hip, LIM = false) and the verify step of speculative decoding (attn_verify.hip, LIM = true: a per-row key limit in phase B).
// LIM is a compile-time parameter: with LIM = false nothing of the limit exists - no struct member, no instruction - so the kernels of
// attn_prefix.hip keep their machine code (scripts/isa_diff.py against the build before a change is the first check, scripts/ab_bits.py attn
// the second).  Users are built with -mllvm -amdgpu-mfma-vgpr-form (build.sh).
#pragma once
#include "common.h"

namespace {

constexpr int PX_CH = 512;                                      // keys per chunk (scores of a chunk live in LDS)

// Shared state of one tile pass.  sbuf: scores [PX_CH][ROWS] fp32 during the chunks, the merge buffer [4 waves][ROWS][HD] at the end.
template <int HD, int ROWS, bool LIM = false>
struct PxShared {
    static constexpr int SMEM_F = (4 * ROWS * HD > PX_CH * ROWS) ? 4 * ROWS * HD : PX_CH * ROWS;
    __attribute__((aligned(16))) float sbuf[SMEM_F];
    float red[4][ROWS];
    float m_run[ROWS], l_run[ROWS], alpha_s[ROWS];
    int lim[LIM ? ROWS : 0];                                    // LIM: keys (from kbase on) visible to the row; 0 for a row without a query.  The last member:
                                                                // everything in front of it sits where it does without a limit
};

template <int EPL> struct PxVec;
template <> struct PxVec<8> { typedef u32x4 T; };
template <> struct PxVec<4> { typedef u32x2 T; };

// ROWS query rows (A-operand rows; this lane's row fr = lane & 15 reads its 8-element fragments from qrow, nullptr = a zero row) against nkeys
// K / V rows of HD elements at kbase / vbase.  On return sh.m_run / sh.l_run hold the running max and sum of every row, and
// sh.sbuf[(w * ROWS + r) * HD + dd], w = 0 .. 3, the four per-wave partial sums of the unnormalised output (relative to m_run); a __syncthreads()
// has been passed.  nkeys <= 0: m = -1e30, l = 0, o = 0.
// LIM: row r sees the keys [0, sh.lim[r]) only (sh.lim written by the caller, with a __syncthreads() behind it, before the call; lim[r] <= nkeys).
// A score at or past the row's limit takes no part in the row's maximum and its probability is an exact 0.  A row with lim 0: m = -1e30, l = 0, o = 0.
template <int HD, int ROWS, bool LIM = false>
__device__ __forceinline__ void px_attend(PxShared<HD, ROWS, LIM>& sh, const bf16_t* __restrict__ qrow, const bf16_t* __restrict__ kbase,
                                          const bf16_t* __restrict__ vbase, int nkeys, float scale) {
    static_assert((HD == 64 || HD == 128) && (ROWS == 8 || ROWS == 16), "head_dim 64 / 128, 8 or 16 operand rows");
    // phase C: a group of LPG lanes takes a V row, EPL head-dim elements per lane, and keeps ROWS x EPL accumulators.  16 rows x 8 elements would be
    // 128 accumulator registers (one wave per SIMD, or spills): the 16-row tile at HD = 128 takes 4 elements per lane - 32-lane groups, 8-byte loads
    constexpr int EPL = (HD == 128 && ROWS == 8) ? 8 : 4, KS = HD / 32;
    constexpr int LPG = HD / EPL, NG = 256 / LPG;               // lanes per key group (16 / 32), key groups per block (16 / 8)
    typedef typename PxVec<EPL>::T vrow_t;
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
    for (int c0 = 0; c0 < nkeys; c0 += PX_CH) {
        const int cn = min(PX_CH, nkeys - c0);
        __syncthreads();                                  // previous chunk's probabilities consumed, m_run / l_run visible
        // ---- A: scores on the matrix pipe.  Wave w takes the 16-key tiles w, w + 4, ...; K rows go straight into B-fragment shape (lane (key = l & 15,
        // g = l >> 4) reads the 16 bytes at d = 32 ks + 8 g of its key row), two tiles per trip with all loads issued before the first MFMA; keys beyond
        // the chunk are clamped and not stored
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
        // the first trip of V rows of phase C is requested here: it flies under phase B (barriers and exponentials, no memory traffic)
        constexpr int RPT = 4;                                  // V rows per trip (8 at 4 elements per lane spilled the 16-row tile)
        const int rounds = (cn + NG - 1) / NG;
        vrow_t vw[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int jc = min(u * NG + grp, cn - 1);
            vw[u] = __builtin_nontemporal_load(reinterpret_cast<const vrow_t*>(vb + (long)(c0 + jc) * HD));
        }
        // ---- B: per-row chunk max -> running max, p = exp(s - m) in place, running sum.  Thread t serves row t % ROWS, keys t / ROWS + k * (256 / ROWS)
        // (LIM: the max over the row's VISIBLE keys, p = 0 for a key the row may not see)
        {
            const int g = tid & (ROWS - 1);
            constexpr int KSTEP = 256 / ROWS;
            int vis = cn;                                       // visible keys of row g inside this chunk (<= 0: none)
            if constexpr (LIM) vis = min(sh.lim[g] - c0, cn);
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
                float pv;
                if constexpr (LIM) pv = j < vis ? __expf(sbuf[j * ROWS + g] - m_new) : 0.f;
                else pv = __expf(sbuf[j * ROWS + g] - m_new);
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
        // ---- C: rescale (once per chunk) and accumulate P.V: each key group takes a V row and the row's ROWS probabilities (broadcast LDS reads)
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
                // the scheduler otherwise hoists the probability reads of ALL rows of the trip above the first product (RPT x ROWS registers: spills)
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

template <int HD, int ROWS, bool LIM>
__device__ __forceinline__ float px_osum(const PxShared<HD, ROWS, LIM>& sh, int idx) {
    return (sh.sbuf[idx] + sh.sbuf[ROWS * HD + idx]) + (sh.sbuf[2 * ROWS * HD + idx] + sh.sbuf[3 * ROWS * HD + idx]);
}

// the (head_dim, H / Hk) combinations the users of px_attend are instantiated and tested for
bool px_supported(int H, int Hk, int d) {
    if (Hk <= 0 || H <= 0 || H % Hk) return false;
    const int g = H / Hk;
    return (d == 64 || d == 128) && (g == 1 || g == 2 || g == 4 || g == 7 || g == 8);
}

}  // namespace
