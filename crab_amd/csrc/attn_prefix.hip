// Decode / suffix attention over a SHARED PREFIX plus an own cache (modeling_llama.py:394-445 on the keys [prefix of the clip ; own keys of the row]).
// Several questions about one clip share everything up to the question text: the prefix K/V of a clip is stored once, [C, Hk, Tp, d], and read once
// per (clip, kv head, tile of query rows) instead of once per row; every row keeps only its own keys (question + decoded tokens) in [B, Hk, Tmax, d].
//
//   attn_prefix_partial_kernel (K1)  one block per (tile, kv head).  A tile is up to 16 / (H / Hk) query rows of ONE clip, each with the H / Hk query
//       heads of the kv head: the (row, head) pairs are the rows of the MFMA A operand, as attn_decode_gqa_kernel (attn.hip) puts its heads there -
//       H == Hk: 16 sibling rows, H / Hk == 7: two siblings x 7 heads.  All P prefix keys are visible to every query (every query sits at a position
//       >= P).  Output per (query row, head), fp32, into the caller's workspace: the unnormalised o[d], the running max m and the sum l.
//   attn_own_merge_row_kernel (K2, H == Hk, one query per row)  attn_decode_kernel (attn.hip) over the row's own keys, from the same streaming loop
//       (HD = 128; the HD = 64 loop is a copy) and group merge (attn_decode_core.h), then the merge.
//   attn_own_merge_kernel (K2, every other form)  one block per (row, kv head, query index): the H / Hk heads as A-operand rows over the own keys -
//       every own K / V row is read once per kv head - then the merge.
// The merge is the log-sum-exp rule in a fixed order (own part, then prefix part): the result is a function of the inputs alone, no atomics, no tickets.
#include "common.h"
#include "crab_internal.h"
#include "attn_decode_core.h"
#include <math.h>

namespace {

constexpr int PX_CH = 512;                                      // keys per chunk (scores of a chunk live in LDS)

// Shared state of one tile pass.  sbuf: scores [PX_CH][ROWS] fp32 during the chunks, the merge buffer [4 waves][ROWS][HD] at the end.
template <int HD, int ROWS>
struct PxShared {
    static constexpr int SMEM_F = (4 * ROWS * HD > PX_CH * ROWS) ? 4 * ROWS * HD : PX_CH * ROWS;
    __attribute__((aligned(16))) float sbuf[SMEM_F];
    float red[4][ROWS];
    float m_run[ROWS], l_run[ROWS], alpha_s[ROWS];
};

template <int EPL> struct PxVec;
template <> struct PxVec<8> { typedef u32x4 T; };
template <> struct PxVec<4> { typedef u32x2 T; };

// ROWS query rows (A-operand rows; this lane's row fr = lane & 15 reads its 8-element fragments from qrow, nullptr = a zero row) against nkeys
// K / V rows of HD elements at kbase / vbase.  On return sh.m_run / sh.l_run hold the running max and sum of every row, and
// sh.sbuf[(w * ROWS + r) * HD + dd], w = 0 .. 3, the four per-wave partial sums of the unnormalised output (relative to m_run); a __syncthreads()
// has been passed.  nkeys <= 0: m = -1e30, l = 0, o = 0.
template <int HD, int ROWS>
__device__ __forceinline__ void px_attend(PxShared<HD, ROWS>& sh, const bf16_t* __restrict__ qrow, const bf16_t* __restrict__ kbase,
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
        {
            const int g = tid & (ROWS - 1);
            constexpr int KSTEP = 256 / ROWS;
            float mx = -1e30f;
#pragma unroll 1
            for (int j = tid / ROWS; j < cn; j += KSTEP) mx = fmaxf(mx, sbuf[j * ROWS + g]);
            if (ROWS == 8) mx = fmaxf(mx, row_xor8(mx));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (lane < ROWS) sh.red[wave][lane] = mx;
            __syncthreads();
            const float m_old = sh.m_run[g];
            const float m_new = fmaxf(fmaxf(fmaxf(sh.red[0][g], sh.red[1][g]), fmaxf(sh.red[2][g], sh.red[3][g])), m_old);
            float sum = 0.f;
#pragma unroll 1
            for (int j = tid / ROWS; j < cn; j += KSTEP) {
                const float pv = __expf(sbuf[j * ROWS + g] - m_new);
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

template <int HD, int ROWS>
__device__ __forceinline__ float px_osum(const PxShared<HD, ROWS>& sh, int idx) {
    return (sh.sbuf[idx] + sh.sbuf[ROWS * HD + idx]) + (sh.sbuf[2 * ROWS * HD + idx] + sh.sbuf[3 * ROWS * HD + idx]);
}

// K1.  grid (tiles, Hk).  tile_rows[2 t], tile_rows[2 t + 1]: first query row and number of query rows of tile t (all of one clip: row_clip[first]).
// A tile outside [0, rows) or a clip outside [0, C) is skipped (nothing is read or written for it).
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_prefix_partial_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ pk,
                                                                  const bf16_t* __restrict__ pv, float* __restrict__ ws,
                                                                  const int* __restrict__ tile_rows, const int* __restrict__ row_clip, int rows,
                                                                  int C, int H, int Hk, int Tp, int P, float scale) {
    __shared__ PxShared<HD, 16> sh;
    const int GH = H / Hk, per = 16 / GH;
    const int t = blockIdx.x, hk = blockIdx.y;
    const int row0 = tile_rows[2 * t];
    const int nr = min(tile_rows[2 * t + 1], per);
    if (row0 < 0 || nr <= 0 || row0 + nr > rows) return;
    const int c = row_clip[row0];
    if (c < 0 || c >= C) return;
    const int fr = threadIdx.x & 15;
    const int sib = fr / GH, hd = fr - sib * GH;
    const bf16_t* qrow = sib < nr ? q + (long)(row0 + sib) * ldq + (long)(hk * GH + hd) * HD : nullptr;
    const long kv0 = ((long)c * Hk + hk) * (long)Tp * HD;
    px_attend<HD, 16>(sh, qrow, pk + kv0, pv + kv0, P, scale);
    const int nvalid = nr * GH;
    for (int idx = threadIdx.x; idx < nvalid * HD; idx += 256) {
        const int r = idx / HD, dd = idx - r * HD;
        const int s2 = r / GH, h2 = hk * GH + (r - s2 * GH);
        float* w = ws + ((long)(row0 + s2) * H + h2) * (HD + 2);
        w[dd] = px_osum<HD, 16>(sh, idx);
        if (dd == 0) { w[HD] = sh.m_run[r]; w[HD + 1] = sh.l_run[r]; }
    }
}

// out = merge(own part (M, L, O), prefix part (ws row)): own first, prefix second
__device__ __forceinline__ float px_merge(float M, float L, float O, float mp, float lp, float op) {
    const float Mt = fmaxf(M, mp);
    const float wa = __expf(M - Mt), wb = __expf(mp - Mt);
    return (O * wa + op * wb) / (L * wa + lp * wb);
}

// K2, general form.  grid (Hk, B, Sq).  Query i of sequence b (row b * Sq + i of q / o / ws) sees its own slots kv_start[b] .. ctx - 1 + i.
template <int HD, int ROWS>
__global__ __launch_bounds__(256, 2) void attn_own_merge_kernel(const bf16_t* __restrict__ q, long ldq, const float* __restrict__ ws,
                                                             const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                                                             bf16_t* __restrict__ o, long ldo, int H, int Hk, int Tmax, int Sq, int ctx_host,
                                                             const int* __restrict__ ctx_dev, float scale, const int* __restrict__ kv_start) {
    __shared__ PxShared<HD, ROWS> sh;
    const int GH = H / Hk;
    const int hk = blockIdx.x, b = blockIdx.y, i = blockIdx.z;
    const long row = (long)b * Sq + i;
    const int ks0 = max(kv_start ? kv_start[b] : 0, 0);
    const int last = min(ctx_host + (ctx_dev ? ctx_dev[0] : 0) + i, Tmax);      // one past the last visible slot, never past the cache
    const int fr = threadIdx.x & 15;
    const bf16_t* qrow = fr < GH ? q + row * ldq + (long)(hk * GH + fr) * HD : nullptr;
    const long kv0 = (((long)b * Hk + hk) * (long)Tmax + ks0) * HD;
    px_attend<HD, ROWS>(sh, qrow, kc + kv0, vc + kv0, last - ks0, scale);
    for (int idx = threadIdx.x; idx < GH * HD; idx += 256) {
        const int r = idx / HD, dd = idx - r * HD;
        const int h2 = hk * GH + r;
        const float* w = ws + (row * H + h2) * (HD + 2);
        o[row * ldo + (long)h2 * HD + dd] = f2bf(px_merge(sh.m_run[r], sh.l_run[r], px_osum<HD, ROWS>(sh, idx), w[HD], w[HD + 1], w[dd]));
    }
}

// K2, H == Hk and one query per row: attn_decode_kernel (attn.hip) over the row's own keys - the same dec_stream / dec_group_merge
// (attn_decode_core.h: 16 groups of 16 lanes, group g takes keys g, g + 16, ..., two keys per trip with the next pair in flight at HD = 128) behind
// this kernel's own clamps of kv_start and ctx - then the merge with the prefix partial instead of the plain O / L.  grid (H, B).
template <int HD>
__global__ __launch_bounds__(256) void attn_own_merge_row_kernel(const bf16_t* __restrict__ q, long ldq, const float* __restrict__ ws,
                                                                 const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                                                                 bf16_t* __restrict__ o, long ldo, int H, int Tmax, int ctx_host,
                                                                 const int* __restrict__ ctx_dev, float scale, const int* __restrict__ kv_start) {
    constexpr int EPL = HD / 16;
    const int tid = threadIdx.x;
    const int grp = tid >> 4, sub = tid & 15;
    const int b = blockIdx.y, h = blockIdx.x;
    const int ks0 = max(kv_start ? kv_start[b] : 0, 0);
    const int ctx = min(ctx_host + (ctx_dev ? ctx_dev[0] : 0), Tmax) - ks0;
    const bf16_t* qp = q + (long)b * ldq + (long)h * HD + sub * EPL;
    float qv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) qv[e] = bf2f(qp[e]) * scale;
    const bf16_t* kb = kc + (((long)b * H + h) * (long)Tmax + ks0) * HD + sub * EPL;
    const bf16_t* vb = vc + (((long)b * H + h) * (long)Tmax + ks0) * HD + sub * EPL;
    float m = -1e30f, l = 0.f, acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    if constexpr (EPL == 8) {
        dec_stream(qv, kb, vb, ctx, grp, m, l, acc);
    } else {
        // HD = 64 (the tiny test models): one key per trip, the dot summed element by element.  Kept here, not in the header: moved into dec_stream
        // the compiler fused the other product of acc * a + pw * v and outputs differed from before in the last bit (scripts/ab_bits.py, volume cases)
        for (int j = grp; j < ctx; j += 16) {
            float kx[EPL], vx[EPL];
            const u32x2 kw = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(kb + (long)j * HD));
            const u32x2 vw = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(vb + (long)j * HD));
#pragma unroll
            for (int e = 0; e < 2; ++e) { kx[2 * e] = lo_bf(kw[e]); kx[2 * e + 1] = hi_bf(kw[e]); vx[2 * e] = lo_bf(vw[e]); vx[2 * e + 1] = hi_bf(vw[e]); }
            float sdot = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) sdot += qv[e] * kx[e];
            sdot = row16_sum(sdot);
            const float mn = fmaxf(m, sdot);
            const float a = __expf(m - mn), pw = __expf(sdot - mn);
            l = l * a + pw;
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] = acc[e] * a + pw * vx[e];
            m = mn;
        }
    }
    float M, L, O;
    dec_group_merge<HD, 16, EPL>(grp, sub, m, l, acc, M, L, O);
    if (tid < HD) {
        const float* w = ws + ((long)b * H + h) * (HD + 2);
        o[(long)b * ldo + (long)h * HD + tid] = f2bf(px_merge(M, L, O, w[HD], w[HD + 1], w[tid]));
    }
}

// the (head_dim, H / Hk) combinations both kernels are instantiated and tested for
bool px_supported(int H, int Hk, int d) {
    if (Hk <= 0 || H <= 0 || H % Hk) return false;
    const int g = H / Hk;
    return (d == 64 || d == 128) && (g == 1 || g == 2 || g == 4 || g == 7 || g == 8);
}

}  // namespace

extern "C" int64_t crab_attn_prefix_workspace(int rows, int H, int d) {
    if (rows <= 0 || H <= 0 || d <= 0) return 0;
    return (int64_t)rows * H * (d + 2) * 4;
}

extern "C" int crab_attn_prefix_partial(crab_ctx* ctx, void* stream, const void* q, int64_t ldq, const void* prefix_k, const void* prefix_v,
                                        void* workspace, int64_t workspace_bytes, const int32_t* tile_rows, int ntiles, const int32_t* row_clip,
                                        int rows, int C, int H, int Hk, int d, int Tp, int P, float scale) {
    if (!ctx) return CRAB_E_INVALID;
    if (!px_supported(H, Hk, d)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_prefix_partial: head_dim 64 / 128 with H / Hk in {1, 2, 4, 7, 8}");
    if (!q || !prefix_k || !prefix_v || !tile_rows || !row_clip || rows <= 0 || C <= 0 || ntiles <= 0 || ntiles > rows)
        return crab_fail(ctx, CRAB_E_INVALID, "attn_prefix_partial: bad argument");
    if (P <= 0 || P > Tp) return crab_fail(ctx, CRAB_E_INVALID, "attn_prefix_partial: 1 <= P <= Tp");
    if ((ldq & 7) || ((uintptr_t)q & 15) || ((uintptr_t)prefix_k & 15) || ((uintptr_t)prefix_v & 15) || ((uintptr_t)workspace & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "attn_prefix_partial: alignment");
    if (!workspace || workspace_bytes < crab_attn_prefix_workspace(rows, H, d))
        return crab_fail(ctx, CRAB_E_WORKSPACE, "attn_prefix_partial: needs crab_attn_prefix_workspace(rows, H, d) bytes");
    dim3 grid(ntiles, Hk), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (d == 128)
        hipLaunchKernelGGL((attn_prefix_partial_kernel<128>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const bf16_t*)prefix_k,
                           (const bf16_t*)prefix_v, (float*)workspace, tile_rows, row_clip, rows, C, H, Hk, Tp, P, scale);
    else
        hipLaunchKernelGGL((attn_prefix_partial_kernel<64>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const bf16_t*)prefix_k,
                           (const bf16_t*)prefix_v, (float*)workspace, tile_rows, row_clip, rows, C, H, Hk, Tp, P, scale);
    return crab_check_launch(ctx, d == 128 ? "attn_prefix_partial_kernel<128>" : "attn_prefix_partial_kernel<64>");
}

extern "C" int crab_attn_own_merge(crab_ctx* ctx, void* stream, const void* q, int64_t ldq, const void* workspace, int64_t workspace_bytes,
                                   const void* k_cache, const void* v_cache, void* o, int64_t ldo, int B, int Sq, int H, int Hk, int d, int Tmax,
                                   int ctx_len_host, const int32_t* ctx_dev, float scale, const int32_t* kv_start) {
    if (!ctx) return CRAB_E_INVALID;
    if (!px_supported(H, Hk, d)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_own_merge: head_dim 64 / 128 with H / Hk in {1, 2, 4, 7, 8}");
    if (!q || !k_cache || !v_cache || !o || B <= 0 || Sq <= 0 || Sq > 65535 || B > 65535 || Tmax <= 0)
        return crab_fail(ctx, CRAB_E_INVALID, "attn_own_merge: bad argument");
    if (!ctx_dev && (ctx_len_host < 0 || ctx_len_host + Sq - 1 > Tmax)) return crab_fail(ctx, CRAB_E_INVALID, "attn_own_merge: ctx_len out of range");
    if ((ldq & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) || ((uintptr_t)workspace & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "attn_own_merge: alignment");
    if (!workspace || workspace_bytes < crab_attn_prefix_workspace(B * Sq, H, d))
        return crab_fail(ctx, CRAB_E_WORKSPACE, "attn_own_merge: needs the crab_attn_prefix_workspace(B * Sq, H, d) bytes crab_attn_prefix_partial filled");
    dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
    const int G = H / Hk;
    if (G == 1 && Sq == 1) {
        dim3 grid(H, B);
        if (d == 128)
            hipLaunchKernelGGL((attn_own_merge_row_kernel<128>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const float*)workspace,
                               (const bf16_t*)k_cache, (const bf16_t*)v_cache, (bf16_t*)o, (long)ldo, H, Tmax, ctx_len_host, ctx_dev, scale, kv_start);
        else
            hipLaunchKernelGGL((attn_own_merge_row_kernel<64>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const float*)workspace,
                               (const bf16_t*)k_cache, (const bf16_t*)v_cache, (bf16_t*)o, (long)ldo, H, Tmax, ctx_len_host, ctx_dev, scale, kv_start);
        return crab_check_launch(ctx, d == 128 ? "attn_own_merge_row_kernel<128>" : "attn_own_merge_row_kernel<64>");
    }
    dim3 grid(Hk, B, Sq);
    if (d == 128)
        hipLaunchKernelGGL((attn_own_merge_kernel<128, 8>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const float*)workspace,
                           (const bf16_t*)k_cache, (const bf16_t*)v_cache, (bf16_t*)o, (long)ldo, H, Hk, Tmax, Sq, ctx_len_host, ctx_dev, scale, kv_start);
    else
        hipLaunchKernelGGL((attn_own_merge_kernel<64, 8>), grid, block, 0, s, (const bf16_t*)q, (long)ldq, (const float*)workspace,
                           (const bf16_t*)k_cache, (const bf16_t*)v_cache, (bf16_t*)o, (long)ldo, H, Hk, Tmax, Sq, ctx_len_host, ctx_dev, scale, kv_start);
    return crab_check_launch(ctx, d == 128 ? "attn_own_merge_kernel<128>" : "attn_own_merge_kernel<64>");
}
