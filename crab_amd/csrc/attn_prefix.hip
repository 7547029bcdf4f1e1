// Decode / suffix attention over a SHARED PREFIX plus an own cache (modeling_llama.py:394-445 on the keys [prefix of the clip ; own keys of the row]).
// Several questions about one clip share everything up to the question text: the prefix K/V of a clip is stored once, [C, Hk, Tp, d], and read once
// per (clip, kv head, tile of query rows) instead of once per row; every row keeps only its own keys (question + decoded tokens) in [B, Hk, Tmax, d].
//
//   attn_prefix_partial_kernel (K1)  one block per (tile, kv head).  A tile is up to 16 / (H / Hk) query rows of ONE clip, each with the H / Hk query
//       heads of the kv head: the (row, head) pairs are the rows of the MFMA A operand, as attn_decode_gqa_kernel (attn.hip) puts its heads there -
//       H == Hk: 16 sibling rows, H / Hk == 7: two siblings x 7 heads.  All P prefix keys are visible to every query (every query sits at a position
//       >= P).  Output per (query row, head), fp32, into the caller's workspace: the unnormalised o[d], the running max m and the sum l.
//       The loop is px_attend (attn_rows_core.h), shared with K2's general form and with attn_verify.hip.
//   attn_own_merge_row_kernel (K2, H == Hk, one query per row)  attn_decode_kernel (attn.hip) over the row's own keys, from the same streaming loop
//       (HD = 128; the HD = 64 loop is a copy) and group merge (attn_decode_core.h), then the merge.
//   attn_own_merge_kernel (K2, every other form)  one block per (row, kv head, query index): the H / Hk heads as A-operand rows over the own keys -
//       every own K / V row is read once per kv head - then the merge.
// The merge is the log-sum-exp rule in a fixed order (own part, then prefix part): the result is a function of the inputs alone, no atomics, no tickets.
#include "common.h"
#include "crab_internal.h"
#include "attn_decode_core.h"
#include "attn_rows_core.h"
#include <math.h>

namespace {

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
