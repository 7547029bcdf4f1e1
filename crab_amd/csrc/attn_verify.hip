// Verify-step attention of prompt-lookup speculative decoding (HF generation/utils.py _assisted_decoding: one forward over [current token ; k draft
// tokens] of ONE sequence; modeling_llama.py:394-445 with the causal mask of the k + 1 new positions): Sq <= 16 queries of a sequence over its cache,
// query i seeing the slots kv_start .. ctx - 1 + i.  The queries are MFMA A-operand rows, as the sibling rows of a clip are in
// attn_prefix_partial_kernel (attn_prefix.hip): one block per (sequence, kv head, group of 16 / (H / Hk) queries), every K / V row up to the group's
// last visible slot read ONCE per block - crab_attn_decode launched Sq times, or attn_own_merge_kernel with its block per query, read the cache Sq
// times.  The causal tail is a per-row key limit: a score at or past the row's limit takes no part in the row's maximum and its probability is an
// exact 0 (not exp of a masked score), so whatever a later query's slot holds cannot reach an earlier query; slots past the group's last visible one
// are never read.  No atomics, fixed reduction order: the output is a function of the inputs alone.
//
// The loop is px_attend (attn_rows_core.h) with LIM = true, the per-row limit of its phase B; the shared-prefix and beam kernels instantiate the same
// loop without it.  Built with -mllvm -amdgpu-mfma-vgpr-form like attn_prefix.hip (build.sh).
#include "common.h"
#include "crab_internal.h"
#include "attn_rows_core.h"
#include <math.h>

namespace {

// grid (Hk, B, query groups).  Group z holds the queries z * per .. of sequence b, per = 16 / (H / Hk) (ROWS == 8: the launcher found all Sq
// queries' heads in 8 operand rows, one group).  Operand row r = query (r / GH) of the group, head hk * GH + r % GH.
template <int HD, int ROWS>
__global__ __launch_bounds__(256, 2) void attn_verify_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, bf16_t* __restrict__ o, long ldo, int H, int Hk, int Tmax,
                                                          int Sq, int per, int ctx_host, const int* __restrict__ ctx_dev, float scale,
                                                          const int* __restrict__ kv_start) {
    __shared__ PxShared<HD, ROWS, true> sh;
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
    px_attend<HD, ROWS, true>(sh, qrow, kc + kv0, vc + kv0, nkeys, scale);
    const int nvalid = nq * GH;
    for (int idx = threadIdx.x; idx < nvalid * HD; idx += 256) {
        const int r = idx / HD, dd = idx - r * HD;
        const int s2 = r / GH, h2 = hk * GH + (r - s2 * GH);
        const float L = sh.l_run[r];
        const float O = (sh.sbuf[idx] + sh.sbuf[ROWS * HD + idx]) + (sh.sbuf[2 * ROWS * HD + idx] + sh.sbuf[3 * ROWS * HD + idx]);
        o[((long)b * Sq + i0 + s2) * ldo + (long)h2 * HD + dd] = f2bf(L > 0.f ? O / L : 0.f);      // an empty range gives 0, as attn_decode_kernel
    }
}

}  // namespace

extern "C" int crab_attn_verify(crab_ctx* ctx, void* stream, const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, void* o,
                                int64_t ldo, int B, int Sq, int H, int Hk, int d, int Tmax, int ctx_len_host, const int32_t* ctx_dev, float scale,
                                const int32_t* kv_start) {
    if (!ctx) return CRAB_E_INVALID;
    if (!px_supported(H, Hk, d)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "attn_verify: head_dim 64 / 128 with H / Hk in {1, 2, 4, 7, 8}");
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
