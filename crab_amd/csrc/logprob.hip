// Per-token log-probabilities of the decode loop: how sure the model was of the token the select kernel chose.  What HF gives with
// output_scores = True + compute_transition_scores(normalize_logits = True) - without a [B, V] clone per step and without a host sync, so the
// step stays capturable in a HIP graph.  Two numbers per row b and step, from the RAW fp32 logits z = logits[b] and the chosen token y:
//   logprob         = z[y] - logsumexp(z[0 .. V))                       the model's own log-probability (what score() gives teacher-forced)
//   logprob_allowed = z[y] - logsumexp(z[i] : i allowed at this step)   renormalised within the set the select kernels choose from:
//                     every token but EOS while step < min_new_tokens, or - with a token trie - the out-edges of the row's node under
//                     constrain.hip's edge_ok rule (token in [0, V), not the suppressed EOS), the node taken BEFORE the step moves it.
// Temperature, top-k and top-p enter neither number: they are a drawing device of sample mode, not a statement of the model.
//
// Two launches around the select (the select kernels are not touched):
//   logprob_norm   (before): one block of 1024 threads per row -> norm[b] = (lse_raw, lse_allowed, live, 0).  `live` is read from finished[b]
//                  BEFORE the select sets it, so the step that emits EOS is a real token even when pad_id == eos_id; it is false as well when
//                  nothing is allowed (the trie's sink, a corrupt node).
//   logprob_gather (after, before crab_advance): one thread per row -> lp[0][b][step] = z[y] - lse_raw, lp[1][b][step] = z[y] - lse_allowed;
//                  both 0.0f for a row that was not live or whose token lies outside [0, V); nothing when step >= n_steps.
//
// The row pass reads the row ONCE (at 512 x 152 064 a second read is another 311 MB): every thread keeps an online (max, sum) pair - a
// running maximum that rescales the sum - over 16-byte loads from the first 16-byte boundary of the row on, with a scalar head and tail (any
// base pointer and any ldl).  Two sums side by side: all tokens, and all tokens but the suppressed EOS.  The pair of a thread holds the
// allowed tokens; the suppressed EOS, which exactly one thread meets, is kept as a term of its own and ADDED to the all-tokens sum in the
// merge - the allowed sum is a sum of its own under a maximum of its own, never S - exp(z_eos - max), which cancels (and underflows) when
// EOS dominates.  expf per element in fp32; the 1024 partials are rescaled to the block maximum and added in double in a fixed order (the
// wave butterfly, then the 16 wave sums in order, as xent_finish_kernel), lse = max + log(sum) is rounded once to fp32.  No float atomics:
// two runs give the same bits.  With a trie the allowed normaliser is a gather over the node's edges instead, every index clamped exactly as
// constrained_select_kernel clamps it (node against n_nodes, the edge range against n_edges, edge_tok against V).
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

typedef float lp_f32x4 __attribute__((ext_vector_type(4)));

struct OnlineLse {                                              // sum of exp(x - m) under the running maximum m
    float m, s;
    __device__ __forceinline__ void add(float x) {
        if (x > m) { s = (m == -INFINITY) ? 0.f : s * expf(m - x); m = x; }
        if (x != -INFINITY) s += expf(x - m);
    }
};

// max + log(sum) of the block's 1024 pairs, in double, fixed order; extra: one more term exp(extra) (-inf: none).  Every thread gets the result.
__device__ __forceinline__ double block_lse(OnlineLse a, float extra, float* shf, double* shd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float mx = a.m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    __syncthreads();
    if (lane == 0) shf[wave] = mx;
    __syncthreads();
    mx = shf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, shf[w]);
    const float top = fmaxf(mx, extra);
    double s = (a.s > 0.f) ? (double)a.s * exp((double)a.m - (double)top) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) shd[wave] = s;
    __syncthreads();
    double t = shd[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += shd[w];
    if (extra != -INFINITY) t += exp((double)extra - (double)top);
    return (double)top + log(t);
}

__global__ __launch_bounds__(1024) void logprob_norm_kernel(const float* __restrict__ logits, long ldl, int V, const int* __restrict__ edge_off,
                                                            const int* __restrict__ edge_tok, int n_nodes, int n_edges,
                                                            const int* __restrict__ node, const int* __restrict__ step_dev,
                                                            const int* __restrict__ finished, int eos_id, int min_new, float* __restrict__ norm) {
    __shared__ float shf[16];
    __shared__ double shd[16];
    __shared__ float sh_eos;
    __shared__ int shi[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = step_dev[0];
    const int suppress = (eos_id >= 0 && step < min_new) ? eos_id : -1;
    const float* row = logits + (long)b * ldl;
    if (tid == 0) sh_eos = -INFINITY;
    __syncthreads();
    // ---- the one pass over the row: scalar head up to the first 16-byte boundary, 16-byte loads, scalar tail
    const int head = min(V, (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u));
    const int nvec = (V - head) >> 2;
    const int tail0 = head + (nvec << 2);
    OnlineLse a{-INFINITY, 0.f};
    float z_sup = -INFINITY;                                     // the suppressed EOS logit, seen by exactly one thread
    if (tid < head) { const float x = row[tid]; if (tid == suppress) z_sup = x; else a.add(x); }
    const lp_f32x4* rv = reinterpret_cast<const lp_f32x4*>(row + head);
    for (int i = tid; i < nvec; i += 1024) {
        const lp_f32x4 v = rv[i];
        const int c0 = head + (i << 2);
        float x0 = v[0], x1 = v[1], x2 = v[2], x3 = v[3];
        if ((unsigned)(suppress - c0) < 4u) {                    // the chunk that holds the suppressed EOS: take it out of the pair
            const int j = suppress - c0;
            z_sup = j == 0 ? x0 : j == 1 ? x1 : j == 2 ? x2 : x3;
            if (j == 0) x0 = -INFINITY; else if (j == 1) x1 = -INFINITY; else if (j == 2) x2 = -INFINITY; else x3 = -INFINITY;
        }
        const float cm = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));     // one rescale per chunk
        if (cm > a.m) { a.s = (a.m == -INFINITY) ? 0.f : a.s * expf(a.m - cm); a.m = cm; }
        if (cm != -INFINITY) {
            a.s += (x0 != -INFINITY ? expf(x0 - a.m) : 0.f) + (x1 != -INFINITY ? expf(x1 - a.m) : 0.f);
            a.s += (x2 != -INFINITY ? expf(x2 - a.m) : 0.f) + (x3 != -INFINITY ? expf(x3 - a.m) : 0.f);
        }
    }
    { const int i = tail0 + tid; if (i < V) { const float x = row[i]; if (i == suppress) z_sup = x; else a.add(x); } }
    if (z_sup != -INFINITY) sh_eos = z_sup;                      // at most one writer (after the barrier inside block_lse it is visible)
    const double lse_alw_row = block_lse(a, -INFINITY, shf, shd);
    const float zs = sh_eos;
    const double lse_raw = block_lse(a, zs, shf, shd);
    double lse_alw = lse_alw_row;
    int n_ok = V - ((suppress >= 0 && suppress < V) ? 1 : 0);
    if (edge_off != nullptr) {
        // ---- trie: the allowed normaliser is a gather over the node's edges (constrained_select_kernel's clamps)
        const int nd = node[b];
        int e0 = 0, e1 = 0;
        if (nd >= 0 && nd < n_nodes) {
            e0 = min(max(edge_off[nd], 0), n_edges);
            e1 = min(max(edge_off[nd + 1], e0), n_edges);
        }
        const int n = e1 - e0;
        const int* etok = edge_tok + e0;
        OnlineLse g{-INFINITY, 0.f};
        int cnt = 0;
        for (int i = tid; i < n; i += 1024) {
            const int t = etok[i];
            if (t >= 0 && t < V && t != suppress) { g.add(row[t]); ++cnt; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if ((tid & 63) == 0) shi[tid >> 6] = cnt;
        lse_alw = block_lse(g, -INFINITY, shf, shd);              // its barriers publish shi
        n_ok = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) n_ok += shi[w];
    }
    if (tid == 0) {
        const bool live = !finished[b] && n_ok > 0;
        float* o = norm + (long)b * 4;
        o[0] = (float)lse_raw;
        o[1] = n_ok > 0 ? (float)lse_alw : 0.f;
        o[2] = live ? 1.f : 0.f;
        o[3] = 0.f;
    }
}

__global__ __launch_bounds__(256) void logprob_gather_kernel(const float* __restrict__ logits, long ldl, int B, int V, const int64_t* __restrict__ cur_ids,
                                                             const int* __restrict__ step_dev, const float* __restrict__ norm,
                                                             float* __restrict__ lp, long ld_lp, long plane, int n_steps) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int step = step_dev[0];
    if (b >= B || step < 0 || step >= n_steps) return;
    const int64_t y = cur_ids[b];
    const float* nb = norm + (long)b * 4;
    float l0 = 0.f, l1 = 0.f;
    if (nb[2] != 0.f && y >= 0 && y < (int64_t)V) {
        const float z = logits[(long)b * ldl + y];
        l0 = z - nb[0];
        l1 = z - nb[1];
    }
    lp[(long)b * ld_lp + step] = l0;
    lp[plane + (long)b * ld_lp + step] = l1;
}

}  // namespace

extern "C" int crab_logprob_norm(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, const int32_t* edge_off,
                                 const int32_t* edge_tok, int n_nodes, int n_edges, const int32_t* node, const int32_t* step_dev,
                                 const int32_t* finished, int eos_id, int min_new_tokens, float* norm) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !step_dev || !finished || !norm || B <= 0 || V <= 0 || ldl < 0) return crab_fail(ctx, CRAB_E_INVALID, "logprob_norm: bad argument");
    if ((edge_off || edge_tok || node) && (!edge_off || !edge_tok || !node || n_nodes <= 0 || n_edges <= 0))
        return crab_fail(ctx, CRAB_E_INVALID, "logprob_norm: edge_off, edge_tok and node come together, with n_nodes >= 1 and n_edges >= 1");
    if ((uintptr_t)logits & 3) return crab_fail(ctx, CRAB_E_INVALID, "logprob_norm: logits must be 4-byte aligned");
    hipLaunchKernelGGL(logprob_norm_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, edge_off, edge_tok, n_nodes, n_edges, node,
                       step_dev, finished, eos_id, min_new_tokens, norm);
    return crab_check_launch(ctx, "logprob_norm");
}

extern "C" int crab_logprob_gather(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, const int64_t* cur_ids,
                                   const int32_t* step_dev, const float* norm, float* lp, int64_t ld_lp, int64_t plane_stride, int n_steps) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !cur_ids || !step_dev || !norm || !lp || B <= 0 || V <= 0 || ldl < 0) return crab_fail(ctx, CRAB_E_INVALID, "logprob_gather: bad argument");
    if (n_steps <= 0 || ld_lp < n_steps || plane_stride < 0) return crab_fail(ctx, CRAB_E_INVALID, "logprob_gather: n_steps >= 1, ld_lp >= n_steps, plane_stride >= 0");
    hipLaunchKernelGGL(logprob_gather_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, (long)ldl, B, V, cur_ids, step_dev, norm,
                       lp, (long)ld_lp, (long)plane_stride, n_steps);
    return crab_check_launch(ctx, "logprob_gather");
}
