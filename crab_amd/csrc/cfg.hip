// Classifier-free guidance of the decode step (generate(guidance_scale = g, negative_inputs...)): HF's
// UnbatchedClassifierFreeGuidanceLogitsProcessor - "visual contrastive decoding" when the negative prompt is the question without its clip -
// without the second model forward from a Python callback, which cannot run between two replays of a captured step.  The conditional and
// the unconditional prompt of a clip are two ROWS of one ragged decode batch: pair b < B is row b (conditional, c) and row B + b
// (unconditional, u) of the raw fp32 logits [2B, V]; the weights stream once per step for both.  Two launches around the select (the select
// kernels are not touched; they read `guided` instead of the logits and write the first B rows' words):
//   cfg_mix    (before): one block of 1024 threads per pair ->
//                  guided[b, i] = lu + g * (lc - lu),   lc = c[i] - lse(c),   lu = u[i] - lse(u)
//              HF's scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond).  `guided` is a buffer of its own: the raw logits
//              are never written, so return_step_logits keeps reporting what the lm_head produced.
//   cfg_follow (after, before crab_advance): one thread per pair -> the unconditional row takes the pair's token, output column and finished
//              flag, so both rows embed the same token at the next step and the step loop's EOS check sees 2B agreeing flags.
//
// cfg_mix is a pure stream: pass 1 reads both rows once with logprob.hip's online (max, sum) pair - 16-byte loads from the row's first 16-byte
// boundary on, scalar head and tail, any 4-byte aligned base and any ldl -, the 1024 partials are merged in double in logprob.hip's fixed
// order (wave butterfly, then the 16 wave sums in order) and each lse is rounded ONCE to fp32; pass 2 re-reads both rows and writes the
// guided row with 16-byte stores from ITS first 16-byte boundary on (the loads of a row whose columns do not share that alignment are typed
// 4-byte aligned and left to the compiler).  5 V floats move per pair; at V = 152 064 the two rows are 1.2 MB per block, so with hundreds of
// blocks in flight the second read comes from L2 only in part.  No float atomics: two runs give the same bits.
//
// Edge cases.  An element that is -inf in EITHER row gives -inf (HF computes -inf - -inf = NaN where both are; a token that one of the two
// distributions excludes stays excluded here - a deliberate deviation).  NaN propagates: a NaN logit makes its row's lse NaN, as
// torch.log_softmax does, and every element of the pair that is not -inf comes out NaN.
// A pair whose finished[b] is set is NOT skipped: greedy_select_kernel and sample_select_kernel scan the whole row of a finished sequence
// as well (only thread 0's last lines look at finished[b], to emit pad_id instead of the result), so they do read a finished row's scores;
// a skipped pair would hand them the previous step's values - harmless for the ids, but `guided` would then depend on history.  `finished`
// stays in the signature for a select that stops reading such rows.
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

typedef float cfg_f32x4 __attribute__((ext_vector_type(4)));
typedef float cfg_f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte access at any 4-byte boundary

struct OnlineLse {                                              // sum of exp(x - m) under the running maximum m (logprob.hip)
    float m, s;
    __device__ __forceinline__ void add(float x) {
        if (x > m) { s = (m == -INFINITY) ? 0.f : s * expf(m - x); m = x; }
        if (x != -INFINITY) s += expf(x - m);
    }
};

// logprob.hip's block_lse without the extra term: max + log(sum) of the block's 1024 pairs, in double, fixed order; every thread gets the
// result.  One difference: a NaN partial sum is kept (there `a.s > 0.f` drops it), so a NaN logit reaches the lse.
__device__ __forceinline__ double block_lse(OnlineLse a, float* shf, double* shd) {
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
    double s = !(a.s <= 0.f) ? (double)a.s * exp((double)a.m - (double)mx) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) shd[wave] = s;
    __syncthreads();
    double t = shd[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += shd[w];
    return (double)mx + log(t);
}

// the one pass over a row of logprob_norm_kernel: scalar head up to the first 16-byte boundary, 16-byte loads, scalar tail
__device__ __forceinline__ OnlineLse row_partial(const float* __restrict__ row, int V, int tid) {
    const int head = min(V, (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u));
    const int nvec = (V - head) >> 2;
    const int tail0 = head + (nvec << 2);
    OnlineLse a{-INFINITY, 0.f};
    if (tid < head) a.add(row[tid]);
    const cfg_f32x4* rv = reinterpret_cast<const cfg_f32x4*>(row + head);
    for (int i = tid; i < nvec; i += 1024) {
        const cfg_f32x4 v = rv[i];
        const float x0 = v[0], x1 = v[1], x2 = v[2], x3 = v[3];
        const float cm = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));     // one rescale per chunk
        if (cm > a.m) { a.s = (a.m == -INFINITY) ? 0.f : a.s * expf(a.m - cm); a.m = cm; }
        if (cm != -INFINITY) {
            a.s += (x0 != -INFINITY ? expf(x0 - a.m) : 0.f) + (x1 != -INFINITY ? expf(x1 - a.m) : 0.f);
            a.s += (x2 != -INFINITY ? expf(x2 - a.m) : 0.f) + (x3 != -INFINITY ? expf(x3 - a.m) : 0.f);
        }
    }
    { const int i = tail0 + tid; if (i < V) a.add(row[i]); }
    return a;
}

__device__ __forceinline__ float mix1(float c, float u, float lse_c, float lse_u, float g) {
    if (c == -INFINITY || u == -INFINITY) return -INFINITY;
    const float lc = c - lse_c, lu = u - lse_u;
    return __fmaf_rn(g, lc - lu, lu);
}

template <typename LoadT>
__device__ __forceinline__ void mix_chunks(const float* __restrict__ c, const float* __restrict__ u, float* __restrict__ g, int nvec, int tid,
                                           float lse_c, float lse_u, float scale) {
    const LoadT* cv = reinterpret_cast<const LoadT*>(c);
    const LoadT* uv = reinterpret_cast<const LoadT*>(u);
    cfg_f32x4* gv = reinterpret_cast<cfg_f32x4*>(g);
    for (int i = tid; i < nvec; i += 1024) {
        const cfg_f32x4 x = cv[i], y = uv[i];
        cfg_f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = mix1(x[j], y[j], lse_c, lse_u, scale);
        gv[i] = o;
    }
}

__global__ __launch_bounds__(1024) void cfg_mix_kernel(const float* __restrict__ logits, long ldl, int B, int V, float scale,
                                                       float* __restrict__ guided, long ldg) {
    __shared__ float shf[16];
    __shared__ double shd[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* c = logits + (long)b * ldl;
    const float* u = logits + (long)(B + b) * ldl;
    float* g = guided + (long)b * ldg;
    // ---- pass 1: both normalisers, each rounded once
    const OnlineLse pc = row_partial(c, V, tid);
    const OnlineLse pu = row_partial(u, V, tid);
    const float lse_c = (float)block_lse(pc, shf, shd);
    const float lse_u = (float)block_lse(pu, shf, shd);
    // ---- pass 2: the guided row, 16-byte stores from its own first 16-byte boundary on
    const int head = min(V, (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u));
    const int nvec = (V - head) >> 2;
    const int tail0 = head + (nvec << 2);
    if (tid < head) g[tid] = mix1(c[tid], u[tid], lse_c, lse_u, scale);
    if (((((uintptr_t)(c + head)) | ((uintptr_t)(u + head))) & 15u) == 0)
        mix_chunks<cfg_f32x4>(c + head, u + head, g + head, nvec, tid, lse_c, lse_u, scale);
    else
        mix_chunks<cfg_f32x4_a4>(c + head, u + head, g + head, nvec, tid, lse_c, lse_u, scale);
    { const int i = tail0 + tid; if (i < V) g[i] = mix1(c[i], u[i], lse_c, lse_u, scale); }
}

__global__ __launch_bounds__(256) void cfg_follow_kernel(int64_t* __restrict__ cur_ids, int64_t* __restrict__ out_ids, long ld_out, int n_steps,
                                                         int* __restrict__ finished, const int* __restrict__ step_dev, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int step = step_dev[0];
    if (b >= B || step < 0 || step >= n_steps) return;
    cur_ids[B + b] = cur_ids[b];
    out_ids[(long)(B + b) * ld_out + step] = out_ids[(long)b * ld_out + step];
    finished[B + b] = finished[b];
}

}  // namespace

extern "C" int crab_cfg_mix(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, float guidance_scale,
                            const int32_t* finished, float* guided, int64_t ldg) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !finished || !guided || B < 1 || V < 1) return crab_fail(ctx, CRAB_E_INVALID, "cfg_mix: bad argument");
    if (ldl < V || ldg < V) return crab_fail(ctx, CRAB_E_INVALID, "cfg_mix: ldl >= V and ldg >= V (2B logits rows are read, B guided rows written)");
    if (((uintptr_t)logits | (uintptr_t)guided) & 3) return crab_fail(ctx, CRAB_E_INVALID, "cfg_mix: logits and guided must be 4-byte aligned");
    if (!(guidance_scale == guidance_scale)) return crab_fail(ctx, CRAB_E_INVALID, "cfg_mix: guidance_scale is NaN");
    hipLaunchKernelGGL(cfg_mix_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, B, V, guidance_scale, guided, (long)ldg);
    return crab_check_launch(ctx, "cfg_mix");
}

extern "C" int crab_cfg_follow(crab_ctx* ctx, void* stream, int64_t* cur_ids, int64_t* out_ids, int64_t ld_out, int n_steps, int32_t* finished,
                               const int32_t* step_dev, int B) {
    if (!ctx) return CRAB_E_INVALID;
    if (!cur_ids || !out_ids || !finished || !step_dev || B < 1) return crab_fail(ctx, CRAB_E_INVALID, "cfg_follow: bad argument");
    if (n_steps < 1 || ld_out < n_steps) return crab_fail(ctx, CRAB_E_INVALID, "cfg_follow: n_steps >= 1, ld_out >= n_steps");
    hipLaunchKernelGGL(cfg_follow_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, cur_ids, out_ids, (long)ld_out, n_steps, finished,
                       step_dev, B);
    return crab_check_launch(ctx, "cfg_follow");
}
