// Sampling step with HF's three further truncation warpers (generation/logits_process.py: MinPLogitsWarper, EpsilonLogitsWarper,
// EtaLogitsWarper), in HF's order (GenerationMixin._get_logits_processor):
//   temperature -> top-k -> top-p -> min_p -> epsilon_cutoff -> eta_cutoff -> softmax -> draw
// sample_select_kernel (sample.hip) with three more stages between its top-p bisection and its draw.  Every stage keeps an upper set
// {x >= t} of the scaled logits, so the state stays what it is there: ONE integer key tp, the draw is the same code, and with all three
// stages off this kernel runs sample_select_kernel's operations in its order - the ids are equal bit for bit (tests/test_warp_gpu.py).
// sample.hip itself is not touched and not routed through here: its object, and with it every result of crab_sample_select, stays what
// it was.  The copied expressions must round as they do there (its code holds no fused multiply-add), hence the pragma below.
//
// With w_i = __expf(x_i - mx) (w of the maximum is exactly 1) and Z, S sums over the CURRENT set {key >= tp} - every stage sees the
// distribution renormalised over what the stages before it kept:
//   min_p   : HF removes p_i < min_p * p_max                                   <=> keep  w_i >= min_p                  (no sum needed)
//   epsilon : HF removes p_i < eps                                             <=> keep  w_i >= eps * Z                (one block sum)
//   eta     : HF removes p_i < min(eps, sqrt(eps) * exp(-H)), H = -sum p ln p;   ln p_i = d_i - ln Z with d_i = x_i - mx, so
//             H = ln Z - S / Z with S = sum w_i d_i (same pass as Z; a token without mass contributes 0, as torch's Categorical has it)
//             and exp(-H) = exp(S / Z) / Z                                     <=> keep  w_i >= min(eps * Z, sqrt(eps) * exp(S / Z))
// No per-token logarithm.  A stage then takes the smallest key among the tokens that pass (one block min) as the new tp; the maximum and
// its exact ties always stay (min_tokens_to_keep = 1: HF keeps `scores >= the largest`).  A token at -inf has w = 0 and passes no stage.
// A row without a finite token (mx = -inf, every w NaN) passes nothing anywhere and emits token 0, as sample_select_kernel does.
// Cost: 1 (min_p) + 2 (epsilon) + 2 (eta) passes over the row next to the 67 of the two bisections, + 1 when kept_n / kept_min are wanted.
#include "common.h"
#include "crab_internal.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ uint32_t fkey(float f) {            // order-preserving float -> uint (NaN-free input)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {            // 1024 threads, fixed tree: deterministic (sample.hip's, term for term)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    T t = sh[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += sh[w];
    return t;
}

__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    uint32_t t = sh[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t = min(t, sh[w]);
    return t;
}

__global__ __launch_bounds__(1024) void sample_select_warped_kernel(const float* __restrict__ logits, long ldl, int V, int64_t* __restrict__ cur_ids,
                                                                    int64_t* __restrict__ out_ids, long ld_out, const int* __restrict__ step_dev,
                                                                    int* __restrict__ finished, int eos_id, int pad_id, int min_new, float inv_t,
                                                                    int top_k, float top_p, unsigned long long seed, float min_p, float eps_cut,
                                                                    float eta_cut, int* __restrict__ kept_n, float* __restrict__ kept_min) {
    __shared__ float shf[16];
    __shared__ int shi[16];
    __shared__ uint32_t shu[16];
    __shared__ float pre[1024];
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = step_dev[0];
    const int suppress = (eos_id >= 0 && step < min_new) ? eos_id : -1;
    const float* row = logits + (long)b * ldl;
    const int chunk = (V + 1023) / 1024, i0 = tid * chunk, i1 = min(V, i0 + chunk);
#define XVAL(i_) ((i_) == suppress ? -INFINITY : row[i_] * inv_t)
    float mx = -INFINITY;
    for (int i = i0; i < i1; ++i) mx = fmaxf(mx, XVAL(i));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) shf[tid >> 6] = mx;
    __syncthreads();
    mx = shf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, shf[w]);
    // ---- top-k: tk = key of the k-th largest value
    uint32_t tk = 0u;
    if (top_k > 0 && top_k < V) {
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = tk | (1u << bit);
            int c = 0;
            for (int i = i0; i < i1; ++i) c += fkey(XVAL(i)) >= cand;
            if (block_sum<int>(c, shi) >= top_k) tk = cand;
        }
    }
    float z = 0.f;
    for (int i = i0; i < i1; ++i) { const float x = XVAL(i); if (fkey(x) >= tk) z += __expf(x - mx); }
    const float Z = block_sum<float>(z, shf);
    // ---- top-p: tp = largest key whose mass (within the top-k set) is >= top_p * Z
    uint32_t tp = tk;
    if (top_p < 1.0f) {
        const float need = top_p * Z;
        uint32_t t = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            float m = 0.f;
            for (int i = i0; i < i1; ++i) { const float x = XVAL(i); const uint32_t k = fkey(x); if (k >= cand && k >= tk) m += __expf(x - mx); }
            if (block_sum<float>(m, shf) >= need) t = cand;
        }
        tp = t > tk ? t : tk;
    }
    // ---- the three further stages: each one narrows tp to the smallest key of {key >= tp, w >= floor}, never past the maximum's key
    // (their passes own no ranges - nothing is drawn from them - so lanes read neighbouring tokens: i = tid, tid + 1024, ...; a thread still
    // sums at most ceil(V / 1024) terms before the fixed tree, which is what the margin of tests/warp_ref.py counts)
    const uint32_t kmax = fkey(mx);
#define NARROW(floor_)                                                                                                             \
    {                                                                                                                              \
        const float fl_ = (floor_);                                                                                                \
        uint32_t km = 0xFFFFFFFFu;                                                                                                 \
        for (int i = tid; i < V; i += 1024) { const float x = XVAL(i); const uint32_t k = fkey(x); if (k >= tp && __expf(x - mx) >= fl_) km = min(km, k); } \
        km = min(block_min(km, shu), kmax);                                                                                        \
        tp = km > tp ? km : tp;                                                                                                    \
    }
    if (min_p > 0.f) NARROW(min_p)
    if (eps_cut > 0.f) {
        float zz = 0.f;
        for (int i = tid; i < V; i += 1024) { const float x = XVAL(i); if (fkey(x) >= tp) zz += __expf(x - mx); }
        const float Zc = block_sum<float>(zz, shf);
        NARROW(eps_cut * Zc)
    }
    if (eta_cut > 0.f) {
        float zz = 0.f, ss = 0.f;
        for (int i = tid; i < V; i += 1024) {
            const float x = XVAL(i);
            if (fkey(x) >= tp) { const float d = x - mx, w = __expf(d); zz += w; if (w > 0.f) ss += w * d; }
        }
        const float Zc = block_sum<float>(zz, shf);
        const float Sc = block_sum<float>(ss, shf);
        NARROW(fminf(eta_cut * Zc, sqrtf(eta_cut) * __expf(Sc / Zc)))
    }
#undef NARROW
    // ---- draw inside the kept set {key >= tp}
    float mine = 0.f;
    int cnt = 0;
    uint32_t kmin = 0xFFFFFFFFu;
    for (int i = i0; i < i1; ++i) {
        const float x = XVAL(i);
        const uint32_t k = fkey(x);
        if (k >= tp) { mine += __expf(x - mx); ++cnt; kmin = min(kmin, k); }
    }
    if (kept_n != nullptr || kept_min != nullptr) {                // the set the draw below walks, token for token
        const int n = block_sum<int>(cnt, shi);
        const uint32_t km = block_min(kmin, shu);
        if (tid == 0) {
            if (kept_n != nullptr) kept_n[b] = n;
            if (kept_min != nullptr) kept_min[b] = fkey_inv(km);
        }
    }
    __syncthreads();
    pre[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(step + 1) + 0xD1B54A32D192ED03ull * (unsigned long long)(b + 1);
        s = (s ^ (s >> 30)) * 0xBF58476D1CE4E5B9ull; s = (s ^ (s >> 27)) * 0x94D049BB133111EBull; s ^= s >> 31;     // splitmix64 finaliser
        const float u01 = (float)(s >> 40) * (1.0f / 16777216.0f);
        float total = 0.f;
        for (int t = 0; t < 1024; ++t) total += pre[t];
        const float r = u01 * total;
        float acc = 0.f, acc_owner = 0.f;
        int owner = -1;
        for (int t = 0; t < 1024; ++t) {
            if (pre[t] > 0.f) { owner = t; acc_owner = acc; if (acc + pre[t] > r) break; acc += pre[t]; }
        }
        acc = acc_owner;
        // walk the owner's range (owner is the last non-empty range when rounding pushed r past the total; no owner - a row without a
        // finite token - is token 0, what sample_select_kernel ends on, without its walk of the range in front of the row)
        int tok = -1;
        const int j0 = owner * chunk, j1 = owner < 0 ? j0 : min(V, j0 + chunk);
        for (int i = j0; i < j1; ++i) {
            const float x = XVAL(i);
            if (fkey(x) >= tp) { tok = i; acc += __expf(x - mx); if (acc > r) break; }
        }
        s_tok = tok < 0 ? 0 : tok;
    }
    __syncthreads();
    if (tid == 0) {
        int tok = finished[b] ? pad_id : s_tok;
        if (eos_id >= 0 && tok == eos_id) finished[b] = 1;
        cur_ids[b] = tok;
        out_ids[(long)b * ld_out + step] = tok;
    }
#undef XVAL
}

}  // namespace

extern "C" int crab_sample_select_warped(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, int64_t* cur_ids,
                                         int64_t* out_ids, int64_t ld_out, const int32_t* step_dev, int32_t* finished, int eos_id, int pad_id,
                                         int min_new_tokens, float temperature, int top_k, float top_p, uint64_t seed, float min_p,
                                         float epsilon_cutoff, float eta_cutoff, int32_t* kept_n, float* kept_min) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !cur_ids || !out_ids || !step_dev || !finished || B <= 0 || V <= 0) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_warped: bad argument");
    if (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_warped: temperature > 0, 0 < top_p <= 1, top_k >= 0");
    if (!(min_p >= 0.f && min_p <= 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_warped: 0 <= min_p <= 1 (0 = off)");
    if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_warped: 0 <= epsilon_cutoff < 1 (0 = off)");
    if (!(eta_cutoff >= 0.f && eta_cutoff < 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_warped: 0 <= eta_cutoff < 1 (0 = off)");
    hipLaunchKernelGGL(sample_select_warped_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, cur_ids, out_ids, (long)ld_out,
                       step_dev, finished, eos_id, pad_id, min_new_tokens, 1.0f / temperature, top_k, top_p, (unsigned long long)seed, min_p,
                       epsilon_cutoff, eta_cutoff, kept_n, kept_min);
    return crab_check_launch(ctx, "sample_select_warped");
}
