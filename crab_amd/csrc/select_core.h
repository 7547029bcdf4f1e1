// The sampling pipeline of the decode step, once: sample_select_kernel and sample_select_warped_kernel (sample.hip) are its two instantiations.
// One block of 1024 threads per row, no sort:
//   max -> top-k bisection -> Z -> top-p bisection -> [WARP: min_p, epsilon_cutoff, eta_cutoff] -> per-thread mass -> draw -> owner walk
// The pipeline sees the row through ITEMS (float operator()(int i) const: the scaled value of item i, -inf for an item that may not be chosen,
// NaN-free otherwise) and returns the chosen item; the kernel does the rest.  The warped kernel with its stages off performs the plain kernel's
// operations in its order.  fkey / block_sum / block_min are shared with constrained_select_kernel (constrain.hip), which keeps a pipeline of
// its own over the out-edges of a trie node (the reason is in its header).
// No fused multiply-add anywhere in the pipeline: a product that feeds a sum rounds on its own in every instantiation.
#pragma once
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ uint32_t fkey(float f) {            // order-preserving float -> uint (NaN-free input)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {            // 1024 threads, fixed tree: deterministic
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

struct SelectShared {
    __attribute__((aligned(16))) float pre[1024];               // per-thread mass of the kept set (thread 0 scans it with 16-byte reads)
    float shf[16];
    int shi[16];
    uint32_t shu[16];
    int pick;
};

// the three further truncation stages of the warped kernel (0 = off) and its two optional outputs
struct SelectWarp {
    float min_p, eps_cut, eta_cut;
    int* kept_n;
    float* kept_min;
};

// The chosen item of row b among items 0 .. n - 1, returned to EVERY thread (a __syncthreads() has been passed); -1: no item carries mass (n == 0,
// or every value at -inf).  Deterministic for a given (seed, step, b).
template <bool WARP, typename ITEMS>
__device__ __forceinline__ int select_draw(SelectShared& sh, const ITEMS& xval, int n, int b, int step, int top_k, float top_p,
                                           unsigned long long seed, const SelectWarp& wp = SelectWarp{}) {
    float* shf = sh.shf;
    int* shi = sh.shi;
    const int tid = threadIdx.x;
    const int chunk = (n + 1023) / 1024, i0 = tid * chunk, i1 = min(n, i0 + chunk);
    float mx = -INFINITY;
    for (int i = i0; i < i1; ++i) mx = fmaxf(mx, xval(i));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) shf[tid >> 6] = mx;
    __syncthreads();
    mx = shf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, shf[w]);
    // ---- top-k: tk = key of the k-th largest value
    uint32_t tk = 0u;
    if (top_k > 0 && top_k < n) {
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = tk | (1u << bit);
            int c = 0;
            for (int i = i0; i < i1; ++i) c += fkey(xval(i)) >= cand;
            if (block_sum<int>(c, shi) >= top_k) tk = cand;
        }
    }
    float z = 0.f;
    for (int i = i0; i < i1; ++i) { const float x = xval(i); if (fkey(x) >= tk) z += __expf(x - mx); }
    const float Z = block_sum<float>(z, shf);
    // ---- top-p: tp = largest key whose mass (within the top-k set) is >= top_p * Z
    uint32_t tp = tk;
    if (top_p < 1.0f) {
        const float need = top_p * Z;
        uint32_t t = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            float m = 0.f;
            for (int i = i0; i < i1; ++i) { const float x = xval(i); const uint32_t k = fkey(x); if (k >= cand && k >= tk) m += __expf(x - mx); }
            if (block_sum<float>(m, shf) >= need) t = cand;
        }
        tp = t > tk ? t : tk;
    }
    // ---- WARP, the three further stages (HF's MinPLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper, in that order).  With w_i = __expf(x_i - mx)
    // (w of the maximum is exactly 1) and Z, S sums over the CURRENT set {key >= tp} - every stage sees the distribution renormalised over what
    // the stages before it kept:
    //   min_p   : HF removes p_i < min_p * p_max                                   <=> keep  w_i >= min_p                  (no sum needed)
    //   epsilon : HF removes p_i < eps                                             <=> keep  w_i >= eps * Z                (one block sum)
    //   eta     : HF removes p_i < min(eps, sqrt(eps) * exp(-H)), H = -sum p ln p;   ln p_i = d_i - ln Z with d_i = x_i - mx, so
    //             H = ln Z - S / Z with S = sum w_i d_i (same pass as Z; an item without mass contributes 0, as torch's Categorical has it)
    //             and exp(-H) = exp(S / Z) / Z                                     <=> keep  w_i >= min(eps * Z, sqrt(eps) * exp(S / Z))
    // No per-item logarithm.  Every stage keeps an upper set {x >= t}, so the state stays ONE integer key: a stage narrows tp to the smallest key
    // of {key >= tp, w >= floor}, never past the maximum's key (min_tokens_to_keep = 1: the maximum and its exact ties always stay).  An item at
    // -inf has w = 0 and passes no stage.  Their passes own no ranges - nothing is drawn from them - so lanes read neighbouring items: i = tid,
    // tid + 1024, ...; a thread still sums at most ceil(n / 1024) terms before the fixed tree, which is what the margin of tests/warp_ref.py counts
    if constexpr (WARP) {
        const uint32_t kmax = fkey(mx);
        auto narrow = [&](float floor_w) {
            uint32_t km = 0xFFFFFFFFu;
            for (int i = tid; i < n; i += 1024) { const float x = xval(i); const uint32_t k = fkey(x); if (k >= tp && __expf(x - mx) >= floor_w) km = min(km, k); }
            km = min(block_min(km, sh.shu), kmax);
            tp = km > tp ? km : tp;
        };
        if (wp.min_p > 0.f) narrow(wp.min_p);
        if (wp.eps_cut > 0.f) {
            float zz = 0.f;
            for (int i = tid; i < n; i += 1024) { const float x = xval(i); if (fkey(x) >= tp) zz += __expf(x - mx); }
            const float Zc = block_sum<float>(zz, shf);
            narrow(wp.eps_cut * Zc);
        }
        if (wp.eta_cut > 0.f) {
            float zz = 0.f, ss = 0.f;
            for (int i = tid; i < n; i += 1024) {
                const float x = xval(i);
                if (fkey(x) >= tp) { const float d = x - mx, w = __expf(d); zz += w; if (w > 0.f) ss += w * d; }
            }
            const float Zc = block_sum<float>(zz, shf);
            const float Sc = block_sum<float>(ss, shf);
            narrow(fminf(wp.eta_cut * Zc, sqrtf(wp.eta_cut) * __expf(Sc / Zc)));
        }
    }
    // ---- draw inside the kept set {key >= tp}
    float mine = 0.f;
    int cnt = 0;
    uint32_t kmin = 0xFFFFFFFFu;
    for (int i = i0; i < i1; ++i) {
        const float x = xval(i);
        const uint32_t k = fkey(x);
        if (k >= tp) {
            mine += __expf(x - mx);
            if constexpr (WARP) { ++cnt; kmin = min(kmin, k); }
        }
    }
    if constexpr (WARP) {
        if (wp.kept_n != nullptr || wp.kept_min != nullptr) {      // the set the draw below walks, item for item
            const int nk = block_sum<int>(cnt, shi);
            const uint32_t km = block_min(kmin, sh.shu);
            if (tid == 0) {
                if (wp.kept_n != nullptr) wp.kept_n[b] = nk;
                if (wp.kept_min != nullptr) wp.kept_min[b] = fkey_inv(km);
            }
        }
    }
    __syncthreads();
    sh.pre[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(step + 1) + 0xD1B54A32D192ED03ull * (unsigned long long)(b + 1);
        s = (s ^ (s >> 30)) * 0xBF58476D1CE4E5B9ull; s = (s ^ (s >> 27)) * 0x94D049BB133111EBull; s ^= s >> 31;     // splitmix64 finaliser
        const float u01 = (float)(s >> 40) * (1.0f / 16777216.0f);
        float total = 0.f;
        for (int t = 0; t < 1024; ++t) total += sh.pre[t];
        const float r = u01 * total;
        float acc = 0.f, acc_owner = 0.f;
        int owner = -1;
        for (int t = 0; t < 1024; ++t) {
            if (sh.pre[t] > 0.f) { owner = t; acc_owner = acc; if (acc + sh.pre[t] > r) break; acc += sh.pre[t]; }
        }
        acc = acc_owner;
        // walk the owner's range (owner is the last non-empty range when rounding pushed r past the total).  No owner - no item with mass - walks
        // nothing: owner * chunk would lie in front of item 0
        int pick = -1;
        const int j0 = owner * chunk, j1 = owner < 0 ? j0 : min(n, j0 + chunk);
        for (int i = j0; i < j1; ++i) {
            const float x = xval(i);
            if (fkey(x) >= tp) { pick = i; acc += __expf(x - mx); if (acc > r) break; }
        }
        sh.pick = pick;
    }
    __syncthreads();
    return sh.pick;
}

}  // namespace
