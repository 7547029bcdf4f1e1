// Constrained selection step of the decode loop: the next token of every row is chosen among the out-edges of the row's node in a token trie
// (crab_amd/constrain.py: a forest of answer sets flattened to CSR, the EOS edge of every end of sequence materialised by the host), and
// the row's node follows the chosen edge.  What HF does with PrefixConstrainedLogitsProcessor (transformers generation/logits_process.py:
// every token the callback does not return is set to -inf; MinNewTokensLength masks EOS before it; the warpers see what is left) - without a
// host callback, so the step stays capturable in a HIP graph.  One block per row, 1024 threads; the logits are read only through the edge
// list (a gather of at most `edges` values, never a scan of V) and never written.
//   * greedy   : greedy_select_kernel's rule over edge indices (larger value wins, on equal values the lower edge = the lower token id);
//   * sampling : sample_select_kernel's algorithm with the edge index in the place of the token index - the same 1024-way partition
//                (chunk = ceil(n / 1024)), the same bisections, the same fixed-order block_sum and the same generator, so a node whose edges
//                are all V tokens in order draws exactly what crab_sample_select draws.  fkey and block_sum are select_core.h's; the
//                pipeline is a copy of select_draw, not an instantiation: as one (bit-identical, scripts/ab_bits.py select) the kernel
//                needed 52 registers instead of 70, two blocks fitted a CU, and 512 rows on a 1000-edge node took 324 us instead of 254
//                (V = 32000) and 585 instead of 340 (V = 152064); held to one block per CU it was still 7 - 15 % slower at 1, 42 and 1000
//                edges (scripts/bench_constrained.py, parent-to-parent spread under 1 %).
// Every index taken from device memory is clamped against the sizes the launch was given (node against n_nodes, the edge range against
// n_edges, edge_tok against V): a bad entry is "not allowed", a corrupt array gives a wrong token and never an out-of-bounds access.
#include "common.h"
#include "crab_internal.h"
#include "select_core.h"
#include <math.h>

namespace {

// edge i of the row's node: allowed iff its token lies in [0, V) and is not the suppressed EOS
__device__ __forceinline__ bool edge_ok(const int* __restrict__ etok, int i, int V, int suppress, int* tok) {
    const int t = etok[i];
    *tok = t;
    return t >= 0 && t < V && t != suppress;
}

__global__ __launch_bounds__(1024) void constrained_select_kernel(const float* __restrict__ logits, long ldl, int V, const int* __restrict__ edge_off,
                                                                  const int* __restrict__ edge_tok, const int* __restrict__ edge_dst, int n_nodes,
                                                                  int n_edges, int* __restrict__ node, int64_t* __restrict__ cur_ids,
                                                                  int64_t* __restrict__ out_ids, long ld_out, const int* __restrict__ step_dev,
                                                                  int* __restrict__ finished, int eos_id, int pad_id, int min_new, float inv_t,
                                                                  int top_k, float top_p, unsigned long long seed) {
    __shared__ float shf[16];
    __shared__ int shi[16];
    __shared__ float pre[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = step_dev[0];
    if (finished[b]) {                                           // uniform over the block; a finished row keeps its node
        if (tid == 0) { cur_ids[b] = pad_id; out_ids[(long)b * ld_out + step] = pad_id; }
        return;
    }
    const int suppress = (eos_id >= 0 && step < min_new) ? eos_id : -1;
    const float* row = logits + (long)b * ldl;
    const int nd = node[b];
    int e0 = 0, e1 = 0;
    if (nd >= 0 && nd < n_nodes) {
        e0 = min(max(edge_off[nd], 0), n_edges);
        e1 = min(max(edge_off[nd + 1], e0), n_edges);
    }
    const int n = e1 - e0;
    const int* etok = edge_tok + e0;
    int pick = -1;                                               // thread 0: the chosen edge of the node, -1 = nothing allowed
    if (inv_t == 0.f) {
        // ---- greedy: first maximum over the allowed edges
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 1024) {
            int t;
            if (!edge_ok(etok, i, V, suppress, &t)) continue;
            const float v = row[t];
            if (v > best || (v == best && i < bi) || bi == 0x7fffffff) { best = v; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { shf[tid >> 6] = best; shi[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 16; ++w)
                if (shi[w] != 0x7fffffff && (bi == 0x7fffffff || shf[w] > best || (shf[w] == best && shi[w] < bi))) { best = shf[w]; bi = shi[w]; }
            pick = bi == 0x7fffffff ? -1 : bi;
        }
    } else {
        // ---- sampling: sample_select_kernel over the edge index
        const int chunk = (n + 1023) / 1024, i0 = min(n, tid * chunk), i1 = min(n, i0 + chunk);
        int tk_;
#define EOK(i_) edge_ok(etok, (i_), V, suppress, &tk_)
#define XVAL(i_) (EOK(i_) ? __fmul_rn(row[tk_], inv_t) : -INFINITY)
        float mx = -INFINITY;
        int first_ok = 0x7fffffff;
        for (int i = i0; i < i1; ++i) {
            const bool ok = EOK(i);
            if (ok) { mx = fmaxf(mx, __fmul_rn(row[tk_], inv_t)); first_ok = min(first_ok, i); }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); first_ok = min(first_ok, __shfl_xor(first_ok, o, 64)); }
        if ((tid & 63) == 0) { shf[tid >> 6] = mx; shi[tid >> 6] = first_ok; }
        __syncthreads();
        mx = shf[0]; first_ok = shi[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) { mx = fmaxf(mx, shf[w]); first_ok = min(first_ok, shi[w]); }
        // ---- top-k: tk = key of the k-th largest value
        uint32_t tk = 0u;
        if (top_k > 0 && top_k < n) {
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
        // ---- draw inside the kept set {key >= tp}
        float mine = 0.f;
        for (int i = i0; i < i1; ++i) { const float x = XVAL(i); if (fkey(x) >= tp) mine += __expf(x - mx); }
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
            // walk the owner's range (owner is the last non-empty range when rounding pushed r past the total); only an allowed edge is taken
            if (owner >= 0) {
                const int j0 = min(n, owner * chunk), j1 = min(n, j0 + chunk);
                for (int i = j0; i < j1; ++i) {
                    const bool ok = EOK(i);
                    if (!ok) continue;
                    const float x = __fmul_rn(row[tk_], inv_t);
                    if (fkey(x) >= tp) { pick = i; acc += __expf(x - mx); if (acc > r) break; }
                }
            }
            // no mass at all (every allowed logit at -inf): the first allowed edge, as the first-maximum rule gives
            if (pick < 0 && first_ok != 0x7fffffff) pick = first_ok;
        }
#undef XVAL
#undef EOK
    }
    if (tid == 0) {
        int tok = pad_id;
        if (pick >= 0 && pick < n) {
            tok = etok[pick];
            node[b] = edge_dst[e0 + pick];
            if (eos_id >= 0 && tok == eos_id) finished[b] = 1;
        } else {
            finished[b] = 1;                                     // nothing allowed (the sink, or a corrupt entry): pad from here on
        }
        cur_ids[b] = tok;
        out_ids[(long)b * ld_out + step] = tok;
    }
}

}  // namespace

extern "C" int crab_constrained_select(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, const int32_t* edge_off,
                                       const int32_t* edge_tok, const int32_t* edge_dst, int n_nodes, int n_edges, int32_t* node,
                                       int64_t* cur_ids, int64_t* out_ids, int64_t ld_out, const int32_t* step_dev, int32_t* finished, int eos_id,
                                       int pad_id, int min_new_tokens, float temperature, int top_k, float top_p, uint64_t seed) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !edge_off || !edge_tok || !edge_dst || !node || !cur_ids || !out_ids || !step_dev || !finished || B <= 0 || V <= 0 || ldl < 0 ||
        n_nodes <= 0 || n_edges <= 0)
        return crab_fail(ctx, CRAB_E_INVALID, "constrained_select: bad argument");
    if (!(temperature >= 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0)
        return crab_fail(ctx, CRAB_E_INVALID, "constrained_select: temperature >= 0 (0 = greedy), 0 < top_p <= 1, top_k >= 0");
    hipLaunchKernelGGL(constrained_select_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, edge_off, edge_tok, edge_dst, n_nodes,
                       n_edges, node, cur_ids, out_ids, (long)ld_out, step_dev, finished, eos_id, pad_id, min_new_tokens,
                       temperature > 0.f ? 1.0f / temperature : 0.f, top_k, top_p, (unsigned long long)seed);
    return crab_check_launch(ctx, "constrained_select");
}
