// Sampling step of the decode loop (the reference never passes do_sample, so HF applies the checkpoint's generation_config: Llama-2-chat
// ships do_sample = true, temperature 0.6, top_p 0.9, and GenerationConfig's default top_k = 50; scripts/quick_start.py:36-43,
// SURVEY.md appendix A.7).  HF order (transformers 4.37.2 generation/utils.py _get_logits_warper, logits_process.py): temperature ->
// top-k -> top-p -> softmax -> multinomial.  One block per row, no sort:
//   * top-k : the k-th largest scaled logit by a 32-step bisection on the order-preserving integer image of the floats (exact);
//   * top-p : TopPLogitsWarper removes, in ascending order, the tokens whose cumulative probability stays <= 1 - top_p, i.e. it keeps
//             token i iff the mass of the strictly larger tokens is < top_p: the kept set is {x >= t} for the largest t whose mass is
//             >= top_p, found by the same bisection on masses;
//   * draw  : u ~ U[0,1) from a counter-based generator keyed by (seed, step, row); threads own contiguous index ranges, a block scan
//             finds the range, its owner walks it.  Deterministic for a given seed; torch.multinomial's stream cannot be reproduced,
//             parity is distributional (tests/test_ops_gpu.py).
// EOS / min_new_tokens / finished-row bookkeeping as greedy_select_kernel (ops.hip).
// sample_select_warped_kernel is the same pipeline with HF's three further truncation warpers (generation/logits_process.py: MinPLogitsWarper,
// EpsilonLogitsWarper, EtaLogitsWarper) between the top-p bisection and the draw, in HF's order (GenerationMixin._get_logits_processor):
//   temperature -> top-k -> top-p -> min_p -> epsilon_cutoff -> eta_cutoff -> softmax -> draw
// Both kernels are instantiations of select_draw (select_core.h, where the stages are described): with all three stages off the warped kernel
// runs the plain kernel's operations in its order and the ids are equal bit for bit (tests/test_warp_gpu.py).  A row without a finite token
// (mx = -inf, every weight NaN) passes nothing anywhere and both kernels emit token 0.
// sample_select_rows_kernel<WARP> (crab_sample_select_rows) is either of the two with one more operand, row_ids: block r works on row r of every
// buffer and hands row_ids[r] to select_draw as the row of the draw's key - the rows of a wave that shed its finished rows (csrc/kv_compact.hip)
// keep the random streams they had.  Same select_draw, same token_epilogue: bit-identical to the kernel above of either form on the same logits.
// Cost of the stages: 1 (min_p) + 2 (epsilon) + 2 (eta) passes over the row next to the 67 of the two bisections, + 1 when kept_n / kept_min
// are wanted.
#include "common.h"
#include "crab_internal.h"
#include "select_core.h"
#include <math.h>

namespace {

// the tokens of a row: the scaled logit, -inf for the suppressed EOS
struct TokenItems {
    const float* __restrict__ row;
    float inv_t;
    int suppress;
    __device__ __forceinline__ float operator()(int i) const { return i == suppress ? -INFINITY : row[i] * inv_t; }
};

// the token of row b from select_draw: finished / pad / EOS bookkeeping as greedy_select_kernel (ops.hip); thread 0 only
__device__ __forceinline__ void token_epilogue(int pick, int b, int step, int64_t* __restrict__ cur_ids, int64_t* __restrict__ out_ids, long ld_out,
                                               int* __restrict__ finished, int eos_id, int pad_id) {
    int tok = finished[b] ? pad_id : (pick < 0 ? 0 : pick);
    if (eos_id >= 0 && tok == eos_id) finished[b] = 1;
    cur_ids[b] = tok;
    out_ids[(long)b * ld_out + step] = tok;
}

__global__ __launch_bounds__(1024) void sample_select_kernel(const float* __restrict__ logits, long ldl, int V, int64_t* __restrict__ cur_ids,
                                                             int64_t* __restrict__ out_ids, long ld_out, const int* __restrict__ step_dev,
                                                             int* __restrict__ finished, int eos_id, int pad_id, int min_new, float inv_t,
                                                             int top_k, float top_p, unsigned long long seed) {
    __shared__ SelectShared sh;
    const int b = blockIdx.x, step = step_dev[0];
    const TokenItems items{logits + (long)b * ldl, inv_t, (eos_id >= 0 && step < min_new) ? eos_id : -1};
    const int pick = select_draw<false>(sh, items, V, b, step, top_k, top_p, seed);
    if (threadIdx.x == 0) token_epilogue(pick, b, step, cur_ids, out_ids, ld_out, finished, eos_id, pad_id);
}

__global__ __launch_bounds__(1024) void sample_select_warped_kernel(const float* __restrict__ logits, long ldl, int V, int64_t* __restrict__ cur_ids,
                                                                    int64_t* __restrict__ out_ids, long ld_out, const int* __restrict__ step_dev,
                                                                    int* __restrict__ finished, int eos_id, int pad_id, int min_new, float inv_t,
                                                                    int top_k, float top_p, unsigned long long seed, float min_p, float eps_cut,
                                                                    float eta_cut, int* __restrict__ kept_n, float* __restrict__ kept_min) {
    __shared__ SelectShared sh;
    const int b = blockIdx.x, step = step_dev[0];
    const TokenItems items{logits + (long)b * ldl, inv_t, (eos_id >= 0 && step < min_new) ? eos_id : -1};
    const int pick = select_draw<true>(sh, items, V, b, step, top_k, top_p, seed, SelectWarp{min_p, eps_cut, eta_cut, kept_n, kept_min});
    if (threadIdx.x == 0) token_epilogue(pick, b, step, cur_ids, out_ids, ld_out, finished, eos_id, pad_id);
}

// The rows of a compacted wave (csrc/kv_compact.hip): block r works on row r of every buffer, but its draw is keyed by row_ids[r], the index the
// row had before the wave shed its finished rows - the random stream of a row does not depend on which rows left.  WARP as select_draw's.
template <bool WARP>
__global__ __launch_bounds__(1024) void sample_select_rows_kernel(const float* __restrict__ logits, long ldl, int V, int64_t* __restrict__ cur_ids,
                                                                  int64_t* __restrict__ out_ids, long ld_out, const int* __restrict__ step_dev,
                                                                  int* __restrict__ finished, int eos_id, int pad_id, int min_new, float inv_t,
                                                                  int top_k, float top_p, unsigned long long seed, float min_p, float eps_cut,
                                                                  float eta_cut, const int* __restrict__ row_ids) {
    __shared__ SelectShared sh;
    const int r = blockIdx.x, step = step_dev[0];
    const TokenItems items{logits + (long)r * ldl, inv_t, (eos_id >= 0 && step < min_new) ? eos_id : -1};
    int pick;
    if constexpr (WARP) pick = select_draw<true>(sh, items, V, row_ids[r], step, top_k, top_p, seed, SelectWarp{min_p, eps_cut, eta_cut, nullptr, nullptr});
    else pick = select_draw<false>(sh, items, V, row_ids[r], step, top_k, top_p, seed);
    if (threadIdx.x == 0) token_epilogue(pick, r, step, cur_ids, out_ids, ld_out, finished, eos_id, pad_id);
}

}  // namespace

extern "C" int crab_sample_select_rows(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, int64_t* cur_ids,
                                       int64_t* out_ids, int64_t ld_out, const int32_t* step_dev, int32_t* finished, int eos_id, int pad_id,
                                       int min_new_tokens, float temperature, int top_k, float top_p, uint64_t seed, float min_p,
                                       float epsilon_cutoff, float eta_cutoff, const int32_t* row_ids) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !cur_ids || !out_ids || !step_dev || !finished || !row_ids || B <= 0 || V <= 0)
        return crab_fail(ctx, CRAB_E_INVALID, "sample_select_rows: bad argument");
    if (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_rows: temperature > 0, 0 < top_p <= 1, top_k >= 0");
    if (!(min_p >= 0.f && min_p <= 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_rows: 0 <= min_p <= 1 (0 = off)");
    if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_rows: 0 <= epsilon_cutoff < 1 (0 = off)");
    if (!(eta_cutoff >= 0.f && eta_cutoff < 1.0f)) return crab_fail(ctx, CRAB_E_INVALID, "sample_select_rows: 0 <= eta_cutoff < 1 (0 = off)");
    // all three stages off: the plain kernel's operations in its order (select_draw<false>), else the warped ones - bit-identical to
    // crab_sample_select / crab_sample_select_warped on the same logits either way
    if (min_p == 0.f && epsilon_cutoff == 0.f && eta_cutoff == 0.f)
        hipLaunchKernelGGL(sample_select_rows_kernel<false>, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, cur_ids, out_ids,
                           (long)ld_out, step_dev, finished, eos_id, pad_id, min_new_tokens, 1.0f / temperature, top_k, top_p,
                           (unsigned long long)seed, 0.f, 0.f, 0.f, row_ids);
    else
        hipLaunchKernelGGL(sample_select_rows_kernel<true>, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, cur_ids, out_ids,
                           (long)ld_out, step_dev, finished, eos_id, pad_id, min_new_tokens, 1.0f / temperature, top_k, top_p,
                           (unsigned long long)seed, min_p, epsilon_cutoff, eta_cutoff, row_ids);
    return crab_check_launch(ctx, "sample_select_rows");
}

extern "C" int crab_sample_select(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int B, int V, int64_t* cur_ids, int64_t* out_ids,
                                  int64_t ld_out, const int32_t* step_dev, int32_t* finished, int eos_id, int pad_id, int min_new_tokens,
                                  float temperature, int top_k, float top_p, uint64_t seed) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !cur_ids || !out_ids || !step_dev || !finished || B <= 0 || V <= 0) return crab_fail(ctx, CRAB_E_INVALID, "sample_select: bad argument");
    if (!(temperature > 0.f) || !(top_p > 0.f) || top_p > 1.0f || top_k < 0) return crab_fail(ctx, CRAB_E_INVALID, "sample_select: temperature > 0, 0 < top_p <= 1, top_k >= 0");
    hipLaunchKernelGGL(sample_select_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, cur_ids, out_ids, (long)ld_out, step_dev,
                       finished, eos_id, pad_id, min_new_tokens, 1.0f / temperature, top_k, top_p, (unsigned long long)seed);
    return crab_check_launch(ctx, "sample_select");
}

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
