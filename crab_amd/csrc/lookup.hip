// Prompt-lookup speculative decoding, the device-side bookkeeping of one verify step (HF generate(prompt_lookup_num_tokens = k,
// max_matching_ngram_size = n): generation/candidate_generator.py PromptLookupCandidateGenerator.get_candidates proposes, generation/utils.py
// _assisted_decoding / _speculative_sampling's greedy branch accepts) - without a host round trip, so draft -> embed -> layers -> lm_head -> accept
// is capturable as one HIP graph.  Batch size 1, greedy, as HF's assisted generation.
//   lookup_draft_kernel   the draft of up to k tokens: the continuation of the earliest earlier occurrence of the history's last n-gram
//   lookup_accept_kernel  the greedy choice of every verified position, the accepted run, the emitted tokens and the counters
// One block each, once per step.  State (all device-resident): hist int32 [S + max_new_tokens] - the prompt's ids row by row (-1: a row that is no
// text token, e.g. a modality embedding, or ids the caller did not give) followed by the emitted tokens; step_dev - tokens emitted so far (the live
// history is hist[0 .. S + step)); pos_dev - the cache slot of the current token.
// Every index taken from device memory is clamped against the sizes the launch was given (as constrain.hip): step against max_new_tokens, the
// number of drafts against k, a history entry outside [0, V) is "no token" - a corrupt array gives a wrong token and never an out-of-bounds access.
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

constexpr int LK_NONE = 0x7fffffff;

__device__ __forceinline__ int lk_tok(const int* __restrict__ hist, int i, int V) {      // entry i, -1 when it is no token
    const int t = hist[i];
    return (t >= 0 && t < V) ? t : -1;
}

// get_candidates: for n = min(max_ngram, len - 1) .. 1 the match positions idx (window hist[idx .. idx + n) == the last n entries) in ascending
// order; the first whose continuation hist[idx + n .. min(idx + n + k, len)) is non-empty after the crop at the first "no token" entry (HF crops at
// the first token its logits processors forbid and, when nothing is left, goes on to the next match) is chosen.  It is then cropped to the tokens
// the call may still emit beside the verify step's own, and before the first EOS - an EOS crop that leaves nothing ends the search with no draft,
// as HF's does (match_found is set before it).
__global__ __launch_bounds__(256) void lookup_draft_kernel(const int* __restrict__ hist, int S, const int* __restrict__ step_dev,
                                                           const int64_t* __restrict__ cur_ids, int k, int max_ngram, int eos_id, int pad_id,
                                                           int max_new, int V, int64_t* __restrict__ ids_out, int* __restrict__ n_draft_dev,
                                                           const int* __restrict__ finished) {
    __shared__ int red[4];
    __shared__ int found;
    const int tid = threadIdx.x;
    if (finished[0]) {                                           // uniform; the ids stay what they were
        if (tid == 0) n_draft_dev[0] = 0;
        return;
    }
    const int step = min(max(step_dev[0], 0), max_new);
    const int len = S + step;
    const int remaining = max_new - step - 1;                   // the verify step itself adds one token
    int start = -1;                                              // first entry of the chosen continuation
    if (remaining > 0) {
        for (int n = min(max_ngram, len - 1); n >= 1 && start < 0; --n) {
            int best = LK_NONE;
            for (int idx = tid; idx < len - n; idx += 256) {    // continuation start idx + n < len
                bool ok = lk_tok(hist, idx + n, V) >= 0;
                for (int e = 0; ok && e < n; ++e) {
                    const int a = lk_tok(hist, idx + e, V), b = lk_tok(hist, len - n + e, V);
                    ok = a >= 0 && a == b;
                }
                if (ok) { best = idx; break; }                  // ascending per thread: its first is its earliest
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
            __syncthreads();                                     // red[] / found of the previous n consumed
            if ((tid & 63) == 0) red[tid >> 6] = best;
            __syncthreads();
            if (tid == 0) {
                const int b4 = min(min(red[0], red[1]), min(red[2], red[3]));
                found = b4 == LK_NONE ? -1 : b4 + n;
            }
            __syncthreads();
            start = found;
        }
    }
    if (tid == 0) {
        int nd = 0;
        if (start >= 0) {
            const int end = min(min(start + k, len), start + remaining);
            while (start + nd < end) {
                const int t = lk_tok(hist, start + nd, V);
                if (t < 0 || t == eos_id) break;
                ++nd;
            }
        }
        const int64_t c = cur_ids[0];
        ids_out[0] = (c >= 0 && c < V) ? c : pad_id;
        for (int i = 0; i < k; ++i) ids_out[1 + i] = i < nd ? hist[start + i] : pad_id;
        n_draft_dev[0] = nd;
    }
}

// Row i of logits is the model's answer at the position of ids[i] (i = 0: the current token): t_i = its greedy choice under
// greedy_select_kernel's rule (ops.hip: the larger value wins, equal values go to the lower id; EOS suppressed while the emitted index
// step + i < min_new).  a = the leading drafts the model agrees with (t_i == ids[i + 1], i < n_draft); t_0 .. t_a are emitted (HF: the accepted
// candidates plus the model's own next token), cut after the first EOS and at max_new_tokens, both of which set `finished`.
__global__ __launch_bounds__(1024) void lookup_accept_kernel(const float* __restrict__ logits, long ldl, int V, int k,
                                                             const int64_t* __restrict__ ids, const int* __restrict__ n_draft_dev,
                                                             int64_t* __restrict__ cur_ids, int64_t* __restrict__ out_ids, int* __restrict__ hist, int S,
                                                             int* __restrict__ pos_dev, int* __restrict__ step_dev, int* __restrict__ finished,
                                                             int eos_id, int pad_id, int min_new, int max_new, int* __restrict__ stats,
                                                             float* __restrict__ step_logits_out) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int tok[16];
    __shared__ int n_emit;
    const int tid = threadIdx.x;
    if (finished[0]) return;                                     // uniform: a finished state changes nothing
    const int step = min(max(step_dev[0], 0), max_new);
    const int nd = min(min(max(n_draft_dev[0], 0), k), 15);
    for (int i = 0; i <= nd; ++i) {
        const int suppress = (eos_id >= 0 && step + i < min_new) ? eos_id : -1;
        const float* row = logits + (long)i * ldl;
        float best = -INFINITY;
        int bi = LK_NONE;
        for (int j = tid; j < V; j += 1024) {
            const float v = (j == suppress) ? -INFINITY : row[j];
            if (v > best || (v == best && j < bi)) { best = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        __syncthreads();                                         // sv / si of the previous row consumed
        if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 16; ++w)
                if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
            tok[i] = bi == LK_NONE ? 0 : bi;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0;
        while (a < nd && (int64_t)tok[a] == ids[a + 1]) ++a;
        int ne = 0, fin = 0;
        for (int i = 0; i <= a && step + i < max_new; ++i) {
            const int t = tok[i];
            out_ids[step + i] = t;
            hist[S + step + i] = t;
            ne = i + 1;
            if (eos_id >= 0 && t == eos_id) { fin = 1; break; }
        }
        if (step + ne >= max_new) fin = 1;
        if (ne > 0) cur_ids[0] = tok[ne - 1];
        pos_dev[0] += ne;
        step_dev[0] = step + ne;
        if (fin) finished[0] = 1;
        stats[0] += 1; stats[1] += nd; stats[2] += min(ne, a); stats[3] += ne;
        n_emit = ne;
    }
    __syncthreads();
    if (step_logits_out) {
        const int ne = n_emit;                                   // step + ne <= max_new
        for (int i = 0; i < ne; ++i) {
            const float* row = logits + (long)i * ldl;
            float* dst = step_logits_out + (long)(step + i) * V;
            for (int j = tid; j < V; j += 1024) dst[j] = row[j];
        }
    }
}

}  // namespace

extern "C" int crab_lookup_draft(crab_ctx* ctx, void* stream, const int32_t* hist, int S, const int32_t* step_dev, const int64_t* cur_ids, int k,
                                 int max_ngram, int eos_id, int pad_id, int max_new_tokens, int V, int64_t* ids_out, int32_t* n_draft_dev,
                                 const int32_t* finished) {
    if (!ctx) return CRAB_E_INVALID;
    if (!hist || !step_dev || !cur_ids || !ids_out || !n_draft_dev || !finished || S < 0 || V <= 0 || max_new_tokens < 1)
        return crab_fail(ctx, CRAB_E_INVALID, "lookup_draft: bad argument");
    if (k < 1 || k > 15 || max_ngram < 1) return crab_fail(ctx, CRAB_E_INVALID, "lookup_draft: 1 <= k <= 15 draft tokens, max_ngram >= 1");
    if (pad_id < 0 || pad_id >= V) return crab_fail(ctx, CRAB_E_INVALID, "lookup_draft: pad_id must be a row of the embedding table");
    hipLaunchKernelGGL(lookup_draft_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, S, step_dev, cur_ids, k, max_ngram, eos_id, pad_id,
                       max_new_tokens, V, ids_out, n_draft_dev, finished);
    return crab_check_launch(ctx, "lookup_draft");
}

extern "C" int crab_lookup_accept(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int V, int k, const int64_t* ids,
                                  const int32_t* n_draft_dev, int64_t* cur_ids, int64_t* out_ids, int32_t* hist, int S, int32_t* pos_dev,
                                  int32_t* step_dev, int32_t* finished, int eos_id, int pad_id, int min_new_tokens, int max_new_tokens,
                                  int32_t* stats, float* step_logits_out) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !ids || !n_draft_dev || !cur_ids || !out_ids || !hist || !pos_dev || !step_dev || !finished || !stats || S < 0 || V <= 0 ||
        ldl < V || max_new_tokens < 1)
        return crab_fail(ctx, CRAB_E_INVALID, "lookup_accept: bad argument");
    if (k < 1 || k > 15) return crab_fail(ctx, CRAB_E_INVALID, "lookup_accept: 1 <= k <= 15 draft tokens");
    hipLaunchKernelGGL(lookup_accept_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, (long)ldl, V, k, ids, n_draft_dev, cur_ids, out_ids,
                       hist, S, pos_dev, step_dev, finished, eos_id, pad_id, min_new_tokens, max_new_tokens, stats, step_logits_out);
    return crab_check_launch(ctx, "lookup_accept");
}
