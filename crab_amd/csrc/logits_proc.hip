// Logits processors of the decode loop: HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and the several-id form of
// MinNewTokensLengthLogitsProcessor / EosTokenCriteria (transformers generation/logits_process.py, generation/stopping_criteria.py) as two
// launches around the select of a step - no host callback can run between two replays of a captured step.
//
// The processors touch at most step + n_stop of the V logits of a row, so nothing of size B x V is copied: logits_edit changes the few
// columns IN PLACE and keeps (column, raw value) pairs in a small save area, the select kernels (ops.hip, sample.hip, constrain.hip; not
// touched) choose from the edited row, logits_restore writes the raw values back.  After the pair the logits buffer holds, bit for bit, what
// the lm_head wrote - return_step_logits and both log-probability planes keep their raw-logit meaning.
//
// History of row b at step = step_dev[0]: h[j] = out_ids[b, j], j < step - the GENERATED tokens only.  HF's generate() with inputs_embeds and
// no input_ids starts from an empty input_ids tensor (transformers 5.15 generation/utils.py:736-744, _maybe_initialize_input_ids_for_generation:
// torch.ones((batch_size, 0))), and the reference always passes inputs_embeds (unified_llama.py:262-267), so the prompt never enters a processor.
//
// logits_edit: one block of 1024 threads per row, the history once into LDS as int32 (an id outside [0, V) becomes -1: it is never edited and
// matches nothing).  Save area: fixed slots, no compaction, no atomics - slot j < n_steps: the penalty edit of history token j; slot
// n_steps + j: the ban found by n-gram window j; slot 2 n_steps + e: stop id e.  Slot s is always handled by thread s % 1024.  Three phases
// between barriers:
//   1 save     every slot that will edit a column c stores (c, raw logits[b, c]), every other slot (-1, 0).  ALL raw values are taken before
//              ANY write, so a column that several slots edit restores to its raw value whichever slot is written back last.
//   2 penalty  (p != 1) the FIRST occurrence of every distinct history token: x = x < 0 ? x * p : x / p - a true fp32 division (__fdiv_rn), bit
//              for bit torch.where(score < 0, score * p, score / p); every distinct token is edited once, as HF's gather / scatter does.
//   3 bans     -inf.  n = no_repeat_ngram_size > 0 and step + 1 >= n: every window j in [0, step - n] with h[j .. j + n - 2] ==
//              h[step - n + 1 .. step - 1] bans h[j + n - 1] (_calc_banned_ngram_tokens; n = 1 bans every seen token).  While
//              step < min_new_tokens every stop_ids[e] is banned.
// A finished row (finished[b] != 0) is not edited: all its slots are -1.
// logits_restore: one block of 256 threads per row writes every saved pair back (duplicate columns carry the same raw value) and sets
// finished[b] |= cur_ids[b] in stop_ids (the select has already done so for its own eos_id).
#include "common.h"
#include "crab_internal.h"
#include <math.h>

#define LOGITS_PROC_MAX_STEPS 8192                              // history words in LDS: 8192 int32 = 32 KB
#define LOGITS_PROC_MAX_STOP 8

namespace {

__global__ __launch_bounds__(1024) void logits_edit_kernel(float* __restrict__ logits, long ldl, int V, const int64_t* __restrict__ out_ids,
                                                           long ld_out, int n_steps, const int* __restrict__ step_dev,
                                                           const int* __restrict__ finished, float penalty, int ngram,
                                                           const int* __restrict__ stop_ids, int n_stop, int min_new, int* __restrict__ save_idx,
                                                           float* __restrict__ save_val, long ld_save) {
    extern __shared__ int h[];                                   // n_steps words
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = min(max(step_dev[0], 0), n_steps);
    float* row = logits + (long)b * ldl;
    int* sidx = save_idx + (long)b * ld_save;
    float* sval = save_val + (long)b * ld_save;
    const int n_slots = 2 * n_steps + n_stop;
    if (finished[b] != 0) {
        for (int s = tid; s < n_slots; s += 1024) { sidx[s] = -1; sval[s] = 0.f; }
        return;
    }
    const int64_t* hist = out_ids + (long)b * ld_out;
    for (int j = tid; j < step; j += 1024) {
        const int64_t t = hist[j];
        h[j] = (t >= 0 && t < (int64_t)V) ? (int)t : -1;
    }
    __syncthreads();
    // ---- 1 save: which column every slot edits, and its raw value
    const bool pen_on = penalty != 1.0f;
    const bool ban_on = ngram > 0 && step + 1 >= ngram;
    const int tail = step - ngram + 1;                           // first token of the n - 1 last ones
    for (int j = tid; j < n_steps; j += 1024) {
        int c = -1;
        if (pen_on && j < step) {
            c = h[j];
            for (int i = 0; i < j && c >= 0; ++i)
                if (h[i] == c) c = -1;                           // not the first occurrence
        }
        sidx[j] = c;
        sval[j] = c >= 0 ? row[c] : 0.f;
        int d = -1;
        if (ban_on && j <= step - ngram) {
            d = h[j + ngram - 1];
            for (int i = 0; i < ngram - 1 && d >= 0; ++i) {
                const int a = h[j + i];
                if (a < 0 || a != h[tail + i]) d = -1;
            }
        }
        sidx[n_steps + j] = d;
        sval[n_steps + j] = d >= 0 ? row[d] : 0.f;
    }
    for (int e = tid; e < n_stop; e += 1024) {
        int c = -1;
        if (step < min_new) {
            c = stop_ids[e];
            if (c < 0 || c >= V) c = -1;
        }
        sidx[2 * n_steps + e] = c;
        sval[2 * n_steps + e] = c >= 0 ? row[c] : 0.f;
    }
    __syncthreads();
    // ---- 2 penalty: from the saved raw value (this thread's own slot)
    if (pen_on) {
        for (int j = tid; j < step; j += 1024) {
            const int c = sidx[j];
            if (c >= 0) {
                const float x = sval[j];
                row[c] = x < 0.f ? x * penalty : __fdiv_rn(x, penalty);
            }
        }
    }
    __syncthreads();
    // ---- 3 bans
    if (ban_on) {
        for (int j = tid; j <= step - ngram; j += 1024) {
            const int c = sidx[n_steps + j];
            if (c >= 0) row[c] = -INFINITY;
        }
    }
    for (int e = tid; e < n_stop; e += 1024) {
        const int c = sidx[2 * n_steps + e];
        if (c >= 0) row[c] = -INFINITY;
    }
}

__global__ __launch_bounds__(256) void logits_restore_kernel(float* __restrict__ logits, long ldl, int V, const int64_t* __restrict__ cur_ids,
                                                             int* __restrict__ finished, const int* __restrict__ stop_ids, int n_stop,
                                                             const int* __restrict__ save_idx, const float* __restrict__ save_val, long ld_save,
                                                             int n_slots) {
    const int b = blockIdx.x, tid = threadIdx.x;
    float* row = logits + (long)b * ldl;
    const int* sidx = save_idx + (long)b * ld_save;
    const float* sval = save_val + (long)b * ld_save;
    for (int s = tid; s < n_slots; s += 256) {
        const int c = sidx[s];
        if (c >= 0 && c < V) row[c] = sval[s];
    }
    if (tid == 0 && n_stop > 0) {
        const int64_t y = cur_ids[b];
        bool hit = false;
        for (int e = 0; e < n_stop; ++e) {
            const int s = stop_ids[e];
            hit |= (s >= 0 && y == (int64_t)s);
        }
        if (hit) finished[b] = 1;
    }
}

}  // namespace

extern "C" int crab_logits_edit(crab_ctx* ctx, void* stream, float* logits, int64_t ldl, int B, int V, const int64_t* out_ids, int64_t ld_out,
                                int n_steps, const int32_t* step_dev, const int32_t* finished, float repetition_penalty, int no_repeat_ngram_size,
                                const int32_t* stop_ids, int n_stop, int min_new_tokens, int32_t* save_idx, float* save_val, int64_t ld_save) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !out_ids || !step_dev || !finished || !save_idx || !save_val) return crab_fail(ctx, CRAB_E_INVALID, "logits_edit: null operand");
    if (B <= 0 || V <= 0 || n_steps <= 0 || ldl < V || ld_out < n_steps)
        return crab_fail(ctx, CRAB_E_INVALID, "logits_edit: B, V, n_steps >= 1, ldl >= V (the rows are written), ld_out >= n_steps");
    if (!(repetition_penalty > 0.f) || no_repeat_ngram_size < 0) return crab_fail(ctx, CRAB_E_INVALID, "logits_edit: repetition_penalty > 0, no_repeat_ngram_size >= 0");
    if (n_stop < 0 || n_stop > LOGITS_PROC_MAX_STOP || (n_stop > 0 && !stop_ids)) return crab_fail(ctx, CRAB_E_INVALID, "logits_edit: 0 <= n_stop <= 8, stop_ids with n_stop > 0");
    if (n_steps > LOGITS_PROC_MAX_STEPS) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "logits_edit: n_steps > 8192 (the history is held in 32 KB of LDS)");
    if (ld_save < 2 * (int64_t)n_steps + n_stop) return crab_fail(ctx, CRAB_E_INVALID, "logits_edit: ld_save < 2 n_steps + n_stop");
    hipLaunchKernelGGL(logits_edit_kernel, dim3(B), dim3(1024), (size_t)n_steps * sizeof(int), (hipStream_t)stream, logits, (long)ldl, V, out_ids,
                       (long)ld_out, n_steps, step_dev, finished, repetition_penalty, no_repeat_ngram_size, stop_ids, n_stop, min_new_tokens, save_idx,
                       save_val, (long)ld_save);
    return crab_check_launch(ctx, "logits_edit");
}

extern "C" int crab_logits_restore(crab_ctx* ctx, void* stream, float* logits, int64_t ldl, int B, int V, const int64_t* cur_ids, int32_t* finished,
                                   const int32_t* stop_ids, int n_stop, const int32_t* save_idx, const float* save_val, int64_t ld_save, int n_slots) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !cur_ids || !finished || !save_idx || !save_val) return crab_fail(ctx, CRAB_E_INVALID, "logits_restore: null operand");
    if (B <= 0 || V <= 0 || ldl < V) return crab_fail(ctx, CRAB_E_INVALID, "logits_restore: B, V >= 1, ldl >= V (the rows are written)");
    if (n_stop < 0 || n_stop > LOGITS_PROC_MAX_STOP || (n_stop > 0 && !stop_ids)) return crab_fail(ctx, CRAB_E_INVALID, "logits_restore: 0 <= n_stop <= 8, stop_ids with n_stop > 0");
    if (n_slots < 1 || ld_save < n_slots) return crab_fail(ctx, CRAB_E_INVALID, "logits_restore: 1 <= n_slots <= ld_save");
    hipLaunchKernelGGL(logits_restore_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, (long)ldl, V, cur_ids, finished, stop_ids, n_stop,
                       save_idx, save_val, (long)ld_save, n_slots);
    return crab_check_launch(ctx, "logits_restore");
}
