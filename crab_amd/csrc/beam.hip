// Beam search inside the decode step: HF's vectorised GenerationMixin._beam_search (transformers generation/utils.py: _get_top_k_continuations,
// _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic, _beam_search_has_unfinished_sequences) as three
// launches that replace the select of a step - no host callback can run between two replays of a captured step.
//
// Rows: the K beams of clip c are the decode rows c K .. c K + K - 1.  State per clip, all device-resident (include/crab_hip.h "Beam search"):
//     run_score [K] fp32, run_seq [K, max_new] int64 (the decode state's out_ids), hyp_score [K] fp32, hyp_seq [K, max_new] int64,
//     hyp_len [K], hyp_fin [K], unsat [1] (is_early_stop_heuristic_unsatisfied), finished [K] (the clip's done flag, on every row).
//
// beam_row_topk   one block of 256 threads per row over the row's raw fp32 logits: lse = max + log(sum exp(z - max)) (thread-serial sums, a
//                 shuffle tree per wave, the four waves in order), score(i) = run_score[row] + (z[i] - lse), EOS at -inf while step < min_new
//                 (MinNewTokensLengthLogitsProcessor acts on the log-probs, no renormalisation).  The best 2K of the clip's K V candidates
//                 lie in the union of the rows' best 2K, so every row writes its own best 2K, sorted.  Selection: every thread holds the best
//                 of its strided elements; per rank one block-wide argmax, then the block looks through the ~V / 256 elements of the winner's
//                 owner for that thread's next best - one full pass and 2K short ones, no per-thread lists.
//                 Total order everywhere: the higher score first, then the lower flat index k V + token.  NaN scores sort as -inf.
// beam_merge      one wave per clip: the K x 2K candidates to the clip's best 2K by rank counting, then steps d-g of HF's loop on one lane (at
//                 most 16 candidates), then all lanes permute the token histories: a lane owns a column t of run_seq / hyp_seq, takes the K
//                 old values of both into its own LDS column and writes the K new ones, so the update is in place.
// kv_beam_reorder the own KV cache [L, C K, Hk, Tmax, d] x 2 in place over slots first_slot .. pos: a thread owns one 16-byte position of a
//                 clip, loads it from the K parent rows into registers, then stores the K results - the same thread reads and writes every
//                 byte of its position, so no second cache, no LDS and no ordering between threads is needed.  Identity and done clips leave.
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

#define BEAM_K CRAB_BEAM_MAX
#define BEAM_2K (2 * CRAB_BEAM_MAX)
#define BEAM_NEG (-1.0e9f)

__device__ __forceinline__ bool beam_beats(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

__device__ __forceinline__ float beam_score(float z, int i, float run, float lse, int eos_masked) {
    float s = run + (z - lse);
    if (i == eos_masked) s = -INFINITY;
    return s != s ? -INFINITY : s;
}

__global__ __launch_bounds__(256) void beam_row_topk_kernel(const float* __restrict__ logits, long ldl, int V, int K,
                                                            const float* __restrict__ run_score, const int* __restrict__ step_dev,
                                                            const int* __restrict__ finished, int eos, int min_new,
                                                            float* __restrict__ cand_score, int* __restrict__ cand_tok) {
    __shared__ float red_f[4];
    __shared__ float win_s[2][4], nxt_s[2][4];
    __shared__ int win_i[2][4], nxt_i[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (finished[row] != 0) return;                              // the clip is done: frozen (the merge leaves it alone as well)
    const float* z = logits + (long)row * ldl;
    const float run = run_score[row];
    const int eos_masked = (eos >= 0 && step_dev[0] < min_new) ? eos : -1;
    // ---- log-sum-exp of the raw row
    float m = -INFINITY;
    for (int i = tid; i < V; i += 256) m = fmaxf(m, z[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red_f[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    __syncthreads();
    float acc = 0.f;
    for (int i = tid; i < V; i += 256) acc += expf(z[i] - m);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) red_f[wave] = acc;
    __syncthreads();
    const float lse = m + logf((red_f[0] + red_f[1]) + (red_f[2] + red_f[3]));
    // ---- the best of every thread's own elements
    float bs = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += 256) {
        const float s = beam_score(z[i], i, run, lse, eos_masked);
        if (beam_beats(s, i, bs, bi)) { bs = s; bi = i; }
    }
    // ---- 2K ranks: block argmax, then the winner's owner finds its next best strictly behind the winner
    const int n = 2 * K;
    for (int r = 0; r < n; ++r) {
        float ws = bs;
        int wi = bi;
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(ws, o);
            const int oi = __shfl_xor(wi, o);
            if (beam_beats(os, oi, ws, wi)) { ws = os; wi = oi; }
        }
        const int p = r & 1;
        if (lane == 0) { win_s[p][wave] = ws; win_i[p][wave] = wi; }
        __syncthreads();
        ws = win_s[p][0]; wi = win_i[p][0];
        for (int w = 1; w < 4; ++w)
            if (beam_beats(win_s[p][w], win_i[p][w], ws, wi)) { ws = win_s[p][w]; wi = win_i[p][w]; }
        if (tid == 0) {
            cand_score[(long)row * n + r] = ws;
            cand_tok[(long)row * n + r] = min(max(wi, 0), V - 1);       // V >= 2K: a rank always has an element; clamped all the same
        }
        if (r + 1 == n) break;
        // the winner's owner (thread wi % 256) needs its next best, strictly behind the winner: the whole block looks through the owner's
        // elements wi % 256 + 256 j, thread `tid` taking j = tid, tid + 256, ..., and reduces again - one thread alone would walk them in series
        float ns = -INFINITY;
        int ni = 0x7fffffff;
        for (long i = (wi & 255) + 256L * tid; i < V; i += 256L * 256L) {
            const float s = beam_score(z[i], (int)i, run, lse, eos_masked);
            const bool behind = s < ws || (s == ws && (int)i > wi);
            if (behind && beam_beats(s, (int)i, ns, ni)) { ns = s; ni = (int)i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(ns, o);
            const int oi = __shfl_xor(ni, o);
            if (beam_beats(os, oi, ns, ni)) { ns = os; ni = oi; }
        }
        if (lane == 0) { nxt_s[p][wave] = ns; nxt_i[p][wave] = ni; }
        __syncthreads();
        if (wi == bi) {                                          // this thread owned the winner
            bs = nxt_s[p][0]; bi = nxt_i[p][0];
            for (int w = 1; w < 4; ++w)
                if (beam_beats(nxt_s[p][w], nxt_i[p][w], bs, bi)) { bs = nxt_s[p][w]; bi = nxt_i[p][w]; }
        }
    }
}

__global__ __launch_bounds__(64) void beam_merge_kernel(const float* __restrict__ cand_score, const int* __restrict__ cand_tok, int V, int K,
                                                        int max_new, const int* __restrict__ step_dev, int eos, int pad, int early, int lp_pos,
                                                        const float* __restrict__ len_tab, float* run_score, int64_t* run_seq, long ld_run,
                                                        float* hyp_score, int64_t* hyp_seq, long ld_hyp, int* hyp_len, int* hyp_fin, int* unsat,
                                                        int64_t* cur_ids, int* beam_idx, int* finished) {
    __shared__ float cs[BEAM_K * BEAM_2K];                       // the K x 2K candidates
    __shared__ int cf[BEAM_K * BEAM_2K];                         // flat index k V + token
    __shared__ float ts[BEAM_2K];                                // the clip's best 2K
    __shared__ int tp[BEAM_2K], tt[BEAM_2K], hit[BEAM_2K], did[BEAM_2K];
    __shared__ float rs[BEAM_2K], fs[3 * BEAM_K];
    __shared__ int ff[3 * BEAM_K], fl[3 * BEAM_K];
    __shared__ int new_par[BEAM_K], new_tok[BEAM_K], hsrc[BEAM_K];
    __shared__ int64_t l_run[BEAM_K][64], l_hyp[BEAM_K][64];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int r0 = c * K, n2 = 2 * K, n = K * n2;
    if (finished[r0] != 0) return;                               // a done clip is frozen
    const int step = min(max(step_dev[0], 0), max_new - 1);
    for (int j = lane; j < n; j += 64) {
        const int k = j / n2;
        const float s = cand_score[(long)r0 * n2 + j];
        cs[j] = s != s ? -INFINITY : s;
        cf[j] = k * V + min(max(cand_tok[(long)r0 * n2 + j], 0), V - 1);
    }
    if (lane < n2) { ts[lane] = -INFINITY; tp[lane] = 0; tt[lane] = 0; }
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
        const float s = cs[j];
        const int f = cf[j];
        int rank = 0;
        for (int i = 0; i < n; ++i)
            rank += (cs[i] > s || (cs[i] == s && (cf[i] < f || (cf[i] == f && i < j)))) ? 1 : 0;
        if (rank < n2) { ts[rank] = s; tp[rank] = f / V; tt[rank] = f % V; }
    }
    __syncthreads();
    if (lane == 0) {
        // d. which candidates hit a stopping criterion (EosTokenCriteria, MaxLengthCriteria)
        const bool last = step + 1 >= max_new;
        bool all_hits = true;
        for (int i = 0; i < n2; ++i) {
            hit[i] = (last || (eos >= 0 && tt[i] == eos)) ? 1 : 0;
            all_hits = all_hits && hit[i];
            rs[i] = hit[i] ? ts[i] + BEAM_NEG : ts[i];
        }
        // e. the next K running beams
        for (int i = 0; i < n2; ++i) {
            int rank = 0;
            for (int j = 0; j < n2; ++j) rank += beam_beats(rs[j], j, rs[i], i) ? 1 : 0;
            if (rank < K) { new_par[rank] = tp[i]; new_tok[rank] = tt[i]; fl[rank] = i; }
        }
        float run0 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float v = rs[fl[k]];
            if (k == 0) run0 = v;
            run_score[r0 + k] = v;
            cur_ids[r0 + k] = new_tok[k];
            beam_idx[r0 + k] = new_par[k];
        }
        // f. finalise the candidates among the first K that stopped; merge with the K kept hypotheses
        const int unsat_old = unsat[c];
        bool full = early == 1;
        for (int k = 0; k < K; ++k) full = full && hyp_fin[r0 + k] != 0;
        const float den = len_tab[step + 1];
        for (int k = 0; k < K; ++k) { fs[k] = hyp_score[r0 + k]; ff[k] = hyp_fin[r0 + k]; fl[k] = hyp_len[r0 + k]; }
        for (int i = 0; i < n2; ++i) {
            did[i] = (hit[i] && i < K) ? 1 : 0;
            float f = __fdiv_rn(ts[i], den);
            if (full) f += BEAM_NEG;
            if (!unsat_old) f += BEAM_NEG;
            if (!did[i]) f += BEAM_NEG;
            fs[K + i] = f != f ? -INFINITY : f;
            ff[K + i] = did[i];
            fl[K + i] = step + 1;
        }
        float worst = INFINITY;
        bool all_fin = true;
        for (int i = 0; i < 3 * K; ++i) {
            int rank = 0;
            for (int j = 0; j < 3 * K; ++j) rank += beam_beats(fs[j], j, fs[i], i) ? 1 : 0;
            if (rank < K) {
                hsrc[rank] = i;
                hyp_score[r0 + rank] = fs[i];
                hyp_fin[r0 + rank] = ff[i];
                hyp_len[r0 + rank] = ff[i] ? fl[i] : 0;
                worst = fminf(worst, fs[i]);
                all_fin = all_fin && ff[i];
            }
        }
        // g. the early-stop heuristic and the clip's done flag
        const int blen = (early == 2 && lp_pos) ? max_new : step + 1;
        const float best = __fdiv_rn(run0, len_tab[blen]);
        bool any = false;
        for (int k = 0; k < K; ++k) any = any || best > (ff[hsrc[k]] ? worst : BEAM_NEG);
        const int unsat_new = (unsat_old && any) ? 1 : 0;
        unsat[c] = unsat_new;
        const bool go_on = unsat_new && !(all_fin && early == 1) && !all_hits;
        for (int k = 0; k < K; ++k) finished[r0 + k] = go_on ? 0 : 1;
    }
    __syncthreads();
    // ---- histories: a lane owns column t of both [K, max_new] blocks
    for (int t0 = 0; t0 < max_new; t0 += 64) {
        const int t = t0 + lane;
        if (t < max_new) {
            for (int k = 0; k < K; ++k) {
                l_run[k][lane] = run_seq[(long)(r0 + k) * ld_run + t];
                l_hyp[k][lane] = hyp_seq[(long)(r0 + k) * ld_hyp + t];
            }
            for (int k = 0; k < K; ++k) {
                run_seq[(long)(r0 + k) * ld_run + t] = t < step ? l_run[new_par[k]][lane] : (t == step ? (int64_t)new_tok[k] : (int64_t)pad);
                const int src = hsrc[k];
                int64_t v;
                if (src < K) v = l_hyp[src][lane];
                else v = t < step ? l_run[tp[src - K]][lane] : (t == step ? (int64_t)tt[src - K] : (int64_t)pad);
                hyp_seq[(long)(r0 + k) * ld_hyp + t] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void kv_beam_reorder_kernel(uint4* kc, uint4* vc, int C, int K, int Hk, int Tmax, int cpr, int first_slot, unsigned groups,
                                                              const int* __restrict__ pos_dev, const int* __restrict__ beam_idx,
                                                              const int* __restrict__ finished) {
    // The work is the LIVE part only - (layer, clip, kv head) x slots first_slot .. pos x 16-byte chunks - walked by a fixed grid: pos is a
    // device word, and a grid over all Tmax slots whose blocks leave costs more than the copy itself while the own context is short.
    const int pos = min(max(pos_dev[0], 0), Tmax - 1);
    if (pos < first_slot) return;
    const unsigned span = (unsigned)(pos - first_slot + 1) * (unsigned)cpr;      // contiguous 16-byte units of one (layer, row, kv head)
    const unsigned total = groups * span;                                         // groups = L * C * Hk < 2^31 / (Tmax * cpr): checked by the caller
    const long row_stride = (long)Hk * Tmax * cpr;                                // in 16-byte units
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned g = e / span, r = e - g * span;
        const int hk = (int)(g % (unsigned)Hk), lc = (int)(g / (unsigned)Hk), c = lc % C, l = lc / C;
        if (finished[c * K] != 0) continue;
        int par[BEAM_K];
        bool ident = true;
#pragma unroll
        for (int k = 0; k < BEAM_K; ++k) {
            par[k] = k < K ? min(max(beam_idx[c * K + k], 0), K - 1) : 0;
            ident = ident && (k >= K || par[k] == k);
        }
        if (ident) continue;
        const long base = ((long)l * C * K + (long)c * K) * row_stride + ((long)hk * Tmax + first_slot) * cpr + r;
        uint4 v[BEAM_K];
#pragma unroll
        for (int k = 0; k < BEAM_K; ++k)
            if (k < K) v[k] = kc[base + par[k] * row_stride];
#pragma unroll
        for (int k = 0; k < BEAM_K; ++k)
            if (k < K && par[k] != k) kc[base + k * row_stride] = v[k];
#pragma unroll
        for (int k = 0; k < BEAM_K; ++k)
            if (k < K) v[k] = vc[base + par[k] * row_stride];
#pragma unroll
        for (int k = 0; k < BEAM_K; ++k)
            if (k < K && par[k] != k) vc[base + k * row_stride] = v[k];
    }
}

int beam_args(crab_ctx* ctx, const char* who, int rows, int V, int K, int max_new) {
    char msg[160];
    if (rows < 1 || K < 1 || rows % K != 0 || max_new < 1 || V < 2 * K || V > (1 << 27)) {
        snprintf(msg, sizeof(msg), "%s: rows >= 1 and a multiple of num_beams >= 1, max_new >= 1, 2 num_beams <= V <= 2^27", who);
        return crab_fail(ctx, CRAB_E_INVALID, msg);
    }
    if (K > CRAB_BEAM_MAX || max_new > CRAB_BEAM_MAX_NEW) {
        snprintf(msg, sizeof(msg), "%s: num_beams > %d or max_new > %d", who, CRAB_BEAM_MAX, CRAB_BEAM_MAX_NEW);
        return crab_fail(ctx, CRAB_E_UNSUPPORTED, msg);
    }
    return CRAB_OK;
}

}  // namespace

extern "C" int crab_beam_row_topk(crab_ctx* ctx, void* stream, const float* logits, int64_t ldl, int rows, int V, int num_beams,
                                  const float* run_score, const int32_t* step_dev, const int32_t* finished, int eos_id, int min_new_tokens,
                                  float* cand_score, int32_t* cand_tok) {
    if (!ctx) return CRAB_E_INVALID;
    if (!logits || !run_score || !step_dev || !finished || !cand_score || !cand_tok) return crab_fail(ctx, CRAB_E_INVALID, "beam_row_topk: null operand");
    if (ldl < 0) return crab_fail(ctx, CRAB_E_INVALID, "beam_row_topk: ldl < 0");
    const int rc = beam_args(ctx, "beam_row_topk", rows, V, num_beams, 1);
    if (rc != CRAB_OK) return rc;
    hipLaunchKernelGGL(beam_row_topk_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, (long)ldl, V, num_beams, run_score, step_dev,
                       finished, eos_id, min_new_tokens, cand_score, cand_tok);
    return crab_check_launch(ctx, "beam_row_topk");
}

extern "C" int crab_beam_merge(crab_ctx* ctx, void* stream, const float* cand_score, const int32_t* cand_tok, int rows, int V, int num_beams,
                               int max_new, const int32_t* step_dev, int eos_id, int pad_id, int early_stopping, int length_penalty_positive,
                               const float* len_tab, float* run_score, int64_t* run_seq, int64_t ld_run, float* hyp_score, int64_t* hyp_seq,
                               int64_t ld_hyp, int32_t* hyp_len, int32_t* hyp_fin, int32_t* unsat, int64_t* cur_ids, int32_t* beam_idx,
                               int32_t* finished) {
    if (!ctx) return CRAB_E_INVALID;
    if (!cand_score || !cand_tok || !step_dev || !len_tab || !run_score || !run_seq || !hyp_score || !hyp_seq || !hyp_len || !hyp_fin || !unsat ||
        !cur_ids || !beam_idx || !finished)
        return crab_fail(ctx, CRAB_E_INVALID, "beam_merge: null operand");
    const int rc = beam_args(ctx, "beam_merge", rows, V, num_beams, max_new);
    if (rc != CRAB_OK) return rc;
    if (ld_run < max_new || ld_hyp < max_new || early_stopping < 0 || early_stopping > 2)
        return crab_fail(ctx, CRAB_E_INVALID, "beam_merge: ld_run, ld_hyp >= max_new; early_stopping 0 (False), 1 (True) or 2 (\"never\")");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(rows / num_beams), dim3(64), 0, (hipStream_t)stream, cand_score, cand_tok, V, num_beams, max_new,
                       step_dev, eos_id, pad_id, early_stopping, length_penalty_positive ? 1 : 0, len_tab, run_score, run_seq, (long)ld_run, hyp_score,
                       hyp_seq, (long)ld_hyp, hyp_len, hyp_fin, unsat, cur_ids, beam_idx, finished);
    return crab_check_launch(ctx, "beam_merge");
}

extern "C" int crab_kv_beam_reorder(crab_ctx* ctx, void* stream, void* k_cache, void* v_cache, int L, int rows, int num_beams, int Hk, int Tmax,
                                    int head_dim, int first_slot, const int32_t* pos_dev, const int32_t* beam_idx, const int32_t* finished) {
    if (!ctx) return CRAB_E_INVALID;
    if (!k_cache || !v_cache || !pos_dev || !beam_idx || !finished) return crab_fail(ctx, CRAB_E_INVALID, "kv_beam_reorder: null operand");
    if (L < 1 || rows < 1 || num_beams < 1 || rows % num_beams != 0 || Hk < 1 || Hk > 65535 || Tmax < 1 || first_slot < 0 || first_slot >= Tmax ||
        head_dim < 8 || head_dim % 8 != 0 || (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "kv_beam_reorder: L, Hk, Tmax >= 1, rows a multiple of num_beams >= 1, 0 <= first_slot < Tmax, head_dim a multiple of 8, 16-byte aligned caches");
    if (num_beams > CRAB_BEAM_MAX) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "kv_beam_reorder: num_beams > 8");
    const int C = rows / num_beams, cpr = head_dim / 8;
    const long groups = (long)L * C * Hk, units = groups * Tmax * cpr;
    if (units >= (1L << 31)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "kv_beam_reorder: more than 2^31 16-byte units per cache");
    const unsigned blocks = (unsigned)((units + 255) / 256 < 4096 ? (units + 255) / 256 : 4096);     // 16 blocks of 256 threads per CU
    hipLaunchKernelGGL(kv_beam_reorder_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)k_cache, (uint4*)v_cache, C, num_beams, Hk,
                       Tmax, cpr, first_slot, (unsigned)groups, pos_dev, beam_idx, finished);
    return crab_check_launch(ctx, "kv_beam_reorder");
}

extern "C" int crab_beam_max(void) { return CRAB_BEAM_MAX; }
extern "C" int crab_beam_max_new(void) { return CRAB_BEAM_MAX_NEW; }
