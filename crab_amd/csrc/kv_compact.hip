// In-place KV row compaction: the live rows of a decode wave move to the front of every layer of the bf16 caches [L, rows, Hk, Tmax, d] x 2, so
// that the views kc[:, :B'] / vc[:, :B'] are the cache of a B'-row state (GenerationEngine: shed_finished).  Every row of a wave appends at the
// same slot pos_dev[0] and the decode kernels take the layer stride separately, so nothing else of the cache has to change.
//
//     for j = 0 .. n_live - 1:   row j <- row src_rows[j]   over the slots row_off[src_rows[j]] .. pos_dev[0], every layer and KV head
//
// (the inclusive slot range of kv_beam_reorder, csrc/beam.hip; row_off null: from slot 0).  Rows >= n_live and slots > pos_dev[0] are never written.
//
// Contract: src_rows is strictly increasing and src_rows[j] >= j (the survivors of a wave in their order).
//
// Why in place is right.  A parallel gather with one thread per (destination row, position) is wrong: destination j may be the source of a
// later pair (src = (1,2,3,4,5): every destination is the next pair's source), and nothing orders the blocks.  Here, as in
// kv_beam_reorder_kernel, ONE thread owns a 16-byte position (layer, KV head, slot, chunk) and walks the rows of that position itself, in
// ascending j, in batches: it loads src_rows[j .. j + n) into registers, then stores rows j .. j + n - 1.
//   * inside a batch every load precedes every store (registers in between);
//   * the stores of a batch hit rows < j + n; a later batch of the same thread reads the rows src_rows[j'] >= j' >= j + n: no store of a batch
//     can hit a source that a later batch still needs;
//   * the sources of a batch are >= j, the stores of the batches before it hit rows < j: no load sees a row this call has already overwritten;
//   * no other thread touches that position, in either cache.
// So every destination receives the ORIGINAL bytes of its source, with no second cache, no LDS and no ordering between threads.
//
// The work is the live span only - (layer, KV head) x slots 0 .. pos x 16-byte chunks - walked by a fixed grid with a grid-stride loop: pos is
// a device word (the launch can be issued without a host read).  Rows with src_rows[j] == j are skipped, and so are the slots of a row below its
// row_off (they hold nothing the row's decode step reads).  Device indices are clamped as in lookup.hip / constrain.hip: pos against Tmax,
// src_rows[j] against rows, row_off against pos - a corrupt array gives a wrong cache, never an out-of-range access.
#include "common.h"
#include "crab_internal.h"

namespace {

#define COMPACT_BATCH 8

__global__ __launch_bounds__(256) void kv_compact_rows_kernel(uint4* kc, uint4* vc, long layer_stride, int rows, int n_live, int Hk, int Tmax, int cpr,
                                                              unsigned groups, const int* __restrict__ pos_dev, const int* __restrict__ src_rows,
                                                              const int* __restrict__ row_off) {
    const int pos = min(max(pos_dev[0], 0), Tmax - 1);
    const unsigned span = (unsigned)(pos + 1) * (unsigned)cpr;                   // contiguous 16-byte units of one (layer, row, kv head)
    const unsigned total = groups * span;                                         // groups = L * Hk; total < 2^31: checked by the caller
    const long row_stride = (long)Hk * Tmax * cpr;                                // in 16-byte units, like layer_stride
    for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const unsigned g = e / span, r = e - g * span;
        const int hk = (int)(g % (unsigned)Hk), l = (int)(g / (unsigned)Hk);
        const int slot = (int)(r / (unsigned)cpr);
        const long base = (long)l * layer_stride + (long)hk * Tmax * cpr + r;    // this position in row 0
        for (int j0 = 0; j0 < n_live; j0 += COMPACT_BATCH) {
            int src[COMPACT_BATCH];
            bool any = false;
#pragma unroll
            for (int k = 0; k < COMPACT_BATCH; ++k) {
                const int j = j0 + k;
                src[k] = j;                                                       // src == j: nothing to move
                if (j < n_live) {
                    const int s = min(max(src_rows[j], 0), rows - 1);
                    const int off = row_off != nullptr ? min(max(row_off[s], 0), pos) : 0;
                    if (slot >= off) src[k] = s;
                }
                any = any || src[k] != j;
            }
            if (!any) continue;
            uint4 v[COMPACT_BATCH];
#pragma unroll
            for (int k = 0; k < COMPACT_BATCH; ++k)
                if (src[k] != j0 + k) v[k] = kc[base + src[k] * row_stride];
#pragma unroll
            for (int k = 0; k < COMPACT_BATCH; ++k)
                if (src[k] != j0 + k) kc[base + (j0 + k) * row_stride] = v[k];
#pragma unroll
            for (int k = 0; k < COMPACT_BATCH; ++k)
                if (src[k] != j0 + k) v[k] = vc[base + src[k] * row_stride];
#pragma unroll
            for (int k = 0; k < COMPACT_BATCH; ++k)
                if (src[k] != j0 + k) vc[base + (j0 + k) * row_stride] = v[k];
        }
    }
}

}  // namespace

extern "C" int crab_kv_compact_rows(crab_ctx* ctx, void* stream, void* k_cache, void* v_cache, int64_t layer_stride, int L, int rows, int Hk, int Tmax,
                                    int head_dim, int n_live, const int32_t* src_rows, const int32_t* row_off, const int32_t* pos_dev) {
    if (!ctx) return CRAB_E_INVALID;
    if (!k_cache || !v_cache || !src_rows || !pos_dev) return crab_fail(ctx, CRAB_E_INVALID, "kv_compact_rows: null operand");
    if (L < 1 || rows < 1 || Hk < 1 || Hk > 65535 || Tmax < 1 || head_dim < 8 || head_dim % 8 != 0 || n_live < 1 || n_live > rows ||
        (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "kv_compact_rows: L, Hk, Tmax >= 1, 1 <= n_live <= rows, head_dim a multiple of 8, 16-byte aligned caches");
    const int cpr = head_dim / 8;
    const long row_units = (long)Hk * Tmax * cpr;
    if (layer_stride % 8 != 0 || layer_stride / 8 < (long)rows * row_units)
        return crab_fail(ctx, CRAB_E_INVALID, "kv_compact_rows: layer_stride (elements) a multiple of 8 and >= rows * Hk * Tmax * head_dim");
    const long groups = (long)L * Hk, units = (long)L * (layer_stride / 8);
    if (units >= (1L << 31)) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "kv_compact_rows: more than 2^31 16-byte units per cache");
    const long work = groups * Tmax * cpr;                                       // <= units: the positions of one row of every layer
    const unsigned blocks = (unsigned)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);       // memory-bound: 8 blocks of 256 threads per CU
    hipLaunchKernelGGL(kv_compact_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint4*)k_cache, (uint4*)v_cache, (long)(layer_stride / 8),
                       rows, n_live, Hk, Tmax, cpr, (unsigned)groups, pos_dev, src_rows, row_off);
    return crab_check_launch(ctx, "kv_compact_rows");
}
