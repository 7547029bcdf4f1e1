// Teacher-forced scoring: the lm_head projection with the cross entropy in its epilogue (models/modeling_llama.py:1261-1274: logits.float(),
// shift, CrossEntropyLoss(ignore_index = -100)).  The fp32 logits z = x[M,K] . W[N,K]^T exist only as MFMA accumulators: every 256 x 256
// output tile is reduced in registers / LDS to one 16-byte record per (row, column tile) - (max, sum exp(z - max), best value, best column) -
// plus the label's logit, and a second small kernel folds the records of a row into lse, log-prob and argmax.  Nothing of size rows x V is
// stored: 2 KB per row at V = 32000 instead of 128 KB.
//
// The main loop is a copy of gemm_bt_ring_kernel<256, 256, 2, 4> (gemm_glds.hip: LDS-DMA ring of four 32-wide K stages, one block per CU, the
// same tile-to-XCD mapping, the same K order - the accumulators are bit-identical to that kernel's fp32 C) with the optional row gather
// folded into the per-lane source address of the activation pieces.  Kept in its own file so that the headline GEMM's code, register
// allocation and launch-trace names do not move.
#include "common.h"
#include "crab_internal.h"
#include <math.h>

namespace {

__device__ __attribute__((aligned(16))) uint32_t g_xent_zero_page[64];      // zero-initialised device memory (256 B)

typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* gbl_vptr;

constexpr int XBM = 256, XBN = 256, XBK = 32, XNS = 4, XWGM = 2, XWGN = 4;

struct XentP {
    const bf16_t* A; const bf16_t* B; const int* row_idx; const int* labels;
    long lda, ldb;
    int M, N, K, tiles_m, tiles_n;
    f32x4_t* part;          // [M][tiles_n] records (max, sum exp(z - max), best value, best column as int bits)
    float* zlab;            // [M] logit of the label column (written for 0 <= label < N only)
};

// (value, column) pairs: the larger value wins, on equal values the lower column (crab_argmax / crab_greedy_select: first maximum)
__device__ __forceinline__ void best_merge(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(XWGM * XWGN * 64) void lm_head_xent_kernel(XentP p) {
    constexpr int NW = XWGM * XWGN;
    constexpr int WM = XBM / XWGM, WN = XBN / XWGN;
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int PA = XBM / 16, PB = XBN / 16;              // 1-KiB pieces (16 rows x 64 B) per operand tile
    constexpr int PPW = (PA + PB) / NW;                      // pieces per wave per K tile (4)
    constexpr int STAGE_ELEMS = (XBM + XBN) * XBK;
    __shared__ __attribute__((aligned(16))) bf16_t lds[XNS * STAGE_ELEMS];
    static_assert(PA == PB && PA % PPW == 0, "operand choice must be uniform per wave");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / XWGN, wn = wave % XWGN;
    const int nwg = p.tiles_m * p.tiles_n;
    const int bid = xcd_remap(blockIdx.x, nwg);
    int tm, tn;
    tile_coords(bid, p.tiles_m, p.tiles_n, 8, tm, tn);          // 8 x 4 tile patch per XCD (32 CUs, one block each)
    const int m0 = tm * XBM, n0 = tn * XBN;
    const int nk = (p.K + XBK - 1) / XBK;

    const bool isA = wave * PPW < PA;
    const int prow = lane >> 2, pc = lane & 3;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(g_xent_zero_page);
    // per-piece source pointer, carried over the K tiles (rows outside the operand keep reading the zero page).  Activation rows are
    // gathered: row i of the problem is x[row_idx[i]]
    const bf16_t* fptr[PPW];
    int fadv[PPW], kc[PPW], ldso[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int q = wave * PPW + i;
        const int pr0 = (isA ? q : q - PA) * 16;
        const int row = pr0 + prow;
        const int c = pc ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3);
        kc[i] = c * 8;
        const int g = (isA ? m0 : n0) + row;
        const bool ok = g < (isA ? p.M : p.N);
        long src = g;
        if (isA && ok && p.row_idx) src = p.row_idx[g];
        fptr[i] = ok ? (isA ? p.A + src * p.lda : p.B + src * p.ldb) + c * 8 : zero;
        fadv[i] = ok ? XBK : 0;
        ldso[i] = (isA ? 0 : XBM * XBK) + pr0 * XBK;
    }
    // K tiles must be staged in order 0, 1, 2, ... (they are: prologue 0..2, then t + 3): a piece costs the LDS-DMA plus one 64-bit add.  Only
    // the last tile of a K that is not a multiple of 32 (K % 8 == 0) selects: its chunks beyond K come from the zero page
    const int nfast = p.K / XBK;
#define XSTAGE(T_)                                                                                        \
    {                                                                                                     \
        const int sb_ = ((T_) & (XNS - 1)) * STAGE_ELEMS;                                                 \
        const bool tail_ = (T_) >= nfast;                                                                 \
        const int k0_ = (T_) * XBK;                                                                       \
        _Pragma("unroll") for (int i = 0; i < PPW; ++i) {                                                 \
            const bf16_t* src_ = fptr[i];                                                                 \
            if (tail_) src_ = (k0_ + kc[i] < p.K) ? src_ : zero;                                          \
            bf16_t* dst_ = &lds[sb_ + __builtin_amdgcn_readfirstlane(ldso[i])];                           \
            __builtin_amdgcn_global_load_lds((gbl_vptr)src_, (lds_vptr)dst_, 16, 0, 0);                   \
            fptr[i] += fadv[i];                                                                           \
        }                                                                                                 \
    }

    f32x4_t acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // prologue: tiles 0..2 in flight, tile 0 retired
    XSTAGE(0);
    if (nk > 1) XSTAGE(1);
    if (nk > 2) XSTAGE(2);
    static_assert(PPW == 4, "vmcnt(8) below = two tiles of 4 LDS-DMA instructions per wave");
    if (nk > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int fr = lane & 15, fg = lane >> 4;
    int wofs[TN], xofs[TM];
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
        const int row = wn * WN + ni * 16 + fr;
        wofs[ni] = XBM * XBK + row * XBK + ((fg ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3)) << 3);
    }
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int row = wm * WM + mi * 16 + fr;
        xofs[mi] = row * XBK + ((fg ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3)) << 3);
    }

    // two wave groups one barrier apart, as in the ring GEMM: one group's LDS-DMA issue and fragment reads hide under the other's MFMAs
    const int grp = wave / (NW / 2);
    if (grp == 1) __builtin_amdgcn_s_barrier();
    for (int t = 0; t < nk; ++t) {
        const bf16_t* st = &lds[(t & (XNS - 1)) * STAGE_ELEMS];
        bf16x8_t wf[TN], xf[TM];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) wf[ni] = *reinterpret_cast<const bf16x8_t*>(st + wofs[ni]);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) xf[mi] = *reinterpret_cast<const bf16x8_t*>(st + xofs[mi]);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 3 < nk) XSTAGE(t + 3);
        if (t + 3 < nk) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();
#undef XSTAGE

    // ---- epilogue.  acc[ni][mi][r] = z[m0 + wm*128 + mi*16 + fr][n0 + wn*64 + ni*16 + fg*4 + r] (gemm_epilogue.h).  The ring's LDS is free now.
    __syncthreads();                                    // every wave is past its last fragment read, no DMA is in flight
    float* redv = reinterpret_cast<float*>(lds);        // [256 rows][4 column waves] best value (= row maximum of the wave's 64 columns)
    int* redi = reinterpret_cast<int*>(lds) + 1024;     // [256][4] its column
    float* reds = reinterpret_cast<float*>(lds) + 2048; // [256][4] sum exp(z - tile row maximum)
    const int ncol0 = n0 + wn * WN + fg * 4;
    if (n0 + XBN > p.N) {                               // ragged last column tile: columns >= N leave the max, the sum and the argmax
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ncol0 + ni * 16 + r >= p.N) {
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) acc[ni][mi][r] = -INFINITY;
                }
    }
    // 1. per row: (best value, column) over (ni, r) in the lane, over the four 16-lane groups by permlane swaps, then per column wave into LDS;
    //    the label's logit leaves from the lane that holds its column
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int row = wm * WM + mi * 16 + fr;
        const int m = m0 + row;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[ni][mi][r];
                if (z > bv) { bv = z; bi = ncol0 + ni * 16 + r; }          // ascending columns: the first maximum stays
            }
        const int lc = (m < p.M ? p.labels[m] : -1) - ncol0;               // label column relative to this lane's first column
        if (lc >= 0 && lc < WN && (lc & 15) < 4) {
            float zl = 0.f;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (lc == ni * 16 + r) zl = acc[ni][mi][r];
            if (ncol0 + lc < p.N) p.zlab[m] = zl;
        }
        float a, b, ia, ib;
        xor32_pair(bv, a, b); xor32_pair(__int_as_float(bi), ia, ib);
        bv = a; bi = __float_as_int(ia); best_merge(bv, bi, b, __float_as_int(ib));
        xor16_pair(bv, a, b); xor16_pair(__int_as_float(bi), ia, ib);
        bv = a; bi = __float_as_int(ia); best_merge(bv, bi, b, __float_as_int(ib));
        if (fg == 0) { redv[row * 4 + wn] = bv; redi[row * 4 + wn] = bi; }
    }
    __syncthreads();
    // 2. sum exp(z - max) against the row maximum of the whole tile (finite: every tile has a column < N)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int row = wm * WM + mi * 16 + fr;
        const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(redv + row * 4);
        const float mx = fmaxf(fmaxf(mv[0], mv[1]), fmaxf(mv[2], mv[3]));
        float s = 0.f;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += __expf(acc[ni][mi][r] - mx);
        float a, b;
        xor32_pair(s, a, b); s = a + b;
        xor16_pair(s, a, b); s = a + b;
        if (fg == 0) reds[row * 4 + wn] = s;
    }
    __syncthreads();
    // 3. one record per row of the tile
    if (tid < XBM && m0 + tid < p.M) {
        const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(redv + tid * 4);
        const f32x4_t sv = *reinterpret_cast<const f32x4_t*>(reds + tid * 4);
        float bv = mv[0];
        int bi = redi[tid * 4];
#pragma unroll
        for (int w = 1; w < 4; ++w) best_merge(bv, bi, mv[w], redi[tid * 4 + w]);
        const float s = ((sv[0] + sv[1]) + sv[2]) + sv[3];
        p.part[(long)(m0 + tid) * p.tiles_n + tn] = f32x4_t{bv, s, bv, __int_as_float(bi)};
    }
}

// One wave per row: the row's tiles_n records -> lse = max + log(sum), logprob = z_label - lse (0 without a label), argmax (first maximum).
// The tile sums are rescaled and added in double, in a fixed order (lane-strided, then the butterfly): two runs give the same bits.
__global__ __launch_bounds__(256) void xent_finish_kernel(const f32x4_t* __restrict__ part, const float* __restrict__ zlab, const int* __restrict__ labels,
                                                          int M, int N, int tiles_n, float* __restrict__ logprob, float* __restrict__ lse,
                                                          int* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const f32x4_t* rec = part + (long)m * tiles_n;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int t = lane; t < tiles_n; t += 64) {
        const f32x4_t r = rec[t];
        best_merge(bv, bi, r[2], __float_as_int(r[3]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        best_merge(bv, bi, ov, oi);
    }
    double s = 0.0;
    for (int t = lane; t < tiles_n; t += 64) {
        const f32x4_t r = rec[t];
        s += (double)r[1] * exp((double)r[0] - (double)bv);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        const double l = (double)bv + log(s);
        const int lab = labels[m];
        lse[m] = (float)l;
        logprob[m] = (lab >= 0 && lab < N) ? (float)((double)zlab[m] - l) : 0.f;
        argmax[m] = bi;
    }
}

// One block per sequence over the compacted rows seq_off[b] .. seq_off[b + 1]: sum of log-probs, labelled tokens, tokens whose argmax is the
// label.  Thread-strided partials in double, then a fixed LDS tree: no atomics, bit-identical between runs.
__global__ __launch_bounds__(256) void xent_seq_reduce_kernel(const float* __restrict__ logprob, const int* __restrict__ labels, const int* __restrict__ argmax,
                                                              const int* __restrict__ seq_off, float* __restrict__ sum_logprob,
                                                              int* __restrict__ n_tokens, int* __restrict__ n_correct) {
    __shared__ double ss[256];
    __shared__ int sn[256], sc[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int r0 = seq_off[b], r1 = seq_off[b + 1];
    double s = 0.0;
    int n = 0, c = 0;
    for (int r = r0 + tid; r < r1; r += 256) {
        const int lab = labels[r];
        if (lab >= 0) { s += (double)logprob[r]; ++n; c += argmax[r] == lab; }
    }
    ss[tid] = s; sn[tid] = n; sc[tid] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { ss[tid] += ss[tid + o]; sn[tid] += sn[tid + o]; sc[tid] += sc[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { sum_logprob[b] = (float)ss[0]; n_tokens[b] = sn[0]; n_correct[b] = sc[0]; }
}

// batch mean NLL = - sum_b sum_logprob[b] / sum_b n_tokens[b], sequences in order; NaN without a labelled token (CrossEntropyLoss's 0 / 0)
__global__ void xent_mean_kernel(const float* __restrict__ sum_logprob, const int* __restrict__ n_tokens, int B, float* __restrict__ mean_nll) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    long n = 0;
    for (int b = 0; b < B; ++b) { s += (double)sum_logprob[b]; n += n_tokens[b]; }
    mean_nll[0] = n > 0 ? (float)(-s / (double)n) : __int_as_float(0x7fc00000);
}

inline hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace

extern "C" int64_t crab_lm_head_xent_workspace(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    const int64_t tiles_n = (N + XBN - 1) / XBN;
    return (int64_t)M * tiles_n * 16 + (((int64_t)M * 4 + 15) & ~(int64_t)15);
}

extern "C" int crab_lm_head_xent(crab_ctx* ctx, void* stream, const void* x, int64_t ldx, const int32_t* row_idx, int M, const void* w, int64_t ldw,
                                 int N, int K, const int32_t* labels, float* logprob, float* lse, int32_t* argmax, void* workspace,
                                 int64_t workspace_bytes) {
    if (!ctx) return CRAB_E_INVALID;
    if (!x || !w || !labels || !logprob || !lse || !argmax || !workspace) return crab_fail(ctx, CRAB_E_INVALID, "lm_head_xent: null operand");
    if (M <= 0 || N <= 0 || K <= 0) return crab_fail(ctx, CRAB_E_INVALID, "lm_head_xent: non-positive dimension");
    if (K & 7) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "lm_head_xent: K must be a multiple of 8 (16-byte operand chunks, as crab_gemm_bf16)");
    if ((ldx & 7) || (ldw & 7) || ldx < K || ldw < K) return crab_fail(ctx, CRAB_E_INVALID, "lm_head_xent: ldx / ldw must be multiples of 8 and >= K");
    if (((uintptr_t)x & 15) || ((uintptr_t)w & 15) || ((uintptr_t)workspace & 15))
        return crab_fail(ctx, CRAB_E_INVALID, "lm_head_xent: x / w / workspace must be 16-byte aligned");
    const int64_t tiles_m = (M + XBM - 1) / XBM, tiles_n = (N + XBN - 1) / XBN;
    if (tiles_m * tiles_n > 0x7fffffffLL) return crab_fail(ctx, CRAB_E_UNSUPPORTED, "lm_head_xent: more than 2^31 output tiles");
    if (workspace_bytes < crab_lm_head_xent_workspace(M, N)) return crab_fail(ctx, CRAB_E_WORKSPACE, "lm_head_xent: workspace smaller than crab_lm_head_xent_workspace(M, N)");
    XentP p;
    p.A = (const bf16_t*)x; p.B = (const bf16_t*)w; p.row_idx = row_idx; p.labels = labels;
    p.lda = ldx; p.ldb = ldw; p.M = M; p.N = N; p.K = K; p.tiles_m = (int)tiles_m; p.tiles_n = (int)tiles_n;
    p.part = (f32x4_t*)workspace;
    p.zlab = (float*)((char*)workspace + (int64_t)M * tiles_n * 16);
    hipLaunchKernelGGL(lm_head_xent_kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(XWGM * XWGN * 64), 0, S_(stream), p);
    int rc = crab_check_launch(ctx, "lm_head_xent_kernel");
    if (rc != CRAB_OK) return rc;
    hipLaunchKernelGGL(xent_finish_kernel, dim3((M + 3) / 4), dim3(256), 0, S_(stream), p.part, p.zlab, labels, M, N, (int)tiles_n, logprob, lse, argmax);
    return crab_check_launch(ctx, "xent_finish_kernel");
}

extern "C" int crab_xent_reduce(crab_ctx* ctx, void* stream, const float* logprob, const int32_t* labels, const int32_t* argmax, const int32_t* seq_off,
                                int B, float* sum_logprob, int32_t* n_tokens, int32_t* n_correct, float* mean_nll) {
    if (!ctx) return CRAB_E_INVALID;
    if (!seq_off || !sum_logprob || !n_tokens || !n_correct || !mean_nll || B <= 0) return crab_fail(ctx, CRAB_E_INVALID, "xent_reduce: bad argument");
    // logprob / labels / argmax may be NULL only when no row is labelled at all (every seq_off equal): the kernels then read none of them
    hipLaunchKernelGGL(xent_seq_reduce_kernel, dim3(B), dim3(256), 0, S_(stream), logprob, labels, argmax, seq_off, sum_logprob, n_tokens, n_correct);
    int rc = crab_check_launch(ctx, "xent_seq_reduce_kernel");
    if (rc != CRAB_OK) return rc;
    hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(64), 0, S_(stream), sum_logprob, n_tokens, B, mean_nll);
    return crab_check_launch(ctx, "xent_mean_kernel");
}
