"""Thin tensor-level wrappers over the C-ABI (plumbing only: pointers, strides, the current HIP stream).

Every function launches HIP kernels from libcrab_hip.so on torch's current stream and returns/fills
caller-visible torch tensors.  No arithmetic happens in PyTorch here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import torch

from . import _lib
from ._lib import AttnDesc, GemmDesc

ACT = {"none": 0, None: 0, "gelu": 1, "quick_gelu": 2, "relu": 3, "silu": 4, "swiglu_pair": 5}
BF16 = torch.bfloat16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise _lib.CrabHipError("crab_amd ops need CUDA/HIP tensors (no CPU fallback exists)")
    return t.device.index or 0


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _chk_bf16(*ts):
    for t in ts:
        if t is not None and t.dtype != BF16:
            raise _lib.CrabHipError(f"expected bfloat16 storage, got {t.dtype}")


class launch_trace:
    """`with ops.launch_trace(device) as t: ...` -> t.counts = {launch-site name: launches} of every kernel the C-ABI entry points issued inside the
    block (crab_trace_begin / crab_trace_end, include/crab_hip.h).  Names carry the template instantiation where the dispatch has one
    ("attn_decode_kernel<128>", "gemm_bt_ring_kernel+rope2").  The parity tests use it to prove which kernel a fixture was compared through."""

    def __init__(self, device: int = 0):
        self.device = device
        self.counts = {}

    def __enter__(self):
        _lib.check(_lib.load().crab_trace_begin(_lib.ctx(self.device)), self.device)
        return self

    def __exit__(self, *exc):
        lib, h = _lib.load(), _lib.ctx(self.device)
        need = lib.crab_trace_end(h, None, 0)
        buf = C.create_string_buffer(int(need) + 1)
        lib.crab_trace_end(h, buf, len(buf))
        self.counts = {}
        for line in buf.value.decode().splitlines():
            name, _, n = line.rpartition("\t")
            self.counts[name] = int(n)
        return False

    def launched(self, name: str) -> int:
        return self.counts.get(name, 0)


class KernelProfiler:
    """Optional HIP-event timing of kernel launches on the current stream (bench.py roofline leg).  Only used outside
    graph capture; adds two event records per profiled launch.  GEMM launches (M >= min_m) are bucketed by kernel
    variant with their algorithmic FLOPs; the decode-attention kernel is sampled with its algorithmic KV bytes on the
    decode steps GenerationEngine.generate runs eagerly (every `decode_every`-th step; the eager step is bit-identical
    to the HIP-graph replay it stands in for, tests/test_model_gpu.py)."""

    def __init__(self, min_m: int = 512, decode_every: int = 32, phase_only: bool = False):
        """phase_only: record nothing but the three phase marks of a generate() call (encode_begin / prefill_end / decode_end) - the SHIPPED path
        runs underneath (native layer sequencers, every decode step a graph replay); three event records per call are the whole footprint."""
        self.phase_only = phase_only
        self.min_m = (1 << 62) if phase_only else min_m
        self.decode_every = 0 if phase_only else decode_every
        self.decode_ctx = 0          # live KV length of the sampled step (host mirror of the device position word)
        self.decode_eager = False    # set by GenerationEngine.generate around a sampled eager decode step
        self.marks = []              # (phase name, event)
        self.records = []            # (variant, work, start_event, end_event); work = FLOPs ("gemm*") or bytes ("attn_decode*")

    def mark(self, name: str):
        """Phase boundary on the current stream (encode_begin / prefill_end / decode_end of one generate call)."""
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def phase_ms(self):
        """Sum over generate calls of (encoders + prefill) and decode time, from the phase marks."""
        torch.cuda.synchronize()
        pre = dec = 0.0
        last = {}
        for name, e in self.marks:
            if name == "prefill_end" and "encode_begin" in last:
                pre += last["encode_begin"].elapsed_time(e)
            if name == "decode_end" and "prefill_end" in last:
                dec += last["prefill_end"].elapsed_time(e)
            last[name] = e
        return pre, dec

    def summary(self):
        """{kernel variant: {launches, work, ms, classes: {class: {launches, work, ms}}}}; a record's variant may carry a class after
        '|' (GEMMs: 'decoder' = hyper-LoRA projections of the decoder, 'encoder' = CLIP / BEATs / Q-Former / head shapes)."""
        torch.cuda.synchronize()
        out = {}
        for variant, work, e0, e1 in self.records:
            variant, _, cls = variant.partition("|")
            ms = e0.elapsed_time(e1)
            d = out.setdefault(variant, {"launches": 0, "work": 0.0, "ms": 0.0, "classes": {}})
            for tgt in (d, d["classes"].setdefault(cls, {"launches": 0, "work": 0.0, "ms": 0.0}) if cls else None):
                if tgt is not None:
                    tgt["launches"] += 1
                    tgt["work"] += work
                    tgt["ms"] += ms
        return out


GemmProfiler = KernelProfiler

PROFILER: Optional[KernelProfiler] = None


def per_launch_profiling() -> bool:
    """True while a profiler that times individual launches is attached: the layer sequences then run launch by launch from Python (same launches,
    same order) so that ops.gemm sees every GEMM; a phase-only profiler leaves the native C sequencers in place."""
    return PROFILER is not None and not PROFILER.phase_only


def _variant(M: int, N: int, batch: int = 1, K: int = 4096) -> str:
    """Mirror of the tile choice in csrc/gemm.hip (crab_gemm_bf16) - the bucket NAME of the profiler's records."""
    if batch == 1 and 256 < M <= DECODE_MAX_ROWS:
        return "gemm_dec2_kernel"                     # two 256-row groups per block (a workspace is always handed in at these row counts)
    if batch == 1 and 64 < M <= 256:
        return "gemm_dec_ws_kernel"
    big = ((M + 127) // 128) * ((N + 127) // 128) * batch
    if M <= 64 or N <= 64 or big < 192:
        return "gemm_bt_kernel<64,64>"
    big256 = ((M + 255) // 256) * ((N + 255) // 256) * batch
    rounds = (big256 + 255) // 256
    ring = big256 >= 120 and big256 * 100 >= rounds * 256 * 55 and M >= 1024 and N >= 1024 and K >= 1024
    return "gemm_bt_ring_kernel<256,256>" if ring else "gemm_bt_glds_kernel<128,128>"


# The residual stream (decoder x, CLIP tower x, the pre-LN sums of the post-LN encoders) is kept in fp32: the reference adds its residuals in
# fp32 (models/modeling_llama.py:805-827 run with --bf16 False, scripts/quick_start.sh:42-44) and a bf16 rounding of x per sub-layer is what put
# the 32-layer logits 1.7e-2 away from it.  CRAB_RESIDUAL_FP32=0 restores the all-bf16 storage of r01-r03 (A/B runs only).
RESIDUAL_FP32 = os.environ.get("CRAB_RESIDUAL_FP32", "1") != "0"
RES_DTYPE = torch.float32 if RESIDUAL_FP32 else torch.bfloat16

# The LayerNorm weights / biases of the encoders (CLIP, BEATs, both Q-Formers, the projector norms, SegModule) are kept in fp32 (r05): they are
# not matrix operands, and rounding them to bf16 put a systematic 2^-9 relative error on every channel of every LayerNorm output - the largest
# single removable contribution to the encoders' distance from the fp32 reference (scripts/parity_floor.py).  CRAB_NORM_FP32=0
# restores the bf16 parameters of r01-r04 (A/B runs only).  The decoder's RMSNorm weights stay bf16 (their row-owning fused forms are tuned at the
# instruction level; measured cost 6e-4 of the logit scale on the tiny stacks).
NORM_PARAMS_FP32 = os.environ.get("CRAB_NORM_FP32", "1") != "0"
NORM_DTYPE = torch.float32 if NORM_PARAMS_FP32 else torch.bfloat16
# ... and so are the decoder's RMSNorm weights (input_layernorm / post_attention_layernorm / model.norm) wherever the residual stream is fp32
# (crab_gemm_desc.norm_w_fp32, crab_llama_layer.norm_w_fp32, crab_rmsnorm_p): with a real checkpoint's weights their bf16 rounding is worth
# 6e-4 of the logit scale on the 2-layer fixtures (the synthetic full-size model has norm weights of exactly 1, which hides it).
RMS_DTYPE = torch.float32 if (NORM_PARAMS_FP32 and os.environ.get("CRAB_RESIDUAL_FP32", "1") != "0") else torch.bfloat16

# CRAB_DECODE_MAX_ROWS, read from include/crab_hip.h (one source; _lib.load() checks it against the built library): up to this many rows a
# GEMM with a workspace streams the weights once
DECODE_MAX_ROWS = _lib.header_const("CRAB_DECODE_MAX_ROWS")

ROWFIN = os.environ.get("CRAB_ROWFIN", "1") != "0"     # the M <= 16 layer tail of csrc/rowfin.hip (same switch, same parse as the library: off iff the value is exactly "0")


def rowfin_lora_ok(nl: int, r: int, N: int) -> bool:
    """crab_rowfin_lora_ok: the library's own predicate for the in-call hyper-LoRA form (lora_self) - the one run_group (csrc/llama_layer.hip) uses."""
    return bool(_lib.load().crab_rowfin_lora_ok(int(nl), int(r), int(N)))

_SPLITK_WS = {}
WS_SLOT = 0      # scratch slot of the launches being issued/captured: groups decoding concurrently on different HIP streams
                 # (GenerationEngine.generate, decode_streams > 1) must not share the split-K partial slabs


def _splitk_workspace(device) -> torch.Tensor:
    """One caller-owned split-K scratch per device (stable address: safe under HIP-graph capture)."""
    key = (device.index or 0, WS_SLOT)
    if key not in _SPLITK_WS:
        _SPLITK_WS[key] = torch.empty((256 << 20,), device=device, dtype=torch.uint8)
    return _SPLITK_WS[key]


def gemm(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
         residual: Optional[torch.Tensor] = None, res_scale: float = 1.0, x2: Optional[torch.Tensor] = None,
         w2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_fp32: bool = False, tune: int = 0,
         post_norm=None, rope=None, route=None, lora_self=None, info: Optional[dict] = None, prof_class: Optional[str] = None,
         rope_row_off: Optional[torch.Tensor] = None, w8=None) -> torch.Tensor:
    """out[M,N] = res_scale*residual + act(x[M,K] @ w[N,K]^T + x2 @ w2^T + bias).  2-D row-strided operands.
    w8 = (codes uint8 [N, K], scale fp32 [N]) (weight_quant_fp8 of w; M <= 16 only): the opt-in FP8 weights - the product is
    scale[n] * sum_k float(codes[n, k]) x[m, k], streamed by gemm_skinny_dma_w8_kernel; w2 / bias / lora_self stay bf16.  The library refuses
    the call (CrabHipError) wherever that kernel would not run; it never falls back to w.
    rope = (tab, k_cache, v_cache, H, Hk, d, Tmax, pos0, pos_dev): packed q|k|v projection of ONE row per sequence followed
    by RoPE + KV-cache append (== qkv_rope_split(B=M, S=1) on out), fused into the split-K reduction when there is one.
    rope = (..., pos_dev = None, S, pos_ids[, vt]): the PREFILL form, S rows per sequence - when the library says so (info["fused_prefill_rope"]
    = crab_gemm_fuses_prefill_rope: 1 or 2) q is rotated in place and k rotated into the cache by the projection's epilogue; at 1 the caller
    finishes with qkv_rope_split(rope_tab=None, k_cache=None) for the v columns, at 2 (vt given) the epilogue did those too; at 0 the caller
    runs the full qkv_rope_split as before.
    route = (RA, nproj, nl, r, ucols, scaling, u_out) (with post_norm, M <= DECODE_MAX_ROWS): u_out = hyperlora_route(post-norm rows, RA)
    for the NEXT projection group, computed inside the row-owning reduction kernel when that path is taken.
    lora_self = (RA, nl, r, scaling, lora_B) (with post_norm, M <= 16, no x2): the hyper-LoRA update of THIS single-projection group is
    evaluated inside the call - its router rows ride on the projection's launch, the update is applied by the M <= 16 layer tail.
    rope_row_off (int32 [M], decode form of `rope` only): the RAGGED decode batch - row m is rotated at slot - rope_row_off[m] while its
    K / V rows land in the common slot (crab_gemm_desc.rope_row_off).
    act == "swiglu_pair": w rows are interleaved (gate_i, up_i) and out is [M, N/2] = silu(gate) * up."""
    _chk_bf16(x, w, bias, x2, w2)
    if residual is not None and residual.dtype not in (BF16, torch.float32):
        raise _lib.CrabHipError(f"residual must be bfloat16 or float32, got {residual.dtype}")
    d = _dev(x)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1
    if out is None:
        out = torch.empty((M, N // 2 if act == "swiglu_pair" else N), device=x.device, dtype=torch.float32 if out_fp32 else BF16)
    g = GemmDesc()
    g.A, g.B, g.C = x.data_ptr(), w.data_ptr(), out.data_ptr()
    g.bias = bias.data_ptr() if bias is not None else None
    g.R = residual.data_ptr() if residual is not None else None
    g.lda, g.ldb, g.ldc = x.stride(0), w.stride(0), out.stride(0)
    g.ldr = residual.stride(0) if residual is not None else 0
    g.r_fp32 = 1 if (residual is not None and residual.dtype == torch.float32) else 0
    if x2 is not None:
        assert w2 is not None and x2.shape[1] == w2.shape[1] and x2.shape[0] == M and w2.shape[0] == N
        g.A2, g.B2, g.lda2, g.ldb2, g.K2 = x2.data_ptr(), w2.data_ptr(), x2.stride(0), w2.stride(0), x2.shape[1]
    g.M, g.N, g.K = M, N, K
    g.act = ACT[act]
    g.c_fp32 = 1 if out.dtype == torch.float32 else 0
    g.res_scale = res_scale
    g.batch, g.nb0 = 1, 1
    g.tune = tune
    if post_norm is not None:                      # (weight, eps, out): out = rmsnorm(result) * weight, fused when possible
        g.norm_w, g.norm_eps, g.norm_out, g.ld_norm = post_norm[0].data_ptr(), post_norm[1], post_norm[2].data_ptr(), post_norm[2].stride(0)
        g.norm_w_fp32 = 1 if post_norm[0].dtype == torch.float32 else 0
    if route is not None:
        assert post_norm is not None and M <= DECODE_MAX_ROWS
        rRA, rnp, rnl, rr, ruc, rsc, ru = route
        g.route_RA, g.route_U, g.route_ldra, g.route_ldu = rRA.data_ptr(), ru.data_ptr(), rRA.stride(0), ru.stride(0)
        g.route_nproj, g.route_nl, g.route_r, g.route_ucols, g.route_scaling = rnp, rnl, rr, ruc, rsc
    if lora_self is not None:
        assert x2 is None and post_norm is not None
        lRA, lnl, lr, lsc, lB = lora_self
        _chk_bf16(lRA, lB)
        g.lora_RA, g.lora_ldra, g.lora_nl, g.lora_r, g.lora_scaling = lRA.data_ptr(), lRA.stride(0), lnl, lr, lsc
        g.B2, g.ldb2, g.K2 = lB.data_ptr(), lB.stride(0), lB.shape[1]
    if rope is not None and len(rope) > 9 and int(rope[9]) <= 1:
        # the prefill form with ONE row per sequence: the library would read these fields as the decode form (rope_S <= 1: rotation at pos0 /
        # pos_dev, no rotary position ids) and still answer "not fused" to the prefill question - the caller's split pass would then rotate a
        # second time (harmless only at position 0).  Nothing to fuse at one row per sequence: plain projection, the caller runs the split.
        if info is not None:
            info["fused_prefill_rope"] = 0
        rope = None
    if rope is not None:
        tab, kcache, vcache, rH, rHk, rd, rT, rp0, rpd = rope[:9]
        g.rope_tab, g.rope_k_cache, g.rope_v_cache = tab.data_ptr(), kcache.data_ptr(), vcache.data_ptr()
        g.rope_pos_dev = rpd.data_ptr() if rpd is not None else None
        g.rope_H, g.rope_Hk, g.rope_d, g.rope_Tmax, g.rope_pos0 = rH, rHk, rd, rT, rp0
        if rope_row_off is not None:
            if len(rope) > 9:
                raise ValueError("rope_row_off belongs to the decode form of the fused RoPE")
            if rope_row_off.dtype != torch.int32 or rope_row_off.numel() < M or not rope_row_off.is_contiguous():
                raise ValueError("rope_row_off must be a contiguous int32 [M] tensor")
            g.rope_row_off = rope_row_off.data_ptr()
        if len(rope) > 9:                          # prefill form: S rows per sequence (+ optional rotary positions [B, S] int32)
            g.rope_S = int(rope[9])
            pid = rope[10] if len(rope) > 10 else None
            if pid is not None:
                assert pid.dtype == torch.int32 and pid.stride(-1) == 1
                g.rope_pos_ids, g.rope_ld_pos = pid.data_ptr(), pid.stride(0)
            if len(rope) > 11 and rope[11] is not None:           # V^T scratch [B, Hk, d, vt_ld]: the v columns in the epilogue too
                g.rope_vt, g.rope_vt_ld = rope[11].data_ptr(), rope[11].stride(-2)
            if info is not None:                                   # 0: not fused; 1: q / k; 2: q / k / v (no split pass left)
                info["fused_prefill_rope"] = int(_lib.load().crab_gemm_fuses_prefill_rope(C.byref(g)))
    if w8 is not None:
        codes, wsc = w8
        if codes.dtype != torch.uint8 or wsc.dtype != torch.float32 or tuple(codes.shape) != (N, K) or codes.stride(1) != 1 or wsc.numel() != N or \
                not wsc.is_contiguous() or codes.device != x.device or wsc.device != x.device:
            raise ValueError("w8 = (codes uint8 [N, K], scale fp32 [N]) on the device of x, as weight_quant_fp8 returns them")
        g.B8, g.ldb8, g.b_scale = codes.data_ptr(), codes.stride(0), wsc.data_ptr()
    if M <= DECODE_MAX_ROWS:
        ws = _splitk_workspace(x.device)
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel()
    prof = PROFILER
    if prof is not None and M >= prof.min_m and not torch.cuda.is_current_stream_capturing():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.load().crab_gemm_bf16(_lib.ctx(d), _stream(), C.byref(g)), d)
        e1.record()
        # class of the launch for bench.py's by_class split: stated by the caller (PackedLinearGroup.prof_class: "decoder" for every projection
        # of the decoder stack, adapted or not; "head" for lm_head); un-tagged launches are the encoders' / projectors'
        k2 = x2.shape[1] if x2 is not None else (lora_self[4].shape[1] if lora_self is not None else 0)
        prof.records.append((_variant(M, N, 1, K) + "|" + (prof_class or "encoder"), 2.0 * M * N * (K + k2), e0, e1))
        return out
    _lib.check(_lib.load().crab_gemm_bf16(_lib.ctx(d), _stream(), C.byref(g)), d)
    return out


def gemm_desc(desc: GemmDesc, device: int = 0):
    """Raw descriptor launch (batched / strided forms)."""
    _lib.check(_lib.load().crab_gemm_bf16(_lib.ctx(device), _stream(), C.byref(desc)), device)


def hyperlora_mix(t: torch.Tensor, nproj: int, nl: int, r: int, ucols: int, scaling: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    d = _dev(t)
    M = t.shape[0]
    if out is None:
        out = torch.empty((M, ucols), device=t.device, dtype=BF16)
    _lib.check(_lib.load().crab_hyperlora_mix(_lib.ctx(d), _stream(), _p(t), t.stride(0), 1 if t.dtype == torch.float32 else 0,
                                              _p(out), out.stride(0), M, nproj, nl, r, ucols, scaling), d)
    return out


def hyperlora_route_workspace(M: int, K: int, tcols: int) -> int:
    return int(_lib.load().crab_hyperlora_route_workspace(M, K, tcols))


def hyperlora_route(x: torch.Tensor, ra: torch.Tensor, nproj: int, nl: int, r: int, ucols: int, scaling: float,
                    out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """U[M,ucols] = routing mix of x @ [R;A]^T (split-K skinny product + fixed-order reduce + fp32 softmax)."""
    _chk_bf16(x, ra)
    d = _dev(x)
    M, K = x.shape
    if out is None:
        out = torch.empty((M, ucols), device=x.device, dtype=BF16)
    need = hyperlora_route_workspace(M, K, ra.shape[0])
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need,), device=x.device, dtype=torch.uint8)
    _lib.check(_lib.load().crab_hyperlora_route(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(ra), ra.stride(0), M, K, nproj, nl, r,
                                                _p(out), out.stride(0), ucols, scaling, _p(workspace),
                                                workspace.numel() * workspace.element_size()), d)
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16, or fp32 (a row of the fp32 residual stream: no intermediate rounding of x_hat); w bf16 or fp32 (RMS_DTYPE); out bf16."""
    d = _dev(x)
    M, D = x.shape
    if out is None:
        out = torch.empty((M, D), device=x.device, dtype=BF16)
    wf = w.dtype == torch.float32
    if not wf:
        _chk_bf16(w)
    if x.dtype != torch.float32:
        _chk_bf16(x)
    _lib.check(_lib.load().crab_rmsnorm_p(_lib.ctx(d), _stream(), _p(x), 1 if x.dtype == torch.float32 else 0, x.stride(0), _p(w), 1 if wf else 0,
                                          _p(out), out.stride(0), M, D, eps), d)
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 or fp32 rows (residual stream / pre-LN sums); w / b bf16 or - both - fp32 (NORM_DTYPE); out bf16."""
    d = _dev(x)
    M, D = x.shape
    if out is None:
        out = torch.empty((M, D), device=x.device, dtype=BF16)
    wf = w.dtype == torch.float32
    if not wf:
        _chk_bf16(w, b)
    elif b is not None and b.dtype != torch.float32:
        raise _lib.CrabHipError("layernorm: weight and bias must have the same storage (both bfloat16 or both float32)")
    if x.dtype != torch.float32:
        _chk_bf16(x)
    _lib.check(_lib.load().crab_layernorm_p(_lib.ctx(d), _stream(), _p(x), 1 if x.dtype == torch.float32 else 0, x.stride(0), _p(w), _p(b),
                                            1 if wf else 0, _p(out), out.stride(0), M, D, eps), d)
    return out


def embedding(ids: torch.Tensor, table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_bf16(table)
    d = _dev(table)
    ids = ids.reshape(-1).to(device=table.device, dtype=torch.int64).contiguous()
    T, D = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty((T, D), device=table.device, dtype=BF16)
    if T:
        fn = _lib.load().crab_embedding_f32 if out.dtype == torch.float32 else _lib.load().crab_embedding      # fp32: the residual stream's first row
        _lib.check(fn(_lib.ctx(d), _stream(), _p(ids), _p(table), _p(out), out.stride(0), T, D, table.shape[0]), d)
    return out


def cast_rows(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, lds: Optional[int] = None):
    """dst[r, :cols] = src[r, :cols] across bf16 <-> fp32 (or a plain copy when the dtypes agree); row-strided 2-D views."""
    d = _dev(src)
    lds = src.stride(0) if lds is None else lds
    if src.dtype == dst.dtype:
        return copy_rows(src, dst, rows, cols, lds=lds)
    if src.dtype == BF16 and dst.dtype == torch.float32:
        _lib.check(_lib.load().crab_cast_rows_bf16_f32(_lib.ctx(d), _stream(), _p(src), lds, _p(dst), dst.stride(0), rows, cols), d)
    elif src.dtype == torch.float32 and dst.dtype == BF16:
        _lib.check(_lib.load().crab_cast_rows_f32_bf16(_lib.ctx(d), _stream(), _p(src), lds, _p(dst), dst.stride(0), rows, cols), d)
    else:
        raise _lib.CrabHipError(f"cast_rows: {src.dtype} -> {dst.dtype} is not supported")
    return dst


def rope_table(max_pos: int, head_dim: int, theta: float, device) -> torch.Tensor:
    tab = torch.empty((max_pos, head_dim // 2, 2), device=device, dtype=torch.float32)
    d = _dev(tab)
    _lib.check(_lib.load().crab_rope_table(_lib.ctx(d), _stream(), _p(tab), max_pos, head_dim, theta), d)
    return tab


def qkv_rope_split(qkv: torch.Tensor, rope_tab: Optional[torch.Tensor], k_cache: Optional[torch.Tensor],
                   v_cache: Optional[torch.Tensor], vt: Optional[torch.Tensor], B: int, S: int, H: int, Hk: int, d_: int,
                   Tmax: int, pos0: int = 0, pos_dev: Optional[torch.Tensor] = None, pos_ids: Optional[torch.Tensor] = None,
                   row_off: Optional[torch.Tensor] = None):
    """pos_ids (int32 [B, S]): explicit rotary positions (forward()'s position_ids); the cache slot stays pos0 + s.
    row_off (int32 [B]): the ragged form - sequence b is rotated at slot - row_off[b] (crab_qkv_rope_split_ragged)."""
    d = _dev(qkv)
    vt_ld = vt.stride(-2) if vt is not None else 0
    if row_off is not None:
        if pos_ids is not None:
            raise ValueError("qkv_rope_split: pos_ids and row_off are alternatives")
        _lib.check(_lib.load().crab_qkv_rope_split_ragged(_lib.ctx(d), _stream(), _p(qkv), qkv.stride(0), _p(rope_tab), _p(k_cache), _p(v_cache),
                                                          _p(vt), vt_ld, B, S, H, Hk, d_, Tmax, pos0, _p(pos_dev), _p(row_off)), d)
        return
    if pos_ids is not None and (pos_ids.dtype != torch.int32 or pos_ids.dim() != 2 or pos_ids.stride(1) != 1):
        raise ValueError("pos_ids must be an int32 [B, S] tensor with contiguous rows")
    _lib.check(_lib.load().crab_qkv_rope_split_ids(_lib.ctx(d), _stream(), _p(qkv), qkv.stride(0), _p(rope_tab), _p(k_cache), _p(v_cache),
                                                   _p(vt), vt_ld, B, S, H, Hk, d_, Tmax, pos0, _p(pos_dev), _p(pos_ids),
                                                   pos_ids.stride(0) if pos_ids is not None else 0), d)


def attn_fwd(q, k, vt, o, *, q_strides, k_strides, vt_strides, o_strides, B, H, Hk, Sq, Skv, head_dim, scale, causal=False,
             bias=None, gate=None, kv_start=None, key_mask=None):
    """Strided flash attention; *_strides = (batch, head, row) element strides, o_strides = (batch, row).
    kv_start (int32 [B]): keys below kv_start[b] are masked (left-pad attention_mask); key_mask (int32 [B, >= ceil(Skv / 32)], one
    visibility bit per key: pack_key_mask): any 2-D attention_mask."""
    d = _dev(q)
    a = AttnDesc()
    a.q, a.k, a.vt, a.o = q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr()
    a.q_bs, a.q_hs, a.q_ss = q_strides
    a.k_bs, a.k_hs, a.k_ss = k_strides
    a.vt_bs, a.vt_hs, a.vt_ds = vt_strides
    a.o_bs, a.o_ss = o_strides
    a.bias = bias.data_ptr() if bias is not None else None
    a.gate = gate.data_ptr() if gate is not None else None
    a.kv_start = kv_start.data_ptr() if kv_start is not None else None
    if key_mask is not None:
        if key_mask.dtype != torch.int32 or key_mask.dim() != 2 or key_mask.stride(1) != 1 or key_mask.shape[0] != B:
            raise ValueError("key_mask must be an int32 [B, words] tensor with contiguous rows (ops.pack_key_mask)")
        a.key_mask, a.key_mask_ld = key_mask.data_ptr(), key_mask.stride(0)
    a.B, a.H, a.Hk, a.Sq, a.Skv, a.head_dim, a.causal, a.scale = B, H, Hk, Sq, Skv, head_dim, 1 if causal else 0, scale
    _lib.check(_lib.load().crab_attn_fwd(_lib.ctx(d), _stream(), C.byref(a)), d)
    return o


def pack_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """2-D attention_mask [B, T] (non-zero = attend) -> int32 [B, ceil(T / 32)] visibility words, bit (j & 31) of word j >> 5 = key j
    (crab_attn_desc.key_mask's layout), on the mask's device."""
    m = mask.reshape(mask.shape[0], -1).ne(0)
    B, T = m.shape
    W = (T + 31) // 32
    mp = torch.zeros(B, W * 32, dtype=torch.int64, device=m.device)
    mp[:, :T] = m
    v = (mp.view(B, W, 32) << torch.arange(32, device=m.device)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).contiguous()


def attn_decode(q, k_cache, v_cache, o, B, H, Hk, head_dim, Tmax, ctx_len, scale, ctx_dev=None, kv_start=None, key_mask=None):
    d = _dev(q)
    if key_mask is not None:                          # general attention_mask over the cache rows: its own (rare-path) kernel
        if kv_start is not None:
            raise ValueError("attn_decode: key_mask already carries the left padding, pass one of the two")
        if key_mask.dtype != torch.int32 or key_mask.dim() != 2 or key_mask.stride(1) != 1 or key_mask.shape[0] != B:
            raise ValueError("key_mask must be an int32 [B, words] tensor with contiguous rows (ops.pack_key_mask)")
        _lib.check(_lib.load().crab_attn_decode_keymask(_lib.ctx(d), _stream(), _p(q), q.stride(0), _p(k_cache), _p(v_cache), _p(o), o.stride(0),
                                                        B, H, Hk, head_dim, Tmax, ctx_len, _p(ctx_dev), scale, _p(key_mask), key_mask.stride(0)), d)
        return o
    prof = PROFILER
    sample = prof is not None and prof.decode_eager and prof.decode_ctx > 0 and not torch.cuda.is_current_stream_capturing()
    if sample:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(_lib.load().crab_attn_decode_masked(_lib.ctx(d), _stream(), _p(q), q.stride(0), _p(k_cache), _p(v_cache), _p(o), o.stride(0),
                                                   B, H, Hk, head_dim, Tmax, ctx_len, _p(ctx_dev), scale, _p(kv_start)), d)
    if sample:
        e1.record()
        # algorithmic bytes (DESIGN.md kernel table): every live K and V row once + q in + o out
        nbytes = 2.0 * B * prof.decode_ctx * Hk * head_dim * 2 + 2.0 * B * H * head_dim * 2
        G = H // Hk                                   # mirror of the kernel choice in csrc/attn.hip (crab_attn_decode)
        gqa = head_dim == 128 and G in (2, 4, 7, 8) and B * Hk >= 256
        prof.records.append((f"attn_decode_gqa_kernel<{head_dim},{G}>" if gqa else f"attn_decode_kernel<{head_dim}>", nbytes, e0, e1))
    return o


ATTN_SPLIT_BELOW = _lib.header_const("CRAB_ATTN_SPLIT_BELOW")


def attn_decode_rope_bytes(B: int, H: int, d: int) -> int:
    return int(_lib.load().crab_attn_decode_rope_workspace(B, H, d))


def attn_decode_rope_workspace(B: int, H: int, d: int, device) -> torch.Tensor:
    """Zero-filled workspace of crab_attn_decode_rope (the tickets at its end must start at zero; the kernel leaves them zero)."""
    return torch.zeros((int(_lib.load().crab_attn_decode_rope_workspace(B, H, d)),), device=device, dtype=torch.uint8)


def attn_decode_rope(qkv, rope_tab, k_cache, v_cache, o, B, H, Hk, head_dim, Tmax, pos0, scale, pos_dev=None, workspace=None):
    """RoPE of q / new k + KV append + decode attention over keys 0 .. pos from the raw packed q|k|v rows (small batch)."""
    d = _dev(qkv)
    _lib.check(_lib.load().crab_attn_decode_rope(_lib.ctx(d), _stream(), _p(qkv), qkv.stride(0), _p(rope_tab), _p(k_cache), _p(v_cache), _p(o),
                                                 o.stride(0), B, H, Hk, head_dim, Tmax, pos0, _p(pos_dev), scale, _p(workspace),
                                                 workspace.numel() if workspace is not None else 0), d)
    return o


def kv_quant_fp8(k_src, v_src, k_codes, v_codes, k_scale, v_scale, b0: int = 0, t0: int = 0, t_dst: int = 0, S: Optional[int] = None,
                 row_off: Optional[torch.Tensor] = None):
    """bf16 cache block [L, Bc, Hk, T_src, d] (rows t0 .. t0 + S - 1 live) -> the FP8 KV cache: e4m3fn codes uint8 [L, B, Hk, Tmax, d] and fp32 row
    scales [L, B, Hk, Tmax], sequences b0 .. b0 + Bc - 1, slots t_dst .. t_dst + S - 1 (crab_kv_quant_fp8; include/crab_hip.h for the format).
    row_off (int32 [Bc]): the first row_off[b] rows of sequence b are front padding - neither read nor written."""
    d = _dev(k_src)
    _chk_bf16(k_src, v_src)
    L, Bc, Hk, Tsrc, hd = k_src.shape
    Tmax = k_codes.shape[3]
    if k_codes.dtype != torch.uint8 or v_codes.dtype != torch.uint8 or k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
        raise _lib.CrabHipError("kv_quant_fp8: codes are uint8, scales float32")
    for t in (k_src, v_src, k_codes, v_codes, k_scale, v_scale):
        if not t[0].is_contiguous():
            raise _lib.CrabHipError("kv_quant_fp8: every layer of the block / cache must be contiguous")
    if (v_src.shape != k_src.shape or v_codes.shape != k_codes.shape or tuple(k_codes.shape[i] for i in (0, 2, 4)) != (L, Hk, hd) or
            tuple(k_scale.shape) != tuple(k_codes.shape[:4]) or v_scale.shape != k_scale.shape or b0 < 0 or b0 + Bc > k_codes.shape[1]):
        raise _lib.CrabHipError("kv_quant_fp8: the block [L, Bc, Hk, T_src, d], the codes [L, B, Hk, Tmax, d] and the scales [L, B, Hk, Tmax] do not match")
    if row_off is not None and (row_off.dtype != torch.int32 or row_off.dim() != 1 or row_off.shape[0] < Bc or not row_off.is_contiguous()):
        raise ValueError("row_off must be a contiguous int32 [Bc] tensor")
    S = Tsrc - t0 if S is None else S
    _lib.check(_lib.load().crab_kv_quant_fp8(_lib.ctx(d), _stream(), _p(k_src), _p(v_src), k_src.stride(0), Tsrc, t0, _p(k_codes), _p(v_codes),
                                             k_codes.stride(0), _p(k_scale), _p(v_scale), k_scale.stride(0), L, Bc, Hk, hd, Tmax, b0, t_dst, S,
                                             _p(row_off)), d)


def weight_quant_fp8(w: torch.Tensor, codes: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """crab_weight_quant_fp8: w [N, K] bf16 (row stride a multiple of 8) -> (codes uint8 [N, K], scale fp32 [N]): OCP e4m3fn with one scale per
    row, scale = amax / 448 (1.0 for an all-zero row, floored at FLT_MIN), code = e4m3fn_rne(w * (1 / scale)) - tests/w8_ref.py states it in
    torch.  codes may be a view with a row stride > K (a multiple of 16 bytes); fresh ones are allocated with K rounded up to 16."""
    _chk_bf16(w)
    d = _dev(w)
    N, K = w.shape
    if w.stride(1) != 1:
        raise ValueError("weight_quant_fp8: rows of w must be contiguous")
    if codes is None:
        codes = torch.empty((N, (K + 15) // 16 * 16), device=w.device, dtype=torch.uint8)[:, :K]
    if scale is None:
        scale = torch.empty((N,), device=w.device, dtype=torch.float32)
    if codes.dtype != torch.uint8 or tuple(codes.shape) != (N, K) or codes.stride(1) != 1 or scale.dtype != torch.float32 or scale.numel() != N or \
            not scale.is_contiguous():
        raise ValueError("weight_quant_fp8: codes uint8 [N, K] (contiguous rows) and scale fp32 [N] expected")
    _lib.check(_lib.load().crab_weight_quant_fp8(_lib.ctx(d), _stream(), _p(w), w.stride(0), N, K, _p(codes), codes.stride(0), _p(scale)), d)
    return codes, scale


def attn_decode_fp8(qkv, rope_tab, k_codes, v_codes, k_scale, v_scale, o, B, H, Hk, head_dim, Tmax, pos0, scale, pos_dev=None, kv_start=None):
    """One decode step's attention over the FP8 KV cache of ONE layer (codes uint8 [B, Hk, Tmax, d], scales fp32 [B, Hk, Tmax]) from the raw packed
    q|k|v rows: RoPE of q / new k at slot - kv_start[b], quantised append at slot = pos0 + pos_dev[0], attention over kv_start[b] .. slot."""
    d = _dev(qkv)
    _chk_bf16(qkv, o)
    if k_codes.dtype != torch.uint8 or v_codes.dtype != torch.uint8 or k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
        raise _lib.CrabHipError("attn_decode_fp8: codes are uint8, scales float32")
    if not (k_codes.is_contiguous() and v_codes.is_contiguous() and k_scale.is_contiguous() and v_scale.is_contiguous()):
        raise _lib.CrabHipError("attn_decode_fp8: the layer's codes / scales must be contiguous")
    if tuple(k_codes.shape) != (B, Hk, Tmax, head_dim) or v_codes.shape != k_codes.shape or tuple(k_scale.shape) != (B, Hk, Tmax) or v_scale.shape != k_scale.shape:
        raise _lib.CrabHipError("attn_decode_fp8: codes [B, Hk, Tmax, d] / scales [B, Hk, Tmax] expected")
    _lib.check(_lib.load().crab_attn_decode_fp8(_lib.ctx(d), _stream(), _p(qkv), qkv.stride(0), _p(rope_tab), _p(k_codes), _p(v_codes), _p(k_scale),
                                                _p(v_scale), _p(o), o.stride(0), B, H, Hk, head_dim, Tmax, pos0, _p(pos_dev), scale, _p(kv_start)), d)
    return o


def enc_layer(kind: str, w, io, device):
    """crab_clip_layer / crab_beats_layer / crab_qformer_layer: one encoder layer's launch sequence in one call."""
    d = device.index or 0
    fn = getattr(_lib.load(), f"crab_{kind}_layer")
    _lib.check(fn(_lib.ctx(d), _stream(), C.byref(w), C.byref(io)), d)


def llama_layers(table, n_layers: int, io, device):
    """crab_llama_layers: every layer of a decoder stack (prefill when io.vt is set, one decode step otherwise) in one call."""
    d = device.index or 0
    _lib.check(_lib.load().crab_llama_layers(_lib.ctx(d), _stream(), table, n_layers, C.byref(io)), d)


def swiglu(gu: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    d = _dev(gu)
    M, I2 = gu.shape
    if out is None:
        out = torch.empty((M, I2 // 2), device=gu.device, dtype=BF16)
    _lib.check(_lib.load().crab_swiglu(_lib.ctx(d), _stream(), _p(gu), gu.stride(0), _p(out), out.stride(0), M, I2 // 2), d)
    return out


def argmax(logits: torch.Tensor, out: Optional[torch.Tensor] = None, suppress: int = -1) -> torch.Tensor:
    d = _dev(logits)
    assert logits.dtype == torch.float32
    B, V = logits.shape
    if out is None:
        out = torch.empty((B,), device=logits.device, dtype=torch.int64)
    _lib.check(_lib.load().crab_argmax(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), _p(out), B, V, suppress), d)
    return out


def im2col_patch(x: torch.Tensor, P: int, ldo: int) -> torch.Tensor:
    """x [N,C,H,W] fp32/bf16 contiguous -> [N*gh*gw, ldo] bf16 patches (k = c,ky,kx)."""
    d = _dev(x)
    x = x.contiguous()
    N, Cc, Hh, Ww = x.shape
    out = torch.empty((N * (Hh // P) * (Ww // P), ldo), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_im2col_patch(_lib.ctx(d), _stream(), _p(x), 1 if x.dtype == torch.float32 else 0, _p(out), ldo, N, Cc, Hh, Ww, P), d)
    return out


def clip_embed_ln(patch, cls, pos, lnw, lnb, N, P, D, eps):
    d = _dev(patch)
    out = torch.empty((N * (P + 1), D), device=patch.device, dtype=BF16)
    wf = lnw.dtype == torch.float32
    if wf != (lnb.dtype == torch.float32):
        raise _lib.CrabHipError("clip_embed_ln: pre_layrnorm weight and bias must have the same storage")
    _lib.check(_lib.load().crab_clip_embed_ln_p(_lib.ctx(d), _stream(), _p(patch), _p(cls), _p(pos), _p(lnw), _p(lnb), 1 if wf else 0, _p(out),
                                                N, P, D, eps), d)
    return out


def beats_posconv_pad(x: torch.Tensor, B: int, n: int, E: int, G: int, Kc: int) -> torch.Tensor:
    d = _dev(x)
    out = torch.empty((G, B, n + Kc - 1, E // G), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_beats_posconv_pad(_lib.ctx(d), _stream(), _p(x), _p(out), B, n, E, G, Kc), d)
    return out


def beats_relpos_bias(table: torch.Tensor, n: int, H: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    d = _dev(table)
    out = torch.empty((H, n, n), device=table.device, dtype=torch.float32)
    _lib.check(_lib.load().crab_beats_relpos_bias(_lib.ctx(d), _stream(), _p(table), _p(out), n, H, num_buckets, max_distance), d)
    return out


def beats_gru_gate(q: torch.Tensor, gw, gb, grep_a, B: int, n: int, H: int, d_: int) -> torch.Tensor:
    d = _dev(q)
    out = torch.empty((B, H, n), device=q.device, dtype=torch.float32)
    _lib.check(_lib.load().crab_beats_gru_gate(_lib.ctx(d), _stream(), _p(q), q.stride(0), _p(gw), _p(gb), _p(grep_a), _p(out), B, n, H, d_), d)
    return out


def copy_rows(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, lds: Optional[int] = None, ldd: Optional[int] = None):
    """dst[r, :cols] = src[r, :cols]; lds/ldd override the row strides (e.g. gather every S-th row)."""
    d = _dev(src)
    _lib.check(_lib.load().crab_copy_rows(_lib.ctx(d), _stream(), _p(src), src.stride(0) if lds is None else lds, _p(dst),
                                          dst.stride(0) if ldd is None else ldd, rows, cols), d)


def copy_rows_batched(src, lds, sbs, dst, ldd, dbs, batch, rows, cols):
    d = _dev(src)
    _lib.check(_lib.load().crab_copy_rows_batched(_lib.ctx(d), _stream(), _p(src), lds, sbs, _p(dst), ldd, dbs, batch, rows, cols), d)


def greedy_select(logits, cur_ids, out_ids, step_dev, finished, eos_id: int, pad_id: int, min_new_tokens: int):
    d = _dev(logits)
    B, V = logits.shape
    _lib.check(_lib.load().crab_greedy_select(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(out_ids),
                                              out_ids.stride(0), _p(step_dev), _p(finished), eos_id, pad_id, min_new_tokens), d)


def sample_select(logits, cur_ids, out_ids, step_dev, finished, eos_id: int, pad_id: int, min_new_tokens: int, temperature: float, top_k: int,
                  top_p: float, seed: int):
    """crab_sample_select: temperature -> top-k -> top-p -> draw (HF sample mode), device-resident like greedy_select."""
    d = _dev(logits)
    B, V = logits.shape
    _lib.check(_lib.load().crab_sample_select(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(out_ids),
                                              out_ids.stride(0), _p(step_dev), _p(finished), eos_id, pad_id, min_new_tokens, float(temperature),
                                              int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF), d)


def sample_select_warped(logits, cur_ids, out_ids, step_dev, finished, eos_id: int, pad_id: int, min_new_tokens: int, temperature: float, top_k: int,
                         top_p: float, seed: int, min_p: float = 0.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0, kept_n=None, kept_min=None):
    """crab_sample_select_warped (csrc/sample.hip): sample_select with HF's min_p -> epsilon_cutoff -> eta_cutoff stages between top-p and
    the draw (0 = that stage is off; all three off gives sample_select's ids bit for bit).  logits [B, V] fp32 rows with unit column stride
    (a row stride of 0 - one row expanded - is fine: the rows are only read); cur_ids int64 [>= B], out_ids int64 [B, n_steps] with unit
    column stride, step_dev int32 [1], finished int32 [>= B].  kept_n (int32 [>= B]) / kept_min (fp32 [>= B]), each optional: the size of
    every row's final kept set and the smallest scaled logit in it."""
    d = _dev(logits)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < 0:
        raise ValueError(f"logits must be float32 [B, V] rows with unit column stride, got {logits.dtype} {tuple(logits.shape)} strides {logits.stride()}")
    B, V = logits.shape
    dev = logits.device
    if cur_ids.dtype != torch.int64 or cur_ids.dim() != 1 or cur_ids.shape[0] < B or not cur_ids.is_contiguous() or cur_ids.device != dev:
        raise ValueError(f"cur_ids must be a contiguous int64 [{B}] tensor on {dev}, got {cur_ids.dtype} {tuple(cur_ids.shape)} on {cur_ids.device}")
    if out_ids.dtype != torch.int64 or out_ids.dim() != 2 or out_ids.shape[0] < B or out_ids.shape[1] < 1 or out_ids.stride(1) != 1 or \
            out_ids.stride(0) < out_ids.shape[1] or out_ids.device != dev:
        raise ValueError(f"out_ids must be an int64 [{B}, n_steps] tensor with unit column stride on {dev}, got {out_ids.dtype} "
                         f"{tuple(out_ids.shape)} strides {out_ids.stride()} on {out_ids.device}")
    _chk_i32("step_dev", step_dev, 1, dev)
    _chk_i32("finished", finished, B, dev)
    _chk_i32("kept_n", kept_n, B, dev)
    if kept_min is not None and (kept_min.dtype != torch.float32 or kept_min.dim() != 1 or kept_min.shape[0] < B or not kept_min.is_contiguous() or
                                 kept_min.device != dev):
        raise ValueError(f"kept_min must be a contiguous float32 [{B}] tensor on {dev}, got {kept_min.dtype} {tuple(kept_min.shape)} on {kept_min.device}")
    _lib.check(_lib.load().crab_sample_select_warped(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(out_ids),
                                                     out_ids.stride(0), _p(step_dev), _p(finished), eos_id, pad_id, min_new_tokens,
                                                     float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, float(min_p),
                                                     float(epsilon_cutoff), float(eta_cutoff), _p(kept_n), _p(kept_min)), d)


def constrained_select(logits, edge_off, edge_tok, edge_dst, node, cur_ids, out_ids, step_dev, finished, eos_id: int, pad_id: int,
                       min_new_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0):
    """crab_constrained_select: the next token of every row among the out-edges of node[b] in a token trie (CSR int32 arrays, crab_amd/constrain.py),
    greedy (temperature == 0) or HF sample mode over the allowed tokens; node[b] follows the chosen edge.  Device-resident like greedy_select.
    logits [B, V] fp32 (a row stride of 0 - one row expanded - is fine: the rows are only read)."""
    d = _dev(logits)
    B, V = logits.shape
    n_nodes, n_edges = int(edge_off.shape[0]) - 1, int(edge_tok.shape[0])
    _chk_i32("edge_off", edge_off, n_nodes + 1, logits.device)
    _chk_i32("edge_tok", edge_tok, n_edges, logits.device)
    _chk_i32("edge_dst", edge_dst, n_edges, logits.device)
    _chk_i32("node", node, B, logits.device)
    _lib.check(_lib.load().crab_constrained_select(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(edge_off), _p(edge_tok), _p(edge_dst),
                                                   n_nodes, n_edges, _p(node), _p(cur_ids), _p(out_ids), out_ids.stride(0), _p(step_dev), _p(finished),
                                                   eos_id, pad_id, min_new_tokens, float(temperature), int(top_k), float(top_p),
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF), d)


def _chk_f32(name: str, t: torch.Tensor, shape, device):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be a float32 {list(shape)} tensor on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def logprob_norm(logits, step_dev, finished, eos_id: int, min_new_tokens: int, norm, edge_off=None, edge_tok=None, node=None):
    """crab_logprob_norm (csrc/logprob.hip), BEFORE the select of a decode step: norm[b] = (logsumexp of the raw row, logsumexp over the tokens the
    select may choose - all but EOS while step < min_new_tokens, or the out-edges of node[b] with a trie -, live, 0).  logits [B, V] fp32 (any row
    stride), norm fp32 [B, 4]; the trie arrays as constrained_select takes them, all three or none."""
    d = _dev(logits)
    B, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError(f"logits must be float32 rows with unit column stride, got {logits.dtype} strides {logits.stride()}")
    _chk_f32("norm", norm, (B, 4), logits.device)
    if not norm.is_contiguous():
        raise ValueError("norm must be contiguous")
    _chk_i32("finished", finished, B, logits.device)
    _chk_i32("step_dev", step_dev, 1, logits.device)
    n_nodes = n_edges = 0
    if edge_off is not None or edge_tok is not None or node is not None:
        if edge_off is None or edge_tok is None or node is None:
            raise ValueError("edge_off, edge_tok and node come together")
        n_nodes, n_edges = int(edge_off.shape[0]) - 1, int(edge_tok.shape[0])
        _chk_i32("edge_off", edge_off, n_nodes + 1, logits.device)
        _chk_i32("edge_tok", edge_tok, n_edges, logits.device)
        _chk_i32("node", node, B, logits.device)
    _lib.check(_lib.load().crab_logprob_norm(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(edge_off), _p(edge_tok), n_nodes, n_edges,
                                             _p(node), _p(step_dev), _p(finished), eos_id, min_new_tokens, _p(norm)), d)


def logprob_gather(logits, cur_ids, step_dev, norm, lp):
    """crab_logprob_gather, AFTER the select and before advance: lp[0, b, step] = z[y] - norm[b, 0], lp[1, b, step] = z[y] - norm[b, 1] with
    y = cur_ids[b], step = step_dev[0]; both 0 for a row that was not live (norm[b, 2] == 0) or a token outside [0, V); nothing when step is
    past lp's last column.  lp fp32 [2, B, n_steps] with unit column stride."""
    d = _dev(logits)
    B, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError(f"logits must be float32 rows with unit column stride, got {logits.dtype} strides {logits.stride()}")
    _chk_f32("norm", norm, (B, 4), logits.device)
    if lp.dtype != torch.float32 or lp.dim() != 3 or lp.shape[0] != 2 or lp.shape[1] != B or lp.shape[2] < 1 or lp.stride(2) != 1 or \
            lp.stride(1) < lp.shape[2] or lp.stride(0) < 0 or lp.device != logits.device or not norm.is_contiguous():
        raise ValueError(f"lp must be a float32 [2, {B}, n_steps] tensor with unit column stride on {logits.device}, got {lp.dtype} {tuple(lp.shape)}")
    if cur_ids.dtype != torch.int64 or cur_ids.shape[0] < B or not cur_ids.is_contiguous():
        raise ValueError(f"cur_ids must be a contiguous int64 [{B}] tensor, got {cur_ids.dtype} {tuple(cur_ids.shape)}")
    _chk_i32("step_dev", step_dev, 1, logits.device)
    _lib.check(_lib.load().crab_logprob_gather(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(step_dev), _p(norm),
                                               _p(lp), lp.stride(1), lp.stride(0), int(lp.shape[2])), d)


def cfg_mix(logits, guided, B: int, scale: float, finished):
    """crab_cfg_mix (csrc/cfg.hip), BEFORE the select of a guided decode step: pair b < B is row b (conditional) and row B + b (unconditional)
    of logits [2B, V] fp32; guided[b] = lu + scale * (lc - lu) over the two rows' log-softmax - fp32 [B, V], a buffer of its own (the logits
    are never written).  Row stride >= V on both; finished int32 [>= B] (a finished pair is computed like any other)."""
    d = _dev(logits)
    B = int(B)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] != 2 * B or B < 1 or \
            logits.stride(0) < logits.shape[1]:
        raise ValueError(f"logits must be float32 [{2 * B}, V] rows (conditional rows first) with unit column stride and a row stride >= V, got "
                         f"{logits.dtype} {tuple(logits.shape)} strides {logits.stride()}")
    V = int(logits.shape[1])
    if guided.dtype != torch.float32 or tuple(guided.shape) != (B, V) or guided.stride(1) != 1 or guided.stride(0) < V or guided.device != logits.device:
        raise ValueError(f"guided must be a float32 [{B}, {V}] tensor with unit column stride and a row stride >= {V} on {logits.device}, got "
                         f"{guided.dtype} {tuple(guided.shape)} strides {guided.stride()} on {guided.device}")
    _chk_i32("finished", finished, B, logits.device)
    _lib.check(_lib.load().crab_cfg_mix(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, float(scale), _p(finished), _p(guided),
                                        guided.stride(0)), d)


def cfg_follow(cur_ids, out_ids, finished, step_dev, B: int):
    """crab_cfg_follow, AFTER the select of a guided decode step and before advance: the unconditional row B + b takes cur_ids[b],
    out_ids[b, step_dev[0]] and finished[b] of its pair; nothing when the step is past out_ids' last column.  cur_ids int64 [2B], out_ids
    int64 [2B, n_steps] with unit column stride, finished int32 [2B]."""
    d = _dev(cur_ids)
    B = int(B)
    dev = cur_ids.device
    if B < 1 or cur_ids.dtype != torch.int64 or cur_ids.dim() != 1 or cur_ids.shape[0] < 2 * B or not cur_ids.is_contiguous():
        raise ValueError(f"cur_ids must be a contiguous int64 [{2 * B}] tensor, got {cur_ids.dtype} {tuple(cur_ids.shape)}")
    if out_ids.dtype != torch.int64 or out_ids.dim() != 2 or out_ids.shape[0] < 2 * B or out_ids.shape[1] < 1 or out_ids.stride(1) != 1 or \
            out_ids.stride(0) < out_ids.shape[1] or out_ids.device != dev:
        raise ValueError(f"out_ids must be an int64 [{2 * B}, n_steps] tensor with unit column stride on {dev}, got {out_ids.dtype} "
                         f"{tuple(out_ids.shape)} on {out_ids.device}")
    _chk_i32("finished", finished, 2 * B, dev)
    _chk_i32("step_dev", step_dev, 1, dev)
    _lib.check(_lib.load().crab_cfg_follow(_lib.ctx(d), _stream(), _p(cur_ids), _p(out_ids), out_ids.stride(0), int(out_ids.shape[1]), _p(finished),
                                           _p(step_dev), B), d)


LOGITS_PROC_MAX_STOP = 8            # stop ids beyond eos_token_id that crab_logits_edit / crab_logits_restore take
LOGITS_PROC_MAX_STEPS = 8192        # history tokens crab_logits_edit holds in LDS


def _chk_logits_proc(logits, stop_ids, save_idx, save_val, n_slots: int):
    B, V = logits.shape
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < V:
        # the rows are WRITTEN: a stride-0 expanded row (fine for the select kernels, which only read) would be edited B times over
        raise ValueError(f"logits must be float32 rows with unit column stride and a row stride >= {V}, got {logits.dtype} strides {logits.stride()}")
    n_stop = 0 if stop_ids is None else int(stop_ids.shape[0])
    if n_stop > LOGITS_PROC_MAX_STOP:
        raise ValueError(f"stop_ids holds {n_stop} ids, at most {LOGITS_PROC_MAX_STOP} are taken")
    _chk_i32("stop_ids", stop_ids, n_stop, logits.device)
    if save_idx.dtype != torch.int32 or save_idx.dim() != 2 or save_idx.shape[0] != B or save_idx.shape[1] < n_slots + n_stop or \
            not save_idx.is_contiguous() or save_idx.device != logits.device:
        raise ValueError(f"save_idx must be a contiguous int32 [{B}, >= {n_slots + n_stop}] tensor on {logits.device}, got {save_idx.dtype} "
                         f"{tuple(save_idx.shape)} on {save_idx.device}")
    _chk_f32("save_val", save_val, save_idx.shape, logits.device)
    if not save_val.is_contiguous():
        raise ValueError("save_val must be contiguous")
    return n_stop


def logits_edit(logits, out_ids, step_dev, finished, repetition_penalty: float, no_repeat_ngram_size: int, stop_ids, min_new_tokens: int,
                save_idx, save_val):
    """crab_logits_edit (csrc/logits_proc.hip), BEFORE the select of a decode step: the repetition penalty, the n-gram bans and - while
    step < min_new_tokens - the bans of stop_ids, written IN PLACE into logits [B, V] fp32 (row stride >= V); the raw values of the edited
    columns go to save_idx (int32) / save_val (fp32) [B, >= 2 * n_steps + n_stop] with n_steps = out_ids.shape[1].  History of row b:
    out_ids[b, :step_dev[0]] (int64).  stop_ids: contiguous int32 [n_stop <= 8] or None."""
    d = _dev(logits)
    B, V = logits.shape
    if out_ids.dtype != torch.int64 or out_ids.dim() != 2 or out_ids.shape[0] != B or out_ids.shape[1] < 1 or out_ids.stride(1) != 1 or \
            out_ids.stride(0) < out_ids.shape[1] or out_ids.device != logits.device:
        raise ValueError(f"out_ids must be an int64 [{B}, n_steps] tensor with unit column stride on {logits.device}, got {out_ids.dtype} "
                         f"{tuple(out_ids.shape)} on {out_ids.device}")
    n_steps = int(out_ids.shape[1])
    n_stop = _chk_logits_proc(logits, stop_ids, save_idx, save_val, 2 * n_steps)
    _chk_i32("finished", finished, B, logits.device)
    _chk_i32("step_dev", step_dev, 1, logits.device)
    _lib.check(_lib.load().crab_logits_edit(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(out_ids), out_ids.stride(0), n_steps,
                                            _p(step_dev), _p(finished), float(repetition_penalty), int(no_repeat_ngram_size), _p(stop_ids), n_stop,
                                            int(min_new_tokens), _p(save_idx), _p(save_val), save_idx.stride(0)), d)


def logits_restore(logits, cur_ids, finished, stop_ids, save_idx, save_val, n_slots: Optional[int] = None):
    """crab_logits_restore, AFTER the select and before logprob_gather / advance: the saved raw values go back into logits (bit for bit what
    the lm_head wrote) and finished[b] |= cur_ids[b] in stop_ids.  n_slots: the slots logits_edit filled, 2 * n_steps + n_stop (default: all
    columns of save_idx)."""
    d = _dev(logits)
    B, V = logits.shape
    n_slots = int(save_idx.shape[1]) if n_slots is None else int(n_slots)
    n_stop = _chk_logits_proc(logits, stop_ids, save_idx, save_val, 0)
    if n_slots < 1 or n_slots > save_idx.shape[1]:
        raise ValueError(f"n_slots = {n_slots} outside 1 .. {save_idx.shape[1]}")
    if cur_ids.dtype != torch.int64 or cur_ids.dim() != 1 or cur_ids.shape[0] < B or not cur_ids.is_contiguous() or cur_ids.device != logits.device:
        raise ValueError(f"cur_ids must be a contiguous int64 [{B}] tensor on {logits.device}, got {cur_ids.dtype} {tuple(cur_ids.shape)}")
    _chk_i32("finished", finished, B, logits.device)
    _lib.check(_lib.load().crab_logits_restore(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(finished), _p(stop_ids),
                                               n_stop, _p(save_idx), _p(save_val), save_idx.stride(0), n_slots), d)


BEAM_MAX = _lib.header_const("CRAB_BEAM_MAX")                # beams per clip
BEAM_MAX_NEW = _lib.header_const("CRAB_BEAM_MAX_NEW")        # max_new_tokens of a beam call
BEAM_EARLY = {False: 0, True: 1, "never": 2}


def beam_len_table(max_new: int, length_penalty: float) -> torch.Tensor:
    """fp32 [max_new + 1]: n ** length_penalty as HF's Python scalar gives it (a double pow), rounded to fp32 once; entry 0 is unused."""
    return torch.tensor([1.0] + [float(n) ** float(length_penalty) for n in range(1, int(max_new) + 1)], dtype=torch.float64).to(torch.float32)


class BeamState:
    """The device-resident beam state of `clips` x K rows (include/crab_hip.h "Beam search"): everything crab_beam_row_topk / crab_beam_merge /
    crab_kv_beam_reorder read and write beside the decode state's own cur_ids, out_ids (= run_seq), finished and step_dev.  reset() puts back
    HF's initial values.  length_penalty / early_stopping are fixed per state (len_tab is built from them)."""

    FIELDS = ("run_score", "hyp_score", "hyp_seq", "hyp_len", "hyp_fin", "unsat", "beam_idx")

    def __init__(self, clips: int, K: int, max_new: int, pad: int, length_penalty: float, early_stopping, device):
        if early_stopping not in (False, True, "never"):
            raise ValueError(f'early_stopping must be False, True or "never", got {early_stopping!r}')
        rows = clips * K
        self.clips, self.K, self.max_new, self.pad = int(clips), int(K), int(max_new), int(pad)
        self.length_penalty, self.early_stopping = float(length_penalty), early_stopping
        self.early = BEAM_EARLY[early_stopping if isinstance(early_stopping, str) else bool(early_stopping)]
        self.len_tab = beam_len_table(max_new, length_penalty).to(device)
        self.run_score = torch.empty((rows,), device=device, dtype=torch.float32)
        self.hyp_score = torch.empty((rows,), device=device, dtype=torch.float32)
        self.hyp_seq = torch.empty((rows, max_new), device=device, dtype=torch.int64)
        self.hyp_len = torch.empty((rows,), device=device, dtype=torch.int32)
        self.hyp_fin = torch.empty((rows,), device=device, dtype=torch.int32)
        self.unsat = torch.empty((clips,), device=device, dtype=torch.int32)
        self.beam_idx = torch.empty((rows,), device=device, dtype=torch.int32)
        self.cand_score = torch.zeros((rows, 2 * K), device=device, dtype=torch.float32)
        self.cand_tok = torch.zeros((rows, 2 * K), device=device, dtype=torch.int32)
        self.reset()

    def reset(self):
        K = self.K
        self.run_score.fill_(-1.0e9)
        self.run_score[::K] = 0.0
        self.hyp_score.fill_(-1.0e9)
        self.hyp_seq.fill_(self.pad)
        self.hyp_len.zero_(); self.hyp_fin.zero_()
        self.unsat.fill_(1)
        self.beam_idx.copy_(torch.arange(K, dtype=torch.int32).repeat(self.clips))

    def snapshot(self) -> dict:
        return {f: getattr(self, f).clone() for f in self.FIELDS}


def beam_row_topk(logits, bs: BeamState, step_dev, finished, eos_id: int, min_new_tokens: int):
    """crab_beam_row_topk (csrc/beam.hip): every row's best 2K continuations by run_score + log_softmax(raw logits) into bs.cand_score /
    bs.cand_tok.  logits [clips * K, V] fp32, unit column stride."""
    d = _dev(logits)
    rows, V = logits.shape
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or rows != bs.clips * bs.K:
        raise ValueError(f"logits must be float32 [{bs.clips * bs.K}, V] with unit column stride, got {logits.dtype} {tuple(logits.shape)}")
    _chk_i32("finished", finished, rows, logits.device)
    _chk_i32("step_dev", step_dev, 1, logits.device)
    _lib.check(_lib.load().crab_beam_row_topk(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), rows, V, bs.K, _p(bs.run_score), _p(step_dev),
                                              _p(finished), int(eos_id), int(min_new_tokens), _p(bs.cand_score), _p(bs.cand_tok)), d)


def beam_merge(bs: BeamState, V: int, step_dev, eos_id: int, cur_ids, run_seq, finished):
    """crab_beam_merge: steps c-g of HF's beam loop on every clip's K x 2K candidates.  run_seq: the decode state's out_ids, int64
    [rows, max_new]; cur_ids int64 [rows]; finished int32 [rows] receives the clip's done flag."""
    d = _dev(run_seq)
    rows = bs.clips * bs.K
    if run_seq.dtype != torch.int64 or run_seq.dim() != 2 or run_seq.shape[0] != rows or run_seq.shape[1] != bs.max_new or run_seq.stride(1) != 1:
        raise ValueError(f"run_seq must be int64 [{rows}, {bs.max_new}] with unit column stride, got {run_seq.dtype} {tuple(run_seq.shape)}")
    if cur_ids.dtype != torch.int64 or cur_ids.dim() != 1 or cur_ids.shape[0] < rows or not cur_ids.is_contiguous() or cur_ids.device != run_seq.device:
        raise ValueError(f"cur_ids must be a contiguous int64 [{rows}] tensor on {run_seq.device}, got {cur_ids.dtype} {tuple(cur_ids.shape)}")
    _chk_i32("finished", finished, rows, run_seq.device)
    _chk_i32("step_dev", step_dev, 1, run_seq.device)
    _lib.check(_lib.load().crab_beam_merge(_lib.ctx(d), _stream(), _p(bs.cand_score), _p(bs.cand_tok), rows, int(V), bs.K, bs.max_new, _p(step_dev),
                                           int(eos_id), bs.pad, bs.early, int(bs.length_penalty > 0.0), _p(bs.len_tab), _p(bs.run_score), _p(run_seq),
                                           run_seq.stride(0), _p(bs.hyp_score), _p(bs.hyp_seq), bs.hyp_seq.stride(0), _p(bs.hyp_len), _p(bs.hyp_fin),
                                           _p(bs.unsat), _p(cur_ids), _p(bs.beam_idx), _p(finished)), d)


def kv_beam_reorder(kc, vc, K: int, beam_idx, finished, pos_dev, first_slot: int = 0):
    """crab_kv_beam_reorder: the own KV cache [L, rows, Hk, Tmax, d] bf16 x 2 in place, row c K + k <- row c K + beam_idx[c K + k], over the
    slots first_slot .. pos_dev[0]; clips with an identity beam_idx or finished rows are skipped."""
    d = _dev(kc)
    _chk_bf16(kc, vc)
    if kc.dim() != 5 or kc.shape != vc.shape or not kc.is_contiguous() or not vc.is_contiguous():
        raise ValueError(f"k / v cache must be contiguous [L, rows, Hk, Tmax, d] tensors of one shape, got {tuple(kc.shape)} and {tuple(vc.shape)}")
    L, rows, Hk, Tmax, hd = kc.shape
    _chk_i32("beam_idx", beam_idx, rows, kc.device)
    _chk_i32("finished", finished, rows, kc.device)
    _chk_i32("pos_dev", pos_dev, 1, kc.device)
    _lib.check(_lib.load().crab_kv_beam_reorder(_lib.ctx(d), _stream(), _p(kc), _p(vc), L, rows, int(K), Hk, Tmax, hd, int(first_slot), _p(pos_dev),
                                                _p(beam_idx), _p(finished)), d)


COMPACT_MAX_UNITS = (1 << 31) - 1      # 16-byte units of one cache a single crab_kv_compact_rows launch spans (the entry point refuses 2^31 and more)


def check_compact_rows(src_rows, rows: int) -> List[int]:
    """The contract of crab_kv_compact_rows on the host, before anything is uploaded: src_rows (a Python list or CPU tensor of the surviving
    rows' indices) is non-empty, strictly increasing, src_rows[j] >= j and every index is below `rows`.  ValueError by name otherwise."""
    src = [int(s) for s in (src_rows.tolist() if isinstance(src_rows, torch.Tensor) else src_rows)]
    if not src:
        raise ValueError("src_rows is empty: kv_compact_rows needs at least one surviving row")
    if len(src) > int(rows):
        raise ValueError(f"src_rows has {len(src)} entries for a cache of {rows} rows")
    for j, s in enumerate(src):
        if j and s == src[j - 1]:
            raise ValueError(f"src_rows[{j}] = {s} repeats src_rows[{j - 1}]: the surviving rows must be distinct (strictly increasing)")
        if j and s < src[j - 1]:
            raise ValueError(f"src_rows[{j}] = {s} is below src_rows[{j - 1}] = {src[j - 1]}: src_rows must be strictly increasing")
        if s < j:
            raise ValueError(f"src_rows[{j}] = {s} is below its destination row {j}: rows only move towards the front")
        if s >= int(rows):
            raise ValueError(f"src_rows[{j}] = {s} is outside the cache's {rows} rows")
    return src


def kv_compact_rows(kc, vc, src_rows, pos_dev, row_off=None):
    """crab_kv_compact_rows (csrc/kv_compact.hip): the bf16 KV caches [L, rows, Hk, Tmax, d] x 2 in place, row j <- row src_rows[j] for
    j < len(src_rows), over the slots row_off[src_rows[j]] .. pos_dev[0]; afterwards kc[:, :len(src_rows)] is the cache of the surviving rows.
    kc / vc may be views of an allocation with more rows (only the layer stride may exceed the packed one).  src_rows: a Python list or CPU
    tensor, checked on the host (check_compact_rows) before it is uploaded.  Returns the device copy of src_rows (int32)."""
    if kc.dim() != 5 or kc.shape != vc.shape:
        raise ValueError(f"k / v cache must be [L, rows, Hk, Tmax, d] tensors of one shape, got {tuple(kc.shape)} and {tuple(vc.shape)}")
    L, rows, Hk, Tmax, hd = kc.shape
    src = check_compact_rows(src_rows, rows)
    d = _dev(kc)
    _chk_bf16(kc, vc)
    packed = (Hk * Tmax * hd, Tmax * hd, hd, 1)
    if kc.stride()[1:] != packed or vc.stride() != kc.stride() or kc.stride(0) < rows * packed[0]:
        raise ValueError(f"k / v cache rows must be packed (only the layer stride may be larger), got strides {kc.stride()} and {vc.stride()}")
    _chk_i32("pos_dev", pos_dev, 1, kc.device)
    _chk_i32("row_off", row_off, rows, kc.device)
    src_dev = torch.tensor(src, dtype=torch.int32).to(kc.device)
    # one launch takes fewer than 2^31 16-byte units per cache (32 GiB): a full-size wave (32 layers x 512 rows x 32 heads x ~900 slots: 120 GiB)
    # goes layer group by layer group - the layers are independent, so the groups are the same launch on kc[l0:l1] / vc[l0:l1]
    per_layer = kc.stride(0) // 8
    step = max(1, min(L, COMPACT_MAX_UNITS // max(per_layer, 1)))
    for l0 in range(0, L, step):
        n = min(step, L - l0)
        _lib.check(_lib.load().crab_kv_compact_rows(_lib.ctx(d), _stream(), _p(kc[l0]), _p(vc[l0]), kc.stride(0), n, rows, Hk, Tmax, hd, len(src),
                                                    _p(src_dev), _p(row_off), _p(pos_dev)), d)
    return src_dev


def sample_select_rows(row_ids, logits, cur_ids, out_ids, step_dev, finished, eos_id: int, pad_id: int, min_new_tokens: int, temperature: float,
                       top_k: int, top_p: float, seed: int, min_p: float = 0.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0):
    """crab_sample_select_rows (csrc/sample.hip): sample_select (all three further stages 0) or sample_select_warped on row r of every buffer, the
    draw keyed by row_ids[r] (device int32 [B]: the row's index before its wave shed rows) instead of r."""
    d = _dev(logits)
    B, V = logits.shape
    _chk_i32("row_ids", row_ids, B, logits.device)
    _chk_i32("step_dev", step_dev, 1, logits.device)
    _chk_i32("finished", finished, B, logits.device)
    if row_ids is None:
        raise ValueError("row_ids must be a contiguous int32 tensor")
    _lib.check(_lib.load().crab_sample_select_rows(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), B, V, _p(cur_ids), _p(out_ids),
                                                   out_ids.stride(0), _p(step_dev), _p(finished), eos_id, pad_id, min_new_tokens, float(temperature),
                                                   int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, float(min_p), float(epsilon_cutoff),
                                                   float(eta_cutoff), _p(row_ids)), d)


def advance(pos_dev, step_dev):
    d = _dev(pos_dev)
    _lib.check(_lib.load().crab_advance(_lib.ctx(d), _stream(), _p(pos_dev), _p(step_dev)), d)


def _chk_i32(name: str, t: Optional[torch.Tensor], n: int, device):
    # the kernels read these through a raw int32 pointer: an int64 or strided tensor would be misread silently
    if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < n or not t.is_contiguous() or t.device != device):
        raise ValueError(f"{name} must be a contiguous int32 [{n}] tensor on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def prefix_tile_plan(rows_per_clip, H: int, Hk: int):
    """The tiles of crab_attn_prefix_partial for a batch whose clip c owns rows_per_clip[c] CONSECUTIVE query rows (its questions in a decode step,
    questions x suffix rows in the suffix prefill): -> (tiles, row_clip), tiles = [(first row, rows)], row_clip[row] = clip.  A tile takes at most
    16 // (H // Hk) rows (every row brings its H // Hk heads of a kv head into the 16 operand rows) and never spans two clips: a clip's rows are
    cut into full tiles from its first row on, and its last tile holds the remainder (a PARTIAL tile: fewer rows, the operand rows behind them zero)."""
    if Hk <= 0 or H % Hk or not 1 <= H // Hk <= 16:
        raise ValueError(f"prefix_tile_plan: H = {H}, Hk = {Hk}")
    per = 16 // (H // Hk)
    tiles, row_clip, r0 = [], [], 0
    for c, R in enumerate(rows_per_clip):
        R = int(R)
        if R < 1:
            raise ValueError("prefix_tile_plan: every clip needs at least one row")
        tiles += [(r0 + t, min(per, R - t)) for t in range(0, R, per)]
        row_clip += [c] * R
        r0 += R
    return tiles, row_clip


def _chk_prefix_ws(name: str, ws, q, rows: int, H: int, d: int):
    # the partials travel as a raw byte pointer + size: a strided, typed or foreign-device tensor would be misread silently
    if ws is not None and (ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous() or ws.device != q.device):
        raise ValueError(f"{name}: ws must be a contiguous uint8 tensor on {q.device} (attn_prefix_bytes(rows, H, d) bytes), got {ws.dtype} {tuple(ws.shape)} on {ws.device}")
    if q.dim() != 2 or q.stride(1) != 1 or q.shape[0] < rows or q.shape[1] < H * d:
        raise ValueError(f"{name}: q must be a [>= {rows}, >= {H * d}] matrix with contiguous rows, got {tuple(q.shape)}")


def attn_prefix_bytes(rows: int, H: int, d: int) -> int:
    return int(_lib.load().crab_attn_prefix_workspace(int(rows), int(H), int(d)))


def attn_prefix_partial(q, prefix_k, prefix_v, ws, tile_rows, row_clip, rows: int, H: int, Hk: int, head_dim: int, P: int, scale: float):
    """K1: the attention partials of `rows` query rows (q [rows, ldq], rotated) over the P live rows of their clips' prefix cache [C, Hk, Tp, d] ->
    ws (uint8, attn_prefix_bytes(rows, H, d)).  tile_rows int32 [2 * tiles] / row_clip int32 [rows]: prefix_tile_plan, on the device."""
    d = _dev(q)
    _chk_bf16(q, prefix_k, prefix_v)
    C_, Tp = prefix_k.shape[0], prefix_k.shape[2]
    if not (prefix_k.is_contiguous() and prefix_v.is_contiguous()) or tuple(prefix_k.shape) != (C_, Hk, Tp, head_dim) or prefix_v.shape != prefix_k.shape:
        raise ValueError("attn_prefix_partial: prefix_k / prefix_v must be contiguous [C, Hk, Tp, d] tensors")
    _chk_prefix_ws("attn_prefix_partial", ws, q, rows, H, head_dim)
    if tile_rows is None or row_clip is None or tile_rows.numel() % 2 or not 2 <= tile_rows.numel() <= 2 * rows:
        raise ValueError("attn_prefix_partial: tile_rows (int32 [2 * tiles], 1 <= tiles <= rows) and row_clip (int32 [rows]) are required")
    _chk_i32("tile_rows", tile_rows, tile_rows.numel(), q.device)
    _chk_i32("row_clip", row_clip, rows, q.device)
    _lib.check(_lib.load().crab_attn_prefix_partial(_lib.ctx(d), _stream(), _p(q), q.stride(0), _p(prefix_k), _p(prefix_v), _p(ws),
                                                    ws.numel() * ws.element_size() if ws is not None else 0, _p(tile_rows), tile_rows.numel() // 2,
                                                    _p(row_clip), rows, C_, H, Hk, head_dim, Tp, P, scale), d)
    return ws


def attn_own_merge(q, ws, k_cache, v_cache, o, B: int, Sq: int, H: int, Hk: int, head_dim: int, Tmax: int, ctx_len: int, scale: float,
                   ctx_dev=None, kv_start=None):
    """K2: query i of sequence b (row b * Sq + i) over its own cache slots kv_start[b] .. ctx_len (+ ctx_dev[0]) - 1 + i, merged with the prefix
    partial of the row in ws -> o [B * Sq, ldo] bf16."""
    d = _dev(q)
    _chk_bf16(q, k_cache, v_cache, o)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or tuple(k_cache.shape) != (B, Hk, Tmax, head_dim) or v_cache.shape != k_cache.shape:
        raise ValueError("attn_own_merge: k_cache / v_cache must be contiguous [B, Hk, Tmax, d] tensors")
    _chk_prefix_ws("attn_own_merge", ws, q, B * Sq, H, head_dim)
    if o.dim() != 2 or o.stride(1) != 1 or o.shape[0] < B * Sq or o.shape[1] < H * head_dim or o.device != q.device:
        raise ValueError("attn_own_merge: o needs B * Sq rows of H * d contiguous columns on q's device")
    _chk_i32("kv_start", kv_start, B, q.device)
    _chk_i32("ctx_dev", ctx_dev, 1, q.device)
    _lib.check(_lib.load().crab_attn_own_merge(_lib.ctx(d), _stream(), _p(q), q.stride(0), _p(ws), ws.numel() * ws.element_size() if ws is not None else 0,
                                               _p(k_cache), _p(v_cache), _p(o), o.stride(0), B, Sq, H, Hk, head_dim, Tmax, ctx_len, _p(ctx_dev),
                                               scale, _p(kv_start)), d)
    return o


LOOKUP_MAX_DRAFT = 15           # draft tokens of one verify step: k + 1 <= 16 rows (crab_attn_verify's Sq, the M <= 16 projection kernels)


def attn_verify(qkv, k_cache, v_cache, o, B: int, Sq: int, H: int, Hk: int, head_dim: int, Tmax: int, ctx_len: int, scale: float,
                ctx_dev=None, kv_start=None):
    """crab_attn_verify: query i of sequence b (row b * Sq + i of qkv / o; rotated, its key appended already) over the cache slots
    kv_start[b] .. ctx_len (+ ctx_dev[0]) - 1 + i -> o [B * Sq, ldo] bf16.  Sq <= 16; every K / V row is read once per (sequence, kv head,
    group of 16 // (H // Hk) queries)."""
    d = _dev(qkv)
    _chk_bf16(qkv, k_cache, v_cache, o)
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()) or tuple(k_cache.shape) != (B, Hk, Tmax, head_dim) or v_cache.shape != k_cache.shape:
        raise ValueError("attn_verify: k_cache / v_cache must be contiguous [B, Hk, Tmax, d] tensors")
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[0] < B * Sq or qkv.shape[1] < H * head_dim:
        raise ValueError(f"attn_verify: qkv must be a [>= {B * Sq}, >= {H * head_dim}] matrix with contiguous rows, got {tuple(qkv.shape)}")
    if o.dim() != 2 or o.stride(1) != 1 or o.shape[0] < B * Sq or o.shape[1] < H * head_dim or o.device != qkv.device:
        raise ValueError("attn_verify: o needs B * Sq rows of H * d contiguous columns on qkv's device")
    _chk_i32("kv_start", kv_start, B, qkv.device)
    _chk_i32("ctx_dev", ctx_dev, 1, qkv.device)
    _lib.check(_lib.load().crab_attn_verify(_lib.ctx(d), _stream(), _p(qkv), qkv.stride(0), _p(k_cache), _p(v_cache), _p(o), o.stride(0), B, Sq, H, Hk,
                                            head_dim, Tmax, ctx_len, _p(ctx_dev), scale, _p(kv_start)), d)
    return o


def _chk_i64(name: str, t, n: int, device):
    if t is None or t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] < n or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous int64 [{n}] tensor on {device}")


def lookup_draft(hist, S: int, step_dev, cur_ids, k: int, max_ngram: int, eos_id: int, pad_id: int, max_new_tokens: int, V: int, ids_out,
                 n_draft, finished):
    """crab_lookup_draft: the prompt-lookup draft of one verify step (HF PromptLookupCandidateGenerator.get_candidates) from hist int32
    [S + max_new_tokens] (live length S + step_dev[0]) -> ids_out int64 [k + 1] (current token, drafts, pad), n_draft int32 [1]."""
    d = _dev(hist)
    dev = hist.device
    for nm, t, n in (("hist", hist, S + max_new_tokens), ("step_dev", step_dev, 1), ("n_draft", n_draft, 1), ("finished", finished, 1)):
        if t is None:
            raise ValueError(f"lookup_draft: {nm} is required")
        _chk_i32(nm, t, n, dev)
    _chk_i64("cur_ids", cur_ids, 1, dev)
    _chk_i64("ids_out", ids_out, k + 1, dev)
    _lib.check(_lib.load().crab_lookup_draft(_lib.ctx(d), _stream(), _p(hist), int(S), _p(step_dev), _p(cur_ids), int(k), int(max_ngram), int(eos_id),
                                             int(pad_id), int(max_new_tokens), int(V), _p(ids_out), _p(n_draft), _p(finished)), d)


def lookup_accept(logits, ids, n_draft, cur_ids, out_ids, hist, S: int, pos_dev, step_dev, finished, eos_id: int, pad_id: int, min_new_tokens: int,
                  max_new_tokens: int, stats, step_logits=None):
    """crab_lookup_accept: greedy verification of the drafts in ids int64 [k + 1] against logits fp32 [k + 1, V]; emits 1 .. k + 1 tokens into
    out_ids int64 [max_new_tokens] / hist, advances pos_dev / step_dev, accumulates stats int32 [4] (steps, proposed, accepted, emitted) and, with
    step_logits fp32 [max_new_tokens, V], keeps the emitted tokens' logits rows."""
    d = _dev(logits)
    dev = logits.device
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("lookup_accept: logits must be an fp32 [k + 1, V] matrix with contiguous rows")
    k, V = logits.shape[0] - 1, logits.shape[1]
    for nm, t, n in (("n_draft", n_draft, 1), ("hist", hist, S + max_new_tokens), ("pos_dev", pos_dev, 1), ("step_dev", step_dev, 1),
                     ("finished", finished, 1), ("stats", stats, 4)):
        if t is None:
            raise ValueError(f"lookup_accept: {nm} is required")
        _chk_i32(nm, t, n, dev)
    _chk_i64("ids", ids, k + 1, dev)
    _chk_i64("cur_ids", cur_ids, 1, dev)
    _chk_i64("out_ids", out_ids.reshape(-1) if out_ids is not None and out_ids.is_contiguous() else out_ids, max_new_tokens, dev)
    if step_logits is not None and (step_logits.dtype != torch.float32 or not step_logits.is_contiguous() or tuple(step_logits.shape) != (max_new_tokens, V)
                                    or step_logits.device != dev):
        raise ValueError(f"lookup_accept: step_logits must be a contiguous fp32 [{max_new_tokens}, {V}] tensor on {dev}")
    _lib.check(_lib.load().crab_lookup_accept(_lib.ctx(d), _stream(), _p(logits), logits.stride(0), V, k, _p(ids), _p(n_draft), _p(cur_ids), _p(out_ids),
                                              _p(hist), int(S), _p(pos_dev), _p(step_dev), _p(finished), int(eos_id), int(pad_id), int(min_new_tokens),
                                              int(max_new_tokens), _p(stats), _p(step_logits)), d)


def lm_head_xent_bytes(M: int, N: int) -> int:
    return int(_lib.load().crab_lm_head_xent_workspace(int(M), int(N)))


def lm_head_xent(x: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, row_idx: Optional[torch.Tensor] = None, logprob=None, lse=None,
                 argmax=None, workspace: Optional[torch.Tensor] = None):
    """crab_lm_head_xent: the lm_head projection reduced to cross-entropy terms in its epilogue - no logits are stored.
    x [R, K] bf16 (row stride any multiple of 8), w [N, K] bf16, labels int32 [M] (already shifted; negative = no target, each < N),
    row_idx int32 [M] or None (row i of the problem is x[row_idx[i]], every index a row of x; None: M = R, the rows of x in order).
    Returns (logprob [M] fp32 - 0 without a target, lse [M] fp32, argmax [M] int32 - first maximum)."""
    _chk_bf16(x, w)
    d = _dev(x)
    K = x.shape[1]
    N = w.shape[0]
    M = labels.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1
    _chk_i32("labels", labels, M, x.device)
    _chk_i32("row_idx", row_idx, M, x.device)
    if row_idx is None and M != x.shape[0]:
        raise ValueError(f"labels has {M} entries for {x.shape[0]} rows of x (no row_idx)")
    if M == 0:
        raise ValueError("lm_head_xent: no rows")
    mk = lambda dt: torch.empty((M,), device=x.device, dtype=dt)
    logprob = mk(torch.float32) if logprob is None else logprob
    lse = mk(torch.float32) if lse is None else lse
    argmax = mk(torch.int32) if argmax is None else argmax
    for nm, t, dt in (("logprob", logprob, torch.float32), ("lse", lse, torch.float32), ("argmax", argmax, torch.int32)):
        if t.dtype != dt or t.dim() != 1 or t.shape[0] < M or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"{nm} must be a contiguous {dt} [{M}] tensor on {x.device}")
    need = lm_head_xent_bytes(M, N)
    if workspace is None:
        workspace = torch.empty((need,), device=x.device, dtype=torch.uint8)
    _lib.check(_lib.load().crab_lm_head_xent(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(row_idx), M, _p(w), w.stride(0), N, K, _p(labels),
                                             _p(logprob), _p(lse), _p(argmax), _p(workspace), workspace.numel() * workspace.element_size()), d)
    return logprob, lse, argmax


def xent_reduce(logprob: torch.Tensor, labels: torch.Tensor, argmax: torch.Tensor, seq_off: torch.Tensor):
    """crab_xent_reduce over the compacted rows of lm_head_xent: seq_off int32 [B + 1] (CSR) -> (sum_logprob [B] fp32, n_tokens [B] int32,
    n_correct [B] int32, mean_nll [1] fp32 = the batch's mean over all labelled tokens, NaN when there is none)."""
    d = _dev(seq_off)
    B = seq_off.shape[0] - 1
    dev = seq_off.device
    _chk_i32("seq_off", seq_off, B + 1, dev)
    n = logprob.shape[0]
    _chk_i32("labels", labels, n, dev)
    _chk_i32("argmax", argmax, n, dev)
    if logprob.dtype != torch.float32 or not logprob.is_contiguous() or logprob.device != dev:
        raise ValueError("logprob must be a contiguous float32 tensor on the device of seq_off")
    s = torch.empty((B,), device=dev, dtype=torch.float32)
    nt = torch.empty((B,), device=dev, dtype=torch.int32)
    nc = torch.empty((B,), device=dev, dtype=torch.int32)
    mean = torch.empty((1,), device=dev, dtype=torch.float32)
    _lib.check(_lib.load().crab_xent_reduce(_lib.ctx(d), _stream(), _p(logprob), _p(labels), _p(argmax), _p(seq_off), B, _p(s), _p(nt), _p(nc),
                                            _p(mean)), d)
    return s, nt, nc, mean


def im2col3x3(x: torch.Tensor, B: int, h: int, w: int) -> torch.Tensor:
    """x [B*h*w, C] token-major -> [B*h*w, 9*C] (Conv2d k=3 pad=1 operand)."""
    d = _dev(x)
    Cc = x.shape[1]
    out = torch.empty((B * h * w, 9 * Cc), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_im2col3x3(_lib.ctx(d), _stream(), _p(x), _p(out), B, h, w, Cc), d)
    return out


def pixel_shuffle2x(g: torch.Tensor, bias: Optional[torch.Tensor], h: int, w: int, Co: int) -> torch.Tensor:
    d = _dev(g)
    out = torch.empty((4 * h * w, Co), device=g.device, dtype=BF16)
    _lib.check(_lib.load().crab_pixel_shuffle2x(_lib.ctx(d), _stream(), _p(g), _p(bias), _p(out), h, w, Co), d)
    return out


def bilinear(x: torch.Tensor, strides, Cc: int, h: int, w: int, out: torch.Tensor, alpha: float = 1.0, beta: float = 0.0):
    """x element (c,y,x) at x.data + c*strides[0] + y*strides[1] + x*strides[2]; out fp32 [C,H,W] (accumulates when beta != 0)."""
    d = _dev(x)
    _lib.check(_lib.load().crab_bilinear(_lib.ctx(d), _stream(), _p(x), 1 if x.dtype == torch.float32 else 0, strides[0], strides[1], strides[2],
                                         Cc, h, w, _p(out), out.shape[-2], out.shape[-1], alpha, beta), d)
    return out


def dense_pe(G: torch.Tensor, h: int, w: int) -> torch.Tensor:
    d = _dev(G)
    assert G.dtype == torch.float32 and G.is_contiguous()
    Fq = G.shape[1]
    pe = torch.empty((h * w, 2 * Fq), device=G.device, dtype=BF16)
    _lib.check(_lib.load().crab_dense_pe(_lib.ctx(d), _stream(), _p(G), _p(pe), h, w, Fq), d)
    return pe


def add_rows(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = a[m] + b[m % b.shape[0]] (2-D, bf16)."""
    d = _dev(a)
    M, D = a.shape
    if out is None:
        out = torch.empty((M, D), device=a.device, dtype=BF16)
    _lib.check(_lib.load().crab_add_rows(_lib.ctx(d), _stream(), _p(a), a.stride(0), _p(b), b.stride(0), b.shape[0], _p(out), out.stride(0), M, D), d)
    return out


def mask_gate(prev: torch.Tensor, src: torch.Tensor):
    d = _dev(src)
    _lib.check(_lib.load().crab_mask_gate(_lib.ctx(d), _stream(), _p(prev), prev.stride(0), prev.shape[1], _p(src), src.stride(0), src.shape[0], src.shape[1]), d)
    return src


def group_mean(x: torch.Tensor, G: int, T: int, scale: float) -> torch.Tensor:
    """out[g] = scale * sum_{k<T} x[g*T + k]  (bf16 rows)."""
    d = _dev(x)
    D = x.shape[1]
    out = torch.empty((G, D), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_group_mean(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(out), out.stride(0), G, T, D, scale), d)
    return out


def act_inplace(x: torch.Tensor, act: str):
    d = _dev(x)
    assert x.is_contiguous()
    _lib.check(_lib.load().crab_act_inplace(_lib.ctx(d), _stream(), _p(x), x.numel(), ACT[act]), d)
    return x


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 on device (harness-side cast of modality inputs)."""
    if x.dtype == BF16:
        return x
    d = _dev(x)
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_cast_f32_bf16(_lib.ctx(d), _stream(), _p(x), _p(out), x.numel()), d)
    return out


def sync():
    d = torch.cuda.current_device()
    _lib.check(_lib.load().crab_sync(_lib.ctx(d), _stream()), d)


# ------------------------------------------------------------------------------------------------ VQGAN (csrc/vq_ops.hip)
def im2col3x3_strided(x: torch.Tensor, B: int, h: int, w: int, stride: int, pad_top: int, pad_left: int, oh: int, ow: int) -> torch.Tensor:
    """x [B*h*w, C] token-major -> [B*oh*ow, 9*C] window operand (zero outside the image)."""
    d = _dev(x)
    Cc = x.shape[1]
    out = torch.empty((B * oh * ow, 9 * Cc), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_im2col3x3_strided(_lib.ctx(d), _stream(), _p(x), _p(out), B, h, w, Cc, stride, pad_top, pad_left, oh, ow), d)
    return out


def groupnorm(x: torch.Tensor, B: int, HW: int, G: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6, swish: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B*HW, C] token-major bf16 -> GroupNorm(G, C) (+ swish)."""
    d = _dev(x)
    Cc = x.shape[1]
    if out is None:
        out = torch.empty_like(x)
    need = int(_lib.load().crab_groupnorm_workspace(B, HW, G))
    ws = torch.empty((need,), device=x.device, dtype=torch.uint8)
    wf = weight.dtype == torch.float32
    if (bias.dtype == torch.float32) != wf or (not wf and weight.dtype != BF16):
        raise _lib.CrabHipError("groupnorm: weight and bias are both bf16 or both fp32")
    _lib.check(_lib.load().crab_groupnorm_p(_lib.ctx(d), _stream(), _p(x), _p(out), B, HW, Cc, G, eps, _p(weight), _p(bias), 1 if wf else 0,
                                            1 if swish else 0, _p(ws), need), d)
    return out


def upsample_nearest2x(x: torch.Tensor, B: int, h: int, w: int) -> torch.Tensor:
    d = _dev(x)
    Cc = x.shape[1]
    out = torch.empty((B * 4 * h * w, Cc), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_upsample_nearest2x(_lib.ctx(d), _stream(), _p(x), _p(out), B, h, w, Cc), d)
    return out


def softmax_rows(x: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [M,N] -> bf16 softmax(scale * x) per row (out: a [M, N] view of a wider buffer, unit column stride)."""
    d = _dev(x)
    assert x.dtype == torch.float32 and x.stride(1) == 1
    M, N = x.shape
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16)
    assert out.dtype == BF16 and tuple(out.shape) == (M, N) and out.stride(1) == 1
    _lib.check(_lib.load().crab_softmax_rows(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(out), out.stride(0), M, N, scale), d)
    return out


def row_sqnorm(e: torch.Tensor) -> torch.Tensor:
    d = _dev(e)
    N, D = e.shape
    out = torch.empty((N,), device=e.device, dtype=torch.float32)
    _lib.check(_lib.load().crab_row_sqnorm(_lib.ctx(d), _stream(), _p(e), e.stride(0), N, D, _p(out)), d)
    return out


def split3(x: torch.Tensor, pattern: int) -> torch.Tensor:
    """fp32 [M, C] -> bf16 [M, 3 * round_up(C, 8)] split operand: x = hi + lo; pattern 0 = [hi | lo | hi] (A side), 1 = [hi | hi | lo] (B side).
    gemm(split3(x, 0), split3(w, 1)) = x_hi.w_hi + x_lo.w_hi + x_hi.w_lo with fp32 accumulation (crab_split3)."""
    d = _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _lib.CrabHipError("split3: fp32 [M, C] rows expected")
    M, Cc = x.shape
    Cp = (Cc + 7) // 8 * 8
    out = torch.empty((M, 3 * Cp), device=x.device, dtype=BF16)
    _lib.check(_lib.load().crab_split3(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(out), out.stride(0), M, Cc, pattern), d)
    return out


def groupnorm_f32(x: torch.Tensor, B: int, HW: int, G: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-6, swish: bool = False) -> torch.Tensor:
    """GroupNorm (+ swish) with fp32 input, output and parameters (the precise VQGAN encoder)."""
    d = _dev(x)
    assert x.dtype == weight.dtype == bias.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x)
    need = int(_lib.load().crab_groupnorm_workspace(B, HW, G))
    ws = torch.empty((need,), device=x.device, dtype=torch.uint8)
    _lib.check(_lib.load().crab_groupnorm_f32(_lib.ctx(d), _stream(), _p(x), _p(out), B, HW, x.shape[1], G, eps, _p(weight), _p(bias), 1 if swish else 0, _p(ws), need), d)
    return out


def add_bias_f32(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    d = _dev(x)
    assert x.dtype == bias.dtype == torch.float32 and x.stride(1) == 1 and bias.numel() == x.shape[1]
    _lib.check(_lib.load().crab_add_bias_f32(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(bias), x.shape[0], x.shape[1]), d)
    return x


def softmax_rows_f32(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    d = _dev(x)
    assert x.dtype == torch.float32 and x.stride(1) == 1
    M, N = x.shape
    out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().crab_softmax_rows_f32(_lib.ctx(d), _stream(), _p(x), x.stride(0), _p(out), out.stride(0), M, N, scale), d)
    return out


def row_sqnorm_f32(e: torch.Tensor) -> torch.Tensor:
    d = _dev(e)
    assert e.dtype == torch.float32 and e.stride(1) == 1
    N, D = e.shape
    out = torch.empty((N,), device=e.device, dtype=torch.float32)
    _lib.check(_lib.load().crab_row_sqnorm_f32(_lib.ctx(d), _stream(), _p(e), e.stride(0), N, D, _p(out)), d)
    return out


def vq_nearest_f32(z: torch.Tensor, e: torch.Tensor, e2: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """z fp32 [M, D] latents, e fp32 [N, D] codebook, e2 = row_sqnorm_f32(e) -> int64 [M]: offset + first argmin_n (|z|^2 + e2[n]) - 2 z . e_n,
    every term in fp32 (quantize.py:286-290): codebook ids are index work."""
    d = _dev(z)
    if z.dtype != torch.float32 or e.dtype != torch.float32 or e2.dtype != torch.float32 or z.stride(1) != 1 or e.stride(1) != 1:
        raise _lib.CrabHipError("vq_nearest_f32: fp32 row-major operands")
    M, D = z.shape
    N = e.shape[0]
    out = torch.empty((M,), device=z.device, dtype=torch.int64)
    need = int(_lib.load().crab_vq_nearest_f32_workspace(M, N))
    ws = torch.empty((need,), device=z.device, dtype=torch.uint8)
    _lib.check(_lib.load().crab_vq_nearest_f32(_lib.ctx(d), _stream(), _p(z), z.stride(0), _p(e), e.stride(0), _p(e2), M, N, D, _p(out), offset, _p(ws), need), d)
    return out


def vq_argmin(dots: torch.Tensor, e2: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """dots fp32 [M,N] = z . e^T, e2 fp32 [N] -> int64 [M]: offset + first argmin_n (e2[n] - 2 dots[m,n])."""
    d = _dev(dots)
    assert dots.dtype == torch.float32 and e2.dtype == torch.float32 and dots.stride(1) == 1
    M, N = dots.shape
    out = torch.empty((M,), device=dots.device, dtype=torch.int64)
    _lib.check(_lib.load().crab_vq_argmin(_lib.ctx(d), _stream(), _p(dots), dots.stride(0), _p(e2), M, N, _p(out), offset), d)
    return out


def mask_labels(pred: torch.Tensor) -> torch.Tensor:
    """pred [C, H, W] fp32 (a SegModule mask) -> uint8 [H, W]: 0 / 255 by sigmoid > 0.5 for C == 1, the argmax class index otherwise
    (what the reference's eval loops write to the PNG)."""
    d = _dev(pred)
    if pred.dtype != torch.float32 or pred.dim() != 3:
        raise _lib.CrabHipError("mask_labels: fp32 [C, H, W] expected")
    pred = pred.contiguous()
    C_, H, W = pred.shape
    out = torch.empty((H, W), device=pred.device, dtype=torch.uint8)
    _lib.check(_lib.load().crab_mask_labels(_lib.ctx(d), _stream(), _p(pred), C_, H * W, _p(out)), d)
    return out
