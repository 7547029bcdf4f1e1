"""tests/fuzz_bounds.py on the CPU: the bounds the differential fuzzers judge with raise no false alarm on an fp64 emulation that has only the
kernels' storage points (bf16 P, fp32 sums in another order, one bf16 store), under the fuzzers' own input laws at their extreme shapes - and
they DO fail single defects applied to the reference (a key too many or too few, swapped V rows, an accumulator rounded early, a bf16 read of an
fp32 residual, a dropped bias tile, a short K2 segment, the norm weight on the wrong side of a rounding), by a stated margin.  The pixel-path bounds (row softmax, in-place
activation, mask gate, group mean, square norms, dense positional encoding, bilinear resize, GroupNorm, the split-operand GEMM, the fp32
quantiser's margin) get the same two assertions each: a torch fp32 emulation in another summation order passes, and the defect a global-maximum
tolerance hid fails.  The last tests pin that the fuzzers hold no tolerance literal of their own."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import fuzz_bounds as FB

BF, F64 = torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bf(t):
    return t.to(BF)


def _ratio(got, ref, bound):
    return FB.worst(got, ref, bound)[0]


# ---------------------------------------------------------------------------------------------------------------------- one rounding
def test_half_ulp_is_attained_and_sufficient():
    """One bf16 rounding moves y by at most half_ulp(y) = U * (top of y's binade): never more, and nearly that much somewhere; the product U |y|
    is exceeded by a correctly rounded value at the bottom of a binade (why the bounds do not use it)."""
    g = torch.Generator().manual_seed(0)
    y = (torch.randn(200000, generator=g, dtype=F64) * 3).exp2()
    err = (FB.bf16_round(y) - y).abs()
    assert bool((err <= FB.half_ulp(y)).all())
    assert float((err / FB.half_ulp(y)).max()) > 0.99
    y1 = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=F64)
    e1 = float((FB.bf16_round(y1) - y1).abs())
    assert FB.U * float(y1) < e1 <= float(FB.half_ulp(y1))
    # stored(): an fp32 value within delta of y, rounded, stays within the bound - also where delta carries it across a binade or exceeds y itself
    yy = torch.cat([y[:50000], torch.full((1000,), 2.0, dtype=F64) - torch.rand(1000, generator=g, dtype=F64) * 1e-4, torch.zeros(10, dtype=F64)])
    for delta in (1e-7, 1e-4, 0.3):
        yh = yy + (torch.rand(yy.shape, generator=g, dtype=F64) * 2 - 1) * delta
        assert bool(((FB.bf16_round(yh) - yy).abs() <= FB.stored(yy, delta)).all())


# ------------------------------------------------------------------------------------------------------------------------- attention
CTXS = [1, 2, 7, 64, 300, 960]


def _attn_case(ctx, d, G, mode, seed):
    """fuzz_attn.py's decode law: q, k, v = 0.7 N(0,1) in bf16, scale d^-1/2, about 64 (sequence, head) rows, a cache one row longer than the context."""
    g = torch.Generator().manual_seed(seed)
    Hk = 1 if G == 7 else 2
    H, B, T = Hk * G, (9 if G == 7 else 32), ctx + 1
    q = _bf(torch.randn(B, H, 1, d, generator=g) * 0.7)
    k = _bf(torch.randn(B, Hk, T, d, generator=g) * 0.7)
    v = _bf(torch.randn(B, Hk, T, d, generator=g) * 0.7)
    keyok = torch.zeros(B, T, dtype=torch.bool); keyok[:, :ctx] = True
    if mode == "kv_start":
        ks = torch.randint(0, ctx, (B,), generator=g)
        keyok &= torch.arange(T)[None] >= ks[:, None]
    elif mode == "key_mask":
        keyok &= torch.rand(B, T, generator=g) > 0.3
        keyok[:, ctx - 1] = True                                            # (the newest key stays visible: the defects below act on it)
    return q, k, v, d ** -0.5, keyok


def _emulate_attn(q, k, v, scale, allow, kind):
    """fp64 arithmetic with the kernel's storage points only: P in bf16 for the forward kernels (the row sum keeps the unrounded p), sums in fp32 in
    another key order, one bf16 store."""
    G = q.shape[1] // k.shape[1]
    kk, vv = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    s = torch.einsum("bhsd,bhtd->bhst", q.double(), kk) * scale
    s = s.masked_fill(~allow.expand(s.shape), -math.inf)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))).float()              # fp32 p~
    pn = p.to(BF).float() if kind == "fwd" else p
    num = torch.einsum("bhst,bhtd->bhsd", pn.flip(-1), vv.float().flip(-2))                          # fp32, reversed key order
    l = p.flip(-1).sum(-1, keepdim=True)
    return torch.where(l > 0, num / l, torch.zeros_like(num)).to(BF)


@pytest.mark.parametrize("d,G", [(64, 1), (128, 1), (128, 7), (64, 7)])
@pytest.mark.parametrize("mode", ["none", "kv_start", "key_mask"])
def test_attention_bounds_no_false_alarm_and_defects(d, G, mode):
    for ctx in CTXS:
        q, k, v, scale, keyok = _attn_case(ctx, d, G, mode, seed=ctx * 7 + d + G)
        allow = keyok[:, None, None, :]
        B, T = keyok.shape
        first = keyok.float().argmax(-1)                                       # first visible key of every sequence
        rows = torch.arange(B)
        defects = {}
        a = keyok.clone(); a[:, ctx - 1] = False; defects["newest key dropped"] = (a, v)
        a = keyok.clone(); a[rows, first] = False; defects["first visible key dropped"] = (a, v)
        a = keyok.clone(); a[:, ctx] = True; defects["one stale key past the context seen"] = (a, v)
        if mode == "key_mask" and ctx >= 7:
            hidden = (~keyok[:, :ctx]).float().argmax(-1)                      # the first masked key (row without one: key 0, already visible)
            a = keyok.clone(); a[rows, hidden] = True; defects["one key_mask bit ignored"] = (a, v)
        if ctx >= 2 and mode == "none":
            v2 = v.clone(); v2[:, :, ctx - 2], v2[:, :, ctx - 1] = v[:, :, ctx - 1], v[:, :, ctx - 2]
            defects["V rows of two adjacent keys swapped"] = (keyok, v2)
        bad_refs = {name: FB.attn_ref(q, k, vd, scale, a[:, None, None, :])[0] for name, (a, vd) in defects.items()}
        for kind in ("decode", "fwd"):
            ref, bound, rel = FB.attn_bound(q, k, v, scale, allow, kind=kind)
            assert rel <= FB.SLACK_CAP, (kind, ctx, rel / FB.SLACK_CAP)
            got = _emulate_attn(q, k, v, scale, allow, kind)
            r = _ratio(got, ref, bound)
            assert r <= 1.0, f"false alarm: {kind} ctx={ctx} d={d} G={G} mask={mode}: err / bound {r:.3f}"
            need = 2.0 if kind == "decode" else (1.5 if ctx == 960 else 1.0)
            for name, bad_ref in bad_refs.items():
                r = _ratio(bad_ref, ref, bound)
                assert r > need, f"missed: {name}, {kind} ctx={ctx} d={d} G={G} mask={mode}: err / bound {r:.3f} (asked > {need})"


def test_forward_causal_future_key_and_bias():
    """The forward law at Sq = Skv = 300 causal (rows beyond 128: the 128-row kernel's second block) and a gated-bias case: no false alarm; one
    future key seen on a row >= 128 is caught."""
    g = torch.Generator().manual_seed(3)
    B, H, Hk, S, d = 1, 4, 2, 300, 128
    q, k, v = (_bf(torch.randn(B, h, S, d, generator=g) * 0.7) for h in (H, Hk, Hk))
    allow = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None].expand(B, H, S, S)
    ref, bound, rel = FB.attn_bound(q, k, v, d ** -0.5, allow, kind="fwd")
    assert rel <= FB.SLACK_CAP
    assert _ratio(_emulate_attn(q, k, v, d ** -0.5, allow, "fwd"), ref, bound) <= 1.0
    a2 = allow.clone(); a2[:, :, 128:, :] |= torch.diag(torch.ones(S - 1, dtype=torch.bool), 1)[128:]     # rows >= 128 see key row + 1
    bad_ref, _ = FB.attn_ref(q, k, v, d ** -0.5, a2)
    assert _ratio(bad_ref[:, :, 128:], ref[:, :, 128:], bound[:, :, 128:]) > 1.5
    bias, gate = torch.randn(H, S, S, generator=g) * 0.5, torch.rand(B, H, S, generator=g) * 2
    full = torch.ones(B, H, S, S, dtype=torch.bool)
    ref, bound, rel = FB.attn_bound(q, k, v, d ** -0.5, full, bias, gate, kind="fwd")
    assert rel <= FB.SLACK_CAP
    G = H // Hk
    s = torch.einsum("bhsd,bhtd->bhst", q.double(), k.double().repeat_interleave(G, 1)) * d ** -0.5 + gate.double()[..., None] * bias.double()[None]
    p = torch.exp(s - s.max(-1, keepdim=True).values).float()
    got = (torch.einsum("bhst,bhtd->bhsd", p.to(BF).float(), v.float().repeat_interleave(G, 1)) / p.sum(-1, keepdim=True)).to(BF)
    assert _ratio(got, ref, bound) <= 1.0


def test_two_key_row_needs_the_full_half_ulp_of_p():
    """Why the forward bound carries 2 U S_e: p~ = (1, 1 + 2^-8 - tiny) / 2 rounds its second entry down by half an ulp at the BOTTOM of a binade; with
    v = (0, 1) the output moves by more than U S_e + the store's half ulp - legitimately."""
    p = torch.tensor([1.0, 0.5 * (1 + 2.0 ** -8 - 2.0 ** -20)], dtype=F64)
    v = torch.tensor([0.0, 1.0], dtype=F64)
    o = float((p * v).sum() / p.sum())
    got = float((FB.bf16_round(p) * v).sum() / p.sum())
    S = o
    assert abs(got - o) > FB.U * S and abs(got - o) <= 2 * FB.U * S


# ------------------------------------------------------------------------------------------------------------------------------ GEMM
def _gemm_case(K, K2, act, res, seed, M=33, N=40):
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(M, K, generator=g) * 0.5)
    w = _bf(torch.randn(N, K, generator=g) * K ** -0.5)
    x2 = _bf(torch.randn(M, K2, generator=g) * 0.5) if K2 else None
    w2 = _bf(torch.randn(N, K2, generator=g) * 0.1) if K2 else None
    b = _bf(torch.randn(N, generator=g) * 0.1)
    No = N // 2 if act == "swiglu_pair" else N
    r = None
    if res and act != "swiglu_pair":
        r = torch.randn(M, No, generator=g)
        r = r if res == "fp32" else _bf(r)
    return x, w, x2, w2, b, r


def _emulate_gemm(x, w, x2, w2, b, act, r, out_bf16, round_acc=False):
    """fp32 accumulation in another order (the K columns reversed, K2 first), the epilogue in fp32, one rounding at a bf16 store."""
    z = torch.zeros(x.shape[0], w.shape[0])
    if x2 is not None: z = z + x2.float().flip(-1) @ w2.float().flip(-1).t()
    z = z + x.float().flip(-1) @ w.float().flip(-1).t()
    if round_acc: z = z.to(BF).float()
    if b is not None: z = z + b.float()
    y = FB.act64(z.double(), act).float()                                # the activation itself correctly rounded to fp32
    if r is not None: y = y + r.float()
    return y.to(BF) if out_bf16 else y


@pytest.mark.parametrize("act", ["none", "gelu", "quick_gelu", "relu", "silu", "swiglu_pair"])
@pytest.mark.parametrize("K,K2", [(8, 0), (8, 32), (72, 0), (72, 32), (4096, 0), (4096, 32)])
def test_gemm_bounds_no_false_alarm_and_defects(act, K, K2):
    for res in (None, "bf16", "fp32"):
        x, w, x2, w2, b, r = _gemm_case(K, K2, act, res, seed=K + K2 + len(act))
        for out_bf16 in (False, True):
            if res == "fp32" and out_bf16: continue                      # the library stores an fp32 stream in fp32
            y, bound = FB.gemm_bound(x, w, x2, w2, b, act, r, out_bf16=out_bf16)
            rr = _ratio(_emulate_gemm(x, w, x2, w2, b, act, r, out_bf16), y, bound)
            assert rr <= 1.0, f"false alarm: K={K}+{K2} {act} res={res} bf16 out={out_bf16}: err / bound {rr:.3f}"
        # the defects, on the fp32 output (what the fuzzer's flat 6e-3 could not see)
        y, bound = FB.gemm_bound(x, w, x2, w2, b, act, r, out_bf16=False)
        defects = {"accumulator rounded to bf16 before the epilogue": _emulate_gemm(x, w, x2, w2, b, act, r, False, round_acc=True).double()}
        if res == "fp32" and r is not None: defects["fp32 residual read as bf16"] = FB.gemm_ref(x, w, x2, w2, b, act, r.to(BF))
        b2 = b.clone(); b2[b.numel() - b.numel() % 16:] = 0
        defects["bias dropped on the last ragged 16-column tile"] = FB.gemm_ref(x, w, x2, w2, b2, act, r)
        if K2:
            x2s = x2.clone(); x2s[:, -8:] = 0
            defects["the last 8 columns of the K2 segment dropped"] = FB.gemm_ref(x, w, x2s, w2, b, act, r)
        for name, bad_y in defects.items():
            rr = _ratio(bad_y, y, bound)
            assert rr > 2.0, f"missed: {name}, K={K}+{K2} {act} res={res}: err / bound {rr:.3f}"


# --------------------------------------------------------------------------------------------------------- norms, SwiGLU, router, RoPE
def _f32_sum_other_order(t):
    return t.float().flip(-1).sum(-1, keepdim=True)


@pytest.mark.parametrize("scale", [0.1, 1.0, 30.0])
@pytest.mark.parametrize("D", [8, 200, 4096])
def test_norm_bounds_no_false_alarm_and_defect(scale, D):
    g = torch.Generator().manual_seed(int(scale * 10) + D)
    M = 65
    xb = torch.randn(M, D, generator=g) * scale + 0.5
    w = _bf(1 + 0.2 * torch.randn(D, generator=g))
    b = _bf(0.1 * torch.randn(D, generator=g))
    for f32 in (False, True):
        x = xb if f32 else _bf(xb)
        for eps in (1e-5, 1e-12):
            xf = x.float()
            rstd = torch.rsqrt(_f32_sum_other_order(xf * xf) / D + eps)
            xh = xf * rstd
            got = ((xh if f32 else xh.to(BF).float()) * w.float()).to(BF)
            ref, bound = FB.rmsnorm_bound(x, w, eps, round_xhat=not f32)
            r = _ratio(got, ref, bound)
            assert r <= 1.0, f"false alarm: rmsnorm scale={scale} D={D} fp32 in={f32} eps={eps}: {r:.3f}"
            if not f32 and D >= 200:
                wrong = (xh * w.float()).to(BF)                         # the weight applied BEFORE the normalisation rounding
                assert _ratio(wrong, ref, bound) > 1.0, f"missed: norm weight before the rounding, scale={scale} D={D}"
            mean = _f32_sum_other_order(xf) / D
            xc = xf - mean
            rs = torch.rsqrt(_f32_sum_other_order(xc * xc) / D + eps)
            got = (xc * rs * w.float() + b.float()).to(BF)
            ref, bound = FB.layernorm_bound(x, w, b, eps)
            r = _ratio(got, ref, bound)
            assert r <= 1.0, f"false alarm: layernorm scale={scale} D={D} fp32 in={f32} eps={eps}: {r:.3f}"
            assert _ratio(ref * (1 + 2.0 ** -7), ref, bound) > 1.0        # a bf16 ulp everywhere is not hidden


def test_swiglu_and_router_bounds():
    g = torch.Generator().manual_seed(11)
    gu = _bf(torch.randn(65, 2 * 1376, generator=g))
    ref, bound = FB.swiglu_bound(gu)
    got = (torch.nn.functional.silu(gu[:, :1376].float()) * gu[:, 1376:].float()).to(BF)
    assert _ratio(got, ref, bound) <= 1.0
    assert _ratio(FB.bf16_round(ref).float().to(BF).float() * (1 + 2.0 ** -7), ref, bound) > 1.0
    for K, (nl, r), nproj in [(64, (3, 8), 3), (4096, (8, 4), 2), (11008, (3, 16), 1)]:
        x = _bf(torch.randn(65, K, generator=g) * 0.5)
        ra = _bf(torch.randn((nproj * (nl + r) + 15) // 16 * 16, K, generator=g) * K ** -0.5)
        ucols = nproj * nl * r + 8
        ref, bound = FB.route_bound(x, ra, nproj, nl, r, ucols, 2.0)
        t = x.float().flip(-1) @ ra.float().flip(-1).t()
        got = torch.zeros(65, ucols)
        for p in range(nproj):
            tt = t[:, p * (nl + r):(p + 1) * (nl + r)]
            got[:, p * nl * r:(p + 1) * nl * r] = (2.0 * torch.softmax(tt[:, :nl], -1)[:, :, None] * tt[:, None, nl:]).reshape(65, nl * r)
        assert _ratio(got.to(BF), ref, bound) <= 1.0, (K, nl, r)
        swapped = ref.clone(); swapped[:, 0], swapped[:, 1] = ref[:, 1], ref[:, 0]
        assert _ratio(swapped, ref, bound) > 2.0


def test_fused_router_has_two_forms_of_its_row():
    """The M <= 16 tail mixes the normalised row BEFORE its bf16 store, the other paths the stored row: each emulation passes its own form through
    Run.judge_any and neither passes the other's reference alone; a swapped column passes neither."""
    g = torch.Generator().manual_seed(21)
    M, N = 8, 1024
    c = _bf(torch.randn(M, N, generator=g))
    nw = _bf(1 + 0.1 * torch.randn(N, generator=g))
    ra = _bf(torch.randn(48, N, generator=g) * 0.05)
    xh = c.float() * torch.rsqrt(c.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    h_st = (xh.to(BF).float() * nw.float()).to(BF)                                         # as stored
    h_un = xh * nw.float()                                                                  # before any rounding

    def mix(h):
        t = h.float().flip(-1) @ ra.float().flip(-1).t()
        u = torch.zeros(M, 96)
        for p in range(3):
            tt = t[:, p * 11:(p + 1) * 11]
            u[:, p * 24:(p + 1) * 24] = (2.0 * torch.softmax(tt[:, :3], -1)[:, :, None] * tt[:, None, 3:]).reshape(M, 24)
        return u.to(BF)

    hx = FB.rmsnorm_bound(c, nw, 1e-5, round_xhat=False)[0]
    forms = [FB.route_bound(h_st, ra, 3, 3, 8, 96, 2.0), FB.route_bound(hx, ra, 3, 3, 8, 96, 2.0, x_rel=FB.rx_rel(N) + 2 * FB.U32)]
    for got, own in ((mix(h_st), 0), (mix(h_un), 1)):
        bad = []
        assert FB.Run().judge_any(bad, "case", "router", got, forms) <= 1.0 and not bad
        assert _ratio(got, *forms[own]) <= 1.0 < _ratio(got, *forms[1 - own])
        wrong = got.clone(); wrong[:, 0], wrong[:, 1] = got[:, 1], got[:, 0]
        assert FB.Run().judge_any(bad, "case", "router", wrong, forms) > 2.0 and len(bad) == 1


def test_rope_pair_bound():
    """Two fp32 summation orders of one projection, each rounded to bf16, rotated with the same fp32 operations and rounded again: within the derived
    bound everywhere, bit-identical where the bound is 0; a rotation by the neighbouring position is not."""
    g = torch.Generator().manual_seed(5)
    M, K, H, d = 300, 1024, 3, 64
    x, w = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(H * d, K, generator=g) * K ** -0.5)
    bias = _bf(torch.randn(H * d, generator=g))
    y64, ceil = FB.gemm_ceiling(x, w, None, None, bias)
    ang = 7 * 10000.0 ** (-torch.arange(d // 2, dtype=F64) * 2 / d)
    cs, sn = torch.cos(ang).float(), torch.sin(ang).float()

    def form(order):
        y = ((x.float()[:, order] @ w.float()[:, order].t()) + bias.float()).to(BF).float().view(M, H, d)
        lo, hi = y[..., :d // 2], y[..., d // 2:]
        return torch.cat([lo * cs - hi * sn, hi * cs + lo * sn], -1).to(BF)

    a, b = form(torch.arange(K)), form(torch.arange(K).flip(0))
    bound = FB.rope_pair_bound(y64.view(M, H, d), ceil.view(M, H, d), cs, sn)
    assert _ratio(a, b.double(), bound) <= 1.0
    same = bound == 0                                                       # where no flip is possible the forms must agree bit for bit
    assert bool(same.any()) and torch.equal(a[same], b[same])
    ang2 = 8 * 10000.0 ** (-torch.arange(d // 2, dtype=F64) * 2 / d)
    cs, sn = torch.cos(ang2).float(), torch.sin(ang2).float()
    assert _ratio(form(torch.arange(K)), b.double(), bound) > 2.0


# ----------------------------------------------------------------------------------------------------------------------- pixel path
ULP = 1 + 2.0 ** -7                                                         # one bf16 ulp on every element: never hidden by a bf16 output's bound


def _softmax_emul(x, scale, f32):
    s = x * torch.tensor(scale, dtype=torch.float32)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    out = p / _f32_sum_other_order(p)
    return out if f32 else out.to(BF)


@pytest.mark.parametrize("N,scale", [(1, 1.0), (63, 0.37), (257, 0.125), (4096, 0.125), (4096, 1.0)])
def test_softmax_rows_bound(N, scale):
    """No false alarm in either output format (a dominant 3e4 entry included: the rest underflows and is held to 2^-126); the fuzzer's own case
    N = 4096, scale 0.125, x[0, 0] = 3e4 with every row but the first zeroed - which the global-maximum rule passed - fails."""
    g = torch.Generator().manual_seed(N)
    x = torch.randn(5, N, generator=g) * 30.0
    x[0, 0] = 3.0e4
    for f32 in (True, False):
        ref, bound = FB.softmax_rows_bound(x, scale, out_bf16=not f32)
        r = _ratio(_softmax_emul(x, scale, f32), ref, bound)
        assert r <= 1.0, f"false alarm: N={N} scale={scale} fp32={f32}: {r:.3f}"
        if N > 1:
            zeroed = ref.clone(); zeroed[1:] = 0
            assert _ratio(zeroed, ref, bound) > 2.0
            if N < 4096: assert _ratio(torch.cat([ref[:, 1:], ref[:, :1]], 1), ref, bound) > 2.0        # columns rotated by one
        if not f32: assert _ratio(ref * ULP, ref, bound) > 1.0
    if N > 1: assert float(FB.softmax_rows_bound(x, scale, False)[1][0, 1:].max()) == FB.TINY          # underflowed entries: the smallest normal, not 0


@pytest.mark.parametrize("act", ["gelu", "quick_gelu", "relu", "silu"])
def test_act_bound(act):
    g = torch.Generator().manual_seed(2)
    x = _bf(torch.randn(100003, generator=g) * 3)                            # the fuzzer's law
    xf = x.float()
    got = {"gelu": F.gelu(xf), "quick_gelu": xf * torch.sigmoid(1.702 * xf), "relu": F.relu(xf), "silu": F.silu(xf)}[act].to(BF)
    ref, bound = FB.act_bound(x, act)
    assert _ratio(got, ref, bound) <= 1.0
    if act == "gelu":
        cut = got.clone(); cut[xf < -2] = 0                                  # worst error 0.044 against the old tolerance of 4.5e-3 max|want| = 0.056
        assert float((cut.float() - ref).abs().max()) < 4.5e-3 * float(ref.abs().max()) and _ratio(cut, ref, bound) > 100.0
    if act != "relu": assert _ratio(ref * ULP, ref, bound) > 1.0
    else: assert _ratio(ref, FB.act_bound(x, "none")[0], bound) > 1.0        # relu left out


def test_mask_gate_and_group_mean_bounds():
    g = torch.Generator().manual_seed(3)
    for M, nc, D in [(1, 1, 1), (5, 64, 63), (784, 65, 256), (3, 130, 100)]:
        prev, src = _bf(torch.randn(M, nc, generator=g) * 3), _bf(torch.randn(M, D, generator=g))
        s = prev.float().flip(-1).sum(-1, keepdim=True)
        ref, bound = FB.mask_gate_bound(prev, src)
        got = (src.float() * (1.0 / (1.0 + torch.exp(-(s / nc))) + 1.0)).to(BF)
        assert _ratio(got, ref, bound) <= 1.0, (M, nc, D)
        assert _ratio(ref * ULP, ref, bound) > 1.0
        if nc == 65:
            wrong = (src.float() * (torch.sigmoid(s / 64) + 1.0)).to(BF)     # the mean taken over 64, not ncls
            assert _ratio(wrong, ref, bound) > 1.0
            wrong = (src.float() * (torch.sigmoid(prev.float()[:, :64].sum(-1, keepdim=True) / nc) + 1.0)).to(BF)      # the 65th class dropped
            assert _ratio(wrong, ref, bound) > 1.0
    for G_, T, D in [(1, 1, 1), (6, 10, 256), (71, 6, 8)]:
        x = _bf(torch.randn(G_ * T, D, generator=g))
        for sc in (1.0, 1.0 / T):
            ref, bound = FB.group_mean_bound(x, T, sc)
            got = (torch.tensor(sc, dtype=torch.float32) * x.float().view(G_, T, D).flip(1).sum(1)).to(BF)
            assert _ratio(got, ref, bound) <= 1.0, (G_, T, D, sc)
            assert _ratio(ref * ULP, ref, bound) > 1.0
            if T > 1:
                short = (sc * x.float().view(G_, T, D)[:, :-1].sum(1)).to(BF)
                assert _ratio(short, ref, bound) > 2.0


@pytest.mark.parametrize("D", [1, 63, 65, 300])
def test_sqnorm_bound(D):
    g = torch.Generator().manual_seed(D)
    for e in (torch.randn(9, D, generator=g), _bf(torch.randn(9, D, generator=g))):
        ref, bound = FB.sqnorm_bound(e)
        ef = e.float()
        assert _ratio((ef * ef).flip(-1).sum(-1), ref, bound) <= 1.0
        if D % 64 and D > 64:
            ec = ef[:, :D - D % 64]
            assert _ratio((ec * ec).sum(-1), ref, bound) > 2.0               # the last D % 64 elements missing


def _dense_pe_emul(G, h, w, half=0.5, swap=False):
    ys, xs = (torch.arange(h).float() + half) / h, (torch.arange(w).float() + half) / w
    if swap: cx, cy = (2 * ys - 1)[:, None, None].expand(h, w, 1), (2 * xs - 1)[None, :, None].expand(h, w, 1)
    else: cx, cy = (2 * xs - 1)[None, :, None], (2 * ys - 1)[:, None, None]
    a = 6.283185307179586 * (cy * G[1] + cx * G[0])
    return torch.cat([a.sin(), a.cos()], -1).reshape(h * w, -1).to(BF)


@pytest.mark.parametrize("h,w,Fq,gs", [(1, 1, 1, 1.0), (3, 7, 16, 1.0), (28, 9, 128, 1.0), (7, 5, 16, 10.0)])
def test_dense_pe_bound(h, w, Fq, gs):
    g = torch.Generator().manual_seed(h * w)
    G = torch.randn(2, Fq, generator=g) * gs
    ref, bound = FB.dense_pe_bound(G, h, w)
    assert _ratio(_dense_pe_emul(G, h, w), ref, bound) <= 1.0
    assert _ratio(ref * ULP, ref, bound) > 1.0
    assert _ratio(_dense_pe_emul(G, h, w, half=0.0), ref, bound) > 2.0       # without the + 0.5
    if h != w: assert _ratio(_dense_pe_emul(G, h, w, swap=True), ref, bound) > 2.0


def _bilinear_emul(v, H, W, alpha, beta, out0, corners=False, clamp=True):
    """The kernel's expression in fp32 with the weights applied in the other order (columns first)."""
    C, h, w = v.shape
    def axis(n, N):
        i = torch.arange(N, dtype=torch.float32)
        f = i * (float(n - 1) / max(N - 1, 1)) if corners else (i + 0.5) * (torch.tensor(float(n)) / torch.tensor(float(N))) - 0.5
        if clamp: f = f.clamp_min(0.0)
        i0 = f.to(torch.int64).clamp(0, n - 1)                               # (int) truncates towards 0
        return i0, (i0 + 1).clamp_max(n - 1), f - i0
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    v, ly = v.float(), ly[:, None]
    left = (1 - ly) * v[:, y0][:, :, x0] + ly * v[:, y1][:, :, x0]
    right = (1 - ly) * v[:, y0][:, :, x1] + ly * v[:, y1][:, :, x1]
    val = (1 - lx) * left + lx * right
    return (beta * out0 if beta != 0 else 0.0) + alpha * val


@pytest.mark.parametrize("h,w,H,W", [(1, 1, 5, 7), (7, 5, 1, 1), (7, 5, 3, 2), (3, 5, 7, 11), (4, 6, 4, 6), (28, 28, 224, 224), (56, 3, 37, 50)])
def test_bilinear_bound(h, w, H, W):
    g = torch.Generator().manual_seed(h + W)
    for bf in (False, True):
        v = torch.randn(3, h, w, generator=g)
        v = _bf(v) if bf else v
        out0 = torch.randn(3, H, W, generator=g)
        for alpha, beta in ((1.0, 0.0), (0.5, 1.0), (0.5, 0.25)):
            ref, bound = FB.bilinear_bound(v, (h * w, w, 1), h, w, H, W, alpha, beta, out0)
            tm = v.permute(1, 2, 0).contiguous()                             # token-major storage of the same image
            ref2, bound2 = FB.bilinear_bound(tm, (1, w * 3, 3), h, w, H, W, alpha, beta, out0)
            assert torch.equal(ref, ref2) and torch.equal(bound, bound2)
            want = beta * out0 + alpha * F.interpolate(v.float()[None], size=(H, W), mode="bilinear", align_corners=False)[0]
            assert _ratio(want, ref, bound) <= 1.0, (bf, alpha, beta)
            assert _ratio(_bilinear_emul(v, H, W, alpha, beta, out0), ref, bound) <= 1.0, (bf, alpha, beta)
            if (h, w) != (H, W) and h * w > 1:
                assert _ratio(_bilinear_emul(v, H, W, alpha, beta, out0, corners=True), ref, bound) > 2.0
            if (H > h > 1) or (W > w > 1):                                    # upsampling along an axis with more than one source row: f < 0 at the edge
                assert _ratio(_bilinear_emul(v, H, W, alpha, beta, out0, clamp=False), ref, bound) > 2.0
    nan0 = torch.full((3, H, W), float("nan"))
    assert bool(torch.isfinite(FB.bilinear_bound(v, (h * w, w, 1), h, w, H, W, 0.5, 0.0, nan0)[0]).all())


def _groupnorm_emul(x, B, HW, G, w, b, eps, swish, out_fp32, shifted=True):
    """The kernels' arithmetic in fp32, sums in another order."""
    C = x.shape[1]
    xg = x.float().view(B, HW, G, C // G)
    k = xg[:, :1, :, :1] if shifted else torch.zeros(())
    v = (xg - k).permute(0, 2, 1, 3).reshape(B, G, -1)
    n = v.shape[-1]
    m = (_f32_sum_other_order(v) / n)
    var = (_f32_sum_other_order(v * v) / n - m * m).clamp_min(0.0)
    mean, rstd = (m.view(B, 1, G, 1) + k), torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)).view(B, 1, G, 1)
    y = ((xg - mean) * rstd * w.float().view(G, -1) + b.float().view(G, -1)).view(B * HW, C)
    if swish: y = y / (1.0 + torch.exp(-y))
    return y if out_fp32 else y.to(BF)


@pytest.mark.parametrize("C,G,HW", [(8, 8, 1), (24, 8, 65), (64, 32, 70), (1024, 32, 130), (32, 32, 4097)])
def test_groupnorm_bound(C, G, HW):
    g = torch.Generator().manual_seed(C + HW)
    B = 3
    wt, bs = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    for scale, shift in ((2.0, 0.5), (0.3, 0.0), (0.01, 100.0)):
        xf = torch.randn(B * HW, C, generator=g) * scale + shift
        for form in ("f32", "bf16, fp32 params", "bf16, bf16 params"):
            x = xf if form == "f32" else _bf(xf)
            w_, b_ = (_bf(wt), _bf(bs)) if form == "bf16, bf16 params" else (wt, bs)
            for sw in (False, True):
                ref, bound = FB.groupnorm_bound(x, B, HW, G, w_, b_, 1e-6, sw, out_fp32=form == "f32")
                r = _ratio(_groupnorm_emul(x, B, HW, G, w_, b_, 1e-6, sw, form == "f32"), ref, bound)
                assert r <= 1.0, f"false alarm: C={C} G={G} HW={HW} {form} swish={sw} scale={scale}: {r:.3f}"
                if form != "f32" and shift < 100.0: assert _ratio(ref * ULP, ref, bound) > 1.0      # (at mean 100 a bf16 image has spread 0 or 1/2 ulp: rstd up to 1000)
                if form == "f32" and shift == 100.0 and HW * (C // G) > 8:       # the unshifted E[x^2] - E[x]^2 in fp32: mean 100, spread 0.01
                    assert _ratio(_groupnorm_emul(x, B, HW, G, w_, b_, 1e-6, sw, True, shifted=False), ref, bound) > 2.0
                if form != "bf16, bf16 params" and HW * C >= 64 * 70 and (form == "f32" or shift < 100.0):            # bf16-rounded parameters where fp32 ones were given
                    wrong = _groupnorm_emul(x, B, HW, G, _bf(wt), _bf(bs), 1e-6, sw, form == "f32")
                    assert _ratio(wrong, ref, bound) > (2.0 if form == "f32" else 1.0), (form, sw, scale)
    # a constant image: var = 0, the output is the bias
    x = torch.full((B * HW, C), 3.25)
    ref, bound = FB.groupnorm_bound(x, B, HW, G, wt, bs, 1e-6, False, out_fp32=True)
    assert float((ref - bs.double()).abs().max()) == 0.0 and _ratio(_groupnorm_emul(x, B, HW, G, wt, bs, 1e-6, False, True), ref, bound) <= 1.0


@pytest.mark.parametrize("K,xs", [(8, 0.1), (24, 1.0), (200, 1.0), (1152, 20.0)])
def test_split_gemm_bound(K, xs):
    g = torch.Generator().manual_seed(K)
    x, w = torch.randn(65, K, generator=g) * xs, torch.randn(96, K, generator=g) * K ** -0.5
    ref, bound = FB.split_gemm_bound(x, w)
    xh, wh = x.to(BF), w.to(BF)
    xl, wl = (x - xh.float()).to(BF), (w - wh.float()).to(BF)
    a, b = torch.cat([xh, xl, xh], 1).float(), torch.cat([wh, wh, wl], 1).float()
    assert _ratio(a.flip(-1) @ b.flip(-1).t(), ref, bound) <= 1.0
    assert _ratio(xh.float() @ wh.float().t() + xh.float() @ wl.float().t(), ref, bound) > 1.0        # the lo.hi term missing (1.4 at K = 1152, 349 at K = 24)
    assert _ratio(xh.float() @ wh.float().t(), ref, bound) > 2.0                                    # plain bf16 operands


VQ_GRID = [(D, N) for D in (4, 32, 64, 256) for N in (1, 63, 64, 65, 1000, 16384)]              # scripts/fuzz_ops.py, 700 rows


def _vq_case(D, N, seed, M=700):
    g = torch.Generator().manual_seed(seed)
    e, z = torch.randn(N, D, generator=g), torch.randn(M, D, generator=g)
    if N > 8:
        e[N // 2] = e[1]
        z[0] = e[1]
    return z, e


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("D,N", VQ_GRID)
def test_vq_margin_share_and_verdict(D, N, seed):
    """From the reference alone: the rows the margin leaves to the fp32 arithmetic stay under VQ_EITHER_CAP (2 %) at every point of the fuzzer's
    grid; torch's fp32 expression passes; an id one place off the fp64 arg-min on a decided row, an id out of range, and the later copy of a
    duplicated entry fail."""
    z, e = _vq_case(D, N, seed=seed)
    want, either, allowed = FB.vq_margin(z, e)
    share = float(either.double().mean())
    print(f"vq_margin D={D} N={N} seed={seed}: EITHER share {share:.4f}")
    assert share <= FB.VQ_EITHER_CAP
    assert bool(allowed.gather(1, want[:, None]).all())
    d = (z ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2 * z @ e.t()
    bad, sh = FB.vq_verdict(torch.argmin(d, 1) + 7, z, e, offset=7)
    assert bad == 0 and sh == share
    if N > 8:
        assert int(want[0]) == 1 and not bool(either[0])
        dup = want.clone(); dup[0] = N // 2
        assert FB.vq_verdict(dup, z, e)[0] == 1
    if N > 1:
        row = int((~either).float().argmax())                               # a decided row: only its fp64 arg-min is allowed
        assert int(allowed[row].sum()) == 1
        for step in (1, N - 1):                                             # one place off, either side
            off = want.clone(); off[row] = (want[row] + step) % N
            assert FB.vq_verdict(off, z, e)[0] == 1
        assert int(((want + 1) % N != want).sum()) == 700 and FB.vq_verdict((want + 1) % N, z, e)[0] >= 700 * (1 - 2 * FB.VQ_EITHER_CAP)
    oob = want.clone(); oob[-1] = 0x7fffffff
    assert FB.vq_verdict(oob, z, e)[0] == 1


# ------------------------------------------------------------------------------------------------------------------------ coverage pin
LITERAL = re.compile(r"(?<![\w.])\d+(?:\.\d+)?e-\d+")


def _src(name):
    with open(os.path.join(ROOT, "scripts", name)) as f:
        return f.read()


def test_fuzzers_hold_no_tolerance_literal():
    """The changed fuzzers judge through tests/fuzz_bounds.py alone: no float literal with a negative exponent is left in them but the epsilons of the
    norms they call (fuzz_ops.py: in the norm / router / SwiGLU branches)."""
    assert set(LITERAL.findall(_src("fuzz_gemm.py"))) <= {"1e-5"}           # the post-norm's eps, an operand
    assert not LITERAL.findall(_src("fuzz_attn.py"))
    assert not LITERAL.findall(_src("fuzz_rope_epilogue.py"))
    with open(os.path.join(ROOT, "tests", "test_attn_laws_gpu.py")) as f:
        laws_src = f.read()
    assert not LITERAL.findall(laws_src) and "attn_bound_weighted" in laws_src and "torch.softmax" not in laws_src
    ops_src = _src("fuzz_ops.py")
    assert set(LITERAL.findall(ops_src)) <= {"1e-5", "1e-6", "1e-12"}       # the whole file: the eps operands of the norms and of GroupNorm, nothing else
    norm = ops_src[ops_src.index('if kind in ("rmsnorm", "layernorm")'):ops_src.index('elif kind == "embedding"')]
    assert set(LITERAL.findall(norm)) <= {"1e-5", "1e-6", "1e-12"}          # the eps choices
    route = ops_src[ops_src.index('elif kind == "route"'):ops_src.index('elif kind == "vq_nearest"')]
    assert not LITERAL.findall(route) and route.count("run.judge(") == 2    # router and SwiGLU
    for name in ("fuzz_gemm.py", "fuzz_attn.py", "fuzz_rope_epilogue.py", "fuzz_ops.py", "fuzz_seg.py"):
        s = _src(name)
        assert "from tests import fuzz_bounds as FB" in s and "run.judge(" in s and "{run}" in s, name
        assert ".float() @" not in s and "torch.softmax" not in s, name      # no fp32 reference left in the changed branches


def _branch(src, start, end):
    return src[src.index(start):src.index(end)]


def test_pixel_path_fuzzers_hold_no_tolerance_literal():
    """scripts/fuzz_seg.py and the r06 branches of scripts/fuzz_ops.py: every floating-point kind goes through run.judge with a bound of
    tests/fuzz_bounds.py (the quantiser through FB.vq_verdict and the cap), and no tolerance literal is left.  The one literal of fuzz_seg.py is
    close64's relative 1e-6 between two fp64 evaluations of the eval loops' metrics - an equality kind, unchanged."""
    seg = _src("fuzz_seg.py")
    assert LITERAL.findall(seg) == ["1e-6"] and "rel=1e-6" in seg and "relerr" not in seg
    assert "run.judge(" in seg and "guarded(" in seg and "intact(" in seg and "ops.copy_rows_batched(" in seg
    for name in ("bilinear", "dense_pe", "mask_gate", "group_mean", "act", "softmax_rows", "sqnorm"):
        assert f"FB.{name}_bound(" in seg, name
    ops_src = _src("fuzz_ops.py")
    vq = _branch(ops_src, 'elif kind == "vq_nearest"', 'elif kind == "split_gemm"')
    assert "FB.vq_verdict(" in vq and "FB.VQ_EITHER_CAP" in vq and "topk" not in vq
    sg = _branch(ops_src, 'elif kind == "split_gemm"', 'elif kind == "groupnorm_f32"')
    assert "run.judge(" in sg and "FB.split_gemm_bound(" in sg
    gn = ops_src[ops_src.index('elif kind == "groupnorm_f32"'):]
    assert "run.judge(" in gn and "FB.groupnorm_bound(" in gn and "guarded(" in gn and "intact(" in gn
    assert FB.VQ_EITHER_CAP == 0.02
