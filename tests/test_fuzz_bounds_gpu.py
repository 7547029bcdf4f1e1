"""The fuzzers' verdict (tests/fuzz_bounds.py) on REAL kernel noise: at shapes only the fuzzers visit the kernel's output passes against the true
fp64 reference on every element - and the same output fails against the reference with one defect in it (a key too many or too few, swapped V
rows, an accumulator rounded early, an fp32 residual read as bf16, a dropped bias tile, a short K2 segment), so none of those can hide in the
kernels' own rounding."""
import pytest
import torch

from tests import fuzz_bounds as FB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _judge(what, got, case, kind, defects):
    """got against the true reference (must pass) and against every defect reference (must fail)."""
    q, k, v, scale, allow = case
    ref, bound, rel = FB.attn_bound(q, k, v, scale, allow, kind=kind)
    assert rel <= FB.SLACK_CAP, (what, rel)
    ratio, idx = FB.worst(got, ref, bound)
    print(f"{what}: worst err / bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (what, ratio, idx)
    for name, (a, vd) in defects.items():
        ref_d, bound_d, _ = FB.attn_bound(q, k, vd, scale, a, kind=kind)
        r = FB.worst(got, ref_d, bound_d)[0]
        print(f"    {name}: {r:.2f}")
        assert r > 1.0, f"{what}: the verdict would pass a kernel with this defect: {name} ({r:.3f})"


def _decode_defects(keyok, v, ctx, Tmax, ks=None):
    B = keyok.shape[0]
    rows = torch.arange(B, device=keyok.device)
    first = keyok.float().argmax(-1)
    out = {}
    a = keyok.clone(); a[:, ctx - 1] = False; out["newest key dropped"] = (a[:, None, None, :], v)
    a = keyok.clone(); a[rows, first] = False; out["first visible key dropped"] = (a[:, None, None, :], v)
    if ctx < Tmax:
        a = keyok.clone(); a[:, ctx] = True; out["one stale key past the context seen"] = (a[:, None, None, :], v)
    v2 = v.clone(); v2[:, :, ctx - 2], v2[:, :, ctx - 1] = v[:, :, ctx - 1], v[:, :, ctx - 2]
    out["V rows of two adjacent keys swapped"] = (keyok[:, None, None, :], v2)
    return out


@pytest.mark.parametrize("B,H,Hk,Tmax,ctx", [(3, 8, 2, 960, 960), (3, 8, 2, 960, 300), (256, 7, 1, 576, 513)])
def test_decode_attention_verdict(B, H, Hk, Tmax, ctx):
    """attn_decode_kernel<128> at a full and a part-filled 960-row cache, and the grouped-query kernel (B Hk = 256, G = 7) past its 512-key chunk."""
    from crab_amd import ops
    d = 128
    g = torch.Generator(device="cuda").manual_seed(ctx + B)
    kc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.7).to(BF)
    vc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.7).to(BF)
    q = (torch.randn(B, H * d, device="cuda", generator=g) * 0.7).to(BF)
    o = torch.empty(B, H * d, device="cuda", dtype=BF)
    ops.attn_decode(q, kc, vc, o, B, H, Hk, d, Tmax, ctx, d ** -0.5)
    keyok = torch.zeros(B, Tmax, device="cuda", dtype=torch.bool); keyok[:, :ctx] = True
    case = (q.view(B, H, 1, d), kc, vc, d ** -0.5, keyok[:, None, None, :])
    _judge(f"decode B={B} H={H} Hk={Hk} ctx={ctx}", o.view(B, H, 1, d), case, "decode", _decode_defects(keyok, vc, ctx, Tmax))


@pytest.mark.parametrize("B,H,Hk,d,Sq,Skv,with_ks", [(1, 4, 2, 128, 300, 300, False), (2, 4, 2, 64, 97, 200, True)])
def test_forward_attention_verdict(B, H, Hk, d, Sq, Skv, with_ks):
    """crab_attn_fwd, causal: the 128-row kernel over three row blocks, and a rectangular head_dim 64 case under a left-pad kv_start."""
    from crab_amd import ops
    g = torch.Generator(device="cuda").manual_seed(Sq)
    q = (torch.randn(B, Sq, H, d, device="cuda", generator=g) * 0.7).to(BF)
    k = (torch.randn(B, Hk, Skv, d, device="cuda", generator=g) * 0.7).to(BF)
    v = (torch.randn(B, Hk, Skv, d, device="cuda", generator=g) * 0.7).to(BF)
    Sp = (Skv + 7) // 8 * 8
    vt = torch.zeros(B, Hk, d, Sp, device="cuda", dtype=BF); vt[..., :Skv] = v.transpose(2, 3)
    o = torch.empty(B, Sq, H * d, device="cuda", dtype=BF)
    kw, start = {}, torch.zeros(B, dtype=torch.long, device="cuda")
    if with_ks:
        start = torch.tensor([5, 60][:B], device="cuda")
        kw["kv_start"] = start.to(torch.int32)
    ops.attn_fwd(q, k, vt, o, q_strides=(Sq * H * d, d, H * d), k_strides=(Hk * Skv * d, Skv * d, d), vt_strides=(Hk * d * Sp, d * Sp, Sp),
                 o_strides=(Sq * H * d, H * d), B=B, H=H, Hk=Hk, Sq=Sq, Skv=Skv, head_dim=d, scale=d ** -0.5, causal=True, **kw)
    ar = torch.arange(Skv, device="cuda")
    causal = ar[None, :] <= torch.arange(Sq, device="cuda")[:, None] + (Skv - Sq)                       # [Sq, Skv]
    shift = lambda n: ar[None, :] <= torch.arange(Sq, device="cuda")[:, None] + (Skv - Sq) + n
    vis = lambda st, c: ((ar[None] >= st[:, None])[:, None, None, :] & c[None, None]).expand(B, H, Sq, Skv)
    allow = vis(start, causal)
    future = causal.clone(); future[128:] = shift(1)[128:]
    defects = {"newest key dropped": (vis(start, shift(-1)), v),
               "first visible key dropped (kv_start off by one)": (vis(start + 1, causal), v),
               "one future key seen on the causal rows >= 128": (vis(start, future), v)}
    v2 = v.clone(); v2[:, :, Skv - 2], v2[:, :, Skv - 1] = v[:, :, Skv - 1], v[:, :, Skv - 2]
    defects["V rows of two adjacent keys swapped"] = (allow, v2)
    if Sq <= 128: del defects["one future key seen on the causal rows >= 128"]
    _judge(f"fwd Sq={Sq} Skv={Skv} d={d}", o.view(B, Sq, H, d).permute(0, 2, 1, 3), (q.permute(0, 2, 1, 3), k, v, d ** -0.5, allow), "fwd", defects)


@pytest.mark.parametrize("M", [8, 300])
def test_fused_post_norm_and_router_verdict(M):
    """ops.gemm with the fused post-RMSNorm and next-group router, bf16 stream: C and h pass their bounds (h: x_hat rounded before the weight); u
    lies within ONE of the router's two forms - mixed from the stored h (split-K reduction, unfused pair) or from the normalised row before its
    store (the M <= 16 tail) - and within neither once two route logits are swapped in the reference."""
    from crab_amd import ops
    N, K = 1024, 256
    g = torch.Generator(device="cuda").manual_seed(M)
    x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF)
    r = torch.randn(M, N, device="cuda", generator=g).to(BF)
    nw = (1.0 + 0.1 * torch.randn(N, device="cuda", generator=g)).to(BF)
    ra = (torch.randn(48, N, device="cuda", generator=g) * 0.05).to(BF)
    out, h, u = (torch.empty(M, n, device="cuda", dtype=BF) for n in (N, N, 96))
    ops.gemm(x, w, residual=r, out=out, post_norm=(nw, 1e-5, h), route=(ra, 3, 3, 8, 96, 2.0, u))
    assert FB.worst(out, *FB.gemm_bound(x, w, residual=r, out_bf16=True))[0] <= 1.0
    assert FB.worst(h, *FB.rmsnorm_bound(out, nw, 1e-5, round_xhat=True))[0] <= 1.0
    hx = FB.rmsnorm_bound(out, nw, 1e-5, round_xhat=False)[0]

    def forms(ra_):
        return [FB.route_bound(h, ra_, 3, 3, 8, 96, 2.0), FB.route_bound(hx, ra_, 3, 3, 8, 96, 2.0, x_rel=FB.rx_rel(N) + 2 * FB.U32)]

    ratios = [FB.worst(u, *f)[0] for f in forms(ra)]
    print(f"router M={M}: err / bound {ratios[0]:.3f} from the stored h, {ratios[1]:.3f} from the unrounded row")
    assert min(ratios) <= 1.0, ratios
    ra2 = ra.clone(); ra2[0], ra2[1] = ra[1], ra[0]
    assert min(FB.worst(u, *f)[0] for f in forms(ra2)) > 1.0


@pytest.mark.parametrize("M,N,K,K2", [(300, 1009, 1096, 32), (16, 1000, 200, 32)])
def test_gemm_fp32_verdict(M, N, K, K2):
    """ops.gemm, fp32 output on an fp32 residual, ragged in M, N and K: passes against the fp64 product; fails against it with the accumulator
    rounded to bf16, the residual read as bf16, the bias of the last ragged 16-column tile dropped, the last 8 columns of the K2 segment dropped."""
    from crab_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M)
    x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF)
    x2 = (torch.randn(M, K2, device="cuda", generator=g) * 0.5).to(BF)
    w2 = (torch.randn(N, K2, device="cuda", generator=g) * 0.1).to(BF)
    b = (torch.randn(N, device="cuda", generator=g) * 0.1).to(BF)
    ld = (N + 3) // 4 * 4                                                   # an fp32 residual needs 16-byte aligned rows
    r = torch.randn(M, ld, device="cuda", generator=g)[:, :N]
    out = torch.empty(M, ld, device="cuda")[:, :N]
    ops.gemm(x, w, bias=b, residual=r, x2=x2, w2=w2, out=out)
    y, bound = FB.gemm_bound(x, w, x2, w2, b, "none", r)
    ratio, idx = FB.worst(out, y, bound)
    print(f"gemm {M}x{N}x{K}+{K2}: worst err / bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, (ratio, idx)
    b2 = b.clone(); b2[N - N % 16:] = 0
    x2s = x2.clone(); x2s[:, -8:] = 0
    acc = FB.bf16_round(FB.gemm_ref(x, w, x2, w2)) + b.double() + r.double()
    defects = {"accumulator rounded to bf16 before the epilogue": (acc, bound),
               "fp32 residual read as bf16": FB.gemm_bound(x, w, x2, w2, b, "none", r.to(BF)),
               "bias dropped on the last ragged 16-column tile": FB.gemm_bound(x, w, x2, w2, b2, "none", r),
               "the last 8 columns of the K2 segment dropped": FB.gemm_bound(x, w, x2s, w2, b, "none", r)}
    for name, (yd, bd) in defects.items():
        rd = FB.worst(out, yd, bd)[0]
        print(f"    {name}: {rd:.1f}")
        assert rd > 1.0, f"the verdict would pass a kernel with this defect: {name} ({rd:.3f})"
