"""Differential fuzz of crab_gemm_bf16 across its kernel regimes (rowfin / skinny M <= 16, 128^2 LDS-DMA, 256^2 ring, split-K, panel kernels for
128 < M <= 512) and epilogues (bias, activations, SwiGLU pairs, bf16 / fp32 residual, fp32 output, K extension, fused post-RMSNorm + next-group
router): random shapes around every dispatch boundary against an fp64 product of the same bf16 operands (on the GPU), every output element held to the
derived bound of tests/fuzz_bounds.py (one bf16 rounding at the store + the fp32 level of the fixed-shape tests + the any-order ceiling; no constant here).
A combination the library rejects must be
rejected with CRAB_E_UNSUPPORTED / CRAB_E_INVALID (counted), never computed wrong.   python scripts/fuzz_gemm.py [cases] [seed]"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crab_amd import ops, _lib
from tests import fuzz_bounds as FB

BF = torch.bfloat16
NCASE = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
Ms = [1, 2, 3, 8, 15, 16, 17, 33, 64, 65, 100, 128, 129, 200, 255, 256, 257, 300, 448, 511, 512, 513, 700, 1024, 2050]
Ns = [8, 16, 64, 96, 104, 128, 200, 256, 384, 1000, 1024, 2048, 4096, 4104, 11008]
Ks = [8, 32, 64, 72, 128, 256, 1000, 1024, 4096]
K2s = [0, 0, 8, 32, 64, 96]
ACTS = ["none", "none", "gelu", "quick_gelu", "relu", "silu", "swiglu_pair"]


run = FB.Run()
bad, rejected, done, why = [], 0, 0, {}
for case in range(NCASE):
    M, N, K, K2, act = rng.choice(Ms), rng.choice(Ns), rng.choice(Ks), rng.choice(K2s), rng.choice(ACTS)
    if M * N * K > 2050 * 4104 * 4096: continue
    bias = rng.random() < 0.5
    res = rng.choice([None, None, "bf16", "fp32"])
    out32 = (res == "fp32") or rng.random() < 0.2
    norm = M <= 512 and act != "swiglu_pair" and N <= 8192 and N % 8 == 0 and rng.random() < 0.3
    route = norm and rng.random() < 0.5
    g = torch.Generator(device="cuda").manual_seed(case)
    x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) * (1.0 / K ** 0.5)).to(BF)
    x2 = (torch.randn(M, K2, device="cuda", generator=g) * 0.5).to(BF) if K2 else None
    w2 = (torch.randn(N, K2, device="cuda", generator=g) * 0.1).to(BF) if K2 else None
    b = (torch.randn(N, device="cuda", generator=g) * 0.1).to(BF) if bias else None
    No = N // 2 if act == "swiglu_pair" else N
    r = None
    if res:
        r = torch.randn(M, No, device="cuda", generator=g)
        r = r if res == "fp32" else r.to(BF)
    # the output sits inside a larger buffer of sentinels: a guard row above and below, and (half of the cases) 8 / 16 guard columns behind every
    # row - a store outside the M x N block shows up as a changed sentinel
    gap = rng.choice([0, 0, 8, 16])
    obuf = torch.full((M + 2, No + gap), 777.0, device="cuda", dtype=torch.float32 if out32 else BF)
    out = obuf[1:M + 1, :No]
    y, ybound = FB.gemm_bound(x, w, x2, w2, b, act, r, out_bf16=not out32)
    kw = {}
    if norm:
        nw = (1.0 + 0.1 * torch.randn(N, device="cuda", generator=g)).to(BF)
        hbuf = torch.full((M + 2, N + gap), 777.0, device="cuda", dtype=BF)
        h = hbuf[1:M + 1, :N]
        kw["post_norm"] = (nw, 1e-5, h)
        if route:
            ra = (torch.randn(48, N, device="cuda", generator=g) * 0.05).to(BF)
            ubuf = torch.full((M + 2, 96 + 8), 777.0, device="cuda", dtype=BF)
            u = ubuf[1:M + 1, :96]
            kw["route"] = (ra, 3, 3, 8, 96, 2.0, u)
    desc = f"case {case}: M={M} N={N} K={K}+{K2} act={act} bias={bias} res={res} out={'fp32' if out32 else 'bf16'} norm={norm} route={route}"
    try:
        ops.gemm(x, w, bias=b, act=act, residual=r, x2=x2, w2=w2, out=out, **kw)
        torch.cuda.synchronize()
    except _lib.CrabHipError as e:
        msg = str(e)
        if "error -1:" in msg or "error -3:" in msg:              # CRAB_E_INVALID / CRAB_E_UNSUPPORTED: a stated limit, not a wrong answer
            rejected += 1
            why[msg.split(":", 2)[-1].strip()[:90]] = why.get(msg.split(":", 2)[-1].strip()[:90], 0) + 1
            continue
        bad.append(desc + " -> " + msg[:200]); continue
    done += 1
    guards = [("out", obuf, No)] + ([("post-norm out", hbuf, N)] if norm else []) + ([("router out", ubuf, 96)] if route else [])
    for gname, gb, cols in guards:
        if not (bool((gb[0] == 777.0).all()) and bool((gb[-1] == 777.0).all()) and bool((gb[:, cols:] == 777.0).all())):
            bad.append(desc + f" gap={gap} -> {gname}: a store landed outside the M x N block")
    run.judge(bad, desc, "out", out, y, ybound)
    if norm:
        hh, hbound = FB.rmsnorm_bound(out, nw, kw["post_norm"][1], round_xhat=not out32)     # from the stored C, as the kernel's norm sees it
        run.judge(bad, desc, "post-norm", h, hh, hbound)
        if route:
            # from the stored h - or, the M <= 16 tail's form, from the normalised row before its store rounding (tests/fuzz_bounds.py, Router)
            hx = FB.rmsnorm_bound(out, nw, kw["post_norm"][1], round_xhat=False)[0]
            forms = [FB.route_bound(h, ra, 3, 3, 8, 96, 2.0), FB.route_bound(hx, ra, 3, 3, 8, 96, 2.0, x_rel=FB.rx_rel(N) + 2 * FB.U32)]
            run.judge_any(bad, desc, "router", u, forms)
for k_, v_ in sorted(why.items(), key=lambda kv: -kv[1]): print(f"  rejected x{v_}: {k_}")
for b_ in bad[:40]: print("FAIL", b_)
print(f"{done} cases computed, {rejected} rejected by the library, {len(bad)} failures; {run}")
sys.exit(1 if bad else 0)
