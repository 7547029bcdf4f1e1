"""Fuzz of the RoPE / KV-append fusions of the q|k|v projection against the unfused pair they replace - BIT-identical by construction:
  prefill: crab_gemm_desc.rope_S (q and k rotated, k / v / V^T written by the 256 x 256 ring kernel's epilogue) vs GEMM + qkv_rope_split,
  decode:  one row per sequence, fused into the small-batch kernel's epilogue (M <= 16) or the split-K reduction (M <= 512) vs GEMM + split(S = 1),
over random batch sizes, sequence lengths (ragged row tiles, several sequences per tile), head counts / grouped kv heads, bias, explicit rotary
positions, cache offsets.  Beyond 256 decode rows the two forms may slice K differently: there they may differ only where the exact sum lies within
the GEMM's fp32 ceiling of a bf16 rounding boundary, by what that one flip becomes (tests/fuzz_bounds.py: rope_pair_bound), bit for bit elsewhere.
python scripts/fuzz_rope_epilogue.py [cases] [seed]"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crab_amd import ops
from tests import fuzz_bounds as FB

BF = torch.bfloat16
NCASE = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad, fused_n, declined, pre_fused = [], 0, 0, 0
run = FB.Run()
for case in range(NCASE):
    g = torch.Generator(device="cuda").manual_seed(case)
    prefill = rng.random() < 0.5
    Hk = rng.choice([1, 2, 4, 8])
    H = Hk * rng.choice([1, 1, 2, 4, 7])
    if H > 32: continue
    bias = rng.random() < 0.4
    if prefill:
        # the ring kernel (and with it the fused epilogue) takes shapes whose 256 x 256 tiles fill most of a round of 256 CUs at K >= 1024:
        # mostly such shapes, some the library declines (it then answers 0 and the caller runs the split pass)
        d, K = 128, rng.choice([256, 1024, 1024, 1024])
        if rng.random() < 0.7:
            Hk = rng.choice([4, 8, 16, 32]); H = Hk * rng.choice([1, 1, 2, 7])
            if H > 32: H = Hk
        B, S = rng.choice([1, 2, 3, 5]), rng.choice([1, 17, 100, 255, 256, 257, 300, 511, 702, 1000, 1000])
        if B * S * (H + 2 * Hk) * d > 160e6: continue
        Tmax = (S + 64 + 63) // 64 * 64
        pos0 = rng.randrange(0, Tmax - S + 1)
        ids = rng.random() < 0.3
        with_vt = rng.random() < 0.7
        M, N = B * S, (H + 2 * Hk) * d
        x = torch.randn(M, K, device="cuda", generator=g).to(BF)
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF)
        bv = torch.randn(N, device="cuda", generator=g).to(BF) if bias else None
        tab = ops.rope_table(4096, d, 10000.0, "cuda")
        pid = torch.randint(0, 4000, (B, S), device="cuda", generator=g).to(torch.int32) if ids else None
        Sp = (S + 7) // 8 * 8 + 8 * rng.randrange(0, 2)
        desc = f"case {case}: prefill B={B} S={S} H={H}/{Hk} K={K} bias={bias} ids={ids} vt={with_vt} pos0={pos0} vt_ld={Sp}"
        outs = []
        lvl = None
        for fused in (True, False):
            kc = torch.zeros(B, Hk, Tmax, d, dtype=BF, device="cuda"); vc = torch.zeros_like(kc)
            vt = torch.zeros(B, Hk, d, Sp, dtype=BF, device="cuda")
            qkv = torch.empty(M, N, dtype=BF, device="cuda")
            if fused:
                info = {}
                ops.gemm(x, w, bias=bv, out=qkv, rope=(tab, kc, vc, H, Hk, d, Tmax, pos0, None, S, pid, vt if with_vt else None), info=info)
                lvl = info["fused_prefill_rope"]
                if lvl == 0: ops.qkv_rope_split(qkv, tab, kc, vc, vt, B, S, H, Hk, d, Tmax, pos0=pos0, pos_ids=pid)
                elif lvl == 1: ops.qkv_rope_split(qkv, None, None, vc, vt, B, S, H, Hk, d, Tmax, pos0=pos0)
            else:
                ops.gemm(x, w, bias=bv, out=qkv)
                ops.qkv_rope_split(qkv, tab, kc, vc, vt, B, S, H, Hk, d, Tmax, pos0=pos0, pos_ids=pid)
            outs.append((qkv[:, :H * d].clone(), kc, vc, vt[..., :S].clone()))
        fused_n += lvl > 0; declined += lvl == 0; pre_fused += lvl > 0
        for name, a, b in zip(("q", "k cache", "v cache", "v^T"), outs[0], outs[1]):
            if not torch.equal(a, b): bad.append(desc + f" (fused level {lvl}) -> {name} differs")
    else:
        d = rng.choice([64, 128])
        M = rng.choice([1, 2, 7, 16, 17, 40, 128, 129, 256, 257, 300, 448, 512])
        K, Tmax, K2 = rng.choice([256, 1024]), 64, rng.choice([0, 32])
        N = (H + 2 * Hk) * d
        x = torch.randn(M, K, device="cuda", generator=g).to(BF)
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF)
        x2 = torch.randn(M, K2, device="cuda", generator=g).to(BF) if K2 else None
        w2 = (torch.randn(N, K2, device="cuda", generator=g) * 0.1).to(BF) if K2 else None
        bv = torch.randn(N, device="cuda", generator=g).to(BF) if bias else None
        tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
        p = rng.randrange(0, Tmax)
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        desc = f"case {case}: decode M={M} H={H}/{Hk} d={d} K={K}+{K2} bias={bias} pos={p}"
        outs = []
        for fused in (False, True):
            kc = torch.zeros(M, Hk, Tmax, d, dtype=BF, device="cuda"); vc = torch.zeros_like(kc)
            y = ops.gemm(x, w, bias=bv, x2=x2, w2=w2, rope=(tab, kc, vc, H, Hk, d, Tmax, 0, pos) if fused else None)
            if not fused: ops.qkv_rope_split(y, tab, kc, vc, None, M, 1, H, Hk, d, Tmax, pos0=0, pos_dev=pos)
            outs.append((y[:, :H * d].clone(), kc, vc))
        fused_n += 1
        if M > 256:
            # beyond 256 rows the two-row-group kernel picks its K slices with the fused reduction priced in (dec2_choose): the two forms may
            # sum in a different order.  Both lie within the GEMM's any-order ceiling of the exact sum, so they may differ only where that
            # interval straddles a bf16 rounding boundary, by what one such flip becomes through the rotation and the second rounding
            # (tests/fuzz_bounds.py: rope_pair_bound); everywhere else, and in every other cache slot, bit for bit
            y64, ceil = FB.gemm_ceiling(x, w, x2, w2, bv)
            cs, sn = tab[p, :, 0], tab[p, :, 1]
            one, zero = torch.ones_like(cs), torch.zeros_like(cs)
            cols = ((0, H, cs, sn), (H, Hk, cs, sn), (H + Hk, Hk, one, zero))
        for i, name in enumerate(("q", "k cache", "v cache")):
            a, b = outs[0][i], outs[1][i]
            if M <= 256:
                if not torch.equal(a, b): bad.append(desc + f" -> {name} differs")
            else:
                h0, nh, c_, s_ = cols[i]
                bound = FB.rope_pair_bound(y64[:, h0 * d:(h0 + nh) * d].view(M, nh, d), ceil[:, h0 * d:(h0 + nh) * d].view(M, nh, d), c_, s_)
                if i > 0:                                                  # a cache: only slot p was written
                    if not torch.equal(a.index_fill(2, pos.long(), 0), b.index_fill(2, pos.long(), 0)): bad.append(desc + f" -> {name} differs outside slot {p}")
                    a, b = a[:, :, p], b[:, :, p]
                run.judge(bad, desc, name, a.reshape(M, nh, d), b.reshape(M, nh, d).double(), bound)
        if float(outs[1][1][:, :, p].float().abs().sum()) == 0: bad.append(desc + " -> nothing appended")
for b_ in bad[:30]: print("FAIL", b_)
print(f"{fused_n} fused cases ({pre_fused} of them prefill) against the unfused pair (bit-identical; decode rows > 256: one derived rounding flip), {declined} prefill shapes the library runs unfused, {len(bad)} failures; rows > 256: {run}")
sys.exit(1 if bad else 0)
