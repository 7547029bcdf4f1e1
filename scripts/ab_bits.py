"""Bit-compare two builds of libcrab_hip.so on the decode GEMMs (csrc/skinny.hip and the split-K reduction of csrc/gemm.hip).

    python scripts/ab_bits.py <a.so> <b.so>

One fresh child process per library (CRAB_HIP_LIB, crab_amd/_lib.py) runs the launch list below on seeded inputs and saves every output
tensor; the parent compares the two sets with torch.equal and prints the first case that differs.  Exit status 0: every case identical."""
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SHAPES = [(48, 64, 0), (100, 8, 0), (1000, 200, 32), (176, 4096, 96)]      # (N, K, K2): idle waves | ragged N, K < one slot | K % 16 == 8 | deep ring


def _rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF).cuda()


def _cases():
    """Yields (name, tensors).  A refused call is a case too: both libraries must refuse it with the same message."""
    from crab_amd import ops
    from crab_amd._lib import CrabHipError

    def run(name, fn):
        try:
            out = fn()
        except CrabHipError as e:
            out = torch.tensor(list(str(e).encode()), dtype=torch.uint8)
        torch.cuda.synchronize()
        return name, [t.cpu() for t in (out if isinstance(out, (list, tuple)) else [out])]

    def operands(M, N, K, K2):
        o = dict(x=_rand(M, K, seed=1), w=_rand(N, K, seed=2, scale=K ** -0.5), bias=_rand(N, seed=3), res=_rand(M, N, seed=4))
        o["seg2"] = dict(x2=_rand(M, K2, seed=5), w2=_rand(N, K2, seed=6, scale=0.1)) if K2 else {}
        return o

    for M in (1, 5, 16):
        for N, K, K2 in SHAPES:
            o = operands(M, N, K, K2)
            x, w, seg2 = o["x"], o["w"], o["seg2"]
            for wt in ("bf16", "fp8"):
                kw = {"w8": ops.weight_quant_fp8(w)} if wt == "fp8" else {}
                tag = f"{wt} M={M} N={N} K={K}+{K2}"
                yield run(f"{tag} bf16 out", lambda: ops.gemm(x, w, **seg2, **kw))
                yield run(f"{tag} fp32 out", lambda: ops.gemm(x, w, out_fp32=True, **seg2, **kw))
                yield run(f"{tag} bias+silu+residual", lambda: ops.gemm(x, w, bias=o["bias"], act="silu", residual=o["res"], res_scale=0.5, **seg2, **kw))
                yield run(f"{tag} swiglu_pair", lambda: ops.gemm(x, w, bias=o["bias"], act="swiglu_pair", **seg2, **kw))
                # the post-norm route (tests/test_w8_gpu.py:_norm_case): raw fp32 sums + the router rows riding on the launch, then the row-owning tail
                nl, r = 3, 8
                RA = torch.zeros(16, K, dtype=BF, device="cuda")
                RA[:nl + r] = _rand(nl + r, K, seed=7, scale=K ** -0.5)
                B2 = torch.zeros(N, 32, dtype=BF, device="cuda")
                B2[:, :nl * r] = _rand(N, nl * r, seed=8, scale=0.2)
                nw = _rand(N, seed=9, scale=0.1) + 1
                for rdt in (torch.float32, BF):
                    for lora in ({"lora_self": (RA, nl, r, 2.0, B2)}, {}):
                        def route():
                            c, h = o["res"].to(rdt), torch.zeros(M, N, dtype=BF, device="cuda")
                            ops.gemm(x, w, bias=o["bias"], residual=c, out=c, post_norm=(nw, 1e-5, h), **lora, **kw)
                            return c, h
                        yield run(f"{tag} post-norm route res={rdt} lora={bool(lora)}", route)
        # fused RoPE + KV append: N = (H + 2 Hk) d
        H, Hk, Tmax, pos = 4, 2, 32, 9
        for d in (64, 128):
            for _, K, K2 in SHAPES:
                o = operands(M, (H + 2 * Hk) * d, K, K2)
                tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
                pd = torch.tensor([pos - 2], dtype=torch.int32, device="cuda")
                for wt in ("bf16", "fp8"):
                    kw = {"w8": ops.weight_quant_fp8(o["w"])} if wt == "fp8" else {}
                    for off in (None, torch.tensor([(3 * m) % (pos + 1) for m in range(M)], dtype=torch.int32, device="cuda")):
                        def rope():
                            kc = torch.full((M, Hk, Tmax, d), 777.0, dtype=BF, device="cuda")
                            vc = kc.clone()
                            y = ops.gemm(o["x"], o["w"], bias=o["bias"], rope=(tab, kc, vc, H, Hk, d, Tmax, 2, pd), rope_row_off=off, **o["seg2"], **kw)
                            return y, kc, vc
                        yield run(f"{wt} M={M} K={K}+{K2} rope d={d} ragged={off is not None}", rope)
    # bf16 only: the register-direct kernel (tune 1 / 2: forced, whatever the workspace says) and the split-K reduction
    for M, tunes in ((17, (0, 1)), (33, (0, 1, 2)), (64, (0, 1, 2, 104)), (128, (0, 1, 2))):
        o = operands(M, 1009, 1096, 32)
        p = operands(M, 1000, 1096, 32)
        for tune in tunes:
            for f32 in (False, True):
                yield run(f"bf16 M={M} tune={tune} fp32={f32} bias+gelu+residual",
                          lambda: ops.gemm(o["x"], o["w"], bias=o["bias"], act="gelu", residual=o["res"], out_fp32=f32, tune=tune, **o["seg2"]))
                yield run(f"bf16 M={M} tune={tune} fp32={f32} swiglu_pair",
                          lambda: ops.gemm(p["x"], p["w"], bias=p["bias"], act="swiglu_pair", out_fp32=f32, tune=tune, **p["seg2"]))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        torch.save(dict(_cases()), sys.argv[2])
        return 0
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    sets = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:]):
            out = os.path.join(tmp, f"{i}.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=dict(os.environ, CRAB_HIP_LIB=os.path.abspath(lib)))
            sets.append(torch.load(out))
    a, b = sets
    assert list(a) == list(b) and len(a) > 0
    refused = [n for n in a if a[n][0].dtype == torch.uint8]
    for name in a:
        if len(a[name]) != len(b[name]) or not all(torch.equal(s, t) for s, t in zip(a[name], b[name])):
            print(f"DIFFERENT: {name}")
            for s, t in zip(a[name], b[name]):
                if s.shape == t.shape and not torch.equal(s, t):
                    i = (s != t).nonzero()[0].tolist()
                    print(f"  first at {i}: {s[tuple(i)].item()} vs {t[tuple(i)].item()} ({(s != t).sum().item()} of {s.numel()} elements)")
            return 1
    print(f"all {len(a)} cases identical ({sum(len(v) for v in a.values())} tensors; {len(refused)} calls refused by both libraries alike)")
    for msg in sorted({bytes(a[n][0].tolist()).decode() for n in refused}):
        print(f"  refused: {msg[:160]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
