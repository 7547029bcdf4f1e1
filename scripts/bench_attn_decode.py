"""Decode-attention micro-benchmark at the bench.py shape (GPU box): B clips x 32 heads x d 128, one layer's KV cache.
usage: bench_attn_decode.py [B] [ctx] [iters] [H] [Hk] [fp8]  -> us per launch and algorithmic GB/s (K and V rows read once).
A trailing `fp8`: the same shapes and seed with the cache quantised by ops.kv_quant_fp8 and ops.attn_decode_fp8 timed the same way (bytes = codes +
scales + q + o); both kernels then run ALTERNATELY in this process (three rounds of `iters` launches each) and both lines and the ratio are printed."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crab_amd import ops
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ctx = int(sys.argv[2]) if len(sys.argv) > 2 else 830
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
H = int(sys.argv[4]) if len(sys.argv) > 4 else 32
Hk = int(sys.argv[5]) if len(sys.argv) > 5 else H
d = 128; Tmax = 960
g = torch.Generator(device="cuda").manual_seed(1)
kc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.5).bfloat16()
vc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.5).bfloat16()
q = torch.randn(B, H * d, device="cuda", generator=g).bfloat16()
o = torch.empty_like(q)
fn = lambda: ops.attn_decode(q, kc, vc, o, B, H, Hk, d, Tmax, ctx, d ** -0.5)
def timed(f):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
nbytes = 2.0 * B * ctx * Hk * d * 2 + 2.0 * B * H * d * 2
if not (len(sys.argv) > 6 and sys.argv[6] == "fp8"):
    us = timed(fn)
    print(f"attn_decode B={B} ctx={ctx} H={H} Hk={Hk}: {us:.1f} us/launch, algorithmic {nbytes/1e9:.3f} GB -> {nbytes/us/1e3:.0f} GB/s", flush=True)
    sys.exit(0)
# ---- fp8 KV cache: the same rows as codes + row scales; the step appends at slot ctx - 1 and attends ctx keys (the new one included)
k8 = torch.empty(1, B, Hk, Tmax, d, device="cuda", dtype=torch.uint8); v8 = torch.empty_like(k8)
ks = torch.empty(1, B, Hk, Tmax, device="cuda", dtype=torch.float32); vs = torch.empty_like(ks)
ops.kv_quant_fp8(kc[None], vc[None], k8, v8, ks, vs)
qkv = torch.randn(B, (H + 2 * Hk) * d, device="cuda", generator=g).bfloat16()
tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
o8 = torch.empty_like(o)
fn8 = lambda: ops.attn_decode_fp8(qkv, tab, k8[0], v8[0], ks[0], vs[0], o8, B, H, Hk, d, Tmax, ctx - 1, d ** -0.5)
nbytes8 = 2.0 * B * ctx * Hk * (d + 4) + 2.0 * B * H * d * 2
t16, t8 = [], []
for _ in range(3):
    t16.append(timed(fn)); t8.append(timed(fn8))
u16, u8 = sorted(t16)[1], sorted(t8)[1]
print(f"attn_decode     B={B} ctx={ctx} H={H} Hk={Hk}: {u16:.1f} us/launch (rounds {' '.join(f'{t:.1f}' for t in t16)}), algorithmic {nbytes/1e9:.3f} GB -> {nbytes/u16/1e3:.0f} GB/s", flush=True)
print(f"attn_decode_fp8 B={B} ctx={ctx} H={H} Hk={Hk}: {u8:.1f} us/launch (rounds {' '.join(f'{t:.1f}' for t in t8)}), algorithmic {nbytes8/1e9:.3f} GB -> {nbytes8/u8/1e3:.0f} GB/s", flush=True)
print(f"fp8 / bf16 time {u8/u16:.3f} (bytes {nbytes8/nbytes:.3f})", flush=True)
