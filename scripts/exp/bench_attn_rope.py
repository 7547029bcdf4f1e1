"""attn_decode_rope_kernel alone at the small-batch sizes (1 clip: 8 context splits; 8 clips: the 512-thread form), H = Hk = 32, d = 128.
usage: bench_attn_rope.py [ctx] [iters]  -> us per launch, three rounds per size.  Run once per CRAB_HIP_LIB build to compare two builds."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from crab_amd import ops
ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 830
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
H = Hk = 32; d = 128; Tmax = 960
tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
g = torch.Generator(device="cuda").manual_seed(1)
for B in (1, 8):
    kc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.5).bfloat16()
    vc = (torch.randn(B, Hk, Tmax, d, device="cuda", generator=g) * 0.5).bfloat16()
    qkv = torch.randn(B, (H + 2 * Hk) * d, device="cuda", generator=g).bfloat16()
    o = torch.empty(B, H * d, device="cuda", dtype=torch.bfloat16)
    ws = ops.attn_decode_rope_workspace(B, H, d, "cuda")
    fn = lambda: ops.attn_decode_rope(qkv, tab, kc, vc, o, B, H, Hk, d, Tmax, ctx - 1, d ** -0.5, workspace=ws)
    rounds = []
    for _ in range(3):
        for _ in range(10): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / iters * 1e3)
    print(f"attn_decode_rope B={B} ctx={ctx}: us/launch per round {' '.join(f'{t:.2f}' for t in rounds)}", flush=True)
