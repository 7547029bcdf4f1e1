"""Bit-compare two builds of libcrab_hip.so on the decode GEMMs (csrc/skinny.hip and the split-K reduction of csrc/gemm.hip) and on the decode
attention kernels (csrc/attn_decode_core.h and its users in attn.hip, attn_prefix.hip, kv_fp8.hip; csrc/attn_rows_core.h and its users in
attn_prefix.hip, attn_verify.hip), and - the list `select`, on request - on the sampling selects (csrc/select_core.h: sample.hip, constrain.hip).

    python scripts/ab_bits.py <a.so> <b.so> [gemm | attn | select]

One fresh child process per library (CRAB_HIP_LIB, crab_amd/_lib.py) runs the launch lists below (gemm and attn, or the one named) on seeded
inputs and saves every output tensor; the parent compares the two sets with torch.equal and prints every case that differs.  Exit status 0:
every case identical.  The attention cases are one or two launches each (edge cases), followed by "volume" cases of 128 x 32 rows per
launch: the kernels write a * b + c * d, which product gets fused is the compiler's choice per build, and the last fp32 bit this moves reaches
about one bf16 output in 10^4 - the edge cases alone pass such a build.  Cache rows outside the visible range hold NaN, and outputs are
compared as bit patterns (a NaN that reaches an output must be the same NaN)."""
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


KEYS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65, 97)                      # visible keys per row: the 16-key group and 32-key prefetch edges
NAN = float("nan")


def _bits(t):
    return t.view({BF: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype)).cpu()


def _attn_cases():
    """Yields (name, tensors) for the one-query-per-row decode attention kernels, with the grouped (MFMA) kernels of the same files as controls."""
    from crab_amd import ops

    def run(name, fn):
        out = fn()
        torch.cuda.synchronize()
        return "attn " + name, [_bits(t) for t in (out if isinstance(out, (list, tuple)) else [out])]

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device="cuda")

    base = {}

    def cache(B, Hk, Tmax, d, lo, hi, seed):
        """K / V with random rows lo[b] .. hi - 1 and NaN everywhere else."""
        key = (B, Hk, Tmax, d, seed)
        if key not in base:
            base.clear()                                                        # one shape at a time: the largest is 40 MB per tensor
            base[key] = _rand(B, Hk, Tmax, d, seed=seed, scale=0.5), _rand(B, Hk, Tmax, d, seed=seed + 1)
        kc, vc = base[key]
        t = torch.arange(Tmax, device="cuda")[None, :]
        dead = ((t < i32(lo)[:, None]) | (t >= hi))[:, None, :, None]
        return kc.masked_fill(dead, NAN), vc.masked_fill(dead, NAN)

    for d in (64, 128):
        sc = d ** -0.5
        # ---- attn_decode_kernel: a device ctx word, the key counts through kv_start; the same rows without kv_start
        H, B, Tmax, ctx = 2, len(KEYS), 104, 97
        q = _rand(B, H * d, seed=10 + d)
        word = i32([ctx - 5])
        for name, lo in (("kv_start", [ctx - n for n in KEYS]), ("no kv_start", [0] * B)):
            kc, vc = cache(B, H, Tmax, d, lo, ctx, seed=20)
            ks = i32(lo) if name == "kv_start" else None
            yield run(f"decode d={d} {name}", lambda: ops.attn_decode(q, kc, vc, torch.zeros_like(q), B, H, H, d, Tmax, 5, sc, ctx_dev=word, kv_start=ks))
        # ---- attn_decode_keymask_kernel: a random mask over the 97 rows (the hidden rows poisoned too), row 3 fully masked
        vis = torch.rand(B, ctx, generator=torch.Generator().manual_seed(30)).cuda() < 0.6
        vis[3] = False
        kc, vc = cache(B, H, Tmax, d, [0] * B, ctx, seed=20)
        hide = ~torch.nn.functional.pad(vis, (0, Tmax - ctx))[:, None, :, None]
        kc, vc = kc.masked_fill(hide, NAN), vc.masked_fill(hide, NAN)
        km = ops.pack_key_mask(torch.nn.functional.pad(vis, (0, Tmax - ctx)))
        yield run(f"keymask d={d} host ctx", lambda: ops.attn_decode(q, kc, vc, torch.zeros_like(q), B, H, H, d, Tmax, ctx, sc, key_mask=km))
        yield run(f"keymask d={d} device ctx", lambda: ops.attn_decode(q, kc, vc, torch.zeros_like(q), B, H, H, d, Tmax, 5, sc, ctx_dev=word, key_mask=km))
        # ---- attn_decode_rope_kernel: 8 splits | 2 splits (d = 128: the 512-thread kernel) | 1 split; one workspace over all positions
        for B, H, Hk in ((2, 2, 2), (8, 32, 8), (16, 32, 8)):
            Tmax = 304
            tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
            ws = ops.attn_decode_rope_workspace(B, H, d, "cuda")
            qkv = _rand(B, (H + 2 * Hk) * d, seed=40 + d)
            for pos in (0, 1, 127, 128, 129, 255, 256, 257, 300):
                def rope():
                    k0, v0 = cache(B, Hk, Tmax, d, [0] * B, pos, seed=50)
                    kc, vc = k0.clone(), v0.clone()
                    o = ops.attn_decode_rope(qkv, tab, kc, vc, torch.zeros(B, H * d, dtype=BF, device="cuda"), B, H, Hk, d, Tmax, pos, sc, workspace=ws)
                    keep = torch.arange(Tmax, device="cuda") != pos              # both caches: the appended rows, and that no other row changed
                    same = torch.tensor([torch.equal(a[:, :, keep].view(torch.int16), b[:, :, keep].view(torch.int16)) for a, b in ((kc, k0), (vc, v0))])
                    return o, kc[:, :, pos].contiguous(), vc[:, :, pos].contiguous(), same, ws.clone()        # ws: the fp32 partials of the splits
                yield run(f"rope d={d} B={B} H={H} pos={pos}", rope)
        # ---- attn_decode_fp8_kernel: n cached keys in front of the slot being decoded
        B, H, Hk, Tmax = 2, 4, 2, 104
        tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
        qkv = _rand(B, (H + 2 * Hk) * d, seed=60 + d)
        for n in (0, 1, 31, 32, 33, 63, 64, 65, 97):
            for ks0 in (0, 3):
                def fp8():
                    pos = ks0 + n
                    src_k, src_v = _rand(1, B, Hk, Tmax, d, seed=70, scale=0.5), _rand(1, B, Hk, Tmax, d, seed=71)
                    codes = [torch.full((1, B, Hk, Tmax, d), 0x7F, dtype=torch.uint8, device="cuda") for _ in range(2)]      # 0x7f: the e4m3fn NaN
                    scales = [torch.full((1, B, Hk, Tmax), NAN, dtype=torch.float32, device="cuda") for _ in range(2)]
                    if n:
                        ops.kv_quant_fp8(src_k, src_v, codes[0], codes[1], scales[0], scales[1], t0=ks0, t_dst=ks0, S=n)
                    o = ops.attn_decode_fp8(qkv, tab, codes[0][0], codes[1][0], scales[0][0], scales[1][0], torch.zeros(B, H * d, dtype=BF, device="cuda"),
                                            B, H, Hk, d, Tmax, pos, sc, kv_start=i32([ks0] * B) if ks0 else None)
                    return [o] + codes + scales
                yield run(f"fp8 d={d} cached={n} kv_start={ks0}", fp8)
        # ---- attn_prefix_partial + attn_own_merge: the row kernel (H == Hk, one query per row); (14, 2, 128): the grouped kernel, a control
        for H, Hk in ((2, 2), (14, 2)) if d == 128 else ((2, 2),):
            B, P, Tp, Tmax, kv0 = 3, 17, 24, 72, 3
            q = _rand(B, H * d, seed=80 + d)
            tiles, row_clip = ops.prefix_tile_plan([B], H, Hk)
            pk, pv = cache(1, Hk, Tp, d, [0], P, seed=81)
            for own in (1, 16, 17, 32, 33, 49, 65):
                def prefix():
                    ws = torch.zeros(ops.attn_prefix_bytes(B, H, d), dtype=torch.uint8, device="cuda")
                    ops.attn_prefix_partial(q, pk, pv, ws, i32(tiles).reshape(-1), i32(row_clip), B, H, Hk, d, P, sc)
                    kc, vc = cache(B, Hk, Tmax, d, [kv0] * B, kv0 + own, seed=82)
                    o = ops.attn_own_merge(q, ws, kc, vc, torch.zeros_like(q), B, 1, H, Hk, d, Tmax, kv0 + own, sc, kv_start=i32([kv0] * B))
                    return o, ws
                yield run(f"prefix pair d={d} H={H} Hk={Hk} own={own}", prefix)
    # ---- volume.  The kernels write a * b + c * d, and which product the compiler fuses is its choice per build: a build that chooses otherwise
    # differs in the last fp32 bit, which reaches about one bf16 output in 10^4.  Enough rows per kernel that such a build cannot pass by luck.
    for d in (64, 128):
        sc = d ** -0.5
        B, H, Tmax, ctx = 128, 32, 136, 131
        gen = torch.Generator(device="cuda").manual_seed(100 + d)
        rn = lambda *shape: (torch.randn(*shape, device="cuda", generator=gen) * 0.5).bfloat16()
        kc, vc = rn(B, H, Tmax, d), rn(B, H, Tmax, d)
        ks = i32([(7 * b) % 64 for b in range(B)])
        km = ops.pack_key_mask(torch.rand(B, Tmax, device="cuda", generator=gen) < 0.7)
        tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
        k8, v8 = (torch.empty(1, B, H, Tmax, d, dtype=torch.uint8, device="cuda") for _ in range(2))
        s8k, s8v = (torch.empty(1, B, H, Tmax, dtype=torch.float32, device="cuda") for _ in range(2))
        ops.kv_quant_fp8(kc[None], vc[None], k8, v8, s8k, s8v)
        wss = {b: ops.attn_decode_rope_workspace(b, H, d, "cuda") for b in (1, 8)}
        for r in range(4):
            q, qkv = rn(B, H * d), rn(B, 3 * H * d)
            o = lambda rows=B: torch.zeros(rows, H * d, dtype=BF, device="cuda")
            part = torch.randn(B * H, d + 2, device="cuda", generator=gen)                  # a prefix partial: o, m, l > 0
            part[:, d + 1] = part[:, d + 1].abs() + 0.5
            yield run(f"volume d={d} #{r} decode", lambda: ops.attn_decode(q, kc, vc, o(), B, H, H, d, Tmax, ctx, sc, kv_start=ks))
            yield run(f"volume d={d} #{r} keymask", lambda: ops.attn_decode(q, kc, vc, o(), B, H, H, d, Tmax, ctx, sc, key_mask=km))
            yield run(f"volume d={d} #{r} own_merge", lambda: ops.attn_own_merge(q, part.view(torch.uint8).reshape(-1), kc, vc, o(), B, 1, H, H, d, Tmax, ctx, sc,
                                                                              kv_start=ks))
            yield run(f"volume d={d} #{r} rope", lambda: ops.attn_decode_rope(qkv, tab, kc, vc, o(), B, H, H, d, Tmax, ctx, sc))
            for b in (1, 8):                                                                  # 8 and 2 splits: the fp32 partials are outputs too
                yield run(f"volume d={d} #{r} rope B={b}", lambda: (ops.attn_decode_rope(qkv, tab, kc, vc, o(b), b, H, H, d, Tmax, ctx, sc, workspace=wss[b]),
                                                                    wss[b].clone()))
            yield run(f"volume d={d} #{r} fp8", lambda: ops.attn_decode_fp8(qkv, tab, k8[0], v8[0], s8k[0], s8v[0], o(), B, H, H, d, Tmax, ctx, sc, kv_start=ks))
        del kc, vc, k8, v8
    # ---- attn_verify (px_attend of csrc/attn_rows_core.h with the per-row limit) and the multi-query form of attn_own_merge (the same loop without
    # it).  G = 1, 4, 7; Sq = 1, 3, 8, 16: both ROWS forms, one to eight query groups.  kv_start > 0; the rows' limits (ctx + i - kv_start) straddle
    # a 16-key tile edge | the 512-key chunk edge | (ctx = 505) end below the chunk edge for sequence 0 and across it for sequence 1
    B, Hk, Tmax = 2, 2, 560
    lo = [3, 9]
    for d in (64, 128):
        sc = d ** -0.5
        for G in (1, 4, 7):
            H, per = G * Hk, 16 // G
            for Sq in (1, 3, 8, 16):
                q = _rand(B * Sq, H * d, seed=110 + d + Sq)
                for ctx in (3 + 16 - Sq // 2, 3 + 512 - Sq // 2, 505):
                    kc, vc = cache(B, Hk, Tmax, d, lo, ctx + Sq - 1, seed=111)
                    yield run(f"verify d={d} G={G} Sq={Sq} ctx={ctx}",
                              lambda: ops.attn_verify(q, kc, vc, torch.zeros_like(q), B, Sq, H, Hk, d, Tmax, ctx, sc, kv_start=i32(lo)))
                    if Sq > per:                                            # several query groups: NaN from the FIRST group's last visible slot on
                        kc, vc = cache(B, Hk, Tmax, d, lo, ctx + per - 1, seed=111)
                        yield run(f"verify d={d} G={G} Sq={Sq} ctx={ctx} first group",
                                  lambda: ops.attn_verify(q, kc, vc, torch.zeros_like(q), B, Sq, H, Hk, d, Tmax, ctx, sc,
                                                          kv_start=i32(lo)).view(B, Sq, H * d)[:, :per].contiguous())
                # the clamp at Tmax: a device ctx word carries the queries past the cache (the host check sees ctx_len alone)
                kc, vc = cache(B, Hk, Tmax, d, lo, Tmax, seed=111)
                yield run(f"verify d={d} G={G} Sq={Sq} clamp at Tmax",
                          lambda: ops.attn_verify(q, kc, vc, torch.zeros_like(q), B, Sq, H, Hk, d, Tmax, Tmax - Sq - 3, sc, ctx_dev=i32([Sq // 2 + 4]),
                                                  kv_start=i32(lo)))
            for Sq in (3, 8):
                rows, P, Tp = B * Sq, 17, 24
                q = _rand(rows, H * d, seed=120 + d + Sq)
                tiles, row_clip = ops.prefix_tile_plan([rows], H, Hk)
                for ctx in (3 + 16 - Sq // 2, 3 + 512 - Sq // 2):
                    def multi():
                        pk, pv = cache(1, Hk, Tp, d, [0], P, seed=81)
                        ws = torch.zeros(ops.attn_prefix_bytes(rows, H, d), dtype=torch.uint8, device="cuda")
                        ops.attn_prefix_partial(q, pk, pv, ws, i32(tiles).reshape(-1), i32(row_clip), rows, H, Hk, d, P, sc)
                        kc, vc = cache(B, Hk, Tmax, d, lo, ctx + Sq - 1, seed=111)
                        return ops.attn_own_merge(q, ws, kc, vc, torch.zeros_like(q), B, Sq, H, Hk, d, Tmax, ctx, sc, kv_start=i32(lo)), ws
                    yield run(f"own_merge d={d} G={G} Sq={Sq} ctx={ctx}", multi)
    for d in (64, 128):                                                     # volume, as above: 64 x 8 (one group of 8 operand rows) and 64 x 16 queries x 32 heads
        B, H, Tmax, ctx = 64, 32, 152, 130
        gen = torch.Generator(device="cuda").manual_seed(130 + d)
        rn = lambda *shape: (torch.randn(*shape, device="cuda", generator=gen) * 0.5).bfloat16()
        kc, vc = rn(B, H, Tmax, d), rn(B, H, Tmax, d)
        ks = i32([(7 * b) % 64 for b in range(B)])
        for Sq in (8, 16):
            q = rn(B * Sq, H * d)
            yield run(f"volume d={d} verify Sq={Sq}", lambda: ops.attn_verify(q, kc, vc, torch.zeros_like(q), B, Sq, H, H, d, Tmax, ctx, d ** -0.5, kv_start=ks))
        del kc, vc
    # ---- attn_decode through attn_decode_gqa_kernel<128, 4>: a control for a file that is recompiled
    B, H, Hk, d, Tmax, ctx = 64, 16, 4, 128, 72, 70
    q = _rand(B, H * d, seed=90)
    lo = [(5 * b) % 40 for b in range(B)]
    kc, vc = cache(B, Hk, Tmax, d, lo, ctx, seed=91)
    yield run("decode grouped-query G=4", lambda: ops.attn_decode(q, kc, vc, torch.zeros_like(q), B, H, Hk, d, Tmax, ctx, d ** -0.5, kv_start=i32(lo)))


def _select_cases():
    """Yields (name, tensors) for the sampling selects (csrc/select_core.h): sample_select, sample_select_warped (ids, kept_n, kept_min) and
    constrained_select (ids, node).  An id moves only when a one-ulp change of a mass crosses the drawn number, so the edge cases are followed by
    launches of 8192 rows.  Every logits tensor is a view from row 1 of a buffer one row taller: a library that reads in front of a row without a
    finite token (sample_select_kernel did) stays inside the allocation."""
    from crab_amd import ops

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device="cuda")

    def rows(B, V, seed):
        g = torch.Generator().manual_seed(seed)
        buf = torch.randn(B + 1, V, generator=g) * 3
        if B == 8:
            buf[2] = 0.5                                                    # exact ties
            buf[3] = -INF
            buf[3, V // 2] = 1.25                                           # one finite token
            buf[4] = -INF                                                   # none
            buf[5, : V // 2] = buf[5, V - 1]                                # ties at one value among random ones
        return buf.cuda()[1:]

    def launch(name, B, step, fn, extra=()):
        """fn(cur, out, step_dev, finished) -> the state after the launch (+ extra tensors)."""
        cur = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        out = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
        fin = i32([1 if b % 8 in (6, 7) else 0 for b in range(B)])          # rows 6 and 7 of every 8 are finished
        fn(cur, out, i32([step]), fin)
        torch.cuda.synchronize()
        return "select " + name, [_bits(t) for t in (cur, out, fin, *extra)]

    def tries(V, eos):
        """name -> (edge_off, edge_tok, edge_dst, node) for 8 rows."""
        ident = ([0, V], list(range(V)), [0] * V, [0] * 8)
        e0 = sorted(set(range(0, V, 7)) | {eos})
        e1 = [eos, V - 1, V // 2]
        off, tok, dst = [0, len(e0), len(e0) + 3, len(e0) + 3], e0 + e1, [1] * len(e0) + [2] * 3
        sparse = (off, tok, dst, [0, 1, 2, 0, 1, 0, 1, 2])                  # node 2: the sink, no edges
        btok = list(tok)
        btok[0], btok[-1], btok[len(btok) // 2] = -5, V + 10, 1 << 30
        bad = ([0, len(e0), len(tok) + 50, -3], btok, dst, [0, 1, 2, -1, 7, 0, 1, 0])       # edge ranges and nodes out of range too
        return {"identity": ident, "sparse": sparse, "corrupt": bad}

    INF = float("inf")
    PAD, MIN_NEW, SEED = 0, 2, 1234
    WARPS = {"min_p": (0.05, 0.0, 0.0), "epsilon": (0.0, 2e-3, 0.0), "eta": (0.0, 0.0, 5e-3), "all": (0.05, 2e-3, 5e-3)}
    for V in (1, 1000, 1025, 5000):                                         # one item per thread with idle threads | ragged chunk of 2 | chunk of 5
        B, eos = 8, min(2, V - 1)
        lg = rows(B, V, seed=200 + V)
        trie = {k: tuple(i32(a) for a in v) for k, v in tries(V, eos).items()}
        for step in (0, 3):                                                 # EOS suppressed | not
            for name, (off, tok, dst, node) in trie.items():
                nd = node.clone()
                yield launch(f"constrained greedy V={V} step={step} {name}", B, step,
                             lambda c, o, s, f: ops.constrained_select(lg, off, tok, dst, nd, c, o, s, f, eos, PAD, MIN_NEW), (nd,))
            for top_k in sorted({0, 1, 50, V}):
                for top_p in (1.0, 0.9, 1e-6):
                    for temp in (1.0, 0.6):
                        tag = f"V={V} step={step} k={top_k} p={top_p} t={temp}"
                        yield launch(f"sample {tag}", B, step, lambda c, o, s, f: ops.sample_select(lg, c, o, s, f, eos, PAD, MIN_NEW, temp, top_k, top_p, SEED))
                        for wn, (mp, ep, et) in WARPS.items():
                            kn, km = i32([-7] * B), torch.full((B,), -7.0, device="cuda")
                            yield launch(f"warped {wn} {tag}", B, step,
                                         lambda c, o, s, f: ops.sample_select_warped(lg, c, o, s, f, eos, PAD, MIN_NEW, temp, top_k, top_p, SEED, mp, ep, et,
                                                                                     kept_n=kn, kept_min=km), (kn, km))
                        for name, (off, tok, dst, node) in trie.items():
                            nd = node.clone()
                            yield launch(f"constrained {name} {tag}", B, step,
                                         lambda c, o, s, f: ops.constrained_select(lg, off, tok, dst, nd, c, o, s, f, eos, PAD, MIN_NEW, temp, top_k, top_p, SEED),
                                         (nd,))
    # ---- volume: 8192 rows per launch
    B, V, eos = 8192, 1025, 2
    lg = rows(B, V, seed=300)
    off, tok, dst, node = (i32(a) for a in ([0, V], list(range(V)), [0] * V, [0] * B))
    kn, km = i32([-7] * B), torch.full((B,), -7.0, device="cuda")
    yield launch("volume sample", B, 3, lambda c, o, s, f: ops.sample_select(lg, c, o, s, f, eos, PAD, MIN_NEW, 0.6, 50, 0.9, SEED))
    yield launch("volume warped all", B, 3, lambda c, o, s, f: ops.sample_select_warped(lg, c, o, s, f, eos, PAD, MIN_NEW, 0.6, 50, 0.9, SEED, *WARPS["all"],
                                                                                        kept_n=kn, kept_min=km), (kn, km))
    yield launch("volume constrained identity", B, 3,
                 lambda c, o, s, f: ops.constrained_select(lg, off, tok, dst, node, c, o, s, f, eos, PAD, MIN_NEW, 0.6, 50, 0.9, SEED), (node,))


LISTS = {"gemm": _cases, "attn": _attn_cases, "select": _select_cases}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        torch.save({k: v for which in sys.argv[3].split("+") for k, v in LISTS[which]()}, sys.argv[2])
        return 0
    if len(sys.argv) not in (3, 4) or (len(sys.argv) == 4 and sys.argv[3] not in LISTS):
        print(__doc__)
        return 2
    which = sys.argv[3] if len(sys.argv) == 4 else "gemm+attn"
    sets = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, f"{i}.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, which], check=True,
                           env=dict(os.environ, CRAB_HIP_LIB=os.path.abspath(lib)))
            sets.append(torch.load(out))
    a, b = sets
    assert list(a) == list(b) and len(a) > 0
    refused = [n for n in a if a[n][0].dtype == torch.uint8]
    bad = 0
    for name in a:
        if len(a[name]) != len(b[name]) or not all(torch.equal(s, t) for s, t in zip(a[name], b[name])):
            bad += 1
            print(f"DIFFERENT: {name}")
            for s, t in zip(a[name], b[name]):
                if s.shape == t.shape and not torch.equal(s, t):
                    i = (s != t).nonzero()[0].tolist()
                    print(f"  first at {i}: {s[tuple(i)].item()} vs {t[tuple(i)].item()} ({(s != t).sum().item()} of {s.numel()} elements)")
    if bad:
        print(f"{bad} of {len(a)} cases differ")
        return 1
    print(f"all {len(a)} cases identical ({sum(len(v) for v in a.values())} tensors; {len(refused)} calls refused by both libraries alike)")
    for msg in sorted({bytes(a[n][0].tolist()).decode() for n in refused}):
        print(f"  refused: {msg[:160]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
