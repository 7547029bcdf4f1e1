"""Shared-prefix generation, measured (GPU box; not a gate): writes profiles/shared_prefix.json.
  kernel level: crab_attn_prefix_partial + crab_attn_own_merge at ~512 rows, P = 800 prefix rows, own context 30 + 128, G questions per clip in
      {1, 2, 5, 8, 16}, against attn_decode_kernel<128> at the same rows x 958 keys (Llama-2-7B heads: H = Hk = 32, d = 128).  Both run ALTERNATELY in
      this process, three rounds of `iters` launches each, the median round is reported: us per launch (pair: both launches) and the algorithmic
      bytes (every live K / V row once, q in, o out; the pair also writes and reads its fp32 partials) over that time.
  call level: questions per second of generate_shared_prefix against generate_many(coalesce=True) on the duplicated prompts, G = 5, on the full-size
      synthetic Llama decoder (encoders not built: the embeddings are random), alternated, 2 rounds.
usage: bench_shared_prefix.py [iters] [--no-call] [--clips N] [--new-tokens N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crab_amd import ops

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flag = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 20
H = Hk = 32; d = 128
P, OWN, ROWS = 800, 30 + 128, 512
scale = d ** -0.5
dev = "cuda"


def timed(f, n):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def kernel_level():
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.5).bfloat16()
    for G in (1, 2, 5, 8, 16):
        C = ROWS // G
        B = C * G
        T_old = 960
        kc, vc = rn(B, Hk, T_old, d), rn(B, Hk, T_old, d)
        q = rn(B, H * d); o = torch.empty_like(q); o2 = torch.empty_like(q)
        old = lambda: ops.attn_decode(q, kc, vc, o, B, H, Hk, d, T_old, P + OWN, scale)
        Tp, Tmax = 832, 192
        pk, pv = rn(C, Hk, Tp, d), rn(C, Hk, Tp, d)
        ok, ov = rn(B, Hk, Tmax, d), rn(B, Hk, Tmax, d)
        tiles, row_clip = ops.prefix_tile_plan([G] * C, H, Hk)
        tile_rows = torch.tensor(tiles, dtype=torch.int32, device=dev).reshape(-1)
        row_clip = torch.tensor(row_clip, dtype=torch.int32, device=dev)
        ws = torch.empty((ops.attn_prefix_bytes(B, H, d),), dtype=torch.uint8, device=dev)

        def new():
            ops.attn_prefix_partial(q, pk, pv, ws, tile_rows, row_clip, B, H, Hk, d, P, scale)
            ops.attn_own_merge(q, ws, ok, ov, o2, B, 1, H, Hk, d, Tmax, OWN, scale)
        k1 = lambda: ops.attn_prefix_partial(q, pk, pv, ws, tile_rows, row_clip, B, H, Hk, d, P, scale)
        t_old, t_new, t_k1 = [], [], []
        for _ in range(3):
            t_old.append(timed(old, iters)); t_new.append(timed(new, iters)); t_k1.append(timed(k1, iters))
        u_old, u_new, u_k1 = sorted(t_old)[1], sorted(t_new)[1], sorted(t_k1)[1]
        qo = 2.0 * B * H * d * 2
        b_old = 2.0 * B * (P + OWN) * Hk * d * 2 + qo
        b_new = 2.0 * (C * P + B * OWN) * Hk * d * 2 + qo + 2.0 * B * H * (d + 2) * 4
        row = {"G": G, "clips": C, "rows": B, "existing_us": round(u_old, 1), "existing_rounds_us": [round(t, 1) for t in t_old],
               "existing_bytes": b_old, "existing_TBps": round(b_old / u_old / 1e6, 3),
               "pair_us": round(u_new, 1), "pair_rounds_us": [round(t, 1) for t in t_new], "prefix_partial_us": round(u_k1, 1),
               "pair_bytes": b_new, "pair_TBps": round(b_new / u_new / 1e6, 3),
               "time_ratio": round(u_new / u_old, 3), "byte_model_ratio": round((P + G * OWN) / (G * (P + OWN)), 3)}
        print(json.dumps(row), flush=True)
        out.append(row)
        del kc, vc, pk, pv, ok, ov
        torch.cuda.empty_cache()
    return out


def call_level(clips, new_tokens, G=5):
    from crab_amd.build_model import build_crab
    model = build_crab("llama", device=dev, visual=False, audio=False)
    eng = model.base_model.model._engine
    D = model.base_model.model.config.hidden_size
    g = torch.Generator(device=dev).manual_seed(2)
    rn = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.5).bfloat16()
    prefix = rn(clips, P, D)
    suffix = [[rn(30, D) for _ in range(G)] for _ in range(clips)]
    seqs = [torch.cat([prefix[c], q], 0)[None] for c in range(clips) for q in suffix[c]]
    kw = dict(eos_token_id=None, pad_token_id=2, min_new_tokens=new_tokens)

    def run(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    old = lambda: eng.generate_many(seqs, new_tokens, coalesce=True, **kw)
    new = lambda: eng.generate_shared_prefix(prefix, suffix, new_tokens, **kw)
    run(old); run(new)                                           # warm-up: module load, graph capture
    t_old, t_new = [], []
    for _ in range(2):
        t_old.append(run(old)); t_new.append(run(new))
    nq = clips * G
    row = {"clips": clips, "G": G, "questions": nq, "new_tokens": new_tokens, "prefix_rows": P, "question_rows": 30,
           "existing_s": [round(t, 3) for t in t_old], "shared_prefix_s": [round(t, 3) for t in t_new],
           "existing_questions_per_s": round(nq / min(t_old), 2), "shared_prefix_questions_per_s": round(nq / min(t_new), 2),
           "note": "decoder only (random embeddings in place of the encoders' output): the encoder saving of one clip per G questions is not in these numbers"}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_shared_prefix.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "shape": {"H": H, "Hk": Hk, "d": d, "P": P, "own": OWN, "rows": ROWS, "iters": iters},
           "kernel": kernel_level()}
    path = os.path.join(ROOT, "profiles", "shared_prefix.json")
    json.dump(res, open(path, "w"), indent=1)
    if "--no-call" not in sys.argv:
        res["call"] = call_level(flag("--clips", 100), flag("--new-tokens", 128))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
