"""shed_finished, measured (GPU box; not a gate): writes profiles/shed_finished.json.  One MI355X, both sides of every comparison alternating in
this process; the kernel part reports medians of rounds (as scripts/bench_beam.py), the call part every timed round and the ratio of the
best rounds (two timed rounds after a warm-up round, as bench_beam.py's call level).
  (a) kernel: crab_kv_compact_rows alone on 512 -> 256, 256 -> 128 (alternate rows survive) and 64 -> 16 rows (every fourth), Llama-2-7B heads
      (Hk = 32, d = 128), 830 + 64 slots live of Tmax = 896, as many of the 32 layers as one launch takes (2^31 16-byte units per cache: 8, 16
      and 32).  us per launch and TB/s of read plus written bytes (every surviving row moves: read once, written once, K and V), next to a
      torch copy of the same bytes inside the same allocation and to the figures on record (docs/measured_headroom.md: item 12,
      crab_kv_beam_reorder 3.5-3.7 TB/s; item 10, the copy rate 4.7-5.0 TB/s).
  (b) calls: the full-size synthetic Llama decoder (encoders not built: random embeddings), 830 prompt rows, 128 new tokens, generate() with and
      without shed_finished=True at 512, 64 and 8 rows.  Every second row is a copy of row 0 (random weights emit near-random ids, so no id
      ends half of 512 different prompts early); the EOS id is the token of a free run, emitted by row 0 at a step in 4 .. 31, that puts the
      share of rows finishing before step 32 closest to one half (the finish-step histogram is recorded); the same pair again with an EOS
      nothing emits - the option's overhead.  Half of the rows leaving at ONE early step is the best case of the default ladder (one shed,
      exactly a rung): the ratios are an upper end, not an expectation.
  (c) break-even: the decode step time at the rungs (calls of 128 and of 2 new tokens, their difference over 126 steps) and, per shed of (b),
      the compaction's cost - ESTIMATED from (a)'s rate x rows moved x layers, no shed is timed on its own - in units of the step time it
      saves: the number the ladder should be tuned by.
usage: bench_shed.py [iters] [--no-kernel] [--no-call] [--break-even-only] [--rounds N] [--rows 512,64,8] [--new-tokens N] [--out PATH]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crab_amd import ops

_valued = ("--rounds", "--rows", "--new-tokens", "--out")
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in _valued]
flag = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 10
rounds = flag("--rounds", 5)
dev = "cuda"
Hk, d, TMAX, LIVE = 32, 128, 896, 830 + 64
ON_RECORD = {"kv_beam_reorder_TBps": [3.5, 3.7], "copy_TBps": [4.7, 5.0]}


def timed(f, n, warm=2):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def spread(v):
    s = sorted(v)
    return {"median_us": round(s[len(s) // 2], 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1), "rounds_us": [round(x, 1) for x in v]}


def kernel_level():
    out = []
    for rows, keep_every, L in ((512, 2, 8), (256, 2, 16), (64, 4, 32)):
        src = list(range(keep_every - 1, rows, keep_every))
        kc = torch.empty((L, rows, Hk, TMAX, d), device=dev, dtype=torch.bfloat16).uniform_(-1, 1)
        vc = torch.empty((L, rows, Hk, TMAX, d), device=dev, dtype=torch.bfloat16).uniform_(-1, 1)
        pos = torch.full((1,), LIVE - 1, dtype=torch.int32, device=dev)
        n = len(src)
        # the same bytes as a strided torch copy inside the allocation: the rows n .. 2n - 1 over the live slots to the rows 0 .. n - 1
        fs = {"kv_compact_rows": lambda: ops.kv_compact_rows(kc, vc, src, pos),
              "torch_copy": lambda: (kc[:, :n, :, :LIVE].copy_(kc[:, n:2 * n, :, :LIVE]), vc[:, :n, :, :LIVE].copy_(vc[:, n:2 * n, :, :LIVE]))}
        t = {k: [] for k in fs}
        for _ in range(rounds):
            for k, f in fs.items():
                t[k].append(timed(f, iters))
        nbytes = 2.0 * 2 * n * L * Hk * LIVE * d * 2               # read + written, K and V
        row = {"rows": rows, "rows_after": n, "layers_allocated": L, "live_slots": LIVE, "Tmax": TMAX, **{k: spread(v) for k, v in t.items()},
               "bytes": nbytes, "on_record": ON_RECORD}
        for k in fs:
            row[k + "_TBps"] = round(nbytes / row[k]["median_us"] / 1e6, 3)
        row["us_per_layer"] = round(row["kv_compact_rows"]["median_us"] / L, 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del kc, vc
        torch.cuda.empty_cache()
    return out


def call_level(row_counts, new_tokens, kernel_rows, prompt=830):
    from crab_amd.build_model import build_crab
    from crab_amd.decoder import shed_default_ladder
    model = build_crab("llama", device=dev, visual=False, audio=False)
    eng = model.base_model.model._engine
    c = model.base_model.model.config
    V = model.base_model.model.lm_head.weight.shape[0]
    g = torch.Generator(device=dev).manual_seed(2)

    def run(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    out, step_ms = [], {}
    for B in row_counts:
        emb = (torch.randn(B, prompt, c.hidden_size, device=dev, generator=g) * 0.5).bfloat16()
        # random weights emit near-random ids: no id ends half of 512 DIFFERENT prompts early (measured: 8 of 512 at best).  So every second row
        # is a copy of row 0 - the copies emit row 0's ids and finish together, the other half are prompts of their own
        emb[0::2] = emb[0]
        free = eng.generate(emb, new_tokens, eos_token_id=None, pad_token_id=2).cpu()
        best = None
        for tok in sorted(set(free[0, 4:32].tolist()) - {2}):
            first = [(row.index(tok) if tok in row else None) for row in free.tolist()]
            share = sum(1 for f in first if f is not None and f < 32) / B
            if best is None or abs(share - 0.5) < abs(best[0] - 0.5):
                best = (share, tok, first)
        share, eos, first = best
        never = next(t for t in range(3, V) if t not in set(free.flatten().tolist()))
        hist = {}
        for f in first:
            key = "never" if f is None else f"{f // 16 * 16}-{f // 16 * 16 + 15}"
            hist[key] = hist.get(key, 0) + 1
        row = {"rows": B, "prompt_rows": prompt, "new_tokens": new_tokens, "eos_id": eos, "share_finished_before_step_32": round(share, 3),
               "finish_step_histogram": hist, "ladder": list(shed_default_ladder())}
        for name, e in (("half_finish_early", eos), ("eos_never_emitted", never)):
            fs = {"plain": lambda: eng.generate(emb, new_tokens, eos_token_id=e, pad_token_id=2),
                  "shed": lambda: eng.generate(emb, new_tokens, eos_token_id=e, pad_token_id=2, shed_finished=True)}
            t = {k: [] for k in fs}
            for r in range(3):                                   # round 0 is the warm-up: graph captures of the root and of the rungs
                for k, f in fs.items():
                    s, res = run(f)
                    if r:
                        t[k].append(s)
                    if k == "shed":
                        plan = {"shed": eng.last_plan["shed"], "shed_captures": eng.last_plan["shed_captures"]}
                    else:
                        cols = int(res.shape[1])
            row[name] = {**{k + "_s": [round(x, 3) for x in v] for k, v in t.items()}, "shed_over_plain": round(min(t["shed"]) / min(t["plain"]), 3),
                         "columns": cols, "sheds_step_before_after_moved": plan["shed"], "captures_in_last_round": plan["shed_captures"]}
        print(json.dumps(row), flush=True)
        out.append(row)
        del emb
    # (c) the step time at every row count a shed above started from or arrived at: a call of new_tokens against a call of 2 (the same prefill),
    # over the steps between them
    met = sorted({b for row in out for _, before, after, _ in row["half_finish_early"]["sheds_step_before_after_moved"] for b in (before, after)}, reverse=True)
    for B in met:
        emb = (torch.randn(B, prompt, c.hidden_size, device=dev, generator=g) * 0.5).bfloat16()
        t_long = min(run(lambda: eng.generate(emb, new_tokens, eos_token_id=None, pad_token_id=2))[0] for _ in range(2))
        t_short = min(run(lambda: eng.generate(emb, 2, eos_token_id=None, pad_token_id=2))[0] for _ in range(2))
        step_ms[B] = (t_long - t_short) / (new_tokens - 2) * 1e3
        del emb
    return out, break_even(out, step_ms, kernel_rows, c.num_hidden_layers)


def break_even(calls, step_ms, kernel_rows, layers=32):
    """(c) per shed of (b): the kernel's time for all `layers` layers (from (a): us per layer and surviving row at the nearest measured row
    count, times the rows moved) in units of the step time the shed saves.  Pure arithmetic on measured numbers: the kernel and the call part
    may come from two runs of this script (--no-call, --no-kernel with the same --out)."""
    step_ms = {int(k): float(v) for k, v in step_ms.items()}
    per_row_layer_us = {r["rows"]: r["us_per_layer"] / r["rows_after"] for r in kernel_rows} if kernel_rows else {}
    even = []
    for row in calls:
        for step, before, after, moved in row["half_finish_early"]["sheds_step_before_after_moved"]:
            if before in step_ms and after in step_ms and per_row_layer_us:
                ref = min(per_row_layer_us, key=lambda r: abs(r - before))
                cost_ms = per_row_layer_us[ref] * moved * layers / 1e3
                saved = step_ms[before] - step_ms[after]
                even.append({"rows_before": before, "rows_after": after, "rows_moved": moved, "compaction_ms_estimated": round(cost_ms, 3),
                             "step_ms_saved": round(saved, 3), "break_even_steps": round(cost_ms / saved, 2) if saved > 0 else None})
    return {"decode_step_ms": {str(k): round(v, 3) for k, v in step_ms.items()}, "per_shed": even,
            "note": "compaction_ms_estimated: (a)'s us per layer and surviving row at the nearest measured row count x rows moved x the model's layers; "
                    "the gather of the per-row words and the child's first replay are inside the whole-call times of (b)"}


if __name__ == "__main__":
    path = flag("--out", os.path.join(ROOT, "profiles", "shed_finished.json"))
    res = json.load(open(path)) if os.path.exists(path) else {}
    if "--break-even-only" in sys.argv:                          # no GPU: (c) again from the (a) and (b) sections the file holds
        res["break_even"] = break_even(res["calls"], res["break_even"]["decode_step_ms"], res.get("kernel"))
        json.dump(res, open(path, "w"), indent=1)
        sys.exit(0)
    assert torch.cuda.is_available(), "bench_shed.py measures on the GPU; there is nothing to report without one"
    res.update({"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds})
    if "--no-kernel" not in sys.argv:
        res["kernel"] = kernel_level()
        json.dump(res, open(path, "w"), indent=1)
    if "--no-call" not in sys.argv:
        rows = [int(x) for x in flag("--rows", "512,64,8").split(",")]
        res["calls"], res["break_even"] = call_level(rows, flag("--new-tokens", 128), res.get("kernel"))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
