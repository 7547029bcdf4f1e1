"""Beam search, measured (GPU box; not a gate): writes profiles/beam_search.json.
  kernel level: the beam step - crab_beam_row_topk + crab_beam_merge + crab_kv_beam_reorder - next to crab_greedy_select alone on the same fp32
      logits [512, 32000] (128 clips x K = 4 beams), with 1, 64 and 256 own cache slots to reorder (Llama-2-7B heads: Hk = 32, d = 128, 8 of
      the 32 layers allocated; random parents, so almost every clip moves).  The reorder's bytes (every parent row read, every changed row
      written, K and V) over its time stand next to the 7.1 TB/s a read stream reaches on this chip.  The launches run ALTERNATELY in this
      process, `rounds` rounds of `iters` launches each; median, min and max of the rounds are reported in us per launch.
  call level: generate_beam on C clips x 4 beams against greedy generate() on C x 4 rows and on C rows - same prompt (830 rows) and length,
      no EOS - on the full-size synthetic Llama decoder (encoders not built: the embeddings are random), alternated, 2 rounds.
  bytes: what the wave holds on the device (shared_prefix_bytes: the prompt KV once per clip) against B K bytes_per_sequence.
usage: bench_beam.py [iters] [--no-call] [--rounds N] [--clips N] [--new-tokens N] [--out PATH]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crab_amd import ops

_valued = ("--rounds", "--clips", "--new-tokens", "--out")
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in _valued]
flag = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 50
rounds = flag("--rounds", 5)
dev = "cuda"
K, ROWS, V, MAX_NEW, STEP = 4, 512, 32000, 256, 5
L, Hk, d, TMAX = 8, 32, 128, 320
HBM_READ_STREAM_TBPS = 7.1


def timed(f, n, warm=3):
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
    g = torch.Generator(device=dev).manual_seed(1)
    clips = ROWS // K
    logits = torch.randn(ROWS, V, device=dev, generator=g) * 4.0
    bs = ops.BeamState(clips, K, MAX_NEW, 0, 1.0, False, dev)
    cur = torch.zeros(ROWS, dtype=torch.int64, device=dev)
    run_seq = torch.zeros((ROWS, MAX_NEW), dtype=torch.int64, device=dev)
    scratch_ids = torch.zeros((ROWS, MAX_NEW), dtype=torch.int64, device=dev)
    fin = torch.zeros(ROWS, dtype=torch.int32, device=dev)
    sd = torch.full((1,), STEP, dtype=torch.int32, device=dev)
    kc = (torch.randn(L, ROWS, Hk, TMAX, d, device=dev, generator=g) * 0.5).bfloat16()
    vc = (torch.randn(L, ROWS, Hk, TMAX, d, device=dev, generator=g) * 0.5).bfloat16()
    idx = torch.randint(0, K, (ROWS,), device=dev, generator=g).int()
    par = idx.view(clips, K).cpu()
    moved = par != torch.arange(K)[None]
    live = moved.any(1)
    reads, writes = int(live.sum()) * K, int(moved.sum())
    out = []
    for ctx in (1, 64, 256):
        pos = torch.full((1,), ctx - 1, dtype=torch.int32, device=dev)

        def select():
            bs.run_score.fill_(0.0)                              # no EOS and a fixed step: the clips never finish; the scores are put back so that they stay finite
            ops.beam_row_topk(logits, bs, sd, fin, -1, 0)
            ops.beam_merge(bs, V, sd, -1, cur, run_seq, fin)
        fs = {"greedy_select": lambda: ops.greedy_select(logits, cur, scratch_ids, sd, fin, -1, 0, 0),
              "beam_row_topk": lambda: ops.beam_row_topk(logits, bs, sd, fin, -1, 0),
              "row_topk_merge": select,
              "kv_beam_reorder": lambda: ops.kv_beam_reorder(kc, vc, K, idx, fin, pos)}
        t = {k: [] for k in fs}
        for _ in range(rounds):
            for k, f in fs.items():
                t[k].append(timed(f, iters))
        torch.cuda.synchronize()
        assert int(fin.sum().item()) == 0, "a clip finished during the timing: later launches would have left at once"
        nbytes = 2.0 * (reads + writes) * L * Hk * ctx * d * 2
        row = {"rows": ROWS, "V": V, "num_beams": K, "own_slots": ctx, "layers_allocated": L, **{k: spread(v) for k, v in t.items()}}
        row["beam_step_us"] = round(row["row_topk_merge"]["median_us"] + row["kv_beam_reorder"]["median_us"], 1)
        row["beam_step_over_greedy_select"] = round(row["beam_step_us"] / row["greedy_select"]["median_us"], 2)
        row["reorder_bytes"] = nbytes
        row["reorder_TBps"] = round(nbytes / row["kv_beam_reorder"]["median_us"] / 1e6, 3)
        row["hbm_read_stream_TBps"] = HBM_READ_STREAM_TBPS
        print(json.dumps(row), flush=True)
        out.append(row)
    del kc, vc, logits
    torch.cuda.empty_cache()
    return out


def call_level(clips, new_tokens, prompt=830):
    from crab_amd.build_model import build_crab
    model = build_crab("llama", device=dev, visual=False, audio=False)
    eng = model.base_model.model._engine
    D = model.base_model.model.config.hidden_size
    g = torch.Generator(device=dev).manual_seed(2)
    emb = (torch.randn(clips, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
    wide = emb.repeat_interleave(K, 0)
    kw = dict(eos_token_id=None, pad_token_id=2)

    def run(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    fs = {"beam": lambda: eng.generate_beam(emb, K, new_tokens, **kw),
          "greedy_CK_rows": lambda: eng.generate(wide, new_tokens, **kw),
          "greedy_C_rows": lambda: eng.generate(emb, new_tokens, **kw)}
    t = {k: [] for k in fs}
    for r in range(3):                                           # round 0 is the warm-up: module load, graph capture
        for k, f in fs.items():
            s = run(f)
            if r:
                t[k].append(s)
    held = eng.shared_prefix_bytes(clips, prompt - 1, clips * K, 1, new_tokens)
    expanded = clips * K * eng.bytes_per_sequence(prompt, new_tokens)
    row = {"clips": clips, "num_beams": K, "prompt_rows": prompt, "new_tokens": new_tokens, **{k + "_s": [round(x, 3) for x in v] for k, v in t.items()},
           "beam_over_greedy_CK_rows": round(min(t["beam"]) / min(t["greedy_CK_rows"]), 3),
           "beam_over_greedy_C_rows": round(min(t["beam"]) / min(t["greedy_C_rows"]), 3),
           "device_bytes_beam_wave": held, "device_bytes_CK_sequences": expanded, "bytes_ratio": round(held / expanded, 3),
           "note": "decoder only (random embeddings in place of the encoders' output); the three calls share one engine, so every call re-captures its graph when the cache slot changes shape"}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_beam.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds, "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "beam_search.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-call" not in sys.argv:
        res["call"] = call_level(flag("--clips", 32), flag("--new-tokens", 64))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
