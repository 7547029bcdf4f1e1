"""The logits processors of the decode step, measured (GPU box; not a gate): writes profiles/logits_processors.json.
  kernel level: the crab_logits_edit + crab_logits_restore PAIR next to crab_greedy_select alone on the same fp32 logits [512, 32000] and
      [512, 152064], at step 255 of 256 (the longest history the usual max_new_tokens gives) with repetition_penalty 1.1, no_repeat_ngram_size 3
      and one further stop id.  The select reads every row once; the pair touches a few hundred words of it.  The launches run ALTERNATELY in
      this process, `rounds` rounds of `iters` launches each; median, min and max of the rounds are reported in us per launch.
  step level: one graph-replayed decode step of the full-size synthetic Llama decoder (encoders not built: the embeddings are random) with
      processors on and off at 1, 8 and 512 rows.  Both states are captured by ordinary generate() calls and kept; their graphs are then
      replayed alternately, `rounds` rounds of `steps` replays each, every round from the same position (step 150 of 260: the counters are put
      back first, so no replay appends past the cache and every round edits histories of 150 - 250 tokens).
usage: bench_logits_proc.py [iters] [--no-step] [--rounds N] [--steps N] [--out PATH]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crab_amd import ops

args = [a for a in sys.argv[1:] if not a.startswith("--") and not (sys.argv[sys.argv.index(a) - 1] in ("--rounds", "--steps", "--out"))]
flag = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 50
rounds = flag("--rounds", 5)
dev = "cuda"
EOS, PAD = 2, 0


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


PROC = (1.1, 3, (7,))                                            # repetition_penalty, no_repeat_ngram_size, stop_token_ids


def kernel_level():
    out = []
    B, n_steps, step = 512, 256, 255
    g = torch.Generator(device=dev).manual_seed(1)
    for V in (32000, 152064):
        logits = torch.randn(B, V, device=dev, generator=g) * 1.5
        cur = torch.zeros(B, dtype=torch.int64, device=dev)
        ids = torch.randint(0, 400, (B, n_steps), dtype=torch.int64, device=dev, generator=g)      # 400 distinct ids over 255 tokens: duplicates and repeated bigrams
        scratch_ids = torch.zeros((B, n_steps), dtype=torch.int64, device=dev)
        fin = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.full((1,), step, dtype=torch.int32, device=dev)
        stops = torch.tensor(PROC[2], dtype=torch.int32, device=dev)
        n_slots = 2 * n_steps + len(PROC[2])
        si = torch.full((B, n_slots), -1, dtype=torch.int32, device=dev)
        sv = torch.zeros((B, n_slots), device=dev)

        def pair():
            ops.logits_edit(logits, ids, sd, fin, PROC[0], PROC[1], stops, 0, si, sv)
            ops.logits_restore(logits, cur, fin, stops, si, sv)

        fs = {"greedy_select": lambda: ops.greedy_select(logits, cur, scratch_ids, sd, fin, -1, PAD, 0),
              "edit_restore_pair": pair,
              "logits_restore": lambda: ops.logits_restore(logits, cur, fin, stops, si, sv)}      # after a pair: the same slots written back once more
        raw = logits.clone()
        t = {k: [] for k in fs}
        for _ in range(rounds):
            for k, f in fs.items():
                t[k].append(timed(f, iters))
        # every edit above was followed by its restore, so the rows are still the random input, bit for bit
        torch.cuda.synchronize()
        assert torch.equal(logits, raw), "the edit + restore pair did not give the raw bits back"
        del raw
        edited = int((si >= 0).sum().item())
        row = {"B": B, "V": V, "step": step, "n_steps": n_steps, "processors": list(PROC[:2]) + [list(PROC[2])], "edited_columns_per_row": round(edited / B, 1),
               **{k: spread(v) for k, v in t.items()}}
        row["pair_over_select"] = round(row["edit_restore_pair"]["median_us"] / row["greedy_select"]["median_us"], 3)
        print(json.dumps(row), flush=True)
        out.append(row)
        del logits
        torch.cuda.empty_cache()
    return out


def step_level(steps, prompt=64, new_tokens=260, first=150):
    from crab_amd.build_model import build_crab
    assert first + steps + 2 < new_tokens, "a round must end before the last column of the state's buffers"
    um = build_crab("llama", device=dev, visual=False, audio=False).base_model.model
    eng = um._engine
    D = um.config.hidden_size
    out = []
    for B in (1, 8, 512):
        g = torch.Generator(device=dev).manual_seed(2 + B)
        emb = (torch.randn(B, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
        states = {}
        for name, proc in (("off", None), ("on", PROC)):
            eng.generate(emb, new_tokens, eos_token_id=None, pad_token_id=PAD, processors=proc)
            st = eng._dec[0]
            assert st.graph is not None and (st.proc is not None) == (proc is not None)
            states[name] = st                                  # the reference keeps the state's buffers and its graph alive

        def round_of(st):
            # back to step `first`: `steps` replays stay inside the cache and the [B, new_tokens] buffers; the history is what generate() left
            st.pos_dev.fill_(prompt + first - 1); st.step_dev.fill_(first); st.finished.zero_()
            return timed(st.graph.replay, steps, warm=2)
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for name in ("off", "on"):
                t[name].append(round_of(states[name]))
        row = {"rows": B, "prompt_rows": prompt, "first_step": first, "replays_per_round": steps, "off": spread(t["off"]), "on": spread(t["on"])}
        row["delta_us"] = round(row["on"]["median_us"] - row["off"]["median_us"], 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del states, emb
        eng.invalidate()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_logits_proc.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds, "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "logits_processors.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-step" not in sys.argv:
        res["step"] = step_level(flag("--steps", 90))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
