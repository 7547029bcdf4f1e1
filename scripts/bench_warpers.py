"""The sample-mode truncation warpers of the decode step (generate(do_sample=True, min_p / epsilon_cutoff / eta_cutoff)), measured (GPU box;
not a gate): writes profiles/sampling_warpers.json.
  kernel level: crab_sample_select_warped with all three stages live next to crab_sample_select on fp32 logits of 512 rows at V = 32000 and
      152064, both behind the reference's sampling defaults (temperature 0.6, top_k 50, top_p 0.9) and behind no top-k / top-p at all (the
      stages then run over the whole row).  The warped kernel with its stages off is timed too: the same operations as crab_sample_select.
      The kernels run ALTERNATELY in this process, `rounds` rounds of `iters` launches each; median, min and max of the rounds are
      reported in us per launch.
  step level: one graph-replayed decode step of the full-size synthetic Llama decoder (encoders not built: the embeddings are random) at 1, 8
      and 512 rows in sample mode with the warpers off (crab_sample_select) and on (crab_sample_select_warped) - the same state but for the
      select.  Both states are captured by ordinary calls and kept; their graphs are replayed alternately, `rounds` rounds of `steps`
      replays each, every round from the same position.
usage: bench_warpers.py [iters] [--no-step] [--rounds N] [--steps N] [--out PATH]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crab_amd import ops

args = [a for a in sys.argv[1:] if not a.startswith("--") and not (sys.argv[sys.argv.index(a) - 1] in ("--rounds", "--steps", "--out"))]
flag = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 20
rounds = flag("--rounds", 3)
dev = "cuda"
PAD = 0
SAMPLING = (0.6, 50, 0.9, 1234)                  # the reference's defaults (Llama-2-chat generation_config + GenerationConfig's top_k)
WARP = (0.05, 3e-4, 2e-3)                        # min_p, epsilon_cutoff, eta_cutoff: all three live


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
    rows = 512
    g = torch.Generator(device=dev).manual_seed(1)
    for V in (32000, 152064):
        logits = torch.randn(rows, V, device=dev, generator=g) * 1.5
        cur = torch.zeros(rows, dtype=torch.int64, device=dev)
        ids = torch.zeros((rows, 4), dtype=torch.int64, device=dev)
        fin = torch.zeros(rows, dtype=torch.int32, device=dev)
        sd = torch.zeros(1, dtype=torch.int32, device=dev)
        for front, (t, k, p, seed) in (("defaults", SAMPLING), ("no_topk_topp", (0.6, 0, 1.0, 1234))):
            fs = {"sample_select": lambda: ops.sample_select(logits, cur, ids, sd, fin, -1, PAD, 0, t, k, p, seed),
                  "warped_stages_off": lambda: ops.sample_select_warped(logits, cur, ids, sd, fin, -1, PAD, 0, t, k, p, seed),
                  "warped_all_live": lambda: ops.sample_select_warped(logits, cur, ids, sd, fin, -1, PAD, 0, t, k, p, seed, *WARP)}
            tm = {name: [] for name in fs}
            for _ in range(rounds):
                for name, f in fs.items():
                    tm[name].append(timed(f, iters))
            row = {"rows": rows, "V": V, "front": front, "temperature": t, "top_k": k, "top_p": p, "min_p": WARP[0], "epsilon_cutoff": WARP[1],
                   "eta_cutoff": WARP[2], **{name: spread(v) for name, v in tm.items()}}
            row["live_over_sample_select"] = round(row["warped_all_live"]["median_us"] / row["sample_select"]["median_us"], 4)
            row["off_over_sample_select"] = round(row["warped_stages_off"]["median_us"] / row["sample_select"]["median_us"], 4)
            print(json.dumps(row), flush=True)
            out.append(row)
        del logits
        torch.cuda.empty_cache()
    return out


def step_level(steps, prompt=64, new_tokens=130):
    from crab_amd.build_model import build_crab
    assert steps + 2 < new_tokens, "a round must end before the last column of the state's buffers"
    um = build_crab("llama", device=dev, visual=False, audio=False).base_model.model
    eng = um._engine
    D = um.config.hidden_size
    out = []
    for rows in (1, 8, 512):
        g = torch.Generator(device=dev).manual_seed(2 + rows)
        emb = (torch.randn(rows, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
        states = {}
        for name in ("off", "on"):
            eng.generate(emb, new_tokens, eos_token_id=None, pad_token_id=PAD, sampling=SAMPLING + (WARP if name == "on" else ()))
            st = eng._dec[0]
            assert st.graph is not None and st.B == rows and (len(st.sampling) == 7) == (name == "on")
            states[name] = st                                  # the reference keeps the state's buffers and its graph alive

        def round_of(st):
            # back to the position after the first token: `steps` replays stay inside the cache and the [rows, new_tokens] buffers
            st.pos_dev.fill_(prompt); st.step_dev.fill_(1); st.finished.zero_()
            return timed(st.graph.replay, steps, warm=2)
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for name in ("off", "on"):
                t[name].append(round_of(states[name]))
        row = {"rows": rows, "prompt_rows": prompt, "replays_per_round": steps, "off": spread(t["off"]), "on": spread(t["on"])}
        row["delta_us"] = round(row["on"]["median_us"] - row["off"]["median_us"], 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del states, emb
        eng.invalidate()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_warpers.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds, "sampling": list(SAMPLING), "warpers": list(WARP),
           "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "sampling_warpers.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-step" not in sys.argv:
        res["step"] = step_level(flag("--steps", 50))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
