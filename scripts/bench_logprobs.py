"""Per-token log-probabilities of generated ids, measured (GPU box; not a gate): writes profiles/token_logprobs.json.
  kernel level: crab_logprob_norm (and crab_logprob_gather) next to crab_greedy_select on the same fp32 logits [512, 32000] and [512, 152064].  Both
      row kernels read every row once, so the select kernel of the same build is the yardstick; the bytes of the logits over the time give the
      achieved read rate.  The kernels run ALTERNATELY in this process, `rounds` rounds of `iters` launches each; median, min and max of the
      rounds are reported in us per launch.
  step level: one graph-replayed decode step of the full-size synthetic Llama decoder (encoders not built: the embeddings are random) with
      return_logprobs on and off at 1, 8 and 512 rows.  Both states are captured by ordinary generate() calls and kept; their graphs are then
      replayed alternately, `rounds` rounds of `steps` replays each, every round from the same position (the counters are put back first, so no
      replay appends past the cache).  The prompt is short (64 rows): the difference of the two steps does not depend on the context length.
usage: bench_logprobs.py [iters] [--no-step] [--rounds N] [--steps N] [--out PATH]"""
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


def kernel_level():
    out = []
    B = 512
    g = torch.Generator(device=dev).manual_seed(1)
    for V in (32000, 152064):
        logits = torch.randn(B, V, device=dev, generator=g) * 1.5
        cur = torch.zeros(B, dtype=torch.int64, device=dev)
        ids = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        fin = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.zeros(1, dtype=torch.int32, device=dev)
        norm = torch.zeros((B, 4), device=dev)
        lp = torch.zeros((2, B, 4), device=dev)
        fs = {"greedy_select": lambda: ops.greedy_select(logits, cur, ids, sd, fin, -1, PAD, 0),
              "logprob_norm": lambda: ops.logprob_norm(logits, sd, fin, EOS, 0, norm),
              "logprob_norm_eos_suppressed": lambda: ops.logprob_norm(logits, sd, fin, EOS, 2, norm),
              "logprob_gather": lambda: ops.logprob_gather(logits, cur, sd, norm, lp)}
        t = {k: [] for k in fs}
        for _ in range(rounds):
            for k, f in fs.items():
                t[k].append(timed(f, iters))
        row = {"B": B, "V": V, "logits_bytes": B * V * 4, **{k: spread(v) for k, v in t.items()}}
        row["norm_over_select"] = round(row["logprob_norm"]["median_us"] / row["greedy_select"]["median_us"], 3)
        row["norm_read_GBps"] = round(B * V * 4 / row["logprob_norm"]["median_us"] / 1e3, 1)
        row["select_read_GBps"] = round(B * V * 4 / row["greedy_select"]["median_us"] / 1e3, 1)
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
    for B in (1, 8, 512):
        g = torch.Generator(device=dev).manual_seed(2 + B)
        emb = (torch.randn(B, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
        states = {}
        for name, on in (("off", False), ("on", True)):
            eng.generate(emb, new_tokens, eos_token_id=None, pad_token_id=PAD, return_logprobs=on)
            st = eng._dec[0]
            assert st.graph is not None and (st.lp is not None) == on
            states[name] = st                                  # the reference keeps the state's buffers and its graph alive

        def round_of(st):
            # back to the position after the first token: `steps` replays stay inside the cache and the [B, new_tokens] buffers
            st.pos_dev.fill_(prompt); st.step_dev.fill_(1); st.finished.zero_()
            return timed(st.graph.replay, steps, warm=2)
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for name in ("off", "on"):
                t[name].append(round_of(states[name]))
        row = {"rows": B, "prompt_rows": prompt, "replays_per_round": steps, "off": spread(t["off"]), "on": spread(t["on"])}
        row["delta_us"] = round(row["on"]["median_us"] - row["off"]["median_us"], 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del states, emb
        eng.invalidate()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_logprobs.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds, "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "token_logprobs.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-step" not in sys.argv:
        res["step"] = step_level(flag("--steps", 100))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
