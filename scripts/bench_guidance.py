"""Classifier-free guidance in the decode step (generate(guidance_scale=...)), measured (GPU box; not a gate): writes profiles/guidance.json.
  kernel level: crab_cfg_mix + crab_cfg_follow next to crab_greedy_select and crab_logprob_norm on fp32 logits of 512 rows (256 pairs) at
      V = 32000 and 152064.  The mix reads two rows twice and writes one row once: its byte model is 5 V 4 bytes per pair, and the achieved
      rate against it stands beside the read rate of crab_logprob_norm (one pass over the same 512 rows) from the same run.  A guided step
      runs the select on the 256 guided rows only, so that launch is timed as well.  The kernels run ALTERNATELY in this process, `rounds`
      rounds of `iters` launches each; median, min and max of the rounds are reported in us per launch.
  step level: one graph-replayed decode step of the full-size synthetic Llama decoder (encoders not built: the embeddings are random) at 2,
      16 and 512 rows, as a guided wave of rows / 2 pairs (on) and as the same two groups coalesced without guidance (off:
      generate_many(coalesce=True), the same ragged state and the same kernels but for the select).  Both states are captured by ordinary
      calls and kept; their graphs are replayed alternately, `rounds` rounds of `steps` replays each, every round from the same position.
      Both prompts are short (64 and 32 rows): the difference of the two steps does not depend on the context length.
usage: bench_guidance.py [iters] [--no-step] [--rounds N] [--steps N] [--out PATH]"""
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
SCALE = 1.5


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
    rows = 512
    B = rows // 2
    g = torch.Generator(device=dev).manual_seed(1)
    for V in (32000, 152064):
        logits = torch.randn(rows, V, device=dev, generator=g) * 1.5
        guided = torch.empty((B, V), device=dev)
        cur = torch.zeros(rows, dtype=torch.int64, device=dev)
        ids = torch.zeros((rows, 4), dtype=torch.int64, device=dev)
        fin = torch.zeros(rows, dtype=torch.int32, device=dev)
        sd = torch.zeros(1, dtype=torch.int32, device=dev)
        norm = torch.zeros((rows, 4), device=dev)

        def mix_follow():
            ops.cfg_mix(logits, guided, B, SCALE, fin)
            ops.cfg_follow(cur, ids, fin, sd, B)

        fs = {"greedy_select": lambda: ops.greedy_select(logits, cur, ids, sd, fin, -1, PAD, 0),
              "greedy_select_guided_rows": lambda: ops.greedy_select(guided, cur, ids, sd, fin, -1, PAD, 0),
              "logprob_norm": lambda: ops.logprob_norm(logits, sd, fin, EOS, 0, norm),
              "cfg_mix": lambda: ops.cfg_mix(logits, guided, B, SCALE, fin),
              "cfg_follow": lambda: ops.cfg_follow(cur, ids, fin, sd, B),
              "cfg_mix_follow": mix_follow}
        t = {k: [] for k in fs}
        for _ in range(rounds):
            for k, f in fs.items():
                t[k].append(timed(f, iters))
        model_bytes = B * 5 * V * 4
        row = {"rows": rows, "pairs": B, "V": V, "mix_model_bytes": model_bytes, "logits_bytes": rows * V * 4, **{k: spread(v) for k, v in t.items()}}
        row["mix_follow_over_select"] = round(row["cfg_mix_follow"]["median_us"] / row["greedy_select"]["median_us"], 3)
        row["mix_follow_over_norm"] = round(row["cfg_mix_follow"]["median_us"] / row["logprob_norm"]["median_us"], 3)
        row["mix_model_GBps"] = round(model_bytes / row["cfg_mix"]["median_us"] / 1e3, 1)
        row["norm_read_GBps"] = round(rows * V * 4 / row["logprob_norm"]["median_us"] / 1e3, 1)
        row["select_read_GBps"] = round(rows * V * 4 / row["greedy_select"]["median_us"] / 1e3, 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del logits, guided
        torch.cuda.empty_cache()
    return out


def step_level(steps, prompt=64, negative=32, new_tokens=130):
    from crab_amd.build_model import build_crab
    assert steps + 2 < new_tokens, "a round must end before the last column of the state's buffers"
    um = build_crab("llama", device=dev, visual=False, audio=False).base_model.model
    eng = um._engine
    D = um.config.hidden_size
    out = []
    for rows in (2, 16, 512):
        B = rows // 2
        g = torch.Generator(device=dev).manual_seed(2 + rows)
        emb = (torch.randn(B, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
        neg = (torch.randn(B, negative, D, device=dev, generator=g) * 0.5).bfloat16()
        states = {}
        for name in ("off", "on"):
            if name == "on":
                eng.generate_guided(emb, neg, SCALE, new_tokens, eos_token_id=None, pad_token_id=PAD)
            else:
                eng.generate_many([emb, neg], new_tokens, eos_token_id=None, pad_token_id=PAD, coalesce=True)
            st = eng._dec[0]
            assert st.graph is not None and st.B == rows and (st.cfg is not None) == (name == "on") and st.row_off is not None
            states[name] = st                                  # the reference keeps the state's buffers and its graph alive

        def round_of(st):
            # back to the position after the first token: `steps` replays stay inside the cache and the [rows, new_tokens] buffers
            st.pos_dev.fill_(prompt); st.step_dev.fill_(1); st.finished.zero_()
            return timed(st.graph.replay, steps, warm=2)
        t = {"off": [], "on": []}
        for _ in range(rounds):
            for name in ("off", "on"):
                t[name].append(round_of(states[name]))
        row = {"rows": rows, "pairs": B, "prompt_rows": prompt, "negative_rows": negative, "replays_per_round": steps, "off": spread(t["off"]),
               "on": spread(t["on"])}
        row["delta_us"] = round(row["on"]["median_us"] - row["off"]["median_us"], 1)
        print(json.dumps(row), flush=True)
        out.append(row)
        del states, emb, neg
        eng.invalidate()
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_guidance.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "rounds": rounds, "guidance_scale": SCALE, "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "guidance.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-step" not in sys.argv:
        res["step"] = step_level(flag("--steps", 100))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
