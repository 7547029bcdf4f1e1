"""Prompt-lookup speculative decoding, measured (GPU box; not a gate): writes profiles/prompt_lookup.json.
  (a) attention, one layer: crab_attn_verify at Sq = 4 / 8 / 16 queries of ONE sequence over 830 cached keys (+ the Sq appended ones), for
      Llama-2-7B heads (H = Hk = 32) and Qwen2-7B heads (H = 28, Hk = 4), d = 128, against Sq launches of crab_attn_decode (ctx = 831 + i) - what
      a verify step would cost without the kernel.  Each side is captured in a HIP graph (the Sq launches as ONE graph), as both would run inside a
      captured step: eager, the per-query side is bound by its Sq host launches, not by the kernel.  The eager times are reported beside them.
      Both sides run ALTERNATELY in this process, `rounds` rounds of `iters` launches each; the median round is reported with the spread (max - min over the rounds) and the algorithmic bytes (every visible K / V row once, q in, o out).
  (b) whole step: the verify step at k = 3 / 7 / 15 against the plain one-row decode step, full-size synthetic Llama decoder (encoders not built:
      the embeddings are random), B = 1, S = 830, each as its captured HIP graph, replayed alternately.  The plain step is the code the parent
      commit runs (generate() is untouched): it is the yardstick.  step_ratio = verify / plain is the worst-case slowdown (nothing ever accepted)
      and the divisor of the best-case speedup (k + 1 tokens per step).
  (c) whole calls at the two ends of the acceptance range: tokens / s of generate_lookup (k = 7) with crafted prompt_ids that make every draft
      right, and that make every draft wrong (tests/lookup_ref.py), against generate() on the same clip, alternated.  The model is random, so
      real acceptance rates are NOT measured here: they need trained weights and real prompts.
usage: bench_lookup.py [iters] [--rounds N] [--no-model] [--new-tokens N]"""
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
iters = int(args[0]) if args else 50
rounds = flag("--rounds", 5)
d = 128
KEYS = 830
dev = "cuda"
med = lambda ts: sorted(ts)[len(ts) // 2]


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


def graphed(f):
    """f captured as one HIP graph (warmed up on a side stream first) -> its replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f()
    return g.replay


def attention_level():
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: (torch.randn(*s, device=dev, generator=g) * 0.5).bfloat16()
    scale = d ** -0.5
    for name, H, Hk in (("llama", 32, 32), ("qwen", 28, 4)):
        for Sq in (4, 8, 16):
            Tmax = 896
            kc, vc = rn(1, Hk, Tmax, d), rn(1, Hk, Tmax, d)
            qkv = rn(Sq, (H + 2 * Hk) * d)
            o, o2 = torch.empty((Sq, H * d), device=dev, dtype=torch.bfloat16), torch.empty((Sq, H * d), device=dev, dtype=torch.bfloat16)
            ctx = KEYS + 1                                       # query 0 sees the 830 cached keys and its own

            def old():
                for i in range(Sq):
                    ops.attn_decode(qkv[i:i + 1], kc, vc, o[i:i + 1], 1, H, Hk, d, Tmax, ctx + i, scale)
            new = lambda: ops.attn_verify(qkv, kc, vc, o2, 1, Sq, H, Hk, d, Tmax, ctx, scale)
            old(); new(); torch.cuda.synchronize()
            diff = (o.float() - o2.float()).abs().max().item()
            g_old, g_new = graphed(old), graphed(new)
            t_old, t_new, e_old, e_new = [], [], [], []
            for _ in range(rounds):
                t_old.append(timed(g_old, iters)); t_new.append(timed(g_new, iters))
                e_old.append(timed(old, iters)); e_new.append(timed(new, iters))
            qo = 2.0 * Sq * H * d * 2
            b_old = sum(2.0 * (ctx + i) * Hk * d * 2 for i in range(Sq)) + qo
            b_new = 2.0 * (ctx + Sq - 1) * Hk * d * 2 * -(-Sq // max(1, 16 // (H // Hk))) + qo          # once per query group
            row = {"heads": name, "H": H, "Hk": Hk, "Sq": Sq, "cached_keys": KEYS,
                   "decode_x_Sq_us": round(med(t_old), 1), "decode_x_Sq_spread_us": round(max(t_old) - min(t_old), 1), "decode_x_Sq_bytes": b_old,
                   "verify_us": round(med(t_new), 1), "verify_spread_us": round(max(t_new) - min(t_new), 1), "verify_bytes": b_new,
                   "verify_GBps": round(b_new / med(t_new) / 1e3, 1), "time_ratio": round(med(t_new) / med(t_old), 3),
                   "timed_as": "one captured graph per side", "eager_decode_x_Sq_us": round(med(e_old), 1), "eager_verify_us": round(med(e_new), 1),
                   "max_abs_diff_of_the_outputs": diff}
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


def _reset(st, S):
    """Put a started state back at its first step (pos = S, step = 1, not finished): a timing window must not run a state past max_new_tokens."""
    st.pos_dev.fill_(S); st.step_dev.fill_(1); st.finished.zero_()
    if st.lookup is not None:
        st.lookup.hist[S + 1:].fill_(-1); st.lookup.stats.zero_()


def step_level(eng, D):
    from crab_amd.decoder import _Request, _ws_slot
    g = torch.Generator(device=dev).manual_seed(2)
    emb = (torch.randn(1, KEYS, D, device=dev, generator=g) * 0.5).bfloat16()
    max_new = 4 * iters + 64                                     # a window of `iters` replays (+ 3 warm-up) stays far below it, k + 1 tokens per replay included
    sides = {}
    with _ws_slot(0):
        st = eng._start(emb, _Request(max_new, pad_token_id=2))
        sides["plain"] = (st, eng._capture(st))
    for slot, k in enumerate((3, 7, 15), start=1):
        with _ws_slot(slot):
            st = eng._start(emb, _Request(16 * iters + 64, pad_token_id=2, lookup=(k, 2, False)), slot)
            st.lookup.hist[KEYS:KEYS + 1].copy_(st.out_ids[0, :1])
            sides[f"k{k}"] = (st, eng._capture(st))
    times = {n: [] for n in sides}
    for _ in range(rounds):
        for n, (st, graph) in sides.items():
            _reset(st, KEYS)
            times[n].append(timed(graph.replay, iters))
    plain = med(times["plain"])
    out = {"S": KEYS, "iters": iters, "rounds": rounds, "plain_step_us": round(plain, 1), "plain_step_spread_us": round(max(times["plain"]) - min(times["plain"]), 1)}
    for k in (3, 7, 15):
        t = times[f"k{k}"]
        out[f"k{k}"] = {"verify_step_us": round(med(t), 1), "verify_step_spread_us": round(max(t) - min(t), 1), "step_ratio": round(med(t) / plain, 3),
                        "best_case_speedup": round((k + 1) / (med(t) / plain), 2), "rows": k + 1}
    print(json.dumps(out), flush=True)
    for st, _ in sides.values():
        _reset(st, KEYS)
    return out


def call_level(eng, D, new_tokens, k=7):
    from tests import lookup_ref as R
    g = torch.Generator(device=dev).manual_seed(3)
    emb = (torch.randn(1, KEYS, D, device=dev, generator=g) * 0.5).bfloat16()
    kw = dict(eos_token_id=None, pad_token_id=2)
    plain_tape = eng.generate(emb, new_tokens, **kw)[0].tolist()
    # the tape the prompts are crafted from is the lookup path's own: a verify step always runs k + 1 rows through row-independent kernels, so what
    # it emits does not depend on the drafts - but on this random model (near-ties everywhere) it leaves the one-row path's ids at the first
    # sub-margin step, and prompts crafted from THAT tape would stop matching there
    tape = eng.generate_lookup(emb, new_tokens, k, max_ngram=2, prompt_ids=None, **kw)[0].tolist()
    differ = next((i for i, (a, b) in enumerate(zip(tape, plain_tape)) if a != b), None)
    V = eng.lm_head.weight.shape[0]
    w = next(t for t in range(3, V) if t not in tape)
    pad = lambda tail: [-1] * (KEYS - len(tail)) + tail
    prompts = {"all_right": pad(R.all_right_prompt(tape)), "all_wrong": pad(R.all_wrong_prompt(tape, w))}

    def run(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    sides = {"plain": lambda: eng.generate(emb, new_tokens, **kw), "prefill_and_first_token": lambda: eng.generate(emb, 1, **kw)}
    for n, p in prompts.items():
        sides[n] = (lambda p=p: eng.generate_lookup(emb, new_tokens, k, max_ngram=2, prompt_ids=p, return_stats=True, **kw))
    for f in sides.values():
        run(f)                                                   # warm-up: module load, graph capture
    ts, last = {n: [] for n in sides}, {}
    for _ in range(rounds):
        for n, f in sides.items():
            t, last[n] = run(f)
            ts[n].append(t)
    out = {"S": KEYS, "new_tokens": new_tokens, "num_draft_tokens": k, "max_ngram": 2, "rounds": rounds,
           "first_index_where_the_lookup_ids_leave_the_plain_ids": differ,
           "note": "decoder only, random weights: the two prompts are crafted ends of the acceptance range, not a measured acceptance rate; "
                   "whole calls, prefill of the 830 rows included (prefill_and_first_token: the same call with max_new_tokens = 1); "
                   "decode_tokens_per_s = (new_tokens - 1) / (call - prefill_and_first_token)"}
    pre = med(ts["prefill_and_first_token"])
    for n in sides:
        out[n] = {"s": [round(t, 4) for t in ts[n]]}
        if n == "prefill_and_first_token":
            continue
        out[n]["tokens_per_s"] = round(new_tokens / med(ts[n]), 1)
        out[n]["decode_tokens_per_s"] = round((new_tokens - 1) / (med(ts[n]) - pre), 1)
        if n != "plain":
            ids, st = last[n]
            out[n]["stats"] = st
            out[n]["ids_equal_the_tape"] = ids[0].tolist() == tape
            out[n]["simulated_stats"] = R.simulate(tape, prompts[n], k, 2, None, new_tokens)[1]
            out[n]["speedup_vs_plain"] = round(med(ts["plain"]) / med(ts[n]), 3)
            out[n]["decode_speedup_vs_plain"] = round((med(ts["plain"]) - pre) / (med(ts[n]) - pre), 3)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_lookup.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "shape": {"d": d, "cached_keys": KEYS, "iters": iters, "rounds": rounds},
           "attention": attention_level()}
    path = os.path.join(ROOT, "profiles", "prompt_lookup.json")
    json.dump(res, open(path, "w"), indent=1)
    if "--no-model" not in sys.argv:
        from crab_amd.build_model import build_crab
        model = build_crab("llama", device=dev, visual=False, audio=False)
        eng = model.base_model.model._engine
        D = model.base_model.model.config.hidden_size
        res["step"] = step_level(eng, D)
        json.dump(res, open(path, "w"), indent=1)
        res["call"] = call_level(eng, D, flag("--new-tokens", 128))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
