"""Constrained (closed-set) selection, measured (GPU box; not a gate): writes profiles/constrained_decode.json.
  kernel level: crab_constrained_select against crab_greedy_select and crab_sample_select at B = 512 rows, V = 32000 and 152064, every row on a node
      with 1, 42 or 1000 edges; greedy and sample mode (temperature 0.6, top_k 50, top_p 0.9).  The kernels run ALTERNATELY in this process, three
      rounds of `iters` launches each, the median round is reported in us per launch.  Expectation from the bytes read alone: a select that gathers
      at most `edges` values should not be slower than one that scans V.
  call level: generate() on the full-size synthetic Llama decoder (encoders not built: the embeddings are random) for 64 clips, max_new_tokens = 32,
      with a 42-answer set of 1-3 tokens against the same call unconstrained, alternated, 2 rounds.
usage: bench_constrained.py [iters] [--no-call] [--clips N] [--prompt N] [--out PATH]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from crab_amd import ops
from crab_amd.constrain import TokenTrie

args = [a for a in sys.argv[1:] if not a.startswith("--") and not (sys.argv[sys.argv.index(a) - 1] in ("--clips", "--prompt", "--out"))]
flag = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
iters = int(args[0]) if args else 50
dev = "cuda"
B = 512
EOS, PAD = 2, 0


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
    for V in (32000, 152064):
        logits = torch.randn(B, V, device=dev, generator=g) * 1.5
        cur = torch.zeros(B, dtype=torch.int64, device=dev)
        ids = torch.zeros((B, 4), dtype=torch.int64, device=dev)
        fin = torch.zeros(B, dtype=torch.int32, device=dev)
        sd = torch.zeros(1, dtype=torch.int32, device=dev)
        samp = (0.6, 50, 0.9, 1234)
        greedy = lambda: (fin.zero_(), ops.greedy_select(logits, cur, ids, sd, fin, EOS, PAD, 0))
        sample = lambda: (fin.zero_(), ops.sample_select(logits, cur, ids, sd, fin, EOS, PAD, 0, *samp))
        for edges in (1, 42, 1000):
            rng = np.random.default_rng(edges)
            toks = (3 + rng.permutation(V - 3)[:edges]).tolist()
            trie = TokenTrie([[[t] for t in toks]], V, EOS)
            up = lambda a: torch.from_numpy(a.copy()).to(dev)
            eo, et, ed = up(trie.edge_off), up(trie.edge_tok), up(trie.edge_dst)
            root = torch.full((B,), int(trie.roots[0]), dtype=torch.int32, device=dev)
            node = root.clone()
            cg = lambda: (fin.zero_(), node.copy_(root), ops.constrained_select(logits, eo, et, ed, node, cur, ids, sd, fin, EOS, PAD, 0))
            cs = lambda: (fin.zero_(), node.copy_(root), ops.constrained_select(logits, eo, et, ed, node, cur, ids, sd, fin, EOS, PAD, 0, *samp))
            reset = lambda: (fin.zero_(), node.copy_(root))      # the two small fills the constrained timings carry
            t = {k: [] for k in ("greedy", "sample", "constrained_greedy", "constrained_sample", "reset")}
            for _ in range(3):
                for k, f in (("greedy", greedy), ("constrained_greedy", cg), ("sample", sample), ("constrained_sample", cs), ("reset", reset)):
                    t[k].append(timed(f, iters))
            med = {k: sorted(v)[1] for k, v in t.items()}
            row = {"B": B, "V": V, "edges": edges, **{k + "_us": round(v, 1) for k, v in med.items()},
                   "rounds_us": {k: [round(x, 1) for x in v] for k, v in t.items()},
                   "greedy_ratio": round(med["constrained_greedy"] / med["greedy"], 3), "sample_ratio": round(med["constrained_sample"] / med["sample"], 3),
                   "note": "every timing includes a fill of the finished flags; the constrained ones also the node reset (reset_us: both fills alone)"}
            print(json.dumps(row), flush=True)
            out.append(row)
        del logits
        torch.cuda.empty_cache()
    return out


def call_level(clips, prompt, new_tokens=32):
    from crab_amd.build_model import build_crab
    model = build_crab("llama", device=dev, visual=False, audio=False)
    um = model.base_model.model
    eng = um._engine
    D, V = um.config.hidden_size, um.lm_head.weight.shape[0]
    g = torch.Generator(device=dev).manual_seed(2)
    emb = (torch.randn(clips, prompt, D, device=dev, generator=g) * 0.5).bfloat16()
    rng = np.random.default_rng(3)
    answers = [[int(t) for t in rng.integers(3, V, int(rng.integers(1, 4)))] for _ in range(42)]
    trie = TokenTrie([answers], V, EOS)
    kw = dict(eos_token_id=EOS, pad_token_id=PAD)
    shapes = {}

    def run(f, name):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        shapes[name] = int(r.shape[1])
        return time.perf_counter() - t0
    free = lambda: eng.generate(emb, new_tokens, **kw)
    cons = lambda: eng.generate(emb, new_tokens, constraint=(trie, None), **kw)
    run(free, "free"); run(cons, "constrained")                  # warm-up: module load, graph capture
    t_free, t_cons = [], []
    for _ in range(2):
        t_free.append(run(free, "free")); t_cons.append(run(cons, "constrained"))
    from crab_amd.decoder import EOS_CHECK_EVERY
    row = {"clips": clips, "prompt_rows": prompt, "max_new_tokens": new_tokens, "answers": 42, "answer_tokens": "1-3",
           "unconstrained_s": [round(t, 3) for t in t_free], "constrained_s": [round(t, 3) for t in t_cons],
           "unconstrained_ids_per_row": shapes["free"], "constrained_ids_per_row": shapes["constrained"],
           "unconstrained_clips_per_s": round(clips / min(t_free), 2), "constrained_clips_per_s": round(clips / min(t_cons), 2),
           "note": f"decoder only (random embeddings in place of the encoders' output; the prefill is in both numbers).  The step loop reads the finished "
                   f"flags every {EOS_CHECK_EVERY} steps: a constrained call whose rows all finish within 4 tokens still runs {EOS_CHECK_EVERY} decode steps"}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_constrained.py measures on the GPU; there is nothing to report without one"
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "kernel": kernel_level()}
    path = flag("--out", os.path.join(ROOT, "profiles", "constrained_decode.json"))
    json.dump(res, open(path, "w"), indent=1)
    if "--no-call" not in sys.argv:
        res["call"] = call_level(flag("--clips", 64), flag("--prompt", 702))
        json.dump(res, open(path, "w"), indent=1)
    print("wrote", path)
