"""Plain CPU reference of constrained (closed-set) decoding over a crab_amd.constrain.TokenTrie - or anything with its CSR arrays edge_off /
edge_tok / edge_dst (numpy int32).  Greedy: the allowed token with the largest logit, on equal values the lowest id (the first-maximum rule of
crab_greedy_select); EOS is not allowed while step < min_new; a finished row emits pad and keeps its node; a row with nothing allowed emits pad and
finishes.  A node outside [0, n_nodes) and an edge token outside [0, V) count as "not allowed"."""
import numpy as np
import torch


def allowed_tokens(trie, node: int, V: int, step: int, eos: int, min_new: int):
    """[(token, destination node)] allowed at `node`, in edge order."""
    n_nodes = len(trie.edge_off) - 1
    if not 0 <= node < n_nodes:
        return []
    out = []
    for e in range(int(trie.edge_off[node]), int(trie.edge_off[node + 1])):
        t = int(trie.edge_tok[e])
        if 0 <= t < V and not (t == eos and step < min_new):
            out.append((t, int(trie.edge_dst[e])))
    return out


def allowed_mask(trie, nodes, V: int, step: int, eos: int, min_new: int) -> torch.Tensor:
    """bool [B, V]: the allowed tokens of every row (what HF's processors leave finite)."""
    m = torch.zeros((len(nodes), V), dtype=torch.bool)
    for b, n in enumerate(nodes):
        for t, _ in allowed_tokens(trie, int(n), V, step, eos, min_new):
            m[b, t] = True
    return m


def select_step(logits: torch.Tensor, trie, nodes, finished, step: int, eos: int, pad: int, min_new: int):
    """One greedy constrained step.  logits [B, V] fp32 (CPU); nodes / finished: sequences of B ints.  Returns (tokens, nodes, finished) lists."""
    B, V = logits.shape
    toks, nn, ff = [], list(int(n) for n in nodes), list(int(f) for f in finished)
    for b in range(B):
        if ff[b]:
            toks.append(pad)
            continue
        al = allowed_tokens(trie, nn[b], V, step, eos, min_new)
        if not al:
            toks.append(pad); ff[b] = 1
            continue
        best = None
        for t, d in al:                                        # ascending ids: strict > keeps the first maximum
            v = float(logits[b, t])
            if best is None or v > best[0]:
                best = (v, t, d)
        toks.append(best[1]); nn[b] = best[2]
        if best[1] == eos:
            ff[b] = 1
    return toks, nn, ff


def walk_greedy(step_logits: torch.Tensor, trie, set_of, eos: int, pad: int, min_new: int = 0):
    """Greedy constrained decoding walked over recorded per-step logits [B, n, V]: ids [B, n] (int64) and the final nodes.  Meaningful as
    long as the logits were produced along these very ids (the engine's return_step_logits of the same call)."""
    lg = step_logits.float().cpu()
    B, n, V = lg.shape
    nodes = [int(trie.roots[s]) for s in set_of]
    fin = [0] * B
    ids = torch.full((B, n), pad, dtype=torch.int64)
    for step in range(n):
        toks, nodes, fin = select_step(lg[:, step], trie, nodes, fin, step, eos, pad, min_new)
        ids[:, step] = torch.tensor(toks)
    return ids, nodes


def cut_at_eos(row, eos: int):
    row = [int(t) for t in row]
    return row[:row.index(eos)] if eos in row else row


def random_sets(rng: np.random.Generator, n_sets: int, V: int, eos: int, n_seqs=(3, 9), length=(1, 4), lo: int = 3):
    """n_sets random answer sets over the ids [lo, V) without eos, with shared prefixes (a small alphabet per position)."""
    alphabet = [t for t in rng.permutation(np.arange(lo, V))[:12].tolist() if t != eos]
    sets = []
    for _ in range(n_sets):
        seqs = []
        for _ in range(int(rng.integers(n_seqs[0], n_seqs[1] + 1))):
            seqs.append([int(rng.choice(alphabet)) for _ in range(int(rng.integers(length[0], length[1] + 1)))])
        sets.append(seqs)
    return sets
