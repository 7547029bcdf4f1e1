"""One decode step's select chain as ONE CPU reference, composed of the references every link already has - nothing is restated here:

    logprob_norm -> logits_edit -> {greedy | sample | constrained}_select -> logits_restore -> logprob_gather -> advance
    (GenerationEngine._select, crab_amd/decoder.py)

    tests/logits_proc_ref.py   edit / finished_after          what logits_edit writes and logits_restore marks
    tests/constrain_ref.py     allowed_tokens / select_step   the trie: what is allowed at a node, the greedy choice, the node that follows
    tests/logprob_ref.py       allowed_rows / step_ref        both log-probability planes of the RAW row, with their fp32 bounds
    oracle.crab_oracle.sampling_probs                         HF's temperature -> top-k -> top-p order (kept_classes follows it in fp64)

What the chain has to get right and no single reference states: the select chooses from the EDITED row (restricted to the trie's edges, EOS
suppressed while step < min_new), both log-probability planes are taken from the RAW row with the finished flags and the node of BEFORE the
step, a row is finished after the step by the select's own EOS, by any stop id or by a trie node with nothing allowed, a finished row emits
pad and is not edited, and the node follows the chosen edge.

The sampled modes cannot be held to one id by a CPU reference (the draw's partial sums are fp32 in a fixed tree), so they are held to the
KEPT SET: every token of the row is `KEEP`, `DROP` or `EITHER`, and a drawn id must not be `DROP`.

The margin of `EITHER` - derived from the kernel's arithmetic (csrc/sample.hip, csrc/constrain.hip), never measured from it.  u = 2^-24 is
the unit roundoff of fp32, X the largest finite |logit / temperature| of the row's allowed tokens, c = ceil(n / 1024) the tokens one of the
1024 threads owns (n = V, or the node's edge count under a trie):

    the scaled logit          x~ = fl(z * fl(1 / T))            two roundings: |x~ - z / T| <= 2 u X                   (top-k ties: rel. 4 u)
    one term                  __expf(x~ - mx~)                  argument: 2 u X (x~) + 2 u X (mx~) + u |d| (the subtraction), |d| <= 2 X;
                                                                __expf = exp2(d * log2 e): the product rounds (u |d|), v_exp_f32 1 ulp (2 u)
                                                                => relative error of a term <= (4 X + 2 X + 2 X + 3) u = (8 X + 3) u
    one thread's serial sum   at most c terms                   (c - 1) u
    the fixed 1024-way tree   6 shuffle levels, 15 serial adds  21 u
    a mass (numerator, or Z)  relative error                    <= (8 X + 3 + c + 20) u
    the comparison            m >= fl(top_p * Z)                two masses, the product's rounding, top_p stored as fp32

    margin = (2 * (8 X + c + 23) + 2) * u        on the fraction m / Z <= 1 (so relative and absolute error coincide)

A token whose fraction of strictly larger mass lies within `margin` of top_p is `EITHER`; so is one whose scaled logit lies within 4 u
(relative) of the k-th largest.  A top-k boundary that is `EITHER` moves Z by that token's mass: the nucleus is then classified against the
smallest and the largest Z the kernel can have formed.  margin = 0 gives exactly the kept set of sampling_probs on tie-free rows."""
import math
import types

import torch

from tests import constrain_ref as C
from tests import logits_proc_ref as P
from tests import logprob_ref as L

U = 2.0 ** -24
DROP, KEEP, EITHER = 0, 1, 2


class Opts:
    """The options of one call.  eos < 0: none.  sampling: (temperature, top_k, top_p) or None = greedy.  trie: a crab_amd.constrain.TokenTrie
    (or anything with its CSR arrays); set_of: the answer set of every row (walk puts the rows on trie.roots[set_of[b]])."""

    def __init__(self, eos=-1, pad=0, min_new=0, penalty=1.0, ngram=0, stops=(), sampling=None, trie=None, set_of=None):
        self.eos, self.pad, self.min_new = (-1 if eos is None else int(eos)), int(pad), int(min_new)
        self.penalty, self.ngram, self.stops = float(penalty), int(ngram), tuple(int(e) for e in stops)
        self.sampling = None if sampling is None else (float(sampling[0]), int(sampling[1]), float(sampling[2]))
        self.trie, self.set_of = trie, set_of

    @property
    def params(self):
        return P.Params(self.penalty, self.ngram, self.stops, self.min_new)

    @property
    def neutral(self):
        return self.penalty == 1.0 and self.ngram == 0 and not self.stops


def margin(X: float, n: int) -> float:
    """The derived margin (module docstring) for a row with largest finite |scaled logit| X and n tokens (or edges) to choose from."""
    return (2.0 * (8.0 * X + -(-n // 1024) + 23.0) + 2.0) * U


def kept_classes(row: torch.Tensor, allowed: torch.Tensor, sampling, exact: bool = False):
    """row [V] fp32: the row the select chooses from; allowed [V] bool.  -> (int8 [V] of DROP / KEEP / EITHER, the margin used).
    fp64 throughout, HF's order: temperature -> top-k (ties with the k-th kept) -> top-p (token kept iff the mass of the strictly larger ones is
    < top_p).  exact: margin 0 everywhere."""
    t, k, top_p = sampling
    top_p = float(torch.tensor(top_p, dtype=torch.float32))     # the kernel's argument is a float
    V = row.shape[0]
    cls = torch.zeros(V, dtype=torch.int8)
    x = row.double() / t
    n_choose = int(allowed.sum())
    idx = torch.nonzero(allowed & torch.isfinite(x))[:, 0]       # a banned token (-inf) has no mass: DROP
    if idx.numel() == 0:
        cls[allowed] = EITHER                                    # no mass at all: the kernels fall back to an allowed token
        return cls, 0.0
    xs = x[idx]
    m = 0.0 if exact else margin(float(xs.abs().max()), n_choose)
    rel = 0.0 if exact else 4.0 * U
    # ---- top-k over everything the kernel counts (banned tokens at -inf count as the smallest values)
    in_k = torch.ones_like(xs, dtype=torch.bool)
    amb_k = torch.zeros_like(in_k)
    if 0 < k < n_choose and k <= xs.numel():
        kth = torch.topk(xs, k).values[-1]
        tol = rel * torch.maximum(xs.abs(), kth.abs())
        in_k = xs >= kth - tol
        near = (xs - kth).abs() <= tol
        above = int((xs > kth + tol).sum())
        if above + int(near.sum()) != k and not bool((xs[near] == kth).all()):
            amb_k = near                                         # more candidates than places left: any of them may be in or out
    sure = in_k & ~amb_k
    w = torch.exp(xs - xs.max())
    z_lo, z_hi = w[sure].sum(), w[in_k].sum()
    if float(z_lo) == 0.0:
        z_lo = z_hi
    # ---- top-p: mass of the strictly larger tokens of the top-k set (the ambiguous ones counted in for `num_hi`, out for `num_lo`)
    order = torch.argsort(xs, descending=True, stable=True)
    xo, wo, so, io = xs[order], w[order], sure[order], in_k[order]
    cum_hi = torch.cumsum(wo * io, 0)
    cum_lo = torch.cumsum(wo * so, 0)
    # strictly larger: the cumulative mass before the first element of a run of equal values
    first = torch.ones_like(xo, dtype=torch.bool)
    first[1:] = xo[1:] != xo[:-1]
    start = torch.cummax(torch.where(first, torch.arange(xo.numel()), torch.zeros(xo.numel(), dtype=torch.long)), 0).values
    prev = lambda cum: torch.where(start > 0, cum[(start - 1).clamp(min=0)], torch.zeros_like(cum))
    num_hi, num_lo = prev(cum_hi), prev(cum_lo)
    keep = (num_hi / z_lo < top_p - m) if top_p < 1.0 else torch.ones_like(io)
    drop = (num_lo / z_hi >= top_p + m) if top_p < 1.0 else torch.zeros_like(io)
    c = torch.full_like(xo, EITHER, dtype=torch.int8)
    c[keep & so] = KEEP
    c[drop | ~io] = DROP
    cls[idx[order]] = c
    return cls, m


def step(raw: torch.Tensor, history: torch.Tensor, step: int, finished, node, opts: Opts):
    """One decode step on raw logits [B, V] fp32.  history [B, >= step] int64: the ids emitted so far; finished: B flags and node: B trie
    nodes (or None), both BEFORE the step.  Returns a namespace:
      edited   [B, V] fp32   what logits_edit leaves in the buffer (a finished row stays raw)
      allowed  [B, V] bool   the set the select chooses from (trie edges; EOS out while step < min_new)
      chosen_from [B, V]     edited, -inf outside `allowed`
      greedy   (ids, nodes, finished) lists after a greedy step (stop ids included)
      classes  int8 [B, V] and margins [B]: the sampled kept set (None when opts.sampling is None)
      after(ids)             (emitted ids, nodes, finished) after the step for the ids a sampling select chose
      lp, live, bound        logprob(ids) -> logprob_ref.step_ref on the RAW row with the flags and nodes of before the step."""
    raw = raw.detach().float().cpu()
    B, V = raw.shape
    fin0 = torch.as_tensor([int(f) for f in finished], dtype=torch.int32)
    node0 = [int(n) for n in node] if opts.trie is not None else None
    edited = raw.clone() if opts.neutral else P.edit(raw, history, step, fin0, opts.params)
    allowed = L.allowed_rows(V, B, step, opts.eos, opts.min_new, opts.trie, node0)
    chosen_from = edited.masked_fill(~allowed, -math.inf)

    def after(ids):
        toks, nodes, fin = [], list(node0) if node0 is not None else None, fin0.clone()
        for b in range(B):
            y = int(ids[b])
            if int(fin0[b]):
                toks.append(opts.pad)
                continue
            if opts.trie is not None:
                nxt = dict(C.allowed_tokens(opts.trie, node0[b], V, step, opts.eos, opts.min_new))
                if y not in nxt:                                 # nothing allowed (or an id that left the trie): pad, finished
                    toks.append(opts.pad if not nxt else y); fin[b] = 1
                    continue
                nodes[b] = nxt[y]
            toks.append(y)
            if opts.eos >= 0 and y == opts.eos:
                fin[b] = 1
        fin = P.finished_after(fin, torch.tensor(toks, dtype=torch.int64), opts.params)
        return toks, nodes, fin

    if opts.trie is not None:
        g_ids, _, _ = C.select_step(edited, opts.trie, node0, fin0.tolist(), step, opts.eos, opts.pad, opts.min_new)
    else:
        g_ids = chosen_from.argmax(1).tolist()                   # torch.argmax: the first maximum
    greedy = after(g_ids)
    if opts.trie is not None:
        assert greedy[0] == g_ids, "the composition and constrain_ref.select_step disagree on the emitted ids"
    classes = margins = None
    if opts.sampling is not None:
        classes, margins = torch.zeros((B, V), dtype=torch.int8), torch.zeros(B, dtype=torch.float64)
        for b in range(B):
            if not int(fin0[b]):
                classes[b], margins[b] = kept_classes(edited[b], allowed[b], opts.sampling)

    def logprob(ids):
        return L.step_ref(raw, ids, step, fin0, opts.eos, opts.min_new, opts.trie, node0)

    return types.SimpleNamespace(edited=edited, allowed=allowed, chosen_from=chosen_from, greedy=greedy, classes=classes, margins=margins,
                                 after=after, logprob=logprob, finished_before=fin0, node_before=node0)


def walk(step_logits: torch.Tensor, ids: torch.Tensor, opts: Opts):
    """`step` over a call's recorded RAW step logits [B, n, V], following the emitted ids [B, n] as logprob_ref.walk_ref does.  Returns a
    namespace: steps (the per-step namespaces), greedy_ids [B, n] (what a greedy select emits at every step GIVEN the ids before it),
    emitted [B, n] (the ids the state machine accepts: pad after a row has finished), lp / bound fp64 [2, B, n], live bool [B, n],
    finished / node after the last step."""
    lg, ids = step_logits.detach().float().cpu(), ids.detach().cpu().long()
    B, n, V = lg.shape
    fin = torch.zeros(B, dtype=torch.int32)
    node = [int(opts.trie.roots[s]) for s in (opts.set_of if opts.set_of is not None else [0] * B)] if opts.trie is not None else None
    out = types.SimpleNamespace(steps=[], greedy_ids=torch.zeros((B, n), dtype=torch.int64), emitted=torch.zeros((B, n), dtype=torch.int64),
                                lp=torch.zeros((2, B, n), dtype=torch.float64), bound=torch.zeros((2, B, n), dtype=torch.float64),
                                live=torch.zeros((B, n), dtype=torch.bool))
    for t in range(n):
        r = step(lg[:, t], ids, t, fin, node, opts)
        out.steps.append(r)
        out.greedy_ids[:, t] = torch.tensor(r.greedy[0])
        out.lp[:, :, t], out.live[:, t], out.bound[:, :, t] = r.logprob(ids[:, t])
        toks, node, fin = r.after(ids[:, t])
        out.emitted[:, t] = torch.tensor(toks)
    out.finished, out.node = fin, node
    return out
