"""Plain torch fp64 statement of the per-token log-probabilities of the decode step (csrc/logprob.hip).  For row b at `step` with raw logits
z = logits[b] and the chosen token y:

    logprob         = z[y] - logsumexp(z[0 .. V))
    logprob_allowed = z[y] - logsumexp(z[i] : i allowed at this step)

"allowed" is what the select kernels choose from: every token but EOS while step < min_new; with a trie the out-edges of the row's node
(tests/constrain_ref.allowed_tokens: token in [0, V), not the suppressed EOS), the node taken BEFORE the step moves it.  A row that was finished
before the step, or that has nothing allowed, is not live: both values are 0.  So are they when the chosen token lies outside [0, V).

Every value comes with the bound the fp32 kernels are held to,

    |got - ref|  <=  eps_fp32 * (2 * (|z_y - max| + |log S|) + 8),        S = sum exp(z_i - max) over the normaliser's set,

three fp32 roundings of quantities of those magnitudes (lse = max + log S, the subtraction, the stored value) plus about 4 eps of absolute
error in log S from expf."""
import torch

from tests import constrain_ref as R

EPS = float(torch.finfo(torch.float32).eps)


def allowed_rows(V: int, B: int, step: int, eos: int, min_new: int, trie=None, nodes=None) -> torch.Tensor:
    """bool [B, V]: the set the select kernels choose from at this step."""
    if trie is not None:
        return R.allowed_mask(trie, nodes, V, step, eos, min_new)
    m = torch.ones((B, V), dtype=torch.bool)
    if 0 <= eos < V and step < min_new:
        m[:, eos] = False
    return m


def step_ref(logits: torch.Tensor, chosen, step: int, finished, eos: int, min_new: int, trie=None, nodes=None):
    """logits [B, V]; chosen / finished (the flags BEFORE the step) / nodes: B ints.  Returns (lp fp64 [2, B], live bool [B], bound fp64 [2, B])."""
    z = logits.detach().double().cpu()
    B, V = z.shape
    allowed = allowed_rows(V, B, step, eos, min_new, trie, nodes)
    lp, bound, live = torch.zeros((2, B), dtype=torch.float64), torch.zeros((2, B), dtype=torch.float64), torch.zeros((B,), dtype=torch.bool)
    for b in range(B):
        if int(finished[b]) or not bool(allowed[b].any()):
            continue
        live[b] = True
        y = int(chosen[b])
        if not 0 <= y < V:
            continue
        for p, zs in enumerate((z[b], z[b][allowed[b]])):
            mx = zs.max()
            log_s = torch.log(torch.exp(zs - mx).sum())
            lp[p, b] = z[b, y] - mx - log_s
            bound[p, b] = EPS * (2 * (abs(float(z[b, y] - mx)) + abs(float(log_s))) + 8)
    return lp, live, bound


def walk_ref(step_logits: torch.Tensor, ids: torch.Tensor, eos: int, min_new: int = 0, trie=None, set_of=None):
    """The same over a call's recorded step logits [B, n, V] and its ids [B, n]: (lp fp64 [2, B, n], live bool [B, n], bound fp64 [2, B, n]).  The
    finished flags and, with a trie, the nodes follow the ids as the select kernels move them: a live row that emits EOS finishes AFTER that step,
    a constrained row with nothing allowed finishes at it."""
    lg, ids = step_logits.detach().float().cpu(), ids.cpu()
    B, n, V = lg.shape
    fin = [0] * B
    nodes = [int(trie.roots[s]) for s in set_of] if trie is not None else None
    lp, bound = torch.zeros((2, B, n), dtype=torch.float64), torch.zeros((2, B, n), dtype=torch.float64)
    live = torch.zeros((B, n), dtype=torch.bool)
    for t in range(n):
        lp[:, :, t], live[:, t], bound[:, :, t] = step_ref(lg[:, t], ids[:, t], t, fin, eos, min_new, trie, nodes)
        for b in range(B):
            if fin[b]:
                continue
            y = int(ids[b, t])
            if trie is not None:
                nxt = dict(R.allowed_tokens(trie, nodes[b], V, t, eos, min_new))
                if y not in nxt:
                    fin[b] = 1                                 # nothing allowed (or ids that left the trie: nothing more to say about the row)
                    continue
                nodes[b] = nxt[y]
            if eos >= 0 and y == eos:
                fin[b] = 1
    return lp, live, bound
