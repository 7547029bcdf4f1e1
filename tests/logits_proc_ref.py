"""Pure-torch CPU restatement of the logits processors of the decode step (crab_amd/csrc/logits_proc.hip): HF's
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor with a list of ids, plus the stop rule
(a row that emits any stop id is finished).  Held bit for bit to transformers.generation.logits_process in tests/test_logits_proc_host.py;
the kernels are held bit for bit to it in tests/test_logits_proc_gpu.py.

Beyond HF (which would raise on them): an id outside [0, V) in a history is never edited and equals nothing in an n-gram comparison, a stop id
outside [0, V) bans nothing, and a finished row is not edited at all."""
import math

import torch


class Params:
    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, stop_ids=(), min_new_tokens=0):
        self.p, self.n, self.stops, self.min_new = float(repetition_penalty), int(no_repeat_ngram_size), tuple(int(e) for e in stop_ids), int(min_new_tokens)


def banned_ngram_tokens(h, n, V):
    """HF's _calc_banned_ngram_tokens for one row: the tokens that would complete an n-gram already in h (a list of ints)."""
    cur = len(h)
    if n <= 0 or cur + 1 < n:
        return []
    ok = lambda t: 0 <= t < V
    tail = h[cur + 1 - n:cur]
    out = []
    for j in range(cur - n + 1):
        w = h[j:j + n]
        if all(ok(t) for t in w) and w[:n - 1] == tail:
            out.append(w[n - 1])
    return out


def edit_row(raw, h, step, prm):
    """The row the select chooses from: raw [V] fp32, h - the row's generated ids so far (only the first `step` count)."""
    V = raw.shape[0]
    h = [int(t) for t in h[:step]]
    out = raw.clone()
    if prm.p != 1.0:
        seen = sorted({t for t in h if 0 <= t < V})
        if seen:
            idx = torch.tensor(seen, dtype=torch.long)
            x = raw[idx]
            out[idx] = torch.where(x < 0, x * prm.p, x / prm.p)          # fp32 on fp32, as HF's gather -> where -> scatter
    for t in banned_ngram_tokens(h, prm.n, V):
        out[t] = -math.inf
    if step < prm.min_new:
        for e in prm.stops:
            if 0 <= e < V:
                out[e] = -math.inf
    return out


def edit(raw, history, step, finished, prm):
    """raw [B, V] fp32, history [B, >= step] int64, finished [B] -> the edited logits [B, V] (a finished row stays raw)."""
    out = raw.clone()
    for b in range(raw.shape[0]):
        if not int(finished[b]):
            out[b] = edit_row(raw[b], history[b].tolist(), step, prm)
    return out


def finished_after(finished, cur_ids, prm):
    """finished[b] |= cur_ids[b] in stop_ids: what crab_logits_restore leaves (the select's own eos_id is the select's business)."""
    out = finished.clone()
    for b in range(out.shape[0]):
        if int(cur_ids[b]) in [e for e in prm.stops if e >= 0]:
            out[b] = 1
    return out
