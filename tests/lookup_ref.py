"""Reference of prompt-lookup speculative decoding (csrc/lookup.hip; GenerationEngine.generate_lookup), pure Python / torch on the CPU.

draft() restates HF's PromptLookupCandidateGenerator.get_candidates (transformers generation/candidate_generator.py) with this project's
extension: an entry -1 (or any id outside [0, V) when V is given) is "no token" - it equals nothing, and a continuation is cropped before it;
a continuation that BEGINS with one is skipped and the search goes on (HF's treatment of a token its logits processors forbid).  The EOS crop is
HF's: it runs after the match is chosen, so a continuation that begins with EOS ends the search with an empty draft.
accept() restates the greedy branch of HF's _assisted_decoding; simulate() runs the whole loop with a token tape in the place of the model."""
import torch


def _tok(hist, i, V=None):
    t = int(hist[i])
    return t if t >= 0 and (V is None or t < V) else -1


def draft(hist, k, max_ngram, eos, remaining, V=None):
    """hist: the live history (prompt ids, -1 = no token, then the emitted tokens; the last entry is the current token).  remaining: how many
    tokens the call may still emit BESIDE the one the verify step adds (max_new_tokens - step - 1).  -> the list of draft tokens (<= k)."""
    n_hist = len(hist)
    if remaining <= 0:
        return []
    for n in range(min(max_ngram, n_hist - 1), 0, -1):
        tail = [_tok(hist, n_hist - n + e, V) for e in range(n)]
        if any(t < 0 for t in tail):
            continue
        for idx in range(0, n_hist - n):                        # continuation start idx + n < len
            if [_tok(hist, idx + e, V) for e in range(n)] != tail:
                continue
            start = idx + n
            end = min(start + k, n_hist)
            chosen = []
            for j in range(start, end):
                t = _tok(hist, j, V)
                if t < 0:
                    break
                chosen.append(t)
            if not chosen:
                continue                                        # nothing but "no token": the next match
            chosen = chosen[:remaining]
            if eos is not None and eos >= 0 and eos in chosen:
                chosen = chosen[:chosen.index(eos)]
            return chosen                                       # possibly empty (EOS first): HF stops searching here too
    return []


def greedy(row, suppress=-1):
    """greedy_select_kernel's rule: the larger value wins, equal values go to the lower id; `suppress` is out of the race."""
    row = row.clone().float()
    if suppress >= 0:
        row[suppress] = float("-inf")
    m = row.max()
    idx = torch.nonzero(row == m).reshape(-1)
    return int(idx[0]) if idx.numel() else 0


def accept(logits, ids, n_draft, step, eos, min_new, max_new):
    """logits [k + 1, V] fp32, ids [k + 1] (current token, drafts, pad).  -> (emitted tokens, accepted count a, finished)."""
    toks = [greedy(logits[i], eos if (eos is not None and eos >= 0 and step + i < min_new) else -1) for i in range(n_draft + 1)]
    a = 0
    while a < n_draft and toks[a] == int(ids[a + 1]):
        a += 1
    emitted, fin = [], False
    for i in range(a + 1):
        if step + i >= max_new:
            break
        emitted.append(toks[i])
        if eos is not None and eos >= 0 and toks[i] == eos:
            fin = True
            break
    if step + len(emitted) >= max_new:
        fin = True
    return emitted, a, fin


def all_right_prompt(g):
    """Prompt ids that make every draft right: the tape itself (every n-gram of the emitted tokens is found with its true continuation)."""
    return [int(t) for t in g]


def all_wrong_prompt(g, w):
    """Prompt ids that make every draft wrong (max_ngram = 2): after the first token, and after every bigram of the tape, the token w, which
    the tape never holds.  The bigram of the last two emitted tokens is always found here first (the prompt precedes the emitted tokens), so
    the first draft token of every step is w.  The prompt ends with a -1 row: the first step's bigram (-1, g[0]) matches nothing and falls back
    to the unigram g[0], whose earliest occurrence is followed by w as well."""
    g = [int(t) for t in g]
    assert w not in g
    out = [g[0], w]
    for a, b in zip(g, g[1:]):
        out += [a, b, w]
    return out + [-1]


def simulate(g, prompt_ids, k, max_ngram, eos, max_new, flags=False):
    """The whole loop with the token tape g standing in for the model: g[j] is the token the model emits at index j whatever it is shown (the
    drafts never change what a greedy model says, only how many steps it takes).  g[0] is the prefill's token.  prompt_ids: list of ints
    (-1 = no token) or None.  -> (emitted ids, [verify steps, drafts proposed, drafts accepted, tokens emitted]); with flags=True also, per
    emitted id, whether it was an accepted draft (False: the prefill's token or the model's own token of a step)."""
    g = [int(t) for t in g]
    hist = [int(t) for t in prompt_ids] if prompt_ids is not None else []
    out = [g[0]]
    hist = hist + [g[0]]
    stats = [0, 0, 0, 0]
    was_draft = [False]
    fin = (eos is not None and eos >= 0 and g[0] == eos) or max_new <= 1
    while not fin:
        step = len(out)
        d = draft(hist, k, max_ngram, eos, max_new - step - 1)
        a = 0
        while a < len(d) and step + a < len(g) and d[a] == g[step + a]:
            a += 1
        ne = 0
        for i in range(a + 1):
            if step + i >= max_new or step + i >= len(g):
                break
            t = g[step + i]
            out.append(t); hist.append(t); was_draft.append(i < a)
            ne += 1
            if eos is not None and eos >= 0 and t == eos:
                fin = True
                break
        if len(out) >= max_new or len(out) >= len(g):
            fin = True
        stats[0] += 1; stats[1] += len(d); stats[2] += min(ne, a); stats[3] += ne
    return (out, stats, was_draft) if flags else (out, stats)


# ------------------------------------------------------------------ shared cases (host tests, GPU tests)
def hf_cases():
    """Seeded random histories over 5 ids (n-grams repeat constantly): lengths 2 .. 40, k in {1, 3, 7}, max_ngram in {1, 2, 3}, with (id 4) and
    without an EOS id.  The cases of the comparison with transformers (tests/test_lookup_host.py)
    and of the GPU test of crab_lookup_draft."""
    out = []
    g = torch.Generator().manual_seed(1234)
    for n in range(2, 41):
        for k in (1, 3, 7):
            for m in (1, 2, 3):
                for eos in (None, 4):
                    hist = torch.randint(0, 5, (n,), generator=g).tolist()
                    out.append((hist, k, m, eos))
    return out


HAND = [
    # (hist, k, max_ngram, eos, remaining, expected): -1 = a row that is no text token
    ([-1, -1, 3, 4, 5, 3, 4], 3, 2, None, 9, [5, 3, 4]),        # the bigram (3, 4) at index 2
    ([3, -1, 5, 3], 3, 2, None, 9, []),                         # the only earlier 3 is followed by -1: nothing to draft
    ([3, -1, 5, 3, 7, 3], 3, 1, None, 9, [7, 3]),               # the first match's continuation begins with -1: skipped, the second is taken
    ([3, 6, -1, 5, 3], 3, 1, None, 9, [6]),                     # cropped before the -1
    ([-1, -1, -1], 3, 2, None, 9, []),                          # -1 equals nothing, itself included
    ([2, -1, 2, -1], 3, 1, None, 9, []),                        # the last entry is -1: no n-gram to look up
    ([1, -1, 9, 1, -1, 8, 1, -1], 3, 2, None, 9, []),           # the bigram (1, -1) never matches
    ([3, 4, 9, 9, 3, 4], 3, 2, 9, 9, []),                       # EOS first: HF sets match_found before the EOS crop - no draft, no further search
    ([3, 4, 7, 9, 3, 4], 3, 2, 9, 9, [7]),                      # cropped before the EOS
    ([5, 1, 5, 2, 5], 3, 1, None, 9, [1, 5, 2]),                # the earliest match wins
    ([5, 1, 5, 2, 5], 3, 1, None, 2, [1, 5]),                   # cropped to what the call may still emit
]
