"""The launch chain of GenerationEngine._select on bare logits (no model), every allowed pairing of its options, against the composed CPU
reference tests/select_chain_ref.py:

    logprob_norm -> logits_edit -> {greedy | sample | constrained}_select -> logits_restore -> logprob_gather -> advance

n = 12 steps through crab_amd.ops; the kernels' own out_ids are the history.  The logits are a column view of a wider buffer (row stride
V + 3) whose three columns behind every row are sentinels.  A run is RECORDED first (the buffer between edit and select, the buffer after
restore, every per-row word after every step), then the reference walks the recorded ids, the share of (row, step) pairs that hold an
`EITHER` token is counted over all runs of the test case (shape x select x processors: its log-probability, min_new, EOS and sampling
settings) and held to the 5 % cap, and only then is anything compared.

The crafted choices sit 0.75 - 2 above the seeded row's maximum, not at a fixed large value: crab_logprob_norm rounds its normaliser
max + log S once to fp32, an error of eps / 2 * |lse| that the bound of tests/logprob_ref.py carries only up to |lse| < 16 (its "+ 8");
a fixed logit of 16 - 22 that dominates its row (log S ~ 0) was measured at 1.05 x that bound on the GPU.

The matrix (CASES) is select x processors x log-probabilities x min_new x EOS minus what check_processors and TokenTrie refuse (REFUSED);
tests/test_select_chain_host.py holds both tables to pairwise coverage on a machine without a GPU."""
import functools
import itertools

import numpy as np
import pytest
import torch

from crab_amd import decoder, ops
from crab_amd.constrain import TokenTrie
from tests import select_chain_ref as S
from tests.util import record_parity

pytestmark = pytest.mark.gpu

N = 12
SHAPES = [(1, 40), (5, 1000), (3, 1025), (2, 4099), (2, 32017)]          # V below, just above and far above the 1024-thread partition; an odd size
SELECTS = ["greedy", "sample", "trie-greedy", "trie-sample"]
EOS, PAD, SEED = 11, 1, 1234
STOPS = lambda V: (12, 13, V + 9)                                # two ids the rows can emit and one outside [0, V)
PROCS = {"none": (1.0, 0, False), "penalty 1.3": (1.3, 0, False), "penalty 0.7": (0.7, 0, False), "penalty + 2-gram": (1.3, 2, False),
         "penalty + 3 stops": (1.3, 0, True), "all three": (1.3, 2, True)}
LOGPROBS, MIN_NEW, EOSES = [False, True], [0, 3], [None, EOS]
SAMPLING = [(0.6, 50, 0.9), (1.3, 7, 0.5), (0.8, 0, 0.95)]      # the last only at V <= 1025: with top_k = 0 a wide tail sits ON the nucleus boundary
EITHER_CAP = 0.05
RAW_SEED = 7                                                     # settled on the CPU: the raw rows meet the EITHER cap by the reference alone (tests/test_select_chain_host.py) and log-sum-exp stays below 16
AXES = dict(select=SELECTS, proc=list(PROCS), logprobs=LOGPROBS, min_new=MIN_NEW, eos=EOSES)


def refusal(c):
    """The message a call with these options is refused with (check_processors / TokenTrie), or None."""
    p, n, st = PROCS[c["proc"]]
    trie = c["select"].startswith("trie")
    try:
        decoder.check_processors((p, n, STOPS(40)[:2] if st else ()), c["min_new"], trie, c["logprobs"], c["eos"])
        if trie and c["eos"] is None:
            TokenTrie([[3]], 40, None)
    except (NotImplementedError, ValueError) as e:
        return str(e)
    return None


_ALL = [dict(zip(AXES, v)) for v in itertools.product(*AXES.values())]
CASES = [c for c in _ALL if refusal(c) is None]
REFUSED = [dict(c, reason=refusal(c)) for c in _ALL if refusal(c) is not None]


def sampling_for(V):
    return [s for s in SAMPLING if s[1] > 0 or V <= 1025]


# ------------------------------------------------------------------ inputs
ALPHABET = [4, 8, 9, 20, 30, 14, 15, 16, 17, 18]                 # crafted columns and ordinary ones; no EOS, no stop id, no column at -inf (a sole edge at -inf has no distribution)


@functools.lru_cache(maxsize=None)
def _trie(V):
    """Set 0: members that begin with the steered ids 8 9 5 4 and end at different depths, and members that do not.  Set 1: [8] is a member
    and nothing else starts with 8 - after 8 the node's ONLY edge is EOS, so with min_new = 3 nothing is allowed at step 1."""
    rng = np.random.default_rng(V)
    tail = lambda k: [int(t) for t in rng.choice(ALPHABET + [V - 1], size=k)]
    set0 = [[8, 9, 5, 4] + tail(k) for k in (0, 2, 3, 5, 6, 8, 8, 8, 8)] + [tail(k) for k in (3, 6, 9, 12)] + [[8, 9] + tail(7), [8, 4] + tail(10)]
    set1 = [[8]] + [[9] + tail(4), [4] + tail(6), [20] + tail(3)]
    return TokenTrie([set0, set1], V, EOS)


@functools.lru_cache(maxsize=None)
def _raw(B, V):
    """[N, B, V + 3] fp32, seeded randn * 3, plus what a chain can get wrong."""
    g = torch.Generator().manual_seed(1000 * B + V + RAW_SEED)
    raw = torch.randn(N, B, V + 3, generator=g) * 3
    raw[:, :, V:] = torch.tensor([1e30, -7.0, 3e-30])            # the sentinels behind every row
    top = raw[:, :, :V].amax(-1)                                 # [N, B]: the crafted choices sit a little above the seeded row's maximum, so that the
    steered = sorted({0, B - 1})                                 # normaliser stays in the range the bound of tests/logprob_ref.py was derived for
    for s, c in enumerate((8, 9, 5, 4, 8, 9)):                  # steps 0 - 5: the first and the last row are steered over the crafted columns (their history
        raw[s, steered, c] = top[s, steered] + 0.75              # meets them) and into a repeated bigram 8 9 (banned at step 5 by the 2-gram rule)
    raw[3:, :, 4] = 0.0                                          # once in the history: a zero, a -inf, a value of either sign (the penalty's sign classes)
    raw[3:, :, 5] = -float("inf")
    raw[6:, :, 8], raw[6:, :, 9], raw[:, :, V - 1] = 2.5, -1.75, 0.625
    raw[4:, :, 21::97] = 0.0
    raw[:, :, 22::113] = -float("inf")
    raw[6, 0, 20] = raw[6, 0, 30] = top[6, 0] + 1.0              # two equal maxima: the lower id wins
    raw[1, B - 1, EOS] = top[1, B - 1] + 1.75                    # EOS as the largest logit while step < min_new (min_new = 0: the row finishes here)
    raw[2, B - 1, 13] = top[2, B - 1] + 2.0                      # a stop id likewise
    for b in range(B):                                           # rows that finish at different steps: EOS (odd rows: a stop id) is the choice of step 7 + b
        if 7 + b < N:
            raw[7 + b, b, 12 if b % 2 else EOS] = top[7 + b, b] + 1.25
    raw[10, 0, 12] = top[10, 0] + 1.5                            # row 0 also meets a stop id
    return raw


def _opts(c, V, smp, B):
    p, n, st = PROCS[c["proc"]]
    trie = _trie(V) if c["select"].startswith("trie") else None
    return S.Opts(eos=c["eos"], pad=PAD, min_new=c["min_new"], penalty=p, ngram=n, stops=STOPS(V) if st else (),
                  sampling=smp if c["select"].endswith("sample") else None, trie=trie,
                  set_of=([0] * (B - 1) + [1] if B > 1 else [0]) if trie is not None else None)


class Chain:
    """The device state of one chain and its launches, in the order of GenerationEngine._select + ops.advance."""

    def __init__(self, B, V, o: S.Opts, logprobs: bool, seed=SEED):
        dev = "cuda"
        self.B, self.V, self.o, self.seed = B, V, o, seed
        self.buf = torch.zeros(B, V + 3, device=dev)
        self.logits = self.buf[:, :V]
        self.snap = torch.zeros_like(self.buf)
        self.cur = torch.zeros(B, dtype=torch.int64, device=dev)
        self.out = torch.full((B, N), PAD, dtype=torch.int64, device=dev)
        self.fin = torch.zeros(B, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.proc = not o.neutral
        self.stops = torch.tensor(o.stops, dtype=torch.int32, device=dev) if o.stops else None
        n_slots = 2 * N + len(o.stops)
        self.save_idx = torch.full((B, n_slots), -1, dtype=torch.int32, device=dev)
        self.save_val = torch.zeros((B, n_slots), device=dev)
        self.lp = torch.zeros((2, B, N), device=dev) if logprobs else None
        self.lp_norm = torch.zeros((B, 4), device=dev) if logprobs else None
        self.node = self.eo = self.et = self.ed = None
        if o.trie is not None:
            up = lambda a: torch.from_numpy(a.copy()).to(dev)
            self.eo, self.et, self.ed = up(o.trie.edge_off), up(o.trie.edge_tok), up(o.trie.edge_dst)
            self.node = torch.tensor([int(o.trie.roots[s]) for s in o.set_of], dtype=torch.int32, device=dev)

    def select(self, logits, node, cur, out, fin):
        o = self.o
        if o.trie is not None:
            t, k, p = o.sampling if o.sampling is not None else (0.0, 0, 1.0)
            ops.constrained_select(logits, self.eo, self.et, self.ed, node, cur, out, self.step, fin, o.eos, o.pad, o.min_new, t, k, p, self.seed)
        elif o.sampling is None:
            ops.greedy_select(logits, cur, out, self.step, fin, o.eos, o.pad, o.min_new)
        else:
            t, k, p = o.sampling
            ops.sample_select(logits, cur, out, self.step, fin, o.eos, o.pad, o.min_new, t, k, p, self.seed)

    def launches(self):
        o = self.o
        if self.lp is not None:
            ops.logprob_norm(self.logits, self.step, self.fin, o.eos, o.min_new, self.lp_norm, self.eo, self.et if self.eo is not None else None, self.node)
        if self.proc:
            ops.logits_edit(self.logits, self.out, self.step, self.fin, o.penalty, o.ngram, self.stops, o.min_new, self.save_idx, self.save_val)
        self.snap.copy_(self.buf)                                # what the select chooses from
        self.select(self.logits, self.node, self.cur, self.out, self.fin)
        if self.proc:
            ops.logits_restore(self.logits, self.cur, self.fin, self.stops, self.save_idx, self.save_val)
        if self.lp is not None:
            ops.logprob_gather(self.logits, self.cur, self.step, self.lp_norm, self.lp)
        ops.advance(self.pos, self.step)

    def words(self):
        """Everything a step leaves, on the CPU."""
        return dict(snap=self.snap.cpu(), buf=self.buf.cpu(), cur=self.cur.cpu(), out=self.out.cpu(), fin=self.fin.cpu(), step=int(self.step.item()),
                    pos=int(self.pos.item()), node=self.node.cpu() if self.node is not None else None, lp=self.lp.cpu() if self.lp is not None else None)

    def put(self, w, raw_row):
        """The state BEFORE a step: the words a previous step left (w) and the step's raw logits."""
        self.buf.copy_(raw_row)
        self.cur.copy_(w["cur"]); self.out.copy_(w["out"]); self.fin.copy_(w["fin"])
        self.step.fill_(w["step"]); self.pos.fill_(w["pos"])
        if self.node is not None:
            self.node.copy_(w["node"])
        if self.lp is not None:
            self.lp.copy_(w["lp"])


def record(B, V, o, logprobs):
    """Run the chain eagerly for N steps: (chain, the words before step 0, the words after every step)."""
    ch = Chain(B, V, o, logprobs)
    raw = _raw(B, V)
    before = ch.words()
    after = []
    for s in range(N):
        ch.buf.copy_(raw[s])
        ch.launches()
        after.append(ch.words())
    return ch, before, after


def either_pairs(walk, B):
    """(row, step) pairs of one run that hold an EITHER token."""
    return sum(int(bool((r.classes[b] == S.EITHER).any())) for r in walk.steps for b in range(B)) if walk.steps[0].classes is not None else 0


def reference(B, V, ch, after):
    """The composed reference walked along the ids the recorded run emitted."""
    return S.walk(_raw(B, V)[:, :, :V].transpose(0, 1), after[-1]["out"], ch.o)


def check(B, V, ch, before, after, walk, what):
    """Everything the issue asks of one recorded run, against its reference walk.  Returns (largest margin, largest lp error / bound)."""
    o, raw = ch.o, _raw(B, V)
    worst, mrg = 0.0, 0.0
    prev = before
    # the log-probabilities with the processors off along the same ids (one norm + one gather per step on the raw rows)
    lp_plain = torch.zeros((2, B, N), device="cuda") if ch.lp is not None else None
    for s in range(N):
        r, a, w = walk.steps[s], after[s], f"{what}: step {s}"
        assert torch.equal(a["snap"][:, :V], r.edited), f"{w}: the buffer between edit and select differs from the reference's edited rows at {torch.nonzero(a['snap'][:, :V] != r.edited)[:6].tolist()}"
        assert torch.equal(a["snap"][:, V:], raw[s][:, V:]), f"{w}: logits_edit wrote behind a row"
        assert torch.equal(a["buf"], raw[s]), f"{w}: after logits_restore the buffer is not the raw one at {torch.nonzero((a['buf'] != raw[s]) & ~(torch.isnan(a['buf']) & torch.isnan(raw[s])))[:6].tolist()}"
        cur = a["cur"]
        if o.sampling is None:
            toks, nodes, fin = r.greedy
        else:
            mrg = max(mrg, float(r.margins.max()))
            for b in range(B):
                if not int(r.finished_before[b]) and bool(r.allowed[b].any()):
                    assert int(r.classes[b, int(cur[b])]) != S.DROP, f"{w}: row {b} drew {int(cur[b])}, which the fp64 kept set drops"
            toks, nodes, fin = r.after(cur)
        assert cur.tolist() == list(toks), f"{w}: emitted {cur.tolist()}, reference {list(toks)}"
        assert a["out"][:, s].tolist() == list(toks) and torch.equal(a["out"][:, :s], prev["out"][:, :s]) and bool((a["out"][:, s + 1:] == PAD).all()), f"{w}: out_ids"
        assert a["fin"].tolist() == fin.tolist(), f"{w}: finished {a['fin'].tolist()}, reference {fin.tolist()}"
        for b in range(B):
            if int(r.finished_before[b]):
                assert int(cur[b]) == PAD, f"{w}: row {b} had finished and must emit pad"
        if o.trie is not None:
            assert a["node"].tolist() == list(nodes), f"{w}: node {a['node'].tolist()}, reference {list(nodes)}"
        assert a["step"] == s + 1 and a["pos"] == s + 1
        if ch.lp is not None:
            want, live, bound = r.logprob(cur)
            got = a["lp"][:, :, s].double()
            err = (got - want).abs()
            assert bool((err <= bound).all()), f"{w}: log-probabilities off by {err.tolist()} (bound {bound.tolist()})"
            assert bool((got[:, ~live] == 0).all()), f"{w}: a row that is not live has a log-probability"
            worst = max(worst, float((err / bound.clamp(min=1e-30))[:, live].max()) if bool(live.any()) else 0.0)
            assert torch.equal(a["lp"][:, :, s + 1:], torch.zeros(2, B, N - s - 1)) and torch.equal(a["lp"][:, :, :s], prev["lp"][:, :, :s])
            # processors off, same ids: the same bits
            fin0 = r.finished_before.cuda()
            norm = torch.zeros((B, 4), device="cuda")
            step_d = torch.full((1,), s, dtype=torch.int32, device="cuda")
            rawd = raw[s].cuda()
            node0 = torch.tensor(r.node_before, dtype=torch.int32, device="cuda") if o.trie is not None else None
            ops.logprob_norm(rawd[:, :V], step_d, fin0, o.eos, o.min_new, norm, ch.eo, ch.et if ch.eo is not None else None, node0)
            ops.logprob_gather(rawd[:, :V], cur.cuda(), step_d, norm, lp_plain)
            assert torch.equal(lp_plain[:, :, s].cpu(), a["lp"][:, :, s]), f"{w}: the processors entered a log-probability plane"
        if o.sampling is not None:
            # composition: the same select kernel, stand-alone on the REFERENCE's edited rows at this (seed, step), draws the same id
            ch.step.fill_(s)
            cur2, out2 = torch.zeros_like(ch.cur), torch.zeros_like(ch.out)
            node2 = torch.tensor(r.node_before, dtype=torch.int32, device="cuda") if o.trie is not None else None
            ch.select(r.edited.cuda(), node2, cur2, out2, r.finished_before.cuda())
            assert torch.equal(cur2.cpu(), cur), f"{w}: in the chain the select drew {cur.tolist()}, stand-alone on the reference's edited rows {cur2.tolist()}"
        prev = a
    return mrg, worst


@pytest.mark.parametrize("proc", list(PROCS))
@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("B,V", SHAPES)
def test_the_chain_equals_the_composed_reference(B, V, select, proc):
    mine = [c for c in CASES if c["select"] == select and c["proc"] == proc]
    if not mine:
        assert all(c["reason"] for c in REFUSED if c["select"] == select and c["proc"] == proc)
        return                                                   # refused as a whole (a trie with stop ids or an n-gram ban): tests/test_decode_matrix_gpu.py walks the refusals
    runs = []
    for c in mine:
        for smp in (sampling_for(V) if select.endswith("sample") else [None]):
            what = f"B = {B}, V = {V}, {select}, {proc}, logprobs = {c['logprobs']}, min_new = {c['min_new']}, eos = {c['eos']}, sampling = {smp}"
            ch, before, after = record(B, V, _opts(c, V, smp, B), c["logprobs"])
            runs.append((ch, before, after, reference(B, V, ch, after), what))
    # the cap first, over all runs of this case and by the reference alone: nothing of the GPU's answer has been compared yet
    share = sum(either_pairs(r[3], B) for r in runs) / float(B * N * len(runs))
    assert share <= EITHER_CAP, f"{share:.1%} of the (row, step) pairs hold an EITHER token - the kept-set check would be hollow"
    mrg = worst = 0.0
    for ch, before, after, walk, what in runs:
        m, w = check(B, V, ch, before, after, walk, what)
        mrg, worst = max(mrg, m), max(worst, w)
    record_parity(f"select chain {select} / {proc} B={B} V={V}: share of (row, step) pairs with an EITHER token", share, 1.0, EITHER_CAP,
                  either_margin=mrg, lp_err_over_bound=worst, runs=len(runs))
    print(f"{len(runs)} runs: either share {share:.2%} (margin {mrg:.2e}), lp error / bound <= {worst:.3f}")
    assert worst <= 1.0


def test_graph_replay_of_the_whole_chain_gives_the_eager_bits():
    """trie-sample, every processor a trie permits (the penalty), log-probabilities on: captured once, replayed at three step values."""
    B, V = 3, 1025
    c = dict(select="trie-sample", proc="penalty 1.3", logprobs=True, min_new=3, eos=EOS)
    assert c in CASES
    o = _opts(c, V, SAMPLING[0], B)
    ch, before, after = record(B, V, o, True)
    walk = reference(B, V, ch, after)
    assert either_pairs(walk, B) <= EITHER_CAP * B * N
    check(B, V, ch, before, after, walk, "eager")
    raw = _raw(B, V)
    g_ch = Chain(B, V, o, True)
    g_ch.put(before, raw[0].cuda())
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        g_ch.launches()                                          # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s_)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_ch.launches()
    for s in (1, 4, 9):                                          # nothing allowed for the last row (1), mid-answer (4), rows finished (9)
        g_ch.put(after[s - 1], raw[s].cuda())
        g.replay()
        torch.cuda.synchronize()
        got, want = g_ch.words(), after[s]
        for k in want:
            same = torch.equal(got[k], want[k]) if isinstance(want[k], torch.Tensor) else got[k] == want[k]
            assert same, f"replay at step {s}: {k} differs from the eager run"
