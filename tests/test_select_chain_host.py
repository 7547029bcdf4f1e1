"""tests/select_chain_ref.py on the CPU: with every option neutral it is argmax, with one option on it is that option's own reference bit
for bit, its kept set at margin 0 is sampling_probs > 0, and the case tables of tests/test_select_chain_gpu.py and
tests/test_decode_matrix_gpu.py cover every allowed PAIR of option values (as tests/test_kv_fp8_host.py pins its fuzzer's coverage)."""
import itertools

import numpy as np
import pytest
import torch

from crab_amd.constrain import TokenTrie
from oracle.crab_oracle import sampling_probs
from tests import constrain_ref as C
from tests import logits_proc_ref as P
from tests import logprob_ref as L
from tests import select_chain_ref as S
from tests import test_decode_matrix_gpu as M
from tests import test_select_chain_gpu as K

B, V, N, EOS, PAD = 4, 203, 10, 7, 2


def _logits(seed=0):
    return torch.randn(B, N, V, generator=torch.Generator().manual_seed(seed)) * 3


def _history(seed=1):
    return torch.randint(0, 12, (B, N), generator=torch.Generator().manual_seed(seed))       # a small alphabet: tokens and bigrams repeat


def _trie():
    return TokenTrie(C.random_sets(np.random.default_rng(3), 2, V, EOS, n_seqs=(5, 8), length=(2, 6)), V, EOS)


def test_every_option_neutral_is_argmax():
    lg = _logits()
    fin, ids = torch.zeros(B, dtype=torch.int32), torch.zeros(B, N, dtype=torch.int64)
    for t in range(N):
        r = S.step(lg[:, t], ids, t, fin, None, S.Opts(pad=PAD))
        toks, nodes, after = r.greedy
        assert toks == lg[:, t].argmax(1).tolist() and nodes is None and not bool(after.any())
        assert torch.equal(r.edited, lg[:, t]) and bool(r.allowed.all())
        ids[:, t] = torch.tensor(toks)
    w = S.walk(lg, ids, S.Opts(pad=PAD))
    assert torch.equal(w.greedy_ids, lg.argmax(-1)) and torch.equal(w.emitted, ids) and bool(w.live.all())


@pytest.mark.parametrize("p,n,stops,min_new", [(1.3, 0, (), 0), (0.7, 0, (), 0), (1.0, 2, (), 0), (1.0, 0, (3, 5, V + 2), 3), (1.4, 3, (3, 5), 2)])
def test_processors_alone_are_logits_proc_ref(p, n, stops, min_new):
    lg, hist = _logits(2), _history()
    prm = P.Params(p, n, stops, min_new)
    o = S.Opts(pad=PAD, min_new=min_new, penalty=p, ngram=n, stops=stops)
    fin = torch.tensor([0, 0, 1, 0], dtype=torch.int32)
    for t in range(N):
        r = S.step(lg[:, t], hist, t, fin, None, o)
        want = P.edit(lg[:, t], hist, t, fin, prm)
        assert torch.equal(r.edited, want)
        toks, _, after = r.greedy
        ref_toks = [PAD if int(fin[b]) else int(want[b].argmax()) for b in range(B)]
        assert toks == ref_toks
        assert torch.equal(after, P.finished_after(fin, torch.tensor(ref_toks), prm))


@pytest.mark.parametrize("min_new", [0, 2])
def test_the_trie_alone_is_constrain_ref(min_new):
    lg, trie = _logits(4), _trie()
    set_of = [0, 1, 1, 0]
    want, nodes = C.walk_greedy(lg, trie, set_of, EOS, PAD, min_new)
    o = S.Opts(eos=EOS, pad=PAD, min_new=min_new, trie=trie, set_of=set_of)
    w = S.walk(lg, want, o)
    assert torch.equal(w.greedy_ids, want) and torch.equal(w.emitted, want) and list(w.node) == list(nodes)
    fin, node = [0] * B, [int(trie.roots[s]) for s in set_of]
    for t in range(N):
        r = S.step(lg[:, t], want, t, fin, node, o)
        toks, node2, fin2 = C.select_step(lg[:, t], trie, node, fin, t, EOS, PAD, min_new)
        assert (r.greedy[0], r.greedy[1], r.greedy[2].tolist()) == (toks, node2, fin2)
        assert torch.equal(r.allowed, C.allowed_mask(trie, node, V, t, EOS, min_new))
        node, fin = node2, fin2


@pytest.mark.parametrize("with_trie", [False, True])
def test_log_probabilities_alone_are_logprob_ref(with_trie):
    lg, trie = _logits(5), _trie()
    set_of = [0, 1, 1, 0]
    if with_trie:
        ids, _ = C.walk_greedy(lg, trie, set_of, EOS, PAD, 1)
    else:
        ids = lg.argmax(-1)
        ids[1, 4] = EOS                                          # a row that finishes
    o = S.Opts(eos=EOS, pad=PAD, min_new=1, trie=trie if with_trie else None, set_of=set_of)
    w = S.walk(lg, ids, o)
    lp, live, bound = L.walk_ref(lg, ids, EOS, 1, trie if with_trie else None, set_of)
    assert torch.equal(w.lp, lp) and torch.equal(w.live, live) and torch.equal(w.bound, bound)
    # and the processors enter neither plane: the same walk with a penalty and stop ids along the same ids
    if not with_trie:
        w2 = S.walk(lg, ids, S.Opts(eos=EOS, pad=PAD, min_new=0, penalty=1.3, stops=(V - 1,)))
        lp0, live0, _ = L.walk_ref(lg, ids, EOS, 0)
        assert torch.equal(w2.lp, lp0) and torch.equal(w2.live, live0)


def test_eos_and_min_new_alone_are_the_allowed_rows_of_logprob_ref():
    lg = _logits(6)
    lg[:, :4, EOS] = 50.0                                        # EOS is the choice of the first four steps
    o = S.Opts(eos=EOS, pad=PAD, min_new=2)
    ids = torch.zeros(B, N, dtype=torch.int64)
    w = S.walk(lg, ids, o)
    for t in range(2):
        masked = lg[:, t].masked_fill(~L.allowed_rows(V, B, t, EOS, 2), -float("inf"))
        assert torch.equal(w.greedy_ids[:, t], masked.argmax(1)) and not bool((w.greedy_ids[:, t] == EOS).any())
    r = S.step(lg[:, 2], ids, 2, [0] * B, None, o)
    assert r.greedy[0] == [EOS] * B and r.greedy[2].tolist() == [1] * B
    r = S.step(lg[:, 3], ids, 3, [1, 0, 1, 0], None, o)
    assert r.greedy[0] == [PAD, EOS, PAD, EOS]


@pytest.mark.parametrize("smp", [(0.6, 50, 0.9), (1.3, 7, 0.5), (0.8, 0, 0.95), (1.0, 5, 1.0)])
@pytest.mark.parametrize("v", [40, 1000, 4099])
def test_the_kept_set_at_margin_zero_is_sampling_probs(v, smp):
    lg = torch.randn(64, v, generator=torch.Generator().manual_seed(v)) * 3
    lg = lg[[b for b in range(lg.shape[0]) if len(set(lg[b].tolist())) == v]]        # tie-free rows only (fp32 randn repeats a value now and then)
    assert lg.shape[0] >= 48
    want = sampling_probs(lg, *smp) > 0
    everything = torch.ones(v, dtype=torch.bool)
    for b in range(lg.shape[0]):
        cls, m = S.kept_classes(lg[b], everything, smp, exact=True)
        assert m == 0.0 and not bool((cls == S.EITHER).any())
        assert torch.equal(cls == S.KEEP, want[b]), b
        # the margin only ever moves a token to EITHER, and it is the derived one
        cls2, m2 = S.kept_classes(lg[b], everything, smp)
        assert bool(((cls2 == S.KEEP) <= (cls == S.KEEP)).all()) and bool(((cls2 == S.DROP) <= (cls == S.DROP)).all())
        assert m2 == S.margin(float((lg[b].double() / smp[0]).abs().max()), v)


def test_the_margin_is_the_derived_one():
    u = 2.0 ** -24
    assert S.margin(0.0, 1) == (2 * (1 + 23) + 2) * u            # one token per thread, logits at 0: the tree, expf and the comparison alone
    assert S.margin(20.0, 32017) == (2 * (160 + 32 + 23) + 2) * u
    assert S.margin(40.0, 32017) < 1e-4                          # far below the spacing the listed inputs keep from top_p


def test_the_kept_set_within_a_trie_and_under_suppressed_eos():
    lg = torch.randn(V, generator=torch.Generator().manual_seed(8)) * 3
    allowed = torch.zeros(V, dtype=torch.bool)
    allowed[[3, 9, 20, 21, 50, 77, 120]] = True
    cls, _ = S.kept_classes(lg, allowed, (0.7, 3, 0.8))
    assert not bool(cls[~allowed].any()), "a token outside the allowed edges is kept"
    sub = sampling_probs(lg[allowed][None], 0.7, 3, 0.8)[0] > 0
    assert torch.equal(cls[allowed] == S.KEEP, sub)
    banned = lg.clone()
    banned[20] = -float("inf")                                   # what an n-gram ban leaves: never kept, counted as the smallest value
    cls, _ = S.kept_classes(banned, allowed, (0.7, 50, 1.0))
    assert int(cls[20]) == S.DROP and bool((cls[allowed & (torch.arange(V) != 20)] == S.KEEP).all())


def test_the_listed_inputs_meet_the_either_cap_by_the_reference_alone():
    """The cap of tests/test_select_chain_gpu.py on its own raw rows (before any GPU answer exists): at most 5 % of the rows hold an EITHER token."""
    for (b_, v), smp in ((s, p) for s in K.SHAPES for p in K.sampling_for(s[1])):
        raw = K._raw(b_, v)
        everything = torch.ones(v, dtype=torch.bool)
        hit = sum(int(bool((S.kept_classes(raw[s, b, :v], everything, smp)[0] == S.EITHER).any())) for s in range(K.N) for b in range(b_))
        assert hit <= K.EITHER_CAP * K.N * b_, (b_, v, smp, hit)


# ------------------------------------------------------------------ the case tables
def _pairs(c, names):
    return {((a, c[a]), (b, c[b])) for a, b in itertools.combinations(names, 2)}


def _product(axes):
    names = list(axes)
    return names, [dict(zip(names, v)) for v in itertools.product(*axes.values())]


def test_the_chain_table_covers_every_allowed_pair_and_lists_every_refused_one():
    names, everything = _product(K.AXES)
    allowed = [c for c in everything if K.refusal(c) is None]
    assert K.CASES == allowed and len(K.CASES) + len(K.REFUSED) == len(everything)
    have = set().union(*[_pairs(c, names) for c in K.CASES])
    need = set().union(*[_pairs(c, names) for c in allowed])
    assert need <= have
    every = set().union(*[_pairs(c, names) for c in everything])
    listed = set().union(*[_pairs(c, names) for c in K.REFUSED])
    assert every - need, "nothing is refused: the refusal function sees nothing"
    assert every - need <= listed and all(r["reason"] for r in K.REFUSED)
    # the pairings no test ran before this table
    for want in (dict(select="trie-greedy", proc="penalty 1.3"), dict(select="trie-sample", proc="penalty 0.7", logprobs=True),
                 dict(select="sample", proc="all three", min_new=3), dict(select="greedy", proc="penalty + 3 stops", logprobs=True, eos=K.EOS)):
        assert any(all(c[k] == v for k, v in want.items()) for c in K.CASES), want


def test_the_engine_table_covers_every_allowed_pair_and_lists_every_refused_one():
    names, everything = _product(M.AXES)
    assert all((M.refusal(c) is not None) == M.engine_refuses(c) for c in everything), "REFUSALS and the code disagree on what is refused"
    allowed = [c for c in everything if M.refusal(c) is None]
    assert all(M.refusal(c) is None for c in M.CASES) and len({tuple(c.values()) for c in M.CASES}) == len(M.CASES)
    have = set().union(*[_pairs(c, names) for c in M.CASES])
    need = set().union(*[_pairs(c, names) for c in allowed])
    assert not need - have, sorted(need - have)[:10]
    every = set().union(*[_pairs(c, names) for c in everything])
    refused_pairs = every - need
    listed = {tuple(sorted(r["axes"].items(), key=lambda kv: names.index(kv[0]))) for r in M.REFUSALS}
    assert refused_pairs and refused_pairs <= listed, sorted(refused_pairs - listed)
    # the pairings nobody ran before this table
    for want in (dict(trie=True, proc="penalty", select="greedy"), dict(trie=True, proc="penalty", select="sample"),
                 dict(trie=True, proc="penalty", logprobs=True), dict(proc="penalty+ngram", w="fp8"), dict(proc="penalty+stops", w="fp8"),
                 dict(logprobs=True, w="fp8"), dict(kv="fp8", w="fp8", trie=True, logprobs=True), dict(proc="penalty+stops", entry="shared"),
                 dict(proc="penalty+ngram", entry="streams"), dict(trie=True, entry="coalesced", proc="penalty")):
        assert any(all(c[k] == v for k, v in want.items()) for c in M.CASES), want
