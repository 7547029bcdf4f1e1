"""crab_constrained_select through ops.constrained_select on synthetic logits: greedy exact against the CPU reference walk (tests/constrain_ref.py),
the identity trie against crab_greedy_select / crab_sample_select, the sampling distribution against HF's warpers over the allowed subset
(oracle.sampling_probs), and corrupt trie arrays handled as "not allowed" without a write outside the row's words."""
import functools
import types

import numpy as np
import pytest
import torch

from crab_amd.constrain import TokenTrie
from tests import constrain_ref as R

pytestmark = pytest.mark.gpu
EOS, PAD = 2, 1


def _dev(trie):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    return up(trie.edge_off), up(trie.edge_tok), up(trie.edge_dst)


def _run(logits, arrays, nodes, finished, step, min_new, eos=EOS, sampling=None, n_cols=4):
    """One call on fresh per-row words, each with a sentinel word before and after: (tokens, nodes, finished) as lists."""
    from crab_amd import ops
    B = logits.shape[0]
    S = -77
    node = torch.full((B + 2,), S, dtype=torch.int32, device="cuda")
    node[1:B + 1] = torch.tensor(nodes, dtype=torch.int32)
    fin = torch.full((B + 2,), S, dtype=torch.int32, device="cuda")
    fin[1:B + 1] = torch.tensor(finished, dtype=torch.int32)
    cur = torch.full((B + 2,), S, dtype=torch.int64, device="cuda")
    out = torch.full((B + 2, n_cols), S, dtype=torch.int64, device="cuda")
    sd = torch.tensor([step], dtype=torch.int32, device="cuda")
    before = logits.clone()
    t, k, p, seed = sampling if sampling is not None else (0.0, 0, 1.0, 0)
    ops.constrained_select(logits, *arrays, node[1:B + 1], cur[1:B + 1], out[1:B + 1], sd, fin[1:B + 1], eos, PAD, min_new, t, k, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(logits, before), "the logits are read only"
    for w in (node, fin, cur):
        assert int(w[0]) == S and int(w[-1]) == S, "a neighbour of the per-row words was written"
    assert bool((out[0] == S).all()) and bool((out[-1] == S).all())
    assert torch.equal(out[1:B + 1, step], cur[1:B + 1])
    cols = [c for c in range(n_cols) if c != step]
    assert bool((out[1:B + 1][:, cols] == S).all()), "only column `step` of out_ids is written"
    return cur[1:B + 1].tolist(), node[1:B + 1].tolist(), fin[1:B + 1].tolist()


@functools.lru_cache(maxsize=None)
def _greedy_case(V):
    """37 rows at different nodes of a forest of 3 sets: set 0 random with shared prefixes, set 1 a root with as many edges as V allows up to
    1500 (plus deeper members), set 2 one sequence (nodes with ONE edge)."""
    rng = np.random.default_rng(V)
    wide = min(1500, V - 8)
    toks = [t for t in rng.permutation(np.arange(3, V)).tolist()]
    set1 = [[t] for t in toks[:wide]] + [[toks[0], toks[1]], [toks[0], toks[2], toks[3]]]
    set2 = [[toks[4], toks[5], toks[6]]]
    sets = [R.random_sets(rng, 1, V, EOS)[0], set1, set2]
    trie = TokenTrie(sets, V, EOS)
    B = 37
    r0, r1, r2 = (int(r) for r in trie.roots)
    one_edge = trie._walk(2, set2[0][:1])
    leaf = trie._walk(2, set2[0])                               # only the EOS edge
    both = trie._walk(1, [toks[0]])                             # children and the EOS edge
    nodes = [r0, r1, r2, one_edge, leaf, both, trie.sink, r1, r0, both, leaf] + [int(n) for n in rng.integers(0, trie.n_nodes, B - 11)]
    finished = [0] * B
    finished[7], finished[8], finished[20] = 1, 1, 1            # finished rows: pad, node kept
    g = torch.Generator().manual_seed(V + 1)
    lg = torch.randn(B, V, generator=g)
    lg[:, EOS] = 30.0                                           # EOS wins wherever it is allowed: its suppression below min_new_tokens shows
    al = lambda b: [t for t, _ in R.allowed_tokens(trie, nodes[b], V, 9, EOS, 0) if t != EOS]
    a = al(1)                                                   # the widest node: a tie between two allowed tokens, both above the rest
    lo, hi = sorted((a[3], a[len(a) // 2]))
    lg[1, lo] = lg[1, hi] = 20.0
    a0 = al(0)
    lg[0, a0[0]] = -float("inf")                                # an allowed token at -inf
    for b in range(B):                                          # the global argmax outside the allowed set
        ok = set(t for t, _ in R.allowed_tokens(trie, nodes[b], V, 9, EOS, 0))
        outside = next(t for t in range(3, V) if t not in ok)
        lg[b, outside] = 50.0
    return trie, nodes, finished, lg, (lo, hi)


@pytest.mark.parametrize("V", [40, 300, 32017])
def test_greedy_is_exact_against_the_reference_walk(V):
    trie, nodes, finished, lg, (lo, hi) = _greedy_case(V)
    n_edges = [int(trie.edge_off[n + 1] - trie.edge_off[n]) for n in nodes]
    assert 1 in n_edges and 0 in n_edges and max(n_edges) == min(1500, V - 8), n_edges      # 1500 edges wherever the vocabulary holds them
    arrays = _dev(trie)
    logits = lg.cuda()
    for step, min_new in [(0, 0), (1, 2), (2, 2)]:
        want = R.select_step(lg, trie, nodes, finished, step, EOS, PAD, min_new)
        got = _run(logits, arrays, nodes, finished, step, min_new)
        assert got[0] == want[0], (step, min_new)
        assert got[1] == want[1] and got[2] == want[2], (step, min_new)
        toks, nn, ff = got
        assert toks[1] == lo, "two allowed tokens with bit-equal logits: the lower id wins"
        assert toks[6] == PAD and ff[6] == 1 and nn[6] == trie.sink, "the sink: pad, finished"
        for b in (7, 8, 20):
            assert toks[b] == PAD and nn[b] == nodes[b] and ff[b] == 1, "a finished row emits pad and keeps its node"
        if step < min_new:
            assert EOS not in toks and toks[4] == PAD and ff[4] == 1, "EOS suppressed: the leaf has nothing allowed"
            assert toks[5] != EOS and ff[5] == 0
        else:
            assert toks[4] == EOS and toks[5] == EOS and nn[4] == trie.sink and ff[4] == ff[5] == 1
        assert all(t != int(lg[b].argmax()) for b, t in enumerate(toks)), "the global argmax lies outside every allowed set"


def test_three_calls_walk_a_member_end_to_end():
    from crab_amd import ops
    V = 300
    member = [17, 250, 9]
    trie = TokenTrie([[member, [17, 40], [250]], [[9, 9]]], V, EOS)
    arrays = _dev(trie)
    B = 3
    g = torch.Generator().manual_seed(4)
    lg = torch.randn(B, V, generator=g) * 0.1
    lg[:, 17] += 8; lg[:, 250] += 6; lg[:, 9] += 4; lg[:, EOS] += 2; lg[:, 40] -= 3
    logits = lg.cuda()
    node = torch.tensor([int(trie.roots[0]), int(trie.roots[1]), int(trie.roots[0])], dtype=torch.int32, device="cuda")
    cur = torch.zeros(B, dtype=torch.int64, device="cuda")
    out = torch.full((B, 6), -1, dtype=torch.int64, device="cuda")
    fin = torch.zeros(B, dtype=torch.int32, device="cuda")
    sd, pos = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(6):
        ops.constrained_select(logits, *arrays, node, cur, out, sd, fin, EOS, PAD, 0)
        ops.advance(pos, sd)
    want, nodes = R.walk_greedy(lg[:, None].expand(B, 6, V), trie, [0, 1, 0], EOS, PAD)
    assert out[0].tolist() == member + [EOS, PAD, PAD] and out[1].tolist() == [9, 9, EOS, PAD, PAD, PAD]
    assert torch.equal(out.cpu(), want) and node.tolist() == nodes == [trie.sink] * 3 and fin.tolist() == [1, 1, 1] and int(sd) == 6


@pytest.mark.parametrize("V", [300, 32017])
def test_identity_trie_equals_the_unconstrained_kernels(V):
    """One node whose edges are all V tokens in order: crab_greedy_select bit for bit, crab_sample_select draw for draw."""
    from crab_amd import ops
    B = 64
    ident = types.SimpleNamespace(edge_off=np.array([0, V, V]), edge_tok=np.arange(V), edge_dst=np.ones(V))
    arrays = _dev(ident)
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(B, V, generator=g) * 1.5).cuda()
    logits[3, 11] = logits[3, 200] = 9.0                         # a tie: the first maximum
    eos = 7

    def plain(step, min_new, sampling):
        cur = torch.zeros(B, dtype=torch.int64, device="cuda")
        out = torch.full((B, 4), -77, dtype=torch.int64, device="cuda")
        fin = torch.zeros(B, dtype=torch.int32, device="cuda")
        sd = torch.tensor([step], dtype=torch.int32, device="cuda")
        if sampling is None:
            ops.greedy_select(logits, cur, out, sd, fin, eos, PAD, min_new)
        else:
            ops.sample_select(logits, cur, out, sd, fin, eos, PAD, min_new, *sampling)
        return cur.tolist(), fin.tolist()

    for step, min_new in [(0, 0), (1, 0), (0, 1)]:
        for sampling in (None, (0.6, 50, 0.9, 1234), (1.3, 0, 0.5, 1234), (0.6, 50, 0.9, 99)):
            toks, nodes, fin = _run(logits, arrays, [0] * B, [0] * B, step, min_new, eos=eos, sampling=sampling)
            ptoks, pfin = plain(step, min_new, sampling)
            assert toks == ptoks and fin == pfin, (step, min_new, sampling)
            assert nodes == [1] * B


@functools.lru_cache(maxsize=None)
def _sampling_case(V, n_allowed):
    """Logits, one node with n_allowed edges and the HF distribution over the allowed subset.  The seed is the first for which the kept set
    (after top-k 50 / top-p 0.9 at temperature 0.6) holds at least two tokens: decided here, on the CPU reference."""
    from oracle import crab_oracle as O
    for seed in range(V, V + 50):
        g = torch.Generator().manual_seed(seed)
        lg = torch.randn(1, V, generator=g) * 1.2
        allowed = sorted(torch.randperm(V - 3, generator=g)[:n_allowed].add(3).tolist())
        masked = lg.masked_fill(~torch.zeros(1, V, dtype=torch.bool).index_fill(1, torch.tensor(allowed), True), -float("inf"))
        probs = O.sampling_probs(masked, 0.6, 50, 0.9)[0]
        if int((probs > 0).sum()) >= 2:
            return lg, allowed, masked, probs
    raise AssertionError("no seed with a kept set of two tokens")


@pytest.mark.parametrize("V,n_allowed", [(300, 23), (32017, 400)])
def test_sampling_draws_from_the_hf_distribution_over_the_allowed_subset(V, n_allowed):
    """As test_sample_select_draws_from_the_hf_distribution, over the allowed subset: 16384 rows of the same logits at one node - no draw
    outside the kept set, total-variation distance < 3 %, every kept token with p >= 2 % drawn (that test's bounds for this draw count);
    deterministic per (seed, step); top_k = 1 is the constrained argmax."""
    lg, allowed, masked, probs = _sampling_case(V, n_allowed)
    assert int((probs > 0).sum()) >= 2, "test input too peaked: the kept set must hold several tokens"
    assert float(probs[[t for t in range(V) if t not in set(allowed)]].sum()) == 0.0
    N = 16384
    trie = TokenTrie([[[t] for t in allowed]], V, EOS)
    arrays = _dev(trie)
    root = int(trie.roots[0])
    logits = lg.cuda().expand(N, V)                             # row stride 0: the rows are only read
    from crab_amd import ops

    def draw(seed, step, kk=50, pp=0.9, tt=0.6):
        node = torch.full((N,), root, dtype=torch.int32, device="cuda")
        cur = torch.zeros(N, dtype=torch.int64, device="cuda")
        out = torch.full((N, 4), -1, dtype=torch.int64, device="cuda")
        fin = torch.zeros(N, dtype=torch.int32, device="cuda")
        sd = torch.tensor([step], dtype=torch.int32, device="cuda")
        ops.constrained_select(logits, *arrays, node, cur, out, sd, fin, EOS, PAD, 0, tt, kk, pp, seed)
        assert torch.equal(out[:, step], cur) and not bool(fin.any())
        return cur.cpu()
    a = draw(1234, 0)
    assert torch.equal(a, draw(1234, 0)), "not deterministic for a given (seed, step)"
    assert not torch.equal(a, draw(1234, 1)) and not torch.equal(a, draw(99, 0))
    hist = torch.bincount(a, minlength=V).float() / N
    assert float(hist[probs == 0].sum()) == 0.0, "a token outside the kept set was drawn"
    tv = 0.5 * float((hist - probs).abs().sum())
    print(f"constrained_select V={V} allowed={n_allowed}: total-variation distance of {N} draws = {tv:.4f}, kept tokens = {int((probs > 0).sum())}")
    assert tv < 3e-2, tv
    assert bool((hist[probs >= 0.02] > 0).all())
    assert torch.equal(draw(7, 2, kk=1), torch.full((N,), int(masked.argmax()), dtype=torch.int64))


def test_corrupt_arrays_count_as_not_allowed():
    """node[b] past the node table and an edge token equal to V: the row is handled as "not allowed" (pad + finished; the bad edge skipped),
    the other rows are unaffected, and the neighbours of out_ids / cur_ids / node keep their sentinels (_run)."""
    V = 300
    trie, nodes, finished, lg, _ = _greedy_case(V)
    B = len(nodes)
    logits = lg.cuda()
    for sampling in (None, (0.6, 50, 0.9, 5)):
        clean = _run(logits, _dev(trie), nodes, finished, 1, 0, sampling=sampling)
        bad_nodes = list(nodes)
        bad_nodes[0] = trie.n_nodes + 5
        bad_nodes[2] = -3
        got = _run(logits, _dev(trie), bad_nodes, finished, 1, 0, sampling=sampling)
        for b in range(B):
            if b in (0, 2):
                assert got[0][b] == PAD and got[2][b] == 1 and got[1][b] == bad_nodes[b]
            else:
                assert all(got[j][b] == clean[j][b] for j in range(3)), b
    # the edge the widest row (row 1) chose now carries token V: it is skipped, the row takes the best of the rest
    want = R.select_step(lg, trie, nodes, finished, 1, EOS, PAD, 0)
    e = next(e for e in range(int(trie.edge_off[nodes[1]]), int(trie.edge_off[nodes[1] + 1])) if int(trie.edge_tok[e]) == want[0][1])
    broken = types.SimpleNamespace(edge_off=trie.edge_off, edge_tok=trie.edge_tok.copy(), edge_dst=trie.edge_dst, roots=trie.roots)
    broken.edge_tok[e] = V
    want2 = R.select_step(lg, broken, nodes, finished, 1, EOS, PAD, 0)
    got2 = _run(logits, _dev(broken), nodes, finished, 1, 0)
    assert got2[0] == want2[0] and got2[1] == want2[1] and got2[2] == want2[2]
    assert got2[0][1] != want[0][1] and 0 <= got2[0][1] < V
    others = [b for b in range(B) if nodes[b] != nodes[1]]
    assert all(got2[0][b] == want[0][b] for b in others)
    # an edge range that runs past the edge table is cut at n_edges (the last node is set 2's leaf: rows 4 and 10 stand on it)
    assert nodes[4] == trie.n_nodes - 1
    cut = types.SimpleNamespace(edge_off=trie.edge_off.copy(), edge_tok=trie.edge_tok, edge_dst=trie.edge_dst)
    cut.edge_off[-1] = trie.n_edges + 4096
    got3 = _run(logits, _dev(cut), nodes, finished, 1, 0)
    assert got3[0] == want[0]
