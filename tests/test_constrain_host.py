"""CPU-side checks of closed-set generation: the token trie (crab_amd/constrain.py) against hand-written sets, its refusals by name, the host
walker pinned to transformers' PrefixConstrainedLogitsProcessor, and the C-ABI boundary of crab_constrained_select (no device needed)."""
import os
import re

import numpy as np
import pytest
import torch

from crab_amd import _lib
from crab_amd.constrain import TokenTrie, as_trie, rows_of
from tests import constrain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 1
SETS = [
    [[5, 6, 7], [5, 6, 9], [5, 8], [5], [4, 6, 7], [5, 8]],      # shared prefixes, [5] a proper prefix of three others, [5, 8] twice
    [[5, 6], [7]],                                               # shares tokens with set 0, not nodes
]


def _members(seqs):
    return sorted({tuple(s) for s in seqs})


def test_trie_construction_on_hand_written_sets():
    t = TokenTrie(SETS, 12, EOS)
    assert t.edge_off.dtype == t.edge_tok.dtype == t.edge_dst.dtype == t.roots.dtype == np.int32
    assert t.n_sets == 2 and t.n_nodes == len(t.edge_off) - 1 and t.n_edges == len(t.edge_tok) == len(t.edge_dst)
    assert t.edge_off[0] == 0 and t.edge_off[-1] == t.n_edges and bool((np.diff(t.edge_off) >= 0).all())
    # set 0: root, 5, 56, 567, 569, 58, 4, 46, 467 = 9 nodes; set 1: root, 5, 56, 7 = 4; one shared sink
    assert t.n_nodes == 9 + 4 + 1
    for n in range(t.n_nodes):
        toks = t.edge_tok[t.edge_off[n]:t.edge_off[n + 1]]
        assert bool((np.diff(toks) > 0).all()), "edges ascending (and distinct) within a node"
    sinks = [n for n in range(t.n_nodes) if t.edge_off[n] == t.edge_off[n + 1]]
    assert sinks == [t.sink], "one shared sink node without edges"
    eos_edges = [e for e in range(t.n_edges) if t.edge_tok[e] == EOS]
    assert all(t.edge_dst[e] == t.sink for e in eos_edges) and all(t.edge_tok[e] == EOS for e in range(t.n_edges) if t.edge_dst[e] == t.sink)
    assert len(eos_edges) == len(_members(SETS[0])) + len(_members(SETS[1])), "the EOS edge exactly at the ends of sequences (duplicates merged)"
    for si, seqs in enumerate(SETS):
        mem = _members(seqs)
        prefixes = {m[:k] for m in mem for k in range(len(m) + 1)}
        for p in prefixes:
            want = sorted({m[len(p)] for m in mem if len(m) > len(p) and m[:len(p)] == p} | ({EOS} if p in mem else set()))
            assert t.allowed(si, list(p)) == want, (si, p)
        for m in mem:
            assert t.allowed(si, list(m) + [EOS]) == [] and t.is_member(si, m)
    assert t.allowed(0, [5]) == [EOS, 6, 8]                      # proper prefix of others: children AND the EOS edge, in sorted position
    assert t.allowed(0, [7]) == [] and t.allowed(0, [5, 7]) == [] and t.allowed(1, [5, 8]) == [] and t.allowed(1, [4]) == []
    assert t.allowed(1, []) == [5, 7] and t.allowed(1, [5]) == [6], "set 1 walks its own nodes"
    assert not t.is_member(0, [5, 6]) and not t.is_member(1, [5])
    assert t.min_len == 1
    assert TokenTrie(SETS, 12, EOS).key == t.key and TokenTrie(SETS[:1], 12, EOS).key != t.key


def test_every_refusal_by_name():
    with pytest.raises(ValueError, match="set 1 is empty"):
        TokenTrie([[[3]], []], 10, EOS)
    with pytest.raises(ValueError, match="empty sequence"):
        TokenTrie([[[3], []]], 10, EOS)
    with pytest.raises(ValueError, match="no answer set"):
        TokenTrie([], 10, EOS)
    for bad in (10, 11, -1):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            TokenTrie([[[3, bad]]], 10, EOS)
    with pytest.raises(ValueError, match="contains the EOS id"):
        TokenTrie([[[3, EOS, 4]]], 10, EOS)
    with pytest.raises(ValueError, match="eos_token_id is None"):
        TokenTrie([[[3]]], 10, None)
    with pytest.raises(ValueError, match="ONE EOS id"):
        TokenTrie([[[3]]], 10, [1, 2])
    with pytest.raises(ValueError, match="min_new_tokens = 3 exceeds the shortest"):
        TokenTrie([[[3, 4, 5]], [[3, 4]]], 10, EOS, min_new_tokens=3)
    t = TokenTrie([[[3, 4, 5]], [[3, 4]]], 10, EOS, min_new_tokens=2)
    t.check(EOS, 2, 10); t.check([EOS], 0)
    with pytest.raises(ValueError, match="min_new_tokens"):
        t.check(EOS, 3)
    with pytest.raises(ValueError, match="eos_token_id"):
        t.check(None, 0)
    with pytest.raises(ValueError, match="eos_token_id"):
        t.check(2, 0)
    with pytest.raises(ValueError, match="vocab_size"):
        t.check(EOS, 0, 11)


def test_allowed_sequences_forms_and_row_mapping():
    one = as_trie([[3, 4], [5]], 10, EOS)
    assert one.n_sets == 1 and one.allowed(0, []) == [3, 5]
    assert as_trie([torch.tensor([3, 4]), torch.tensor([5])], 10, EOS).key == one.key
    two = as_trie([[[3, 4], [5]], [[6]]], 10, EOS)
    assert two.n_sets == 2 and two.allowed(1, []) == [6]
    assert as_trie(two, 10, EOS) is two
    with pytest.raises(ValueError, match="eos_token_id"):
        as_trie(two, 10, None)
    assert rows_of(one, None, 3) == [0, 0, 0] and rows_of(two, [1, 0, 1], 3) == [1, 0, 1] and rows_of(two, torch.tensor([1, 0]), 2) == [1, 0]
    with pytest.raises(ValueError, match="holds 2 sets"):
        rows_of(two, None, 3)
    with pytest.raises(ValueError, match="2 set indices for 3 rows"):
        rows_of(two, [0, 1], 3)
    with pytest.raises(ValueError, match="outside"):
        rows_of(two, [0, 2, 0], 3)


class _StubTokenizer:
    """tokenize = whitespace split, ids from a fixed table: what the reference's rule needs and nothing else."""
    eos_token_id = EOS
    table = {"yes": 3, "no": 4, "two": 5, "pia": 6, "no_": 7, "acc": 8, "ordion": 9}

    def __len__(self):
        return 12

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [self.table[t] for t in toks]


def test_from_strings_uses_the_reference_rule():
    tok = _StubTokenizer()
    t = TokenTrie.from_strings(tok, ["yes", "no", "pia no_", "acc ordion"])
    assert t.vocab_size == 12 and t.eos_token_id == EOS and t.n_sets == 1
    assert t.allowed(0, []) == [3, 4, 6, 8] and t.allowed(0, [6]) == [7] and t.allowed(0, [6, 7]) == [EOS]
    t2 = TokenTrie.from_strings(tok, [["yes", "no"], ["two"]], vocab_size=12, eos_token_id=EOS)
    assert t2.n_sets == 2 and t2.allowed(1, []) == [5]


def test_host_walker_is_pinned_to_hf_prefix_constrained_processor():
    """For random logits [4, 320] and random generated prefixes: HF's PrefixConstrainedLogitsProcessor fed with TokenTrie.allowed leaves
    finite exactly the trie's mask, and the reference greedy walker chooses the argmax of HF's processed scores (no ties in the input)."""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    V, eos = 320, 2
    rng = np.random.default_rng(11)
    sets = R.random_sets(rng, 3, V, eos)
    trie = TokenTrie(sets, V, eos)
    g = torch.Generator().manual_seed(3)
    checked = 0
    for depth in range(0, 4):
        set_of, prefixes = [], []
        for b in range(4):
            si = int(rng.integers(0, 3))
            cands = [s for s in sets[si] if len(s) >= depth]
            if not cands:
                si, cands = next((i, [s for s in ss if len(s) >= depth]) for i, ss in enumerate(sets) if any(len(s) >= depth for s in ss))
            set_of.append(si); prefixes.append(cands[int(rng.integers(0, len(cands)))][:depth])
        scores = torch.randn(4, V, generator=g)
        assert scores.unique().numel() == scores.numel()
        prefix = torch.tensor(prefixes, dtype=torch.int64).reshape(4, depth)
        hf = PrefixConstrainedLogitsProcessor(lambda b, ids: trie.allowed(set_of[b], ids.tolist()), 1)(prefix, scores.clone())
        nodes = [trie._walk(set_of[b], prefixes[b]) for b in range(4)]
        mask = R.allowed_mask(trie, nodes, V, depth, eos, 0)
        assert torch.equal(hf, scores.masked_fill(~mask, -float("inf")))
        toks, _, _ = R.select_step(scores, trie, nodes, [0] * 4, depth, eos, 0, 0)
        assert toks == hf.argmax(-1).tolist()
        checked += 4
    assert checked == 16


def test_symbol_is_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    assert re.search(r"^int\s+crab_constrained_select\s*\(", txt, flags=re.M) and "PrefixConstrainedLogitsProcessor" in txt
    assert hasattr(lib, "crab_constrained_select") and "crab_constrained_select" in _lib.SYMBOLS
    assert lib.crab_abi_version() == 13


def test_entry_point_rejects_null_context_and_operands_without_a_gpu():
    import ctypes as C
    lib = _lib.load()
    f, u = C.c_float, C.c_uint64
    assert lib.crab_constrained_select(None, None, None, 0, 1, 8, None, None, None, 1, 1, None, None, None, 1, None, None, 1, 0, 0, f(0.0), 0, f(1.0), u(0)) < 0
    # a context is plain host memory to the validation (crab_fail writes its message there): a zeroed block stands in for one, so the refusals
    # of null operands and bad sizes are reached without a device - no HIP call may precede them
    ctx = C.create_string_buffer(1 << 16)
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.crab_constrained_select(h, None, None, 0, 1, 8, None, None, None, 1, 1, None, None, None, 1, None, None, 1, 0, 0, f(0.0), 0, f(1.0), u(0)) < 0
    assert b"constrained_select" in ctx.raw
    for B, V, nn, ne, t, k, p in [(0, 8, 1, 1, 0.0, 0, 1.0), (1, 0, 1, 1, 0.0, 0, 1.0), (1, 8, 0, 1, 0.0, 0, 1.0), (1, 8, 1, 0, 0.0, 0, 1.0),
                                  (1, 8, 1, 1, -1.0, 0, 1.0), (1, 8, 1, 1, 0.5, -1, 1.0), (1, 8, 1, 1, 0.5, 0, 0.0), (1, 8, 1, 1, 0.5, 0, 1.5)]:
        assert lib.crab_constrained_select(h, None, one, 8, B, V, one, one, one, nn, ne, one, one, one, 1, one, one, 1, 0, 0, f(t), k, f(p), u(0)) < 0, (B, V, nn, ne, t, k, p)
