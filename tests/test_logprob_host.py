"""CPU-side checks of the per-token log-probabilities of the decode step: the fp64 reference (tests/logprob_ref.py) against torch.log_softmax
and, on a hand-made trie, against constrain_ref.allowed_mask; the C-ABI boundary of crab_logprob_norm / crab_logprob_gather (no device needed);
the row bookkeeping of the public fields."""
import ctypes as C
import os
import re
import types

import torch

from crab_amd import _lib
from crab_amd.constrain import TokenTrie
from tests import constrain_ref as R
from tests import logprob_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 1


def test_reference_equals_log_softmax_without_a_constraint():
    g = torch.Generator().manual_seed(1)
    z = torch.randn(5, 97, generator=g) * 4
    y = torch.randint(0, 97, (5,), generator=g)
    y[2] = EOS
    lp, live, bound = L.step_ref(z, y, 3, [0, 0, 0, 1, 0], EOS, 0)
    want = torch.log_softmax(z.double(), -1).gather(1, y[:, None])[:, 0]
    assert live.tolist() == [True, True, True, False, True]
    keep = torch.tensor([0, 1, 2, 4])
    assert torch.equal(lp[0], lp[1]), "nothing is suppressed at step >= min_new: one normaliser"
    assert float((lp[0][keep] - want[keep]).abs().max()) < 1e-12
    assert float(lp[0, 3]) == 0.0 and float(lp[1, 3]) == 0.0 and float(bound[0, 3]) == 0.0
    assert bool((bound[:, keep] >= 8 * L.EPS).all())
    # EOS suppressed: the allowed plane is the log-softmax of the row with EOS at -inf, the raw plane does not move
    y2 = y.clone()
    y2[2] = 7
    lp2, live2, _ = L.step_ref(z, y2, 0, [0] * 5, EOS, 2)
    zm = z.double().clone()
    zm[:, EOS] = -float("inf")
    assert float((lp2[1] - torch.log_softmax(zm, -1).gather(1, y2[:, None])[:, 0]).abs().max()) < 1e-12
    assert float((lp2[0] - torch.log_softmax(z.double(), -1).gather(1, y2[:, None])[:, 0]).abs().max()) < 1e-12
    assert bool((lp2[1] > lp2[0]).all()) and bool(live2.all())
    # a chosen token outside the vocabulary has no value, the row is live all the same
    lp3, live3, _ = L.step_ref(z, [97, -1, 0, 0, 0], 0, [0] * 5, EOS, 0)
    assert lp3[:, :2].abs().sum() == 0 and bool(live3.all())


def test_reference_equals_the_masked_log_softmax_on_a_hand_made_trie():
    V = 12
    trie = TokenTrie([[[5, 6, 7], [5, 6, 9], [5, 8], [5], [4, 6, 7]], [[5, 6], [7]]], V, EOS)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(4, V, generator=g) * 3
    n56 = trie._walk(0, [5, 6])
    n5 = trie._walk(0, [5])
    nodes = [int(trie.roots[0]), n5, n56, int(trie.roots[1])]
    for step, min_new in [(0, 0), (1, 2), (3, 2)]:
        mask = R.allowed_mask(trie, nodes, V, step, EOS, min_new)
        y = [int(mask[b].nonzero()[0, 0]) for b in range(4)]
        lp, live, _ = L.step_ref(z, y, step, [0] * 4, EOS, min_new, trie, nodes)
        want = torch.log_softmax(z.double().masked_fill(~mask, -float("inf")), -1)
        raw = torch.log_softmax(z.double(), -1)
        for b in range(4):
            assert abs(float(lp[1, b] - want[b, y[b]])) < 1e-12 and abs(float(lp[0, b] - raw[b, y[b]])) < 1e-12
        assert bool(live.all())
    # node [5] allows {6, 8, EOS}: with EOS suppressed two tokens are left
    assert sorted(t for t, _ in R.allowed_tokens(trie, n5, V, 0, EOS, 1)) == [6, 8]
    # the sink, a node outside the trie: nothing allowed, not live, zeros
    sink = trie._walk(0, [5, 8, EOS])
    lp, live, _ = L.step_ref(z[:2], [3, 3], 0, [0, 0], EOS, 0, trie, [sink, trie.n_nodes + 3])
    assert live.tolist() == [False, False] and float(lp.abs().sum()) == 0.0


def test_walk_follows_the_ids():
    """Over recorded steps: the EOS column is a token, the columns after it are not; pad == eos changes nothing."""
    V = 9
    g = torch.Generator().manual_seed(4)
    lg = torch.randn(2, 4, V, generator=g)
    ids = torch.tensor([[3, EOS, EOS, EOS], [4, 5, 6, 7]])
    lp, live, _ = L.walk_ref(lg, ids, EOS)
    assert live.tolist() == [[True, True, False, False], [True] * 4]
    assert float(lp[0, 0, 1]) != 0.0 and float(lp[:, 0, 2:].abs().sum()) == 0.0
    trie = TokenTrie([[[3, 4]], [[5]]], V, EOS)
    ids = torch.tensor([[3, 4, EOS, 2], [5, EOS, 2, 2]])
    lp, live, _ = L.walk_ref(lg, ids, EOS, 0, trie, [0, 1])
    assert live.tolist() == [[True, True, True, False], [True, True, False, False]]
    assert float(lp[1].abs().sum()) == 0.0, "one edge everywhere: probability 1 within the set"
    assert bool((lp[0][live] < 0).all())


def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_logprob_norm", "crab_logprob_gather"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert "compute_transition_scores" in txt
    assert lib.crab_abi_version() == 13


def test_entry_points_reject_null_context_and_operands_without_a_gpu():
    lib = _lib.load()
    assert lib.crab_logprob_norm(None, None, None, 0, 1, 8, None, None, 0, 0, None, None, None, 1, 0, None) < 0
    assert lib.crab_logprob_gather(None, None, None, 0, 1, 8, None, None, None, None, 4, 4, 4) < 0
    # a zeroed block stands in for a context (crab_fail writes its message there): the refusals are reached without a device
    ctx = C.create_string_buffer(1 << 16)
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.crab_logprob_norm(h, None, None, 0, 1, 8, None, None, 0, 0, None, None, None, 1, 0, None) == -1
    assert b"logprob_norm" in ctx.raw
    for B, V, ldl in [(0, 8, 8), (1, 0, 8), (1, 8, -1)]:
        assert lib.crab_logprob_norm(h, None, one, ldl, B, V, None, None, 0, 0, None, one, one, 1, 0, one) == -1
    for eo, et, nd, nn, ne in [(one, None, None, 1, 1), (None, one, one, 1, 1), (one, one, None, 1, 1), (one, one, one, 0, 1), (one, one, one, 1, 0)]:
        ctx.raw = bytes(len(ctx.raw))
        assert lib.crab_logprob_norm(h, None, one, 8, 1, 8, eo, et, nn, ne, nd, one, one, 1, 0, one) == -1
        assert b"come together" in ctx.raw
    for missing in range(4):                                   # logits, step_dev, finished, norm
        a = [one] * 4
        a[missing] = None
        assert lib.crab_logprob_norm(h, None, a[0], 8, 1, 8, None, None, 0, 0, None, a[1], a[2], 1, 0, a[3]) == -1
    ctx.raw = bytes(len(ctx.raw))
    assert lib.crab_logprob_gather(h, None, None, 8, 1, 8, one, one, one, one, 4, 4, 4) == -1
    assert b"logprob_gather" in ctx.raw
    for missing in range(5):                                   # logits, cur_ids, step_dev, norm, lp
        a = [one] * 5
        a[missing] = None
        assert lib.crab_logprob_gather(h, None, a[0], 8, 1, 8, a[1], a[2], a[3], a[4], 4, 4, 4) == -1
    for B, V, ld, plane, n in [(0, 8, 4, 4, 4), (1, 0, 4, 4, 4), (1, 8, 4, 4, 0), (1, 8, 3, 4, 4), (1, 8, 4, -1, 4)]:
        assert lib.crab_logprob_gather(h, None, one, 8, B, V, one, one, one, one, ld, plane, n) == -1


def test_public_fields_from_the_engine_scores():
    from crab_amd.unified_llama import _fill_logprob_fields, _logprob_output
    ids = torch.tensor([[4, EOS, EOS, EOS], [5, 6, 7, 8], [EOS, EOS, EOS, EOS]])
    lp = torch.zeros(3, 4, 2)
    lp[0, :2] = torch.tensor([[-1.0, -0.5], [-2.0, -0.25]])
    lp[1] = -1.0
    lp[2, 0] = torch.tensor([-3.0, 0.0])
    out = types.SimpleNamespace()
    _fill_logprob_fields(out, ids, lp, EOS)
    assert out.num_tokens.tolist() == [2, 4, 1] and out.num_tokens.dtype == torch.int32
    assert out.sum_logprob.tolist() == [-3.0, -4.0, -3.0] and out.sum_logprob_allowed.tolist() == [-0.75, -4.0, 0.0]
    assert tuple(out.token_logprobs.shape) == tuple(out.token_logprobs_allowed.shape) == (3, 4)
    _fill_logprob_fields(out, ids, lp, None)
    assert out.num_tokens.tolist() == [4, 4, 4]
    r = _logprob_output((ids, torch.ones(3, 9), lp), True, [EOS])
    assert torch.equal(r.sequences, ids) and tuple(r.first_logits.shape) == (3, 9) and r.num_tokens.tolist() == [2, 4, 1]
