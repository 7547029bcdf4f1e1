"""Closed-set generation at the engine and the public surface (generate / generate_batches / generate_questions with allowed_sequences /
allowed_set) on the tiny models of scripts/fuzz_engine_state.py (Llama V = 320, Qwen2 V = 515): the subset property against free decoding, the
reference walk (tests/constrain_ref.py) over the call's own step logits, membership in every mode, the state a call carries (node reset, graph
capture, graph key) and the row mapping wherever rows are split or merged.

The answer sets of one test draw their tokens from disjoint id ranges, one range per set: a row that walked another row's set cannot pass the
membership check."""
import functools
import os
import runpy

import numpy as np
import pytest
import torch

from crab_amd.constrain import TokenTrie
from tests import constrain_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EOS, PAD = 1, 2


@functools.lru_cache(maxsize=None)
def _model(qwen=False):
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    model = ns["build"](qwen)
    um = model.base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


def _sets(n_sets, V, seed, first=10):
    """n_sets answer sets of 5 sequences of 1-4 tokens; set i draws from 6 ids of its own range [first + i * span, first + (i + 1) * span)."""
    rng = np.random.default_rng(seed)
    span = (V - first) // n_sets
    sets = []
    for i in range(n_sets):
        alphabet = (first + i * span + rng.permutation(span)[:6]).tolist()
        sets.append([[int(rng.choice(alphabet)) for _ in range(int(rng.integers(1, 5)))] for _ in range(5)])
    return sets


def _assert_members(ids, trie, set_of, what=""):
    ids = ids.cpu()
    assert ids.shape[0] == len(set_of)
    for b, s in enumerate(set_of):
        row = ids[b].tolist()
        assert EOS in row, f"{what} row {b}: no EOS in {row}"
        cut = R.cut_at_eos(row, EOS)
        assert trie.is_member(s, cut), f"{what} row {b}: {cut} is no member of set {s}"
        assert all(t == PAD for t in row[len(cut) + 1:]), f"{what} row {b}: {row} is not padded after EOS"


def test_subset_property_against_free_decoding():
    """An argmax over a subset that contains the global argmax is that argmax: rows constrained to their own free continuation plus decoys
    return exactly that continuation, then EOS, then pad."""
    um, hid, V = _model()
    emb = _emb(3, 6, hid, 21)
    free = um.generate(inputs_embeds=emb, max_new_tokens=5, eos_token_id=None, pad_token_id=PAD).cpu()
    assert tuple(free.shape) == (3, 5)
    rng = np.random.default_rng(5)
    sets = []
    for b in range(3):
        cont = free[b, :4].tolist()
        assert EOS not in cont
        decoys = [[int(t) for t in rng.integers(3, V, 4)] for _ in range(4)]
        sets.append([cont] + decoys)
    out = um.generate(inputs_embeds=emb, max_new_tokens=8, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=sets, allowed_set=[0, 1, 2]).cpu()
    assert out.shape[1] >= 5
    assert torch.equal(out[:, :4], free[:, :4]) and bool((out[:, 4] == EOS).all()) and bool((out[:, 5:] == PAD).all())


def test_ids_equal_the_reference_walk_over_the_returned_step_logits():
    um, hid, V = _model()
    B = 17
    sets = _sets(4, V, 31)
    trie = TokenTrie(sets, V, EOS)
    set_of = [b % 4 for b in range(B)]
    for min_new in (0, 1):
        r = um.generate(inputs_embeds=_emb(B, 5, hid, 22), max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, min_new_tokens=min_new,
                        allowed_sequences=trie, allowed_set=set_of, output_logits=True, return_dict_in_generate=True)
        ids, lg = r.sequences.cpu(), torch.stack(r.logits, 1).float().cpu()
        want, _ = R.walk_greedy(lg, trie, set_of, EOS, PAD, min_new)
        assert torch.equal(ids, want[:, :ids.shape[1]])
        _assert_members(ids, trie, set_of)
        assert int(lg.argmax(-1).ne(ids).sum()) > 0, "the constraint never bound: the test shows nothing"


@pytest.mark.parametrize("mode", ["greedy", "sample", "kv_fp8", "w_fp8", "qwen"])
def test_every_row_cut_at_eos_is_a_member_of_its_set(mode):
    um, hid, V = _model(mode == "qwen")
    B = 9
    sets = _sets(3, V, 41)
    trie = TokenTrie(sets, V, EOS)
    set_of = [(b * 2) % 3 for b in range(B)]
    kw = {"sample": dict(do_sample=True, seed=11, temperature=1.3, top_k=0, top_p=0.95), "kv_fp8": dict(kv_cache_dtype="fp8_e4m3"),
          "w_fp8": dict(weight_dtype="fp8_e4m3")}.get(mode, {})
    out = um.generate(inputs_embeds=_emb(B, 7, hid, 23), max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie,
                      allowed_set=set_of, **kw)
    _assert_members(out, trie, set_of, mode)
    if mode == "sample":
        again = um.generate(inputs_embeds=_emb(B, 7, hid, 23), max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie,
                            allowed_set=set_of, **kw)
        assert torch.equal(out, again), "a seeded sampling call is deterministic"


def test_state_carried_between_calls():
    """use_graph on / off agree; the same call twice on one engine agrees (the node reset and the capture's snapshot would each break it); a
    second trie at the same shapes gives ITS members (the graph key holds the trie's pointers)."""
    um, hid, V = _model()
    eng = um._engine
    B = 6
    emb = _emb(B, 5, hid, 24)
    set_of = [b % 3 for b in range(B)]
    first, second = TokenTrie(_sets(3, V, 51), V, EOS), TokenTrie(_sets(3, V, 52, first=12), V, EOS)
    call = lambda trie, **kw: um.generate(inputs_embeds=emb, max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie,
                                          allowed_set=set_of, **kw).cpu()
    eng.invalidate()
    eager = call(first, use_graph=False)
    a = call(first)
    graph = eng._dec[0].graph
    assert graph is not None
    b = call(first)
    assert eng._dec[0].graph is graph, "the same sets reuse the captured graph (device copies cached by content)"
    c = call(TokenTrie(_sets(3, V, 51), V, EOS))
    assert eng._dec[0].graph is graph, "an equal trie built anew meets the same device arrays"
    assert torch.equal(a, eager) and torch.equal(a, b) and torch.equal(a, c)
    _assert_members(a, first, set_of)
    other = call(second)
    assert eng._dec[0].graph is not graph
    _assert_members(other, second, set_of, "second trie")
    assert not all(first.is_member(s, R.cut_at_eos(other[i].tolist(), EOS)) for i, s in enumerate(set_of))
    assert torch.equal(call(first), a)
    eng.invalidate()
    assert not eng._tries


def _stub_inputs(um):
    """generate_batches / generate_questions on a model without encoders: the `batch_input_ids` entry already holds the embeddings."""
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    um.prepare_multimodal_inputs_many = lambda batches, **k: [{"inputs_embeds": b["batch_input_ids"]} for b in batches]


def _unstub(um):
    del um.prepare_multimodal_inputs, um.prepare_multimodal_inputs_many


def test_row_mapping_two_decode_streams():
    um, hid, V = _model()
    B = 5
    trie = TokenTrie(_sets(5, V, 61), V, EOS)
    set_of = [3, 0, 4, 1, 2]
    emb = _emb(B, 6, hid, 25)
    kw = dict(max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie)
    out = um.generate(inputs_embeds=emb, decode_streams=2, allowed_set=set_of, **kw).cpu()
    _assert_members(out, trie, set_of, "decode_streams=2")
    # the two groups are rows 0-1 and 2-4: bit-identical to separate calls
    for r0, r1 in ((0, 2), (2, 5)):
        alone = um.generate(inputs_embeds=emb[r0:r1], allowed_set=set_of[r0:r1], **kw).cpu()
        n = min(alone.shape[1], out.shape[1])
        assert torch.equal(out[r0:r1, :n], alone[:, :n]) and bool((out[r0:r1, n:] == PAD).all()) and bool((alone[:, n:] == PAD).all())


@pytest.mark.parametrize("coalesce,sizes,max_rows,waves", [(False, [2, 3, 1], None, None), (True, [2, 3, 1], 4, [2, 3, 1]), (True, [2, 3, 1], None, [6]),
                                                          (True, [2, 1, 3, 1], 4, [3, 4])])
def test_row_mapping_generate_batches(coalesce, sizes, max_rows, waves):
    """Batches of [2, 3, 1] rows: in flight (bit-identical to separate calls) and coalesced with max_rows = 4 (membership, and the reference
    walk over the path's own step logits at the engine).  _pack_waves aims at waves of equal size (6 rows at a cap of 4: a target of 3), so
    [2, 3, 1] at max_rows = 4 runs as three lone batches; the ragged wave itself is met by the same batches in ONE wave (no cap) and by
    [2, 1, 3, 1] at max_rows = 4, which packs as two ragged waves of 3 and 4 rows."""
    um, hid, V = _model()
    trie = TokenTrie(_sets(7, V, 62), V, EOS)
    flat = [5, 2, 0, 4, 1, 3, 6][:sum(sizes)]
    set_of = [flat[sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
    embs = [_emb(n, 4 + 2 * i, hid, 30 + i) for i, n in enumerate(sizes)]
    kw = dict(max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie)
    _stub_inputs(um)
    try:
        outs = um.generate_batches([dict(batch_input_ids=e, batch_X_modals=None) for e in embs], coalesce=coalesce, max_rows=max_rows,
                                   allowed_set=set_of, **kw)
    finally:
        _unstub(um)
    assert len(outs) == len(sizes)
    for g, o in enumerate(outs):
        _assert_members(o, trie, set_of[g], f"batch {g}")
        if not coalesce:
            assert torch.equal(o, um.generate(inputs_embeds=embs[g], allowed_set=set_of[g], **kw))
    if coalesce:
        assert um._engine.last_plan["groups"] == waves, um._engine.last_plan
        res = um._engine.generate_many(embs, 6, eos_token_id=EOS, pad_token_id=PAD, coalesce=True, max_rows=max_rows, return_step_logits=True,
                                       constraint=(trie, set_of))
        for g, (ids, lg) in enumerate(res):
            want, _ = R.walk_greedy(lg, trie, set_of[g], EOS, PAD)
            assert torch.equal(ids.cpu(), want[:, :ids.shape[1]]) and torch.equal(ids, outs[g])


def test_row_mapping_generate_questions():
    """2 clips x [2, 3] questions on a shared prefix, one set index per question."""
    um, hid, V = _model()
    trie = TokenTrie(_sets(5, V, 63), V, EOS)
    set_of = [[4, 1], [0, 3, 2]]
    prefixes = [_emb(1, 9, hid, 40), _emb(1, 9, hid, 41)]
    g = torch.Generator().manual_seed(9)
    questions = [[torch.randint(3, V, (int(n),), generator=g) for n in ns] for ns in ([2, 4], [3, 1, 5])]
    kw = dict(max_new_tokens=6, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie)
    _stub_inputs(um)
    try:
        outs = um.generate_questions([dict(batch_input_ids=p, batch_X_modals=None, question_ids=q) for p, q in zip(prefixes, questions)],
                                     allowed_set=set_of, **kw)
    finally:
        _unstub(um)
    assert [tuple(o.shape)[0] for o in outs] == [2, 3]
    for c, o in enumerate(outs):
        _assert_members(o, trie, set_of[c], f"clip {c}")
    suffix = [[um.encode_ids(q.cuda()).to(BF) for q in qs] for qs in questions]
    res = um._engine.generate_shared_prefix(torch.cat(prefixes, 0), suffix, 6, eos_token_id=EOS, pad_token_id=PAD, return_step_logits=True,
                                            constraint=(trie, set_of))
    for c, (ids, lg) in enumerate(res):
        want, _ = R.walk_greedy(lg, trie, set_of[c], EOS, PAD)
        assert torch.equal(ids.cpu(), want[:, :ids.shape[1]]) and torch.equal(ids, outs[c])


def test_refusals_by_name():
    um, hid, V = _model()
    emb = _emb(2, 4, hid, 26)
    kw = dict(inputs_embeds=emb, max_new_tokens=4, pad_token_id=PAD)
    with pytest.raises(ValueError, match="eos_token_id"):
        um.generate(eos_token_id=None, allowed_sequences=[[5, 6]], **kw)
    with pytest.raises(ValueError, match="outside the vocabulary"):
        um.generate(eos_token_id=EOS, allowed_sequences=[[5, V]], **kw)
    with pytest.raises(ValueError, match="min_new_tokens"):
        um.generate(eos_token_id=EOS, allowed_sequences=[[5, 6, 7], [8]], min_new_tokens=2, **kw)
    with pytest.raises(ValueError, match="allowed_set"):
        um.generate(eos_token_id=EOS, allowed_sequences=[[[5, 6]], [[7]]], **kw)
    with pytest.raises(ValueError, match="1 set indices for 2 rows"):
        um.generate(eos_token_id=EOS, allowed_sequences=[[[5, 6]], [[7]]], allowed_set=[0], **kw)
    with pytest.raises(NotImplementedError, match="prefix_allowed_tokens_fn"):
        um.generate(eos_token_id=EOS, prefix_allowed_tokens_fn=lambda b, ids: [5], **kw)
    out = um.generate(eos_token_id=EOS, allowed_sequences=[[5, 6], [7]], **kw)      # one set for every row
    _assert_members(out, TokenTrie([[[5, 6], [7]]], V, EOS), [0, 0])
