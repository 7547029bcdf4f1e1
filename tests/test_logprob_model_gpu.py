"""Per-token log-probabilities of generated ids at the engine and the public surface (return_logprobs / output_token_logprobs), B <= 4, prompts of
6-9 rows, <= 8 new tokens.

Yardsticks.  (1) The call's OWN step logits through the fp64 reference (tests/logprob_ref.py), held to the kernel bound - greedy, min_new_tokens,
sample mode, constrained greedy and sampling, the FP8 KV cache.  (2) The fp32 oracle fed teacher-forced with the ids the HIP path generated, held
to tests/score_bounds.logprob_bound on those inputs (1.5 x max(operand floor, storage emulation), computed in the session) - Llama and Qwen2.
(3) Bit equality between graph replay and eager steps, and wherever rows only move between identical launches; 2 x the bound of (2) wherever a
batch is split or merged and the rows meet other kernels.  The tiny models are those of scripts/fuzz_engine_state.py (Llama V = 320, Qwen2
V = 515) and, for the oracle, the fixture models of tests/test_score_gpu.py."""
import functools
import os
import runpy
import warnings

import numpy as np
import pytest
import torch

from crab_amd.constrain import TokenTrie
from tests import logprob_ref as L
from tests import score_bounds as SB
from tests.util import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EOS, PAD = 1, 2


@functools.lru_cache(maxsize=None)
def _model(qwen=False):
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](qwen).base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


def _sets(n_sets, V, seed, first=10):
    """n_sets answer sets of 5 sequences of 1-4 tokens; set i draws from 6 ids of its own range (as tests/test_constrain_model_gpu.py)."""
    rng = np.random.default_rng(seed)
    span = (V - first) // n_sets
    sets = []
    for i in range(n_sets):
        alphabet = (first + i * span + rng.permutation(span)[:6]).tolist()
        sets.append([[int(rng.choice(alphabet)) for _ in range(int(rng.integers(1, 5)))] for _ in range(5)])
    return sets


def _stub_inputs(um):
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    um.prepare_multimodal_inputs_many = lambda batches, **k: [{"inputs_embeds": b["batch_input_ids"]} for b in batches]


def _unstub(um):
    del um.prepare_multimodal_inputs, um.prepare_multimodal_inputs_many


def _assert_own_logits(ids, lg, lp, eos, min_new, what, trie=None, set_of=None):
    """lp [B, n, 2] of a call against the fp64 reference over the call's own step logits lg [B, n, V]; returns (reference, live)."""
    ids, lp = ids.cpu(), lp.cpu()
    assert tuple(lp.shape) == tuple(ids.shape) + (2,) and lp.dtype == torch.float32 and tuple(lg.shape[:2]) == tuple(ids.shape)
    ref, live, bound = L.walk_ref(lg, ids, -1 if eos is None else eos, min_new, trie, set_of)
    got = lp.permute(2, 0, 1).double()
    dead = ~live[None].expand_as(got)
    assert bool((got[dead] == 0).all()), f"{what}: a step without a token holds {got[dead]}"
    err = (got - ref).abs()
    ratio = float((err[~dead] / bound[~dead]).max())
    print(f"{what}: {int(live.sum())} live steps, max |got - ref| {float(err.max()):.3e}, largest ratio to the kernel bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: {err.max()} exceeds the kernel bound"
    return ref, live


# ------------------------------------------------------------------------------------------------------------ (1) own logits
@pytest.mark.parametrize("mode", ["greedy", "min_new", "sample", "constrained", "constrained_sample", "kv_fp8"])
def test_scores_equal_the_reference_on_the_calls_own_logits(mode):
    um, hid, V = _model()
    eng = um._engine
    B, S, n = 4, 7, 8
    emb = _emb(B, S, hid, 70)
    free = eng.generate(emb, n, eos_token_id=None, pad_token_id=PAD).cpu()
    eos = int(free[0, 2])                                        # row 0 meets its EOS at step 2 at the latest in the greedy modes
    min_new = 2 if mode == "min_new" else 0
    kw, trie, set_of = {}, None, None
    if mode in ("sample", "constrained_sample"):
        kw["sampling"] = (1.2, 0, 0.95, 11)
    if mode == "kv_fp8":
        kw["kv_cache_dtype"] = "fp8_e4m3"
    if mode.startswith("constrained"):
        eos = EOS
        trie = TokenTrie(_sets(2, V, 71), V, EOS)
        set_of = [0, 1, 1, 0]
        kw["constraint"] = (trie, set_of)
    ids, lg, lp = eng.generate(emb, n, eos_token_id=eos, pad_token_id=eos, min_new_tokens=min_new, return_step_logits=True, return_logprobs=True, **kw)
    ref, live = _assert_own_logits(ids, lg, lp, eos, min_new, mode, trie, set_of)
    ids = ids.cpu()
    hit = ids == eos
    if mode in ("greedy", "min_new") or trie is not None:
        early = [b for b in range(B) if bool(hit[b].any()) and int(hit[b].int().argmax()) < ids.shape[1] - 1]
        assert early, f"{mode}: no row met EOS before the last column - the mixed batch shows nothing: {ids.tolist()}"
    for b in range(B):
        if bool(hit[b].any()):
            k = int(hit[b].int().argmax())                       # pad == eos: only the FIRST one is a token
            assert live[b, :k + 1].all() and not live[b, k + 1:].any()
            assert float(lp[b, k, 0]) != 0.0 and bool((lp[b, k + 1:] == 0).all())
    if mode == "min_new":
        sup = lp[:, :2].cpu()
        assert not bool(hit[:, :2].any()) and bool((sup[..., 1] >= sup[..., 0]).all()) and bool((sup[..., 1] > sup[..., 0]).any()), \
            "EOS is outside the allowed set while it is suppressed"
        assert torch.equal(lp[:, 2:, 1], lp[:, 2:, 0])
    elif trie is None:
        assert torch.equal(lp[..., 0], lp[..., 1]), "nothing suppressed: one normaliser"
    else:
        assert bool((lp[..., 1] >= lp[..., 0]).all()) and bool((lp[..., 1] <= 0).all())


# ------------------------------------------------------------------------------------------------------------ (2) the oracle
@functools.lru_cache(maxsize=None)
def _oracle_case(qwen):
    from oracle import crab_oracle as O
    from tests import test_score_gpu as T
    if qwen:
        model, Wo, dcfg = T._qwen_case()[:3]
    else:
        meta, _ = SB.load_scoring_fixture()
        model, W = T._model(meta)
        Wo, dcfg = O.strip_peft_prefix(W), O.DecoderConfig(**meta["dec"])
    um = model.base_model.model
    B, S, n = 4, 7, 6
    emb = _emb(B, S, um.config.hidden_size, 80 + int(qwen))
    r = um.generate(inputs_embeds=emb, max_new_tokens=n, eos_token_id=None, pad_token_id=PAD, output_token_logprobs=True)
    ids = r.sequences.cpu()
    assert tuple(ids.shape) == (B, n)
    # teacher-forced: the prompt rows, then the embeddings of the generated ids (the last one only completes the shape: the last row never scores)
    full = torch.cat([emb.float().cpu(), Wo["model.embed_tokens.weight"].float()[ids]], 1)
    labels = torch.full((B, S + n), -100, dtype=torch.long)
    labels[:, S:] = ids
    bd, ref, parts = SB.logprob_bound(full, Wo, dcfg, labels)
    return um, emb, r, bd, ref.reshape(B, n), parts


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
def test_greedy_logprobs_against_the_fp32_oracle_teacher_forced(qwen):
    um, emb, r, bd, ref, parts = _oracle_case(qwen)
    got = r.token_logprobs.double().cpu()
    e = float((got - ref).abs().max())
    print(f"{'qwen2' if qwen else 'llama'} decode-path per-token log-prob vs the fp32 oracle: {e:.3e}; {parts} -> bound {bd:.3e}")
    record_parity("generate(output_token_logprobs) per-token log-probs vs the fp32 oracle", e, float(ref.abs().max()), bd)
    assert torch.equal(r.token_logprobs, r.token_logprobs_allowed) and r.num_tokens.tolist() == [ref.shape[1]] * ref.shape[0]
    assert e <= bd
    assert float((r.sum_logprob.double().cpu() - ref.sum(1)).abs().max()) <= ref.shape[1] * bd


# ------------------------------------------------------------------------------------------------------------ (3) same bits on every route
def test_graph_replay_and_eager_steps_give_the_same_bits():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 6, hid, 90)
    for kw in (dict(), dict(sampling=(0.8, 20, 0.9, 5)), dict(constraint=(TokenTrie(_sets(2, V, 91), V, EOS), [1, 0, 1]), eos_token_id=EOS)):
        kw = dict(dict(eos_token_id=None, pad_token_id=PAD, return_logprobs=True), **kw)
        eng.invalidate()
        ids_g, lp_g = eng.generate(emb, 7, **kw)
        assert eng._dec[0].graph is not None
        ids_g2, lp_g2 = eng.generate(emb, 7, **kw)               # the captured graph again: the reset of lp, not the capture's warm-up
        ids_e, lp_e = eng.generate(emb, 7, use_graph=False, **kw)
        assert torch.equal(ids_g, ids_e) and torch.equal(lp_g, lp_e) and torch.equal(ids_g, ids_g2) and torch.equal(lp_g, lp_g2)
        assert lp_g.data_ptr() != eng._dec[0].lp.data_ptr() and bool((lp_g[..., 0] < 0).any())


def _compare_rows(ids_a, lp_a, ids_b, lp_b, tol, what):
    """Scores of the same rows through other kernels: compared column by column while the ids agree (a bf16 near-tie may part two routes)."""
    ids_a, ids_b, lp_a, lp_b = ids_a.cpu(), ids_b.cpu(), lp_a.cpu(), lp_b.cpu()
    n = min(ids_a.shape[1], ids_b.shape[1])
    same = (ids_a[:, :n] == ids_b[:, :n]).int().cumprod(1).bool()
    assert int(same.sum()) * 2 > same.numel() and bool(same[:, 0].all()), f"{what}: the ids part too early to compare: {ids_a.tolist()} / {ids_b.tolist()}"
    e = float((lp_a[:, :n] - lp_b[:, :n])[same].abs().max())
    print(f"{what}: {int(same.sum())} of {same.numel()} columns compared, max difference {e:.3e} (tolerance {tol:.3e})")
    assert e <= tol
    return same


def test_split_batches_keep_rows_in_the_callers_order():
    um, emb, r, bd, _, _ = _oracle_case(False)
    eng = um._engine
    n = r.sequences.shape[1]
    kw = dict(inputs_embeds=emb, max_new_tokens=n, eos_token_id=None, pad_token_id=PAD, output_token_logprobs=True)
    two = um.generate(decode_streams=2, **kw)
    same = _compare_rows(r.sequences, torch.stack([r.token_logprobs, r.token_logprobs_allowed], -1), two.sequences,
                         torch.stack([two.token_logprobs, two.token_logprobs_allowed], -1), 2 * bd, "decode_streams=2")
    assert bool(same.all()), "ids equal"
    B, S = emb.shape[:2]
    eng.kv_budget_bytes = int(eng.fixed_bytes(B, S) / 0.94 + 0.6 * B * eng.bytes_per_sequence(S, n) / 0.94)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            split = um.generate(**kw)
        assert len(eng.last_plan["groups"]) > 1, eng.last_plan
    finally:
        eng.kv_budget_bytes = None
    same = _compare_rows(r.sequences, torch.stack([r.token_logprobs, r.token_logprobs_allowed], -1), split.sequences,
                         torch.stack([split.token_logprobs, split.token_logprobs_allowed], -1), 2 * bd, "KV-budget split")
    assert bool(same.all()), "ids equal"
    # rows differ from one another, so a permuted join could not pass
    assert float((r.token_logprobs[0] - r.token_logprobs[-1]).abs().max()) > 4 * bd


# ------------------------------------------------------------------------------------------------------------ (4) every form
def test_in_flight_batches_equal_separate_calls_bit_for_bit():
    um, hid, V = _model()
    eng = um._engine
    embs = [_emb(2, 6, hid, 100), _emb(3, 9, hid, 101), _emb(1, 7, hid, 102)]
    free = eng.generate(embs[1], 6, eos_token_id=None, pad_token_id=PAD)
    kw = dict(eos_token_id=int(free[0, 1]), pad_token_id=PAD, return_logprobs=True)
    outs = eng.generate_many(embs, 6, return_first_logits=True, **kw)
    for e, (ids, fl, lp) in zip(embs, outs):
        ids1, fl1, lp1 = eng.generate(e, 6, return_first_logits=True, **kw)
        assert torch.equal(ids, ids1) and torch.equal(fl, fl1) and torch.equal(lp, lp1) and tuple(lp.shape) == tuple(ids.shape) + (2,)


def test_coalesced_and_shared_prefix_forms_agree_with_separate_calls():
    um, _, _, bd, _, _ = _oracle_case(False)
    eng = um._engine
    hid = um.config.hidden_size
    kw = dict(eos_token_id=None, pad_token_id=PAD, return_logprobs=True)
    embs = [_emb(2, 6, hid, 110), _emb(1, 9, hid, 111), _emb(1, 8, hid, 112)]
    outs = eng.generate_many(embs, 6, coalesce=True, **kw)
    assert eng.last_plan["groups"] == [4], eng.last_plan
    for g, (e, (ids, lp)) in enumerate(zip(embs, outs)):
        ids1, lp1 = eng.generate(e, 6, **kw)
        _compare_rows(ids1, lp1, ids, lp, 2 * bd, f"coalesced batch {g}")
    # 2 clips x {1, 3} questions on a shared prefix
    prefix = _emb(2, 6, hid, 113)
    g_ = torch.Generator().manual_seed(9)
    V = um.lm_head.weight.shape[0]
    questions = [[torch.randint(3, V, (int(s),), generator=g_) for s in ss] for ss in ([2], [3, 1, 2])]
    suffix = [[um.encode_ids(q.cuda()).to(BF) for q in qs] for qs in questions]
    res = eng.generate_shared_prefix(prefix, suffix, 6, **kw)
    assert [tuple(ids.shape)[0] for ids, _ in res] == [1, 3]
    for c, (ids, lp) in enumerate(res):
        for q in range(len(suffix[c])):
            ids1, lp1 = eng.generate(torch.cat([prefix[c], suffix[c][q]], 0)[None], 6, **kw)
            _compare_rows(ids1, lp1, ids[q:q + 1], lp[q:q + 1], 2 * bd, f"shared prefix clip {c} question {q}")


def test_closed_set_answer_probability_within_its_set():
    """Two answer sets from disjoint id ranges: the sum of the allowed plane over an answer is the log of its probability renormalised within
    the set - equal to the reference walk over the call's own logits, exp of it in (0, 1]."""
    um, hid, V = _model()
    trie = TokenTrie(_sets(2, V, 120), V, EOS)
    set_of = [0, 1, 1, 0]
    r = um.generate(inputs_embeds=_emb(4, 8, hid, 121), max_new_tokens=8, eos_token_id=EOS, pad_token_id=PAD, allowed_sequences=trie,
                    allowed_set=set_of, output_logits=True, return_dict_in_generate=True, output_token_logprobs=True)
    ids = r.sequences.cpu()
    lg = torch.stack(r.logits, 1).float().cpu()
    ref, live, bound = L.walk_ref(lg, ids, EOS, 0, trie, set_of)
    for b, s in enumerate(set_of):
        row = ids[b].tolist()
        assert EOS in row and trie.is_member(s, row[:row.index(EOS)])
        assert int(r.num_tokens[b]) == row.index(EOS) + 1 == int(live[b].sum())
    got = r.sum_logprob_allowed.double().cpu()
    tol = bound[1].sum(1) + L.EPS * ref[1].sum(1).abs()          # the kernel bound per column, and the fp32 sum of the columns
    print(f"sum_logprob_allowed {got.tolist()} vs the reference walk {ref[1].sum(1).tolist()}")
    assert bool(((got - ref[1].sum(1)).abs() <= tol).all())
    p = torch.exp(got)
    assert bool((p > 0).all()) and bool((p <= 1).all())
    assert bool((r.sum_logprob < r.sum_logprob_allowed).all()), "the whole vocabulary holds more mass than the answer set"


# ------------------------------------------------------------------------------------------------------------ (5) off means off
def test_off_means_off():
    from crab_amd import ops
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 6, hid, 130)
    kw = dict(eos_token_id=None, pad_token_id=PAD)
    eng.generate(emb, 5, use_graph=False, **kw)                  # whatever a first call does once (packing, tables) stays out of the two traces
    with ops.launch_trace(emb.device.index or 0) as t_off:
        off = eng.generate(emb, 5, use_graph=False, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_on:
        on, lp = eng.generate(emb, 5, use_graph=False, return_logprobs=True, **kw)
    assert t_off.launched("logprob_norm") == 0 and t_off.launched("logprob_gather") == 0
    assert t_on.launched("logprob_norm") == 5 and t_on.launched("logprob_gather") == 5 and t_on.launched("greedy_select") == 5
    assert {k: v for k, v in t_on.counts.items() if not k.startswith("logprob_")} == t_off.counts, "the option adds its two launches and nothing else"
    assert torch.equal(off, on)
    # the graph key: alternating calls on one engine equal what a fresh engine state gives for each
    eng.invalidate()
    on_only = eng.generate(emb, 6, return_logprobs=True, **kw)
    eng.invalidate()
    off_only = eng.generate(emb, 6, **kw)
    eng.invalidate()
    for _ in range(2):
        a = eng.generate(emb, 6, return_logprobs=True, **kw)
        g_on = eng._dec[0].graph
        b = eng.generate(emb, 6, **kw)
        assert eng._dec[0].graph is not g_on and eng._dec[0].lp is None
        assert torch.equal(a[0], on_only[0]) and torch.equal(a[1], on_only[1]) and torch.equal(b, off_only) and torch.equal(b, a[0])


# ------------------------------------------------------------------------------------------------------------ (6) public surface
def test_public_surface():
    um, hid, V = _model()
    emb = _emb(4, 7, hid, 140)
    free = um.generate(inputs_embeds=emb, max_new_tokens=6, eos_token_id=None, pad_token_id=PAD).cpu()
    eos = int(free[1, 2])
    kw = dict(max_new_tokens=6, eos_token_id=eos, pad_token_id=PAD)
    plain = um.generate(inputs_embeds=emb, **kw)
    r = um.generate(inputs_embeds=emb, output_token_logprobs=True, output_first_logits=True, **kw)
    B, n = r.sequences.shape
    assert torch.equal(r.sequences, plain) and tuple(r.first_logits.shape) == (B, V)
    for f in (r.token_logprobs, r.token_logprobs_allowed):
        assert tuple(f.shape) == (B, n) and f.dtype == torch.float32
    for f in (r.sum_logprob, r.sum_logprob_allowed, r.num_tokens):
        assert tuple(f.shape) == (B,)
    cut = [row.index(eos) + 1 if eos in row else n for row in r.sequences.tolist()]
    assert r.num_tokens.tolist() == cut and min(cut) < n
    for b in range(B):
        assert bool((r.token_logprobs[b, :cut[b]] < 0).all()) and bool((r.token_logprobs[b, cut[b]:] == 0).all())
    assert torch.equal(r.sum_logprob, r.token_logprobs.sum(1))
    # the batch forms
    embs = [_emb(2, 6, hid, 141), _emb(1, 9, hid, 142)]
    _stub_inputs(um)
    try:
        batches = [dict(batch_input_ids=e, batch_X_modals=None) for e in embs]
        for coalesce in (False, True):
            outs = um.generate_batches(batches, coalesce=coalesce, output_token_logprobs=True, **kw)
            ids_only = um.generate_batches(batches, coalesce=coalesce, **kw)
            assert len(outs) == 2
            for e, o, i in zip(embs, outs, ids_only):
                assert torch.equal(o.sequences, i) and tuple(o.token_logprobs.shape) == tuple(i.shape) == tuple(o.token_logprobs_allowed.shape)
                assert tuple(o.sum_logprob.shape) == tuple(o.num_tokens.shape) == (e.shape[0],)
                if not coalesce:
                    one = um.generate(inputs_embeds=e, output_token_logprobs=True, **kw)
                    assert torch.equal(o.token_logprobs, one.token_logprobs) and torch.equal(o.num_tokens, one.num_tokens)
        with pytest.raises(NotImplementedError, match="output_logits"):
            um.generate_batches(batches, output_logits=True, output_token_logprobs=True, **kw)
        g_ = torch.Generator().manual_seed(3)
        qs = [[torch.randint(3, V, (2,), generator=g_)], [torch.randint(3, V, (int(s),), generator=g_) for s in (3, 1, 2)]]
        outs = um.generate_questions([dict(batch_input_ids=_emb(1, 6, hid, 143 + c), batch_X_modals=None, question_ids=q) for c, q in enumerate(qs)],
                                     output_token_logprobs=True, **kw)
        assert [tuple(o.token_logprobs.shape) for o in outs] == [tuple(o.sequences.shape) for o in outs] and [o.num_tokens.shape[0] for o in outs] == [1, 3]
    finally:
        _unstub(um)
