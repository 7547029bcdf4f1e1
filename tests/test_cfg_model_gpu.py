"""Classifier-free guidance at the engine and the public surface (GenerationEngine.generate_guided / generate(guidance_scale=...)): B <= 3
clips, prompts of 6-9 rows, negative prompts of 3-5 rows, <= 8 new tokens.

Yardsticks.  (1) The call's OWN raw step logits through the fp64 reference of the mix (tests/cfg_ref.py): the id chosen at every step lies
within the two elements' bounds of the reference maximum.  (2) The fp32 oracle fed teacher-forced with the negative prompt and the ids the HIP
path generated, held to tests/score_bounds.logprob_bound on those inputs: the unconditional rows really are fed the conditional rows' tokens.
(3) Bit equality between graph replay and eager steps, and between the two prompts' raw logits where they are the same prompt; twice the
bound of (2) wherever the rows meet other kernels (other wave sizes, the plain call) - the split / merge rule of
tests/test_logprob_model_gpu.py - compared column by column while the ids agree.  The tiny models are those of scripts/fuzz_engine_state.py
(Llama V = 320, Qwen2 V = 515) and, wherever the oracle gives the bound, the fixture models of tests/test_score_gpu.py."""
import functools
import os
import runpy

import pytest
import torch

from tests import cfg_ref as R
from tests import score_bounds as SB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 2


@functools.lru_cache(maxsize=None)
def _model(qwen=False):
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](qwen).base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


@functools.lru_cache(maxsize=None)
def _fixture(qwen=False):
    """(model, oracle weights, oracle decoder config) of the scoring fixtures: the models the fp32 oracle can follow."""
    from oracle import crab_oracle as O
    from tests import test_score_gpu as T
    if qwen:
        model, Wo, dcfg = T._qwen_case()[:3]
    else:
        meta, _ = SB.load_scoring_fixture()
        model, W = T._model(meta)
        Wo, dcfg = O.strip_peft_prefix(W), O.DecoderConfig(**meta["dec"])
    return model.base_model.model, Wo, dcfg


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


def _chosen_logprobs(sl, ids):
    """log_softmax (fp64) of step logits [B, n, V] at ids [B, n]."""
    return torch.log_softmax(sl.double().cpu(), -1).gather(-1, ids.cpu()[..., None])[..., 0]


def _teacher_forced(Wo, dcfg, prompt, ids):
    """The fp32 oracle teacher-forced on `prompt` followed by the embeddings of `ids`: (bound in nats, its log-probs of the ids [B, n], the
    bound's parts, the inputs, the labels) - tests/score_bounds.logprob_bound on exactly these inputs."""
    ids = ids.cpu()
    B, n = ids.shape
    P = prompt.shape[1]
    full = torch.cat([prompt.float().cpu(), Wo["model.embed_tokens.weight"].float()[ids]], 1)
    labels = torch.full((B, P + n), -100, dtype=torch.long)
    labels[:, P:] = ids
    bd, ref, parts = SB.logprob_bound(full, Wo, dcfg, labels)
    return bd, ref.reshape(B, n), parts, full, labels


def _assert_choices(ids, sl, B, scale, what):
    """(a): at every step the chosen id's reference score lies within the two elements' bounds of the reference maximum of the guided scores,
    computed in fp64 from the call's own raw logits.  No step is skipped."""
    ids, sl = ids.cpu(), sl.float().cpu()
    assert tuple(sl.shape[:2]) == (2 * B, ids.shape[1]) and sl.dtype == torch.float32
    worst = 0.0
    for t in range(ids.shape[1]):
        ref, bound = R.mix_ref(sl[:, t], B, scale)
        for b in range(B):
            below, allowed = R.choice_margin(ref[b], bound[b], int(ids[b, t]))
            worst = max(worst, below / allowed)
            assert below <= allowed, f"{what}: step {t} row {b} chose {int(ids[b, t])}, {below:.3e} below the reference maximum (allowed {allowed:.3e})"
    print(f"{what}: {B * ids.shape[1]} choices, the largest distance below the reference maximum is {worst:.3f} of what the bound allows")


# ------------------------------------------------------------------------------------------------------------ (a) (b) own logits, pair consistency
@pytest.mark.parametrize("qwen, scale", [(False, 1.5), (True, 7.5)], ids=["llama-1.5", "qwen2-7.5"])
def test_choices_follow_the_reference_on_the_calls_own_logits(qwen, scale):
    um, hid, V = _model(qwen)
    eng = um._engine
    B, S, Sn, n = 3, 8, 4, 8
    emb, neg = _emb(B, S, hid, 200 + int(qwen)), _emb(B, Sn, hid, 210 + int(qwen))
    ids, sl = eng.generate_guided(emb, neg, scale, n, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    assert tuple(ids.shape) == (B, n) and tuple(sl.shape) == (2 * B, n, V) and eng.last_ragged_prefill == "per_group"
    assert eng.last_plan["groups"] == [B] and eng.last_plan["guided"] is True
    _assert_choices(ids, sl, B, scale, f"{'qwen2' if qwen else 'llama'} scale {scale}")
    st = eng._dec[0]
    assert st.cfg == (scale, B) and tuple(st.guided.shape) == (B, V) and ids.data_ptr() != st.out_ids.data_ptr()
    # (b) the unconditional rows carry the conditional rows' words
    assert torch.equal(st.out_ids[:B], ids) and torch.equal(st.out_ids[B:], st.out_ids[:B])
    assert torch.equal(st.cur_ids[B:], st.cur_ids[:B]) and torch.equal(st.finished[B:], st.finished[:B])
    # guidance changes something: the plain call on the same prompt parts from it (the scale would otherwise be untested)
    plain = eng.generate(emb, n, eos_token_id=None, pad_token_id=PAD)
    assert not torch.equal(plain, ids), "guided and plain ids agree everywhere: the case shows nothing"
    # with an EOS: a finished pair pads, both rows' flags agree, the call is trimmed like generate() trims it
    eos = int(ids[0, 2])
    ids2, sl2 = eng.generate_guided(emb, neg, scale, n, eos_token_id=eos, pad_token_id=PAD, return_step_logits=True)
    st = eng._dec[0]
    k = ids[0].tolist().index(eos)
    assert torch.equal(ids2[0, :k + 1], ids[0, :k + 1]) and bool((ids2[0, k + 1:] == PAD).all()) and ids2.shape[1] == sl2.shape[1] <= n
    assert torch.equal(st.finished[B:], st.finished[:B]) and int(st.finished[0]) == 1
    assert torch.equal(st.out_ids[B:, :ids2.shape[1]], ids2)
    # min_new_tokens suppresses the EOS in the guided scores' select as in the plain one
    ids3 = eng.generate_guided(emb, neg, scale, n, eos_token_id=eos, pad_token_id=PAD, min_new_tokens=k + 2)
    assert not bool((ids3[:, :k + 2] == eos).any())


# ------------------------------------------------------------------------------------------------------------ (c) teacher forcing, against the oracle
@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
def test_unconditional_rows_are_teacher_forced_with_the_conditional_tokens(qwen):
    um, Wo, dcfg = _fixture(qwen)
    eng = um._engine
    hid = um.config.hidden_size
    B, S, Sn, n = 3, 7, 4, 6
    emb, neg = _emb(B, S, hid, 220 + int(qwen)), _emb(B, Sn, hid, 230 + int(qwen))
    ids, sl = eng.generate_guided(emb, neg, 1.5, n, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    ids = ids.cpu()
    assert tuple(ids.shape) == (B, n)
    for name, prompt, rows in (("unconditional", neg, sl[B:]), ("conditional", emb, sl[:B])):
        bd, ref, parts, full, labels = _teacher_forced(Wo, dcfg, prompt, ids)
        got = _chosen_logprobs(rows, ids)
        e = float((got - ref).abs().max())
        sc = um.score(inputs_embeds=full.to(BF).cuda(), labels=labels, return_token_logprobs=True)
        e_hip = float((got - torch.stack(sc.token_logprobs).double().cpu()).abs().max())
        print(f"{'qwen2' if qwen else 'llama'} {name} rows, log-prob of the emitted ids from the step logits: {e:.3e} from the fp32 oracle "
              f"teacher-forced ({parts} -> bound {bd:.3e}), {e_hip:.3e} from score() on the same rows (2 x bound)")
        assert e <= bd and e_hip <= 2 * bd
    # the rows differ from one another and the ids are not what the negative prompt alone would give: a row fed its OWN argmax could not pass
    own = eng.generate(neg, n, eos_token_id=None, pad_token_id=PAD).cpu()
    assert not torch.equal(own, ids)


# ------------------------------------------------------------------------------------------------------------ (d) (f) same bits on every route
def test_graph_replay_and_eager_steps_give_the_same_bits_and_sampling_is_deterministic():
    um, hid, V = _model()
    eng = um._engine
    B, n = 3, 7
    emb, neg = _emb(B, 6, hid, 240), _emb(B, 3, hid, 241)
    for kw in (dict(), dict(sampling=(1.2, 0, 0.95, 5))):
        kw = dict(dict(eos_token_id=None, pad_token_id=PAD, return_step_logits=True), **kw)
        eng.invalidate()
        ids_g, sl_g = eng.generate_guided(emb, neg, 1.5, n, **kw)
        assert eng._dec[0].graph is not None
        ids_g2, sl_g2 = eng.generate_guided(emb, neg, 1.5, n, **kw)          # the captured graph again, not the capture's warm-up
        ids_e, sl_e = eng.generate_guided(emb, neg, 1.5, n, use_graph=False, **kw)
        assert torch.equal(ids_g, ids_e) and torch.equal(sl_g, sl_e) and torch.equal(ids_g, ids_g2) and torch.equal(sl_g, sl_g2)
        if "sampling" not in kw:
            _assert_choices(ids_g, sl_g, B, 1.5, "graph replay")
    # (f) a seed is a stream: the same seed the same ids (above: three calls), another seed other ids; the scale is part of the graph's key
    other = eng.generate_guided(emb, neg, 1.5, n, eos_token_id=None, pad_token_id=PAD, sampling=(1.2, 0, 0.95, 6))
    assert not torch.equal(other, ids_g)
    g0 = eng._dec[0].graph
    eng.generate_guided(emb, neg, 2.5, n, eos_token_id=None, pad_token_id=PAD, sampling=(1.2, 0, 0.95, 6))
    assert eng._dec[0].graph is not g0 and eng._dec[0].cfg == (2.5, B)
    # and a plain call after a guided one meets a state without guidance
    eng.generate(torch.cat([emb, emb], 0), n, eos_token_id=None, pad_token_id=PAD)
    assert eng._dec[0].cfg is None and eng._dec[0].guided is None


def test_off_means_off():
    from crab_amd import ops
    um, hid, V = _model()
    eng = um._engine
    emb, neg = _emb(2, 6, hid, 250), _emb(2, 4, hid, 251)
    kw = dict(eos_token_id=None, pad_token_id=PAD)
    eng.generate(emb, 5, use_graph=False, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_off:
        eng.generate(emb, 5, use_graph=False, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_on:
        eng.generate_guided(emb, neg, 1.5, 5, use_graph=False, **kw)
    assert t_off.launched("cfg_mix") == 0 and t_off.launched("cfg_follow") == 0 and t_off.launched("greedy_select") == 5
    assert t_on.launched("cfg_mix") == 5 and t_on.launched("cfg_follow") == 5 and t_on.launched("greedy_select") == 5


# ------------------------------------------------------------------------------------------------------------ (e) negative == positive
def _walk_against(ids_a, lp_a, ids_b, lp_b, margin_b, tol, what):
    """Two routes over the same rows: log-probs compared column by column while the ids agree (tolerance tol); where they part, the step's
    top-2 margin on route b must be within 2 tol (each of the two scores may move by tol).  Returns the agreeing columns."""
    ids_a, ids_b = ids_a.cpu(), ids_b.cpu()
    n = min(ids_a.shape[1], ids_b.shape[1])
    same = (ids_a[:, :n] == ids_b[:, :n]).int().cumprod(1).bool()
    for b in range(ids_a.shape[0]):
        if not bool(same[b].all()):
            t = int(same[b].int().sum())
            assert float(margin_b[b, t]) <= 2 * tol, f"{what}: row {b} parts at step {t} where the top-2 margin is {float(margin_b[b, t]):.3e} > {2 * tol:.3e}"
    assert int(same.sum()) * 2 > same.numel() and bool(same[:, 0].all()), f"{what}: the ids part too early to compare: {ids_a.tolist()} / {ids_b.tolist()}"
    e = float((lp_a[:, :n] - lp_b[:, :n])[same].abs().max())
    print(f"{what}: {int(same.sum())} of {same.numel()} columns agree, max log-prob difference there {e:.3e} (tolerance {tol:.3e})")
    assert e <= tol
    return same


def test_negative_equal_to_positive_is_plain_greedy():
    """With the same prompt on both sides the two rows of a pair run the same launches at row b and row B + b of one batch.  Their raw logits are
    bit-equal (asserted; it held on the MI355X at these shapes: the one-length prefill and the decode step treat a row the same wherever it
    sits in the batch), so lc - lu is exactly 0, the guided scores are the log-softmax and the ids are plain greedy's wherever the plain
    call - B rows, possibly other kernels - does not sit on a near-tie."""
    um, Wo, dcfg = _fixture(False)
    eng = um._engine
    hid = um.config.hidden_size
    B, S, n = 3, 7, 8
    emb = _emb(B, S, hid, 260)
    ids, sl = eng.generate_guided(emb, emb.clone(), 7.5, n, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    diff = float((sl[:B] - sl[B:]).abs().max())
    print(f"negative == positive: raw logits of the two rows of a pair differ by at most {diff:.3e} ({'bit-equal' if torch.equal(sl[:B], sl[B:]) else 'NOT bit-equal'})")
    assert torch.equal(sl[:B], sl[B:])
    plain, slp = eng.generate(emb, n, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    bd = _teacher_forced(Wo, dcfg, emb, plain)[0]
    top2 = slp.float().cpu().topk(2, -1).values
    same = _walk_against(ids, _chosen_logprobs(sl[:B], ids), plain, _chosen_logprobs(slp, plain), top2[..., 0] - top2[..., 1], 2 * bd,
                         "guided with negative == positive vs plain greedy")
    print(f"ids equal plain greedy at {int(same.sum())} of {same.numel()} steps")


# ------------------------------------------------------------------------------------------------------------ (g) waves
def test_one_pair_per_wave_gives_the_single_wave_ids():
    um, Wo, dcfg = _fixture(False)
    eng = um._engine
    hid = um.config.hidden_size
    B, S, Sn, n = 3, 9, 5, 6
    emb, neg = _emb(B, S, hid, 270), _emb(B, Sn, hid, 271)
    kw = dict(eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    ids1, sl1 = eng.generate_guided(emb, neg, 1.5, n, **kw)
    assert eng.last_plan["groups"] == [B]
    ids3, sl3 = eng.generate_guided(emb, neg, 1.5, n, max_rows=2, **kw)
    assert eng.last_plan["groups"] == [1, 1, 1] and tuple(sl3.shape) == tuple(sl1.shape) and tuple(ids3.shape) == tuple(ids1.shape)
    ids2, sl2 = eng.generate_guided(emb, neg, 1.5, n, max_rows=5, **kw)                                    # 5 rows hold two pairs: waves of 2 + 1
    assert eng.last_plan["groups"] == [2, 1] and tuple(ids2.shape) == tuple(ids1.shape) and tuple(sl2.shape) == tuple(sl1.shape)
    bd = max(_teacher_forced(Wo, dcfg, emb, ids1)[0], _teacher_forced(Wo, dcfg, neg, ids1)[0])
    # the guided scores' top-2 margin of the single-wave call decides where another wave size may part from it
    margin = torch.empty((B, n))
    for t in range(n):
        ref, _ = R.mix_ref(sl1[:, t], B, 1.5)
        top2 = ref.topk(2, -1).values
        margin[:, t] = (top2[:, 0] - top2[:, 1]).float()
    # a guided score g lc - (g - 1) lu moves by (2 g - 1) times what the two log-probs move by: the margin is taken in those units
    for other, sl_o, what in ((ids3, sl3, "one pair per wave"), (ids2, sl2, "waves of 2 + 1 pairs")):
        for rows, name in ((slice(0, B), "conditional"), (slice(B, 2 * B), "unconditional")):
            _walk_against(other, _chosen_logprobs(sl_o[rows], other), ids1, _chosen_logprobs(sl1[rows], ids1), margin / (2 * 1.5 - 1), 2 * bd,
                          f"{what} vs one wave, {name} rows")
    # rows differ from one another, so a permuted join could not pass
    assert float((_chosen_logprobs(sl1[:B], ids1)[0] - _chosen_logprobs(sl1[:B], ids1)[-1]).abs().max()) > 4 * bd


# ------------------------------------------------------------------------------------------------------------ (h) FP8 KV cache
def test_fp8_kv_cache_runs_and_starts_from_the_same_logits():
    um, hid, V = _model()
    eng = um._engine
    B, n = 2, 6
    emb, neg = _emb(B, 9, hid, 280), _emb(B, 3, hid, 281)
    kw = dict(eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    ids, sl = eng.generate_guided(emb, neg, 1.5, n, **kw)
    ids8, sl8 = eng.generate_guided(emb, neg, 1.5, n, kv_cache_dtype="fp8_e4m3", **kw)
    assert len(eng._kv[(0,)]) == 4, "the fp8 cache holds codes and scales"
    assert tuple(ids8.shape) == (B, n) and torch.equal(sl8[:, 0], sl[:, 0]) and torch.equal(ids8[:, 0], ids[:, 0])
    assert not torch.equal(sl8[:, 1:], sl[:, 1:]), "the decode steps read the quantised cache"
    _assert_choices(ids8, sl8, B, 1.5, "fp8 KV cache")
    assert eng.kv_cache_dtype == "bf16"
    ids_w = eng.generate_guided(emb, neg, 1.5, n, weight_dtype="fp8_e4m3", eos_token_id=None, pad_token_id=PAD)
    assert tuple(ids_w.shape) == (B, n) and eng.last_plan["weight_dtype_used"] == "fp8_e4m3" and torch.equal(ids_w[:, 0], ids[:, 0])


# ------------------------------------------------------------------------------------------------------------ (i) public surface
def test_public_surface():
    um, hid, V = _model()
    eng = um._engine
    B, n = 3, 6
    emb, neg = _emb(B, 7, hid, 290), _emb(B, 4, hid, 291)
    kw = dict(max_new_tokens=n, eos_token_id=None, pad_token_id=PAD)
    want, sl = eng.generate_guided(emb, neg, 1.5, n, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    got = um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=1.5, **kw)
    assert torch.equal(got, want)
    r = um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=1.5, output_logits=True, return_dict_in_generate=True, **kw)
    assert torch.equal(r.sequences, want) and len(r.logits) == n and torch.equal(torch.stack(r.logits, 1), sl[:B])
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    try:
        got = um.generate(batch_input_ids=emb, negative_inputs=dict(batch_input_ids=neg, batch_X_modals=None), guidance_scale=1.5, **kw)
    finally:
        del um.prepare_multimodal_inputs
    assert torch.equal(got, want)
    plain = um.generate(inputs_embeds=emb, **kw)
    assert torch.equal(um.generate(inputs_embeds=emb, guidance_scale=1, negative_inputs_embeds=neg, **kw), plain)
    assert torch.equal(um.generate(inputs_embeds=emb, guidance_scale=None, **kw), plain) and not torch.equal(plain, want)
    s1 = um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=1.5, do_sample=True, temperature=1.2, top_k=0, top_p=0.95, seed=3, **kw)
    s2 = um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=1.5, do_sample=True, temperature=1.2, top_k=0, top_p=0.95, seed=3, **kw)
    assert torch.equal(s1, s2) and tuple(s1.shape) == (B, n)
    with pytest.raises(ValueError, match="negative_inputs_embeds"):
        um.generate(inputs_embeds=emb, guidance_scale=1.5, **kw)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=0.5, **kw)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        um.generate_batches([dict(batch_input_ids=emb, batch_X_modals=None)], guidance_scale=1.5, **kw)
