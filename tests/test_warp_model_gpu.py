"""min_p / epsilon_cutoff / eta_cutoff through generate() and its siblings on the device: the tiny Llama of scripts/fuzz_engine_state.py (V = 320,
head dim 128 - the decode attention kernels take 64 and 128, so the head-dim-16 config of the host tests cannot run here), B <= 3 rows,
prompts of 5-9 rows, <= 8 new tokens.

Yardstick: the call's OWN raw step logits through tests/warp_ref.py (HF's warpers in fp64, derived margins): no emitted id is `DROP` at its
step.  Where the select reads something other than the raw logits, the reference reads the same thing: the edited row of
tests/select_chain_ref.step under repetition_penalty, and under guidance the fp32 scores crab_cfg_mix forms from the recorded raw logits (the
same kernel on the same bits as the step's).  Graph replay, eager steps and a second call agree bit for bit; min_p = 1 is the greedy call; off
values are the plain sampling call, launch for launch; a changed value re-captures the step."""
import functools
import os
import runpy

import pytest
import torch

from tests import select_chain_ref as SC
from tests import warp_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 2
SMP = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.95, seed=5)
WARP = dict(min_p=0.1, epsilon_cutoff=0.02, eta_cutoff=0.05)          # after top_k = 40 a typical probability is 1 / 40: all three bite


@functools.lru_cache(maxsize=None)
def _model():
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](False).base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


def _stub_inputs(um):
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    um.prepare_multimodal_inputs_many = lambda batches, **k: [{"inputs_embeds": b["batch_input_ids"]} for b in batches]


def _unstub(um):
    del um.prepare_multimodal_inputs, um.prepare_multimodal_inputs_many


def _chain(kw):
    """(sampling triple, the three stage values) of a call's keyword arguments."""
    return (kw["temperature"], kw["top_k"], kw["top_p"]), (kw.get("min_p") or 0.0, kw.get("epsilon_cutoff") or 0.0, kw.get("eta_cutoff") or 0.0)


def _assert_never_drop(ids, step_logits, kw, eos, min_new, what, penalty=1.0, chosen_from=None, exercised=True):
    """ids [B, n] and the raw step logits [B, n, V] of one call: at every step of every live row the emitted id is not DROP under
    warp_ref.warp_classes of the row the select chose from (the edited row of select_chain_ref.step; chosen_from(t) overrides it: guidance).
    Returns (steps checked, steps at which the three stages removed tokens that temperature / top-k / top-p had left)."""
    ids, lg = ids.cpu(), step_logits.float().cpu()
    B, n, V = lg.shape
    assert tuple(ids.shape) == (B, n)
    smp, stages = _chain(kw)
    opts = SC.Opts(eos=eos, pad=PAD, min_new=min_new, penalty=penalty)
    fin, checked, cut = torch.zeros(B, dtype=torch.int32), 0, 0
    for t in range(n):
        r = SC.step(lg[:, t], ids, t, fin, None, opts)
        rows = r.edited if chosen_from is None else chosen_from(t)
        for b in range(B):
            if int(fin[b]):
                assert int(ids[b, t]) == PAD, (what, b, t)
                continue
            cls, _ = R.warp_classes(rows[b], r.allowed[b], smp, *stages)
            y = int(ids[b, t])
            assert int(cls[y]) != R.DROP, f"{what}: row {b} step {t} emitted {y}, which the chain removes ({int((cls == R.KEEP).sum())} tokens kept)"
            checked += 1
            cut += int((cls != R.DROP).sum()) < int((SC.kept_classes(rows[b], r.allowed[b], smp)[0] != R.DROP).sum())
        _, _, fin = r.after(ids[:, t])
    print(f"{what}: {checked} steps checked, {cut} with tokens removed by the new stages")
    assert not exercised or cut >= max(1, checked // 4), f"{what}: the new stages removed nothing at most steps - the call does not exercise them"
    return checked, cut


def _logits_of(r):
    return torch.stack(list(r.logits), 1)


# ------------------------------------------------------------------ (a) one seed, one answer
def test_graph_eager_and_a_second_call_agree():
    um, hid, V = _model()
    emb = _emb(3, 7, hid, 401)
    kw = dict(max_new_tokens=8, eos_token_id=7, pad_token_id=PAD, min_new_tokens=2, **SMP, **WARP)
    a = um.generate(inputs_embeds=emb, **kw)
    b = um.generate(inputs_embeds=emb, use_graph=False, **kw)
    c = um.generate(inputs_embeds=emb, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    d = um.generate(inputs_embeds=emb, **dict(kw, seed=6))
    assert d.shape[0] == 3 and not torch.equal(a[:, :d.shape[1]], d[:, :a.shape[1]]), "another seed drew the same 24 tokens"


def test_no_emitted_id_is_drop_under_the_reference():
    um, hid, V = _model()
    emb = _emb(3, 7, hid, 402)
    for name, warp in (("all", WARP), ("min_p", dict(min_p=0.1)), ("epsilon", dict(epsilon_cutoff=0.03)), ("eta", dict(eta_cutoff=0.08))):
        kw = dict(SMP, **warp)
        r = um.generate(inputs_embeds=emb, max_new_tokens=8, eos_token_id=7, pad_token_id=PAD, min_new_tokens=2, output_logits=True,
                        return_dict_in_generate=True, **kw)
        _assert_never_drop(r.sequences, _logits_of(r), kw, 7, 2, name)


def test_min_p_one_is_the_greedy_call():
    um, hid, V = _model()
    emb = _emb(3, 6, hid, 403)
    kw = dict(max_new_tokens=8, eos_token_id=None, pad_token_id=PAD)
    g = um.generate(inputs_embeds=emb, output_logits=True, return_dict_in_generate=True, **kw)
    top2 = torch.topk(_logits_of(g).float().cpu(), 2, dim=-1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-3 * top2[..., 0].abs().clamp(min=1.0)).all(1)      # rows whose top-2 margin is clear at every step
    assert int(clear.sum()) >= 2, f"top-2 margins {(top2[..., 0] - top2[..., 1]).min(1).values.tolist()}: pick another prompt seed"
    for front in (dict(temperature=0.8, top_k=0, top_p=1.0), dict(temperature=0.7, top_k=50, top_p=0.9)):
        s = um.generate(inputs_embeds=emb, do_sample=True, seed=9, min_p=1.0, **front, **kw)
        assert torch.equal(s[clear.cuda()], g.sequences[clear.cuda()]), front


# ------------------------------------------------------------------ (b) which kernel ran
def test_off_values_launch_sample_select_and_live_values_the_warped_kernel():
    from crab_amd import ops
    um, hid, V = _model()
    emb = _emb(2, 6, hid, 404)
    kw = dict(max_new_tokens=5, eos_token_id=None, pad_token_id=PAD, use_graph=False, **SMP)
    dev = emb.device.index or 0
    um.generate(inputs_embeds=emb, **kw)
    with ops.launch_trace(dev) as t_plain:
        plain = um.generate(inputs_embeds=emb, **kw)
    with ops.launch_trace(dev) as t_off:
        off = um.generate(inputs_embeds=emb, min_p=0, epsilon_cutoff=0.0, eta_cutoff=None, **kw)
    with ops.launch_trace(dev) as t_on:
        on = um.generate(inputs_embeds=emb, **WARP, **kw)
    with ops.launch_trace(dev) as t_greedy:
        um.generate(inputs_embeds=emb, max_new_tokens=5, eos_token_id=None, pad_token_id=PAD, use_graph=False, **WARP)      # no do_sample: the greedy call
    assert torch.equal(plain, off) and t_plain.counts == t_off.counts
    assert t_off.launched("sample_select") == 5 and t_off.launched("sample_select_warped") == 0
    assert t_on.launched("sample_select_warped") == 5 and t_on.launched("sample_select") == 0 and t_on.launched("greedy_select") == 0
    assert {k: v for k, v in t_on.counts.items() if k != "sample_select_warped"} == {k: v for k, v in t_off.counts.items() if k != "sample_select"}
    assert t_greedy.launched("greedy_select") == 5 and t_greedy.launched("sample_select_warped") == 0 and t_greedy.launched("sample_select") == 0
    assert tuple(on.shape) == tuple(plain.shape)


def test_a_changed_value_recaptures_the_step():
    um, hid, V = _model()
    emb = _emb(2, 6, hid, 405)
    kw = dict(max_new_tokens=8, eos_token_id=None, pad_token_id=PAD, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=3)
    loose = um.generate(inputs_embeds=emb, min_p=0.02, output_logits=True, return_dict_in_generate=True, **kw)
    g1 = um._engine._dec[0].graph
    tight = um.generate(inputs_embeds=emb, min_p=1.0, output_logits=True, return_dict_in_generate=True, **kw)
    g2 = um._engine._dec[0].graph
    assert g1 is not None and g2 is not None and g1 is not g2, "the second call replayed the first call's graph"
    greedy = um.generate(inputs_embeds=emb, max_new_tokens=8, eos_token_id=None, pad_token_id=PAD)
    lg = _logits_of(tight).float().cpu()
    top2 = torch.topk(lg, 2, dim=-1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-3 * top2[..., 0].abs().clamp(min=1.0)).all(1)
    assert bool(clear.any())
    assert torch.equal(tight.sequences[clear.cuda()], greedy[clear.cuda()]), "the ids of the second call do not follow its own min_p"
    _assert_never_drop(loose.sequences, _logits_of(loose), dict(kw, min_p=0.02), None, 0, "min_p = 0.02")
    again = um.generate(inputs_embeds=emb, min_p=0.02, **kw)
    assert torch.equal(again, loose.sequences)


# ------------------------------------------------------------------ (c) alongside the other options
def test_with_repetition_penalty_and_token_logprobs():
    um, hid, V = _model()
    emb = _emb(3, 8, hid, 406)
    kw = dict(SMP, **WARP)
    call = dict(max_new_tokens=8, eos_token_id=7, pad_token_id=PAD, min_new_tokens=1, repetition_penalty=1.3, **kw)
    r = um.generate(inputs_embeds=emb, output_logits=True, return_dict_in_generate=True, **call)
    _assert_never_drop(r.sequences, _logits_of(r), kw, 7, 1, "repetition_penalty", penalty=1.3)
    lp = um.generate(inputs_embeds=emb, output_token_logprobs=True, **call)
    assert torch.equal(lp.sequences, r.sequences)
    ref = torch.log_softmax(_logits_of(r).double().cpu(), -1).gather(-1, r.sequences.cpu()[..., None])[..., 0]
    live = lp.token_logprobs.cpu() != 0
    assert float((lp.token_logprobs.cpu().double() - ref)[live].abs().max()) < 1e-3, "token_logprobs are those of the RAW logits"


def test_generate_batches_coalesced_and_generate_questions():
    um, hid, V = _model()
    kw = dict(SMP, **WARP)
    call = dict(max_new_tokens=6, eos_token_id=None, pad_token_id=PAD, output_first_logits=True, **kw)
    embs = [_emb(2, 6, hid, 407), _emb(1, 9, hid, 408)]
    _stub_inputs(um)
    try:
        outs = um.generate_batches([dict(batch_input_ids=e, batch_X_modals=None) for e in embs], coalesce=True, **call)
        for g_, (ids, first) in enumerate(outs):
            assert ids.shape[0] == embs[g_].shape[0] and ids.shape[1] == 6
            _assert_never_drop(ids[:, :1], first[:, None], kw, None, 0, f"generate_batches(coalesce=True) batch {g_}, first step", exercised=False)
        g = torch.Generator().manual_seed(3)
        qs = [torch.randint(3, V, (int(s),), generator=g) for s in (3, 1, 2)]
        (ids, first), = um.generate_questions([dict(batch_input_ids=_emb(1, 6, hid, 409), batch_X_modals=None, question_ids=qs)], **call)
        assert tuple(ids.shape) == (3, 6)
        _assert_never_drop(ids[:, :1], first[:, None], kw, None, 0, "generate_questions, first step", exercised=False)
    finally:
        _unstub(um)
    # every step of a coalesced wave, through the engine, which hands out the step logits
    res_sampling = (SMP["temperature"], SMP["top_k"], SMP["top_p"], 5, WARP["min_p"], WARP["epsilon_cutoff"], WARP["eta_cutoff"])
    res = um._engine.generate_many(embs, 6, eos_token_id=None, pad_token_id=PAD, coalesce=True, return_step_logits=True, sampling=res_sampling)
    for g_, (ids, sl) in enumerate(res):
        _assert_never_drop(ids, sl, kw, None, 0, f"generate_many(coalesce=True) batch {g_}")
    # ... and of the shared prefix, the route generate_questions takes
    suffixes = [[um.encode_ids(q.cuda()).to(BF) for q in qs]]
    (ids, sl), = um._engine.generate_shared_prefix(_emb(1, 6, hid, 409), suffixes, 6, eos_token_id=None, pad_token_id=PAD, return_step_logits=True,
                                                   sampling=res_sampling)
    assert tuple(ids.shape) == (3, 6)
    _assert_never_drop(ids, sl, kw, None, 0, "generate_shared_prefix")


def test_with_guidance_the_guided_scores_go_through_the_warpers():
    from crab_amd import ops
    um, hid, V = _model()
    B, n, scale = 2, 6, 1.5
    emb, neg = _emb(B, 7, hid, 410), _emb(B, 4, hid, 411)
    kw = dict(SMP, **WARP)
    smp7 = (SMP["temperature"], SMP["top_k"], SMP["top_p"], 5, WARP["min_p"], WARP["epsilon_cutoff"], WARP["eta_cutoff"])
    ids, sl = um._engine.generate_guided(emb, neg, scale, n, eos_token_id=None, pad_token_id=PAD, sampling=smp7, return_step_logits=True)
    via_model = um.generate(inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=scale, max_new_tokens=n, eos_token_id=None, pad_token_id=PAD, **kw)
    assert torch.equal(via_model, ids) and tuple(sl.shape) == (2 * B, n, V)
    fin = torch.zeros(2 * B, dtype=torch.int32, device="cuda")

    def guided(t):                                               # the scores the step's select read: the same kernel on the same bits
        out = torch.empty((B, V), dtype=torch.float32, device="cuda")
        ops.cfg_mix(sl[:, t].contiguous(), out, B, scale, fin)
        return out.cpu()

    _assert_never_drop(ids, sl[:B], kw, None, 0, "guidance", chosen_from=guided)
