"""The logits processors of the decode step at the engine and the public surface: repetition_penalty, no_repeat_ngram_size and a
list-valued eos_token_id on the tiny models of scripts/fuzz_engine_state.py (Llama V = 320, Qwen2 V = 515), B <= 4, <= 16 new tokens.

The yardstick is EXACT: the call returns its raw step logits, the CPU restatement of HF's processors (tests/logits_proc_ref.py) edits them
with the ids emitted so far, and the first maximum (greedy) or the unchanged ops.sample_select (sample mode) must give the emitted id at
every step - no tolerance anywhere."""
import functools
import os
import runpy

import pytest
import torch

from crab_amd import decoder, ops
from tests import logits_proc_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 2
N_NEW = 16
SEED = {False: 208, True: 201}                                   # prompts whose FREE greedy run repeats a token and a bigram within N_NEW tokens (asserted below)


@functools.lru_cache(maxsize=None)
def _model(qwen=False):
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](qwen).base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


def _repeats(row):
    """(a token occurs twice, a bigram occurs twice) in a list of ids."""
    big = list(zip(row, row[1:]))
    return len(set(row)) < len(row), len(set(big)) < len(big)


def _cut(row, stops):
    for j, t in enumerate(row):
        if t in stops:
            return row[:j]
    return row


def _replay_greedy(ids, lg, prm, what):
    ids, lg = ids.cpu(), lg.float().cpu()
    assert tuple(lg.shape[:2]) == tuple(ids.shape)
    assert bool(torch.isfinite(lg).all()), f"{what}: the returned logits are the RAW ones (nothing banned in them)"
    fin = torch.zeros(ids.shape[0], dtype=torch.int32)
    for t in range(ids.shape[1]):
        want = R.edit(lg[:, t], ids, t, fin, prm).argmax(1)      # torch.argmax: the first maximum
        assert torch.equal(want, ids[:, t]), f"{what}: step {t}: restatement {want.tolist()} emitted {ids[:, t].tolist()}"


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen"])
def test_greedy_ids_replay_exactly_from_the_raw_step_logits(qwen):
    um, hid, V = _model(qwen)
    emb = _emb(4, 7, hid, SEED[qwen])
    kw = dict(inputs_embeds=emb, max_new_tokens=N_NEW, eos_token_id=None, pad_token_id=PAD)
    free = um.generate(**kw).cpu().tolist()
    tok, big = zip(*[_repeats(r) for r in free])
    assert any(tok) and any(big), f"the free run repeats nothing, the edited run would show nothing: {free}"
    for p, n in ((1.3, 2), (1.0, 3), (1.5, 0), (0.8, 0)):
        r = um.generate(output_logits=True, return_dict_in_generate=True, repetition_penalty=p, no_repeat_ngram_size=n, **kw)
        _replay_greedy(r.sequences, torch.stack(r.logits, 1), R.Params(p, n), f"p = {p}, n = {n}")
        rows = r.sequences.cpu().tolist()
        if n:
            grams = [list(zip(*[row[i:] for i in range(n)])) for row in rows]
            assert all(len(set(g)) == len(g) for g in grams), f"an {n}-gram repeats: {rows}"
        if (p, n) == (1.3, 2):
            assert rows != free


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen"])
def test_sampled_ids_replay_exactly_through_the_unchanged_sample_select(qwen):
    um, hid, V = _model(qwen)
    B = 3
    emb = _emb(B, 6, hid, 210 + int(qwen))
    p, n, seed, t_, k_, pp = 1.4, 2, 5, 1.1, 40, 0.95
    r = um.generate(inputs_embeds=emb, max_new_tokens=10, eos_token_id=None, pad_token_id=PAD, do_sample=True, temperature=t_, top_k=k_, top_p=pp, seed=seed,
                    output_logits=True, return_dict_in_generate=True, repetition_penalty=p, no_repeat_ngram_size=n)
    ids, lg = r.sequences.cpu(), torch.stack(r.logits, 1).float().cpu()
    fin = torch.zeros(B, dtype=torch.int32)
    cur, out = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, ids.shape[1], dtype=torch.int64, device="cuda")
    step, fin_d = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    for t in range(ids.shape[1]):
        edited = R.edit(lg[:, t], ids, t, fin, R.Params(p, n)).cuda()
        step.fill_(t)
        ops.sample_select(edited, cur, out, step, fin_d, -1, PAD, 0, t_, k_, pp, seed)
        assert torch.equal(cur.cpu(), ids[:, t]), f"step {t}: {cur.tolist()} vs emitted {ids[:, t].tolist()}"
    grams = [list(zip(row, row[1:])) for row in ids.tolist()]
    assert all(len(set(g)) == len(g) for g in grams)


def test_ngram_size_one_makes_every_id_before_the_stop_distinct():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(4, 7, hid, SEED[False])
    free = eng.generate(emb, N_NEW, eos_token_id=None, pad_token_id=PAD).cpu()
    eos = int(free[0, 5])
    ids = eng.generate(emb, N_NEW, eos_token_id=eos, pad_token_id=PAD, processors=(1.0, 1, ())).cpu().tolist()
    for row in ids:
        live = _cut(row, {eos})
        assert len(set(live)) == len(live), row
    assert any(len(_cut(row, {eos})) >= 8 for row in ids)


def test_graph_eager_and_the_python_sequencer_give_the_same_bits():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 6, hid, SEED[False])
    for kw in (dict(processors=(1.3, 2, ())), dict(processors=(1.2, 3, ()), sampling=(0.9, 30, 0.9, 3))):
        kw = dict(dict(eos_token_id=None, pad_token_id=PAD, return_step_logits=True), **kw)
        eng.invalidate()
        a, la = eng.generate(emb, 9, **kw)
        assert eng._dec[0].graph is not None and eng._dec[0].proc is not None
        a2, la2 = eng.generate(emb, 9, **kw)                     # the captured graph again
        b, lb = eng.generate(emb, 9, use_graph=False, **kw)
        decoder.NATIVE_LAYERS = False
        try:
            eng.invalidate()
            c, lc = eng.generate(emb, 9, **kw)
        finally:
            decoder.NATIVE_LAYERS = True
            eng.invalidate()
        assert torch.equal(a, b) and torch.equal(a, a2) and torch.equal(a, c)
        assert torch.equal(la, lb) and torch.equal(la, la2) and torch.equal(la, lc)


def _stub_inputs(um):
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    um.prepare_multimodal_inputs_many = lambda batches, **k: [{"inputs_embeds": b["batch_input_ids"]} for b in batches]


def _unstub(um):
    del um.prepare_multimodal_inputs, um.prepare_multimodal_inputs_many


def test_coalesced_batches_equal_separate_calls():
    um, hid, V = _model()
    eng = um._engine
    embs = [_emb(2, 6, hid, 220), _emb(1, 9, hid, 221), _emb(2, 8, hid, 222)]
    kw = dict(max_new_tokens=10, eos_token_id=None, pad_token_id=PAD, repetition_penalty=1.3, no_repeat_ngram_size=2)
    _stub_inputs(um)
    try:
        outs = um.generate_batches([dict(batch_input_ids=e, batch_X_modals=None) for e in embs], coalesce=True, **kw)
        assert eng.last_plan["groups"] == [5], eng.last_plan
        flight = um.generate_batches([dict(batch_input_ids=e, batch_X_modals=None) for e in embs], coalesce=False, **kw)
    finally:
        _unstub(um)
    for e, ids, fl in zip(embs, outs, flight):
        one = um.generate(inputs_embeds=e, **kw)
        assert torch.equal(fl, one), "in flight: the same launches, bit for bit"
        assert torch.equal(ids, one), (ids.tolist(), one.tolist())
    # and the wave's own raw logits replay exactly, whatever kernels its row count selected
    res = eng.generate_many(embs, 10, eos_token_id=None, pad_token_id=PAD, coalesce=True, return_step_logits=True, processors=(1.3, 2, ()))
    for ids, lg in res:
        _replay_greedy(ids, lg, R.Params(1.3, 2), "coalesced wave")


def test_a_shared_prefix_wave_equals_the_coalesced_one():
    um, hid, V = _model()
    eng = um._engine
    prefix = _emb(2, 6, hid, 230)
    g_ = torch.Generator().manual_seed(9)
    questions = [[torch.randint(3, V, (int(s),), generator=g_) for s in ss] for ss in ([2], [3, 1, 2])]
    suffix = [[um.encode_ids(q.cuda()).to(BF) for q in qs] for qs in questions]
    kw = dict(eos_token_id=None, pad_token_id=PAD, processors=(1.3, 2, ()))
    res = eng.generate_shared_prefix(prefix, suffix, 10, return_step_logits=True, **kw)
    assert eng._dec[0].proc == (1.3, 2, ())
    for c, (ids, lg) in enumerate(res):
        _replay_greedy(ids, lg, R.Params(1.3, 2), f"shared prefix clip {c}")
        co = eng.generate_many([torch.cat([prefix[c], q], 0)[None] for q in suffix[c]], 10, coalesce=True, **kw)
        assert torch.equal(ids, torch.cat(co, 0)), (ids.tolist(), [o.tolist() for o in co])


def test_fp8_kv_cache_runs_with_processors():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 7, hid, SEED[False])
    ids, lg = eng.generate(emb, 10, eos_token_id=None, pad_token_id=PAD, kv_cache_dtype="fp8_e4m3", return_step_logits=True, processors=(1.3, 2, ()))
    _replay_greedy(ids, lg, R.Params(1.3, 2), "fp8 KV")


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen"])
def test_several_stop_ids(qwen):
    um, hid, V = _model(qwen)
    eng = um._engine
    emb = _emb(2, 7, hid, 240 + int(qwen))
    n = 10
    kw = dict(inputs_embeds=emb, max_new_tokens=n, pad_token_id=PAD)
    free = um.generate(eos_token_id=None, **kw).cpu()
    # two different ids that the two rows emit at different steps, read off the free run
    rows = free.tolist()
    first_of = lambda ids: [min([j for j, t in enumerate(row) if t in ids] or [n]) for row in rows]
    picks = [(rows[0][i], rows[1][j]) for i in range(1, n - 3) for j in range(1, n - 3)
             if rows[0][i] != rows[1][j] and PAD not in (rows[0][i], rows[1][j]) and max(first_of((rows[0][i], rows[1][j]))) < n - 3
             and len(set(first_of((rows[0][i], rows[1][j])))) == 2]
    assert picks, f"no two stop ids at different steps in {rows}"
    a, b = picks[0]
    firsts = first_of((a, b))
    got = um.generate(eos_token_id=[a, b], **kw).cpu()
    assert got.shape[1] == max(firsts) + 1 < n, "trimmed where all rows have stopped"
    for r, row in enumerate(got.tolist()):
        k = firsts[r]
        assert row[:k + 1] == free[r].tolist()[:k + 1], "the free run up to and including whichever id comes first"
        assert all(t == PAD for t in row[k + 1:]), "padding after the stop"
    assert torch.equal(um.generate(eos_token_id=[b, a], **kw).cpu(), got), "with a pad id given the order of the stop ids means nothing"
    # no pad id: the first stop id pads, as in HF
    dflt = eng.generate(emb, n, eos_token_id=a, pad_token_id=None, processors=(1.0, 0, [b])).cpu()
    assert torch.equal(dflt, torch.where(got == PAD, torch.full_like(got, a), got)) and bool((got == PAD).any())
    # min_new_tokens suppresses BOTH ids
    m = max(firsts) + 2
    sup = um.generate(eos_token_id=[a, b], min_new_tokens=m, **kw).cpu()
    assert sup.shape[1] >= m and not bool(((sup[:, :m] == a) | (sup[:, :m] == b)).any()), sup.tolist()
    assert torch.equal(sup[:, :min(firsts)], free[:, :min(firsts)])
    # [a] and [a, a] are the one-id call: same ids, same decode state, no processors
    one = um.generate(eos_token_id=a, **kw)
    st = eng._dec[0]
    for form in ([a], [a, a]):
        assert torch.equal(um.generate(eos_token_id=form, **kw), one) and eng._dec[0] is st and st.proc is None
    # the engine keeps its one-id rule for eos_token_id and takes the rest as stop_token_ids
    with pytest.raises(NotImplementedError, match="ONE id"):
        eng.generate(emb, n, eos_token_id=[a, b], pad_token_id=PAD)
    assert torch.equal(eng.generate(emb, n, eos_token_id=a, pad_token_id=PAD, processors=(1.0, 0, [b])).cpu(), got)
    # the public log-probability fields count the first of ANY stop id as the row's last token
    r = um.generate(eos_token_id=[a, b], output_token_logprobs=True, **kw)
    assert torch.equal(r.sequences.cpu(), got) and r.num_tokens.tolist() == [k + 1 for k in firsts]
    for row, k in zip(r.token_logprobs.cpu(), firsts):
        assert bool((row[:k + 1] < 0).all()) and bool((row[k + 1:] == 0).all())


def test_the_penalty_enters_neither_logprob_plane():
    um, hid, V = _model()
    emb = _emb(3, 7, hid, SEED[False])
    r = um.generate(inputs_embeds=emb, max_new_tokens=10, eos_token_id=None, pad_token_id=PAD, repetition_penalty=1.4, output_token_logprobs=True,
                    output_logits=True, return_dict_in_generate=True)
    plain = um.generate(inputs_embeds=emb, max_new_tokens=10, eos_token_id=None, pad_token_id=PAD, repetition_penalty=1.4)
    assert torch.equal(plain, r.sequences)
    ids, lg = r.sequences.cpu(), torch.stack(r.logits, 1).float().cpu()
    _replay_greedy(ids, lg, R.Params(1.4, 0), "penalty with logprobs")
    # score()-style values from the RAW step logits: z[y] - logsumexp(z), in fp64; the kernel's own bound (tests/logprob_ref.py) is far below 1e-4,
    # a penalised logit (x / 1.4 or x * 1.4 on |x| ~ 1) would move the value by ~ 0.3
    ref = torch.log_softmax(lg.double(), -1).gather(2, ids[..., None])[..., 0]
    err = float((r.token_logprobs.cpu().double() - ref).abs().max())
    print(f"token_logprobs vs the raw-logit log-softmax: max |difference| {err:.3e}")
    from tests import logprob_ref as L
    want, live, bound = L.walk_ref(lg, ids, -1, 0, None, None)
    got = torch.stack([r.token_logprobs, r.token_logprobs_allowed], 0).cpu().double()
    assert bool(((got - want).abs() <= bound).all())
    assert torch.equal(r.token_logprobs, r.token_logprobs_allowed)
    for kw in (dict(no_repeat_ngram_size=2), dict(eos_token_id=[5, 6], min_new_tokens=2)):
        with pytest.raises(NotImplementedError, match="output_token_logprobs with"):
            um.generate(inputs_embeds=emb, max_new_tokens=4, pad_token_id=PAD, output_token_logprobs=True, **kw)


def test_nothing_changes_when_off():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 6, hid, 250)
    kw = dict(inputs_embeds=emb, max_new_tokens=6, eos_token_id=None, pad_token_id=PAD)
    um.generate(use_graph=False, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_plain:
        plain = um.generate(use_graph=False, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_off:
        off = um.generate(use_graph=False, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw)
    with ops.launch_trace(emb.device.index or 0) as t_on:
        um.generate(use_graph=False, repetition_penalty=1.2, **kw)
    assert t_off.launched("logits_edit") == 0 and t_off.launched("logits_restore") == 0 and t_off.counts == t_plain.counts
    assert t_on.launched("logits_edit") == 6 and t_on.launched("logits_restore") == 6
    assert {k: v for k, v in t_on.counts.items() if not k.startswith("logits_")} == t_plain.counts, "the option adds its two launches and nothing else"
    assert torch.equal(plain, off)
    a = um.generate(**kw)
    st = eng._dec[0]
    b = um.generate(repetition_penalty=1.0, no_repeat_ngram_size=0, **kw)
    assert eng._dec[0] is st and st.proc is None and torch.equal(a, b) and torch.equal(a, plain)
    c = eng.generate(emb, 6, eos_token_id=None, pad_token_id=PAD, processors=(1.0, 0, ()))
    assert eng._dec[0] is st and torch.equal(c, a)
    um.generate(repetition_penalty=1.2, **kw)
    assert eng._dec[0] is not st and eng._dec[0].proc == (1.2, 0, ()), "a state with the pair never serves a call without it, nor the reverse"
    d = um.generate(**kw)
    assert eng._dec[0].proc is None and torch.equal(d, a)
