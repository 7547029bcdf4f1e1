"""GenerationEngine.generate_beam and generate(num_beams > 1) on the tiny Llama and Qwen2 models of scripts/fuzz_engine_state.py.

Yardsticks.  (1) Every call replayed step by step from its own `trace` through tests/beam_ref.step (the device's state before a step and the
step's logits in, the state after it out), under the EITHER rule and cap of tests/test_beam_gpu.py; the returned ids and scores are the
trace's final hypotheses.  (2) Graph replay equals eager steps bit for bit.  (3) The KV check, independent of the trace: a returned
hypothesis's sequences_scores x len ** length_penalty is the sum of its tokens' log-probs, and GenerationEngine.score() gives the same sum
teacher-forced on prompt + hypothesis through the ordinary prefill; both are bf16 executions of one stack, held to n x the per-token bound of
tests/score_bounds.py on those inputs.  A wrong cache reorder breaks this (a beam would attend another beam's keys); a right one cannot.
(4) One beam is greedy.  (5) The model surface."""
import functools
import os
import runpy

import pytest
import torch

from tests import beam_ref as R
from tests import bounds as PB
from tests import score_bounds as SB
from tests.util import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, N_NEW = 2, 12


@functools.lru_cache(maxsize=None)
def _model(qwen: bool):
    ns = runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_engine_state.py"), run_name="lib")
    return ns["build"](qwen)


def _um(qwen):
    um = _model(qwen).base_model.model
    return um, um._engine, um.config.hidden_size, um.lm_head.weight.shape[0]


@functools.lru_cache(maxsize=None)
def _oracle(qwen: bool):
    from oracle import crab_oracle as O
    model = _model(qwen)
    c = model.base_model.model.config
    W = {k: v.detach().float().cpu() for k, v in O.strip_peft_prefix(model.state_dict()).items() if v.dtype.is_floating_point}
    ocfg = O.DecoderConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads, vocab_size=c.vocab_size,
                           rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, lora_r=8, lora_alpha=16, lora_nums=3)
    return W, ocfg


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


@functools.lru_cache(maxsize=None)
def _eos(qwen: bool, B: int, S: int, seed: int):
    """An id the greedy path emits early on row 0: hypotheses then finish inside the 12 steps."""
    um, eng, hid, V = _um(qwen)
    free = eng.generate(_emb(B, S, hid, seed), N_NEW, eos_token_id=None, pad_token_id=PAD).cpu()
    return int(free[0, 3])


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def _replay(trace, K, V, eos, min_new, lp, early, what):
    """Every step of a call against the reference; returns (EITHER pairs, live pairs, the final state of every wave as a list)."""
    p = R.Params(K, V, N_NEW, eos, PAD, min_new, lp, early)
    hit = live = 0
    finals = []
    for i, e in enumerate(trace):
        before, got, z, s = _cpu(e["before"]), _cpu(e["after"]), e["logits"].float().cpu(), e["step"]
        clips = z.shape[0] // K
        if s == 0:
            init = R.init_state(clips, p)
            for f in init:
                if f != "cur_ids":
                    assert torch.equal(before[f].to(init[f].dtype), init[f]), f"{what}: initial {f}"
        want, either, tol = R.step(before, z, s, p)
        for cl in range(clips):
            if int(before["finished"][cl * K]) != 0:
                assert all(torch.equal(got[f], before[f]) if f == "unsat" else torch.equal(got[f][cl * K:cl * K + K], before[f][cl * K:cl * K + K])
                           for f in got), f"{what}: step {s} changed the done clip {cl}"
                continue
            live += 1
            if either[cl]:
                hit += 1
                continue
            bad = R.compare(got, want, tol, cl, K)
            assert not bad, f"{what}: step {s}, clip {cl}:\n  " + "\n  ".join(bad)
        if i + 1 == len(trace) or trace[i + 1]["step"] == 0:
            finals.append(got)
    return hit, live, finals


def _assert_result_is_the_final_state(ids, scores, finals, K, Rn, what):
    seq = torch.cat([f["hyp_seq"].view(-1, K, N_NEW)[:, :Rn] for f in finals], 0)
    sc = torch.cat([f["hyp_score"].view(-1, K)[:, :Rn] for f in finals], 0)
    ln = torch.cat([f["hyp_len"].view(-1, K)[:, :Rn] for f in finals], 0)
    n = max(1, int(ln.max()))
    ids, scores = ids.cpu(), scores.cpu()
    assert tuple(ids.shape) == (seq.shape[0] * Rn, n) and torch.equal(ids, seq[:, :, :n].reshape(-1, n)), f"{what}: ids"
    assert scores.dtype == torch.float32 and torch.equal(scores, sc.reshape(-1)), f"{what}: scores"
    flat_ln = ln.reshape(-1)
    for r in range(ids.shape[0]):
        assert bool((ids[r, int(flat_ln[r]):] == PAD).all()), f"{what}: row {r} is not padded after its {int(flat_ln[r])} tokens"


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
@pytest.mark.parametrize("K", [2, 4])
def test_calls_replay_through_the_reference_and_graph_equals_eager(qwen, K):
    um, eng, hid, V = _um(qwen)
    B, S = 3, 9
    emb = _emb(B, S, hid, 90 + K)
    eos = _eos(qwen, B, S, 90 + K)
    lp, early, min_new = (1.0, False, 0) if K == 2 else (2.0, "never", 2)
    runs = {}
    for graph in (True, False):
        tr = []
        ids, sc = eng.generate_beam(emb, K, N_NEW, eos_token_id=eos, pad_token_id=PAD, min_new_tokens=min_new, length_penalty=lp, early_stopping=early,
                                    num_return_sequences=K, use_graph=graph, return_scores=True, trace=tr)
        what = f"{'qwen2' if qwen else 'llama'} K={K} {'graph' if graph else 'eager'}"
        hit, live, finals = _replay(tr, K, V, eos, min_new, lp, early, what)
        share = hit / max(1, live)
        record_parity(f"generate_beam {what}: share of live (clip, step) pairs with a near-tie (EITHER)", share, 1.0, R.EITHER_CAP, live=live)
        print(f"{what}: {live} live (clip, step) pairs, {hit} EITHER ({share:.2%}); lengths {finals[0]['hyp_len'].tolist()}")
        assert share <= R.EITHER_CAP
        _assert_result_is_the_final_state(ids, sc, finals, K, K, what)
        runs[graph] = (ids.cpu(), sc.cpu(), tr)
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1]), "graph replay and eager steps differ"
    n = min(len(runs[True][2]), len(runs[False][2]))
    for a, b in zip(runs[True][2][:n], runs[False][2][:n]):
        assert torch.equal(a["logits"], b["logits"]) and all(torch.equal(a["after"][f], b["after"][f]) for f in a["after"]), f"step {a['step']}: graph vs eager"


def test_two_waves_through_max_rows():
    um, eng, hid, V = _um(False)
    B, S, K = 3, 9, 2
    emb = _emb(B, S, hid, 95)
    eos = _eos(False, B, S, 95)
    tr = []
    ids, sc = eng.generate_beam(emb, K, N_NEW, eos_token_id=eos, pad_token_id=PAD, num_return_sequences=2, max_rows=4, return_scores=True, trace=tr)
    n_waves = sum(1 for e in tr if e["step"] == 0)
    assert n_waves >= 2 and n_waves == len(eng.last_plan["groups"]), "max_rows = 4 cannot hold the six rows: whole clips in several waves (plan_shared_prefix)"
    hit, live, finals = _replay(tr, K, V, eos, 0, 1.0, False, "several waves")
    assert hit <= R.EITHER_CAP * live
    assert [f["hyp_score"].shape[0] for f in finals] == eng.last_plan["groups"] and sum(eng.last_plan["groups"]) == B * K
    _assert_result_is_the_final_state(ids, sc, finals, K, 2, "several waves")


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
def test_scores_are_the_teacher_forced_sums_of_score(qwen):
    """The KV check: independent of the trace and of the reference."""
    um, eng, hid, V = _um(qwen)
    B, S, K, lp = 2, 9, 4, 1.0
    emb = _emb(B, S, hid, 97)
    eos = _eos(qwen, B, S, 97)
    tr = []
    ids, sc = eng.generate_beam(emb, K, N_NEW, eos_token_id=eos, pad_token_id=PAD, length_penalty=lp, num_return_sequences=K, return_scores=True, trace=tr)
    ids, sc = ids.cpu(), sc.cpu()
    ln = _cpu(tr[-1]["after"])["hyp_len"].view(B, K).reshape(-1)
    real = ln > 0                                                # a slot no hypothesis reached keeps its placeholder (score -1e9, length 0): nothing to score
    assert int(real.sum()) >= B * 2 and bool(real.view(B, K)[:, 0].all()), f"too few finished hypotheses to check: lengths {ln.tolist()}"
    assert int(ln[real].max()) >= 4, f"no hypothesis is long enough to have been reordered: {ln.tolist()}"
    n = ids.shape[1]
    rows = B * K
    tok = um.model.embed_tokens.weight[ids.cuda().clamp(0, V - 1)]
    full = torch.cat([emb.repeat_interleave(K, 0), tok.to(BF)], 1)
    labels = torch.full((rows, S + n), -100, dtype=torch.long)
    for r in range(rows):
        labels[r, S:S + int(ln[r])] = ids[r, :int(ln[r])]
    got = eng.score(full, labels).sum_logprob.double().cpu()
    tab = R.len_table(N_NEW, lp).double()
    beam = sc.double() * tab[ln.long()]
    W, ocfg = _oracle(qwen)
    bd, ref, parts = SB.logprob_bound(full.float().cpu(), W, ocfg, labels)
    err = torch.where(real, (beam - got).abs(), torch.zeros_like(got))
    lim = ln.double().clamp(min=1) * bd
    print(f"{'qwen2' if qwen else 'llama'}: beam sums {beam.tolist()} vs score() {got.tolist()}; per-token bound {bd:.3e} ({parts}); "
          f"largest |difference| / (n x bound) {float((err / lim).max()):.3f}")
    record_parity("generate_beam: sequences_scores x len ** length_penalty vs score() teacher-forced", float(err.max()), float(got.abs().max()),
                  float(lim.max()) / float(got.abs().max()))
    assert bool((err <= lim).all()), f"|beam - score()| {err.tolist()} exceeds n x bound {lim.tolist()}"


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
def test_one_beam_is_greedy(qwen):
    um, eng, hid, V = _um(qwen)
    B, S = 3, 9
    emb = _emb(B, S, hid, 99)
    ref, lg = eng.generate(emb, N_NEW, eos_token_id=None, pad_token_id=PAD, return_step_logits=True)
    ref, lg = ref.cpu(), lg.float().cpu()
    got = eng.generate_beam(emb, 1, N_NEW, eos_token_id=None, pad_token_id=PAD).cpu()
    assert tuple(got.shape) == tuple(ref.shape)
    W, ocfg = _oracle(qwen)
    covered = 0
    for b in range(B):
        bnd = PB.decoder_bound(emb[b:b + 1].cpu(), W, ocfg, ref[b:b + 1]) * lg[b].abs().max().item()
        top2 = lg[b].topk(2, -1).values
        margin = top2[:, 0] - top2[:, 1]
        for s in range(N_NEW):
            if int(got[b, s]) != int(ref[b, s]):
                # within the bf16 bound of the logits either id is right; later steps see another context, so the row ends here
                assert float(margin[s]) <= 2 * bnd, f"row {b} step {s}: one beam chose {int(got[b, s])}, greedy {int(ref[b, s])} at margin {float(margin[s]):.3f} (bound {bnd:.3f})"
                break
            covered += float(margin[s]) > 2 * bnd
    print(f"one beam vs greedy: {covered} of {B * N_NEW} (row, step) pairs compared at a margin above the bound")
    assert covered >= 1, "no step had a margin above the bound: the comparison shows nothing"


def test_model_surface_and_a_following_greedy_call():
    um, eng, hid, V = _um(False)
    B, S, K, Rn = 2, 9, 4, 3
    emb = _emb(B, S, hid, 101)
    eos = _eos(False, B, S, 101)
    before = um.generate(inputs_embeds=emb, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=PAD).cpu()
    out = um.generate(inputs_embeds=emb, num_beams=K, num_return_sequences=Rn, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=PAD,
                      return_dict_in_generate=True, output_scores=True)
    ids, sc = out.sequences.cpu(), out.sequences_scores.cpu()
    assert ids.shape[0] == B * Rn and 1 <= ids.shape[1] <= N_NEW and ids.dtype == torch.int64 and tuple(sc.shape) == (B * Rn,) and sc.dtype == torch.float32
    s2 = sc.view(B, Rn)
    assert bool((s2[:, :-1] >= s2[:, 1:]).all()), "best hypothesis first per clip"
    for r in range(B * Rn):
        hit = torch.nonzero(ids[r] == eos)
        if hit.numel():
            assert bool((ids[r, int(hit[0]) + 1:] == PAD).all()), f"row {r}: pad after the hypothesis's EOS"
    plain = um.generate(inputs_embeds=emb, num_beams=K, num_return_sequences=Rn, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=PAD)
    assert torch.equal(plain.cpu(), ids)
    direct, dsc = eng.generate_beam(emb, K, N_NEW, eos_token_id=eos, pad_token_id=PAD, num_return_sequences=Rn, return_scores=True)
    assert torch.equal(direct.cpu(), ids) and torch.equal(dsc.cpu(), sc)
    after = um.generate(inputs_embeds=emb, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=PAD).cpu()
    assert torch.equal(before, after), "a greedy call after a beam call on the same engine"
    with pytest.raises(NotImplementedError, match="do_sample"):
        um.generate(inputs_embeds=emb, num_beams=K, do_sample=True, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="num_beams"):
        um.generate_batches([{"batch_input_ids": emb, "batch_X_modals": None}], num_beams=K, max_new_tokens=4)
