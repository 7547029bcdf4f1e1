"""GenerationEngine.generate_shared_prefix / UnifiedForCausalLM.generate_questions against the path that existed before them:
generate_many(coalesce=True, return_step_logits=True) on the concatenated embeddings cat(prefix_c, suffix_cg), every question a batch of its own.

Rules (the project's): logits of the first token and of every step within tests/bounds.decoder_bound of this stack (1.5 x max(bf16-operand floor,
bf16-storage emulation) of the oracle teacher-forced along the existing path's ids, per row); a differing id is accepted only at a step where the
EXISTING path's own top-2 margin is below 10 x that bound, and ends the comparison of its row (later steps see different contexts).

Coverage, as measured on an MI355X by running the existing path alone on data seeds 1 .. 8 (both models, P = 5 and 17): on this tiny random model the
bound is 1-3 % of the logit scale, and 10 x the bound exceeds almost every top-2 margin - only 0 .. 3 of the 24 (row, step) pairs of a case lie before
the first sub-margin step, for EVERY seed, so no seed can put 75 % of the pairs in front of it.  The 75 % are therefore required of what that
coverage is for: at least 75 % of all (row, step) pairs must actually be COMPARED - ids equal and logits within the bound - before a row's first
(legitimate) divergence.  Measured with DATA_SEED = 5 (and 6 for the second call of the graph test): 24 / 24 pairs in every case, ids equal at every
step, worst |dlogit| 0.17 .. 0.31 of the bound.  Every test prints its figures (pytest -s)."""
import functools
import os
import runpy

import pytest
import torch

from tests import bounds as PB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = 6
SUFFIX_LENS = ((2, 5, 3), (4,))                                   # C = 2 clips with G = (3, 1): ragged questions, a clip with one question
DATA_SEED = 5


@functools.lru_cache(maxsize=None)
def _model(qwen: bool):
    ns = runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_engine_state.py"), run_name="lib")
    return ns["build"](qwen)


def _oracle(qwen: bool):
    from oracle import crab_oracle as O
    model = _model(qwen)
    c = model.base_model.model.config
    W = {k: v.detach().float().cpu() for k, v in O.strip_peft_prefix(model.state_dict()).items() if v.dtype.is_floating_point}
    ocfg = O.DecoderConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads, vocab_size=c.vocab_size,
                           rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, lora_r=8, lora_alpha=16, lora_nums=3)
    return W, ocfg


def _data(qwen: bool, P: int, seed: int = DATA_SEED):
    D = _model(qwen).base_model.model.config.hidden_size
    g = torch.Generator().manual_seed(1000 * seed + P)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(BF).cuda()
    prefix = rn(len(SUFFIX_LENS), P, D)
    suffix = [[rn(S, D) for S in lens] for lens in SUFFIX_LENS]
    return prefix, suffix


def _concat(prefix, suffix):
    return [torch.cat([prefix[c], q], 0)[None] for c, qs in enumerate(suffix) for q in qs]


@functools.lru_cache(maxsize=None)
def _reference(qwen: bool, P: int, seed: int = DATA_SEED):
    """The existing path, greedy, no EOS, computed once per (model, P): per row (ids [n], logits [n, V], absolute bound)."""
    eng = _model(qwen).base_model.model._engine
    seqs = _concat(*_data(qwen, P, seed))
    res = eng.generate_many(seqs, N_NEW, eos_token_id=None, pad_token_id=2, coalesce=True, return_step_logits=True)
    W, ocfg = _oracle(qwen)
    rows = []
    for e, (ids, logits) in zip(seqs, res):
        ids, logits = ids.cpu(), logits.float().cpu()
        bnd = PB.decoder_bound(e.cpu(), W, ocfg, ids) * logits.abs().max().item()
        rows.append((ids[0], logits[0], bnd))
    return tuple(rows)


def _compare(what, outs, ref_rows, sampled=False):
    """outs: per clip (ids [G, n], logits [G, n, V]) of the new path -> share of (row, step) pairs compared before a legitimate divergence."""
    r, covered, total, worst = 0, 0, 0, 0.0
    for ids_c, log_c in outs:
        ids_c, log_c = ids_c.cpu(), log_c.float().cpu()
        for g in range(ids_c.shape[0]):
            rid, rlog, bnd = ref_rows[r]
            assert ids_c.shape[1] == rid.shape[0] == N_NEW
            total += N_NEW
            for s in range(N_NEW):
                err = (log_c[g, s] - rlog[s]).abs().max().item()
                worst = max(worst, err / bnd)
                assert err <= bnd, f"{what}: row {r} step {s}: |dlogit| {err:.4e} above the bound {bnd:.4e}"
                if ids_c[g, s] != rid[s]:
                    if not sampled:
                        top2 = rlog[s].topk(2).values
                        assert (top2[0] - top2[1]).item() < 10 * bnd, f"{what}: row {r} step {s}: id {ids_c[g, s]} vs {rid[s]} at margin {(top2[0] - top2[1]).item():.4f} >= 10 x bound {bnd:.4e}"
                    break
                covered += 1
            r += 1
    share = covered / total
    print(f"\n{what}: {covered}/{total} (row, step) pairs compared ({share:.2f}), worst |dlogit| / bound {worst:.3f}")
    assert share >= 0.75, f"{what}: only {share:.2f} of the (row, step) pairs lie before the first sub-margin step"
    return share


@pytest.mark.parametrize("P", [5, 17])
@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_logits_and_ids_equal_the_existing_path(qwen, P, graph):
    eng = _model(qwen).base_model.model._engine
    prefix, suffix = _data(qwen, P)
    ref = _reference(qwen, P)
    outs = eng.generate_shared_prefix(prefix, suffix, N_NEW, eos_token_id=None, pad_token_id=2, use_graph=graph, return_step_logits=True)
    assert [tuple(o[0].shape) for o in outs] == [(len(l), N_NEW) for l in SUFFIX_LENS]
    _compare(f"{'qwen' if qwen else 'llama'} P={P} {'graph' if graph else 'eager'}", outs, ref)
    first = eng.generate_shared_prefix(prefix, suffix, N_NEW, eos_token_id=None, pad_token_id=2, use_graph=graph, return_first_logits=True)
    for (i0, l0), (i1, l1) in zip(outs, first):
        assert torch.equal(i0, i1) and torch.equal(l0[:, 0], l1)       # same call twice: bit-equal, first logits = step 0


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen"])
def test_captured_graph_is_reused_on_new_inputs_of_the_same_shapes(qwen):
    eng = _model(qwen).base_model.model._engine
    P = 17
    outs = eng.generate_shared_prefix(*_data(qwen, P), N_NEW, eos_token_id=None, pad_token_id=2, use_graph=True, return_step_logits=True)
    g0 = eng._dec[0].graph
    assert g0 is not None
    _compare("first call", outs, _reference(qwen, P))
    outs2 = eng.generate_shared_prefix(*_data(qwen, P, DATA_SEED + 1), N_NEW, eos_token_id=None, pad_token_id=2, use_graph=True, return_step_logits=True)
    assert eng._dec[0].graph is g0, "the second call of the same shapes captured a new graph"
    _compare("second call, replayed graph", outs2, _reference(qwen, P, DATA_SEED + 1))


def test_eos_trim_and_padding_equal_the_existing_path():
    """An EOS id that one row hits early (the id the existing path emits for row 1 at step 2): per clip the ids are the existing path's rows, padded
    with the pad id to the clip's longest row and cut where all of the clip's rows have finished."""
    qwen, P = False, 17
    eng = _model(qwen).base_model.model._engine
    prefix, suffix = _data(qwen, P)
    ref = _reference(qwen, P)
    # the trim / pad layout is compared exactly; that is determined only where the two paths' greedy ids agree without an EOS (the margin rule lets
    # them differ at sub-margin steps: measured equal at every step with DATA_SEED)
    free = eng.generate_shared_prefix(prefix, suffix, N_NEW, eos_token_id=None, pad_token_id=2)
    r = 0
    for ids_c in free:
        for g in range(ids_c.shape[0]):
            assert torch.equal(ids_c[g].cpu(), ref[r][0]), "pick another DATA_SEED: the greedy ids differ at a sub-margin step, the EOS case is undetermined"
            r += 1
    eos, pad = int(ref[1][0][2]), 2
    old = eng.generate_many(_concat(prefix, suffix), N_NEW, eos_token_id=eos, pad_token_id=pad, coalesce=True)
    new = eng.generate_shared_prefix(prefix, suffix, N_NEW, eos_token_id=eos, pad_token_id=pad)
    assert old[1].shape[1] == 3 and int(old[1][0, -1]) == eos         # row 1 really stops early
    r = 0
    for ids_c, lens in zip(new, SUFFIX_LENS):
        rows = [old[r + g][0] for g in range(len(lens))]
        n = max(x.shape[0] for x in rows)
        want = torch.stack([torch.cat([x, x.new_full((n - x.shape[0],), pad)]) for x in rows])
        assert torch.equal(ids_c, want), (ids_c, want)
        r += len(lens)


def test_sampling_with_a_fixed_seed():
    """Sample mode draws per (seed, step, row of the wave); both paths hold the same rows in the same order, so the draws are the same numbers and the
    ids agree wherever the logits' difference does not move a CDF edge across the draw.  The position of the draw inside the CDF is not observable
    from outside, so a divergence cannot be held to a margin: the logits are compared up to the first differing id (teacher-forced bound of the
    greedy reference rows does not apply to sampled contexts, so the existing sampled path's own logits are the reference) and 75 % of the pairs must
    lie before it."""
    qwen, P = False, 17
    eng = _model(qwen).base_model.model._engine
    prefix, suffix = _data(qwen, P)
    samp = (0.7, 20, 0.9, 1234)
    old = eng.generate_many(_concat(prefix, suffix), N_NEW, eos_token_id=None, pad_token_id=2, coalesce=True, return_step_logits=True, sampling=samp)
    ref = tuple((ids.cpu()[0], lg.float().cpu()[0], b) for (ids, lg), (_, _, b) in zip(old, _reference(qwen, P)))
    new = eng.generate_shared_prefix(prefix, suffix, N_NEW, eos_token_id=None, pad_token_id=2, return_step_logits=True, sampling=samp)
    _compare("sampling", new, ref, sampled=True)


def test_fp8_modes_are_refused_by_name():
    eng = _model(False).base_model.model._engine
    prefix, suffix = _data(False, 5)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        eng.generate_shared_prefix(prefix, suffix, 3, kv_cache_dtype="fp8_e4m3")
    with pytest.raises(NotImplementedError, match="weight_dtype"):
        eng.generate_shared_prefix(prefix, suffix, 3, weight_dtype="fp8_e4m3")
    assert eng.kv_cache_dtype == "bf16" and eng.weight_dtype == "bf16"


def test_generate_questions_on_a_synthetic_clip():
    """Model level: one synthetic clip (crab_amd/synth.py) with two questions == generate() on the two full id sequences under the margin rule;
    prepare_multimodal_inputs ran once."""
    from crab_amd import synth
    from tests.util import build_tiny_crab, load_fixture, weights_from_table
    meta, A = load_fixture("full_tiny_llama")
    model = build_tiny_crab(meta, device="cuda:0")
    assert not model.load_state_dict(weights_from_table(meta), strict=False).missing_keys
    um = model.base_model.model
    p = meta["prompts"]
    mods = [{'<video>': synth.synth_video(p["t_v"], seed=meta["seed"], clip=p["clip0"]),
             '<audio>': synth.synth_audio(p["t_a"], p["l_a"], seed=meta["seed"], clip=p["clip0"])}]
    ids0 = A["ids0"]
    g = torch.Generator().manual_seed(3)
    questions = [torch.randint(10, 200, (n,), generator=g) for n in (3, 6)]
    n = 5
    refs = []
    for q in questions:
        full = torch.cat([ids0, q])
        r = model.generate(batch_input_ids=[full], batch_labels=[torch.full_like(full, -100)], batch_X_modals=mods, batch_task_names=['avqa'],
                           use_cache=True, max_new_tokens=n, pad_token_id=2, eos_token_id=None, output_logits=True, return_dict_in_generate=True)
        refs.append((r.sequences.cpu()[0], torch.stack(r.logits, 1).float().cpu()[0]))
    calls = []
    inner = um.prepare_multimodal_inputs

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    um.prepare_multimodal_inputs = counted
    try:
        out = model.generate_questions([dict(batch_input_ids=[ids0], batch_labels=[torch.full_like(ids0, -100)], batch_X_modals=mods,
                                             batch_task_names=['avqa'], question_ids=questions)],
                                       max_new_tokens=n, pad_token_id=2, eos_token_id=None, output_first_logits=True)
    finally:
        del um.prepare_multimodal_inputs
    assert len(calls) == 1
    (ids, first), = out
    ids, first = ids.cpu(), first.float().cpu()
    assert tuple(ids.shape) == (2, n)
    bnd = PB.bound("full_tiny_llama: end to end")
    covered = 0
    for gq, (rid, rlog) in enumerate(refs):
        tol = bnd * rlog.abs().max().item()
        err = (first[gq] - rlog[0]).abs().max().item()
        print(f"\nquestion {gq}: first-token |dlogit| {err:.4e}, bound {tol:.4e}; ids {ids[gq].tolist()} vs {rid.tolist()}")
        assert err <= tol
        top2 = rlog.topk(2, -1).values
        margin = top2[:, 0] - top2[:, 1]
        for s in range(n):
            if ids[gq, s] != rid[s]:
                assert margin[s].item() < 10 * tol, (gq, s, margin[s].item(), tol)
                break
            covered += 1
    # the same coverage floor as _compare: a divergence at a sub-margin step is legitimate, but 75 % of the (question, step) pairs must be equal before
    # one (measured on an MI355X: 10 / 10, both questions equal at every step)
    assert covered >= 0.75 * 2 * n, f"only {covered} of {2 * n} (question, step) pairs equal before the first divergence"
