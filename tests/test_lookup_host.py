"""Prompt-lookup speculative decoding without a device: the CPU restatement (tests/lookup_ref.py) against transformers' own
PromptLookupCandidateGenerator.get_candidates, the -1 extension against hand-written expectations, the refusals of the engine and the model
surface (all before any device work) and of the three C entry points (csrc/attn_verify.hip, csrc/lookup.hip)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder, ops
from crab_amd.unified_llama import UnifiedForCausalLM as U
from tests import lookup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ (a) the restatement equals HF
def test_draft_equals_hf_get_candidates():
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except Exception as e:                                       # pragma: no cover
        pytest.skip(f"transformers' PromptLookupCandidateGenerator is not importable here: {e}")
    cases = R.hf_cases()
    nonempty = 0
    for hist, k, m, eos in cases:
        gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor([eos]) if eos is not None else None, num_output_tokens=k,
                                             max_matching_ngram_size=m, max_length=len(hist) + 64)
        ids = torch.tensor([hist], dtype=torch.long)
        cand, _ = gen.get_candidates(ids)
        want = cand[0, len(hist):].tolist()
        got = R.draft(hist, k, m, eos, remaining=63)
        assert got == want, f"hist {hist} k={k} max_ngram={m} eos={eos}: {got} vs HF {want}"
        nonempty += bool(want)
    assert nonempty * 2 >= len(cases), f"only {nonempty} of {len(cases)} cases drafted anything: the comparison would be hollow"


def test_no_room_left_means_no_draft_as_in_hf():
    """HF: `if self.max_length == input_length + 1: return` - the verify step's own token is the last one."""
    assert R.draft([1, 2, 1, 2, 1], 3, 2, None, remaining=0) == []
    assert R.draft([1, 2, 1, 2, 1], 3, 2, None, remaining=1) == [2]
    assert R.draft([1, 2, 1, 2, 1], 3, 2, None, remaining=5) == [2, 1]      # the continuation ends with the history


@pytest.mark.parametrize("hist, k, m, eos, remaining, want", R.HAND)
def test_draft_extension_by_hand(hist, k, m, eos, remaining, want):
    assert R.draft(hist, k, m, eos, remaining) == want


def test_out_of_vocabulary_entries_are_no_tokens():
    assert R.draft([3, 99, 5, 3, 7, 3], 3, 1, None, 9, V=10) == [7, 3]
    assert R.draft([3, 99, 5, 3, 7, 3], 3, 1, None, 9) == [99, 5, 3]


def test_simulate_both_ends_of_the_acceptance_range():
    g = [7, 8, 9, 10, 11, 12, 13, 14]
    out, st = R.simulate(g, [0, 0] + g, 3, 2, None, len(g))     # the prompt holds the whole tape: every draft is right
    assert out == g and st == [2, 5, 5, 7]                       # drafts (8 9 10) + the model's 11, then (12 13) - cut to what may still be emitted - + 14
    out, st = R.simulate(g, R.all_wrong_prompt(g, 100), 3, 2, None, len(g))
    assert out == g and st[0] == len(g) - 1 and st[2] == 0 and st[3] == len(g) - 1
    out, st = R.simulate(g, None, 3, 2, None, len(g))           # no repeats in the tape: nothing is ever drafted
    assert out == g and st == [7, 0, 0, 7]
    out, st = R.simulate(g, [0, 0] + g, 3, 2, 10, len(g))       # the EOS ends the call inside the run: drafts stop before it, the model emits it
    assert out == [7, 8, 9, 10]


def test_accept_rule():
    V = 6
    lg = torch.full((4, V), -1.0)
    lg[0, 2] = lg[1, 3] = lg[2, 5] = lg[3, 1] = 1.0
    em, a, fin = R.accept(lg, [0, 2, 3, 4], 3, step=1, eos=-1, min_new=0, max_new=20)
    assert (em, a, fin) == ([2, 3, 5], 2, False)
    em, a, fin = R.accept(lg, [0, 2, 3, 4], 3, step=1, eos=3, min_new=0, max_new=20)
    assert (em, a, fin) == ([2, 3], 2, True)                    # the EOS inside the accepted run ends it
    em, a, fin = R.accept(lg, [0, 2, 3, 4], 3, step=1, eos=3, min_new=3, max_new=20)
    assert em[0] == 2 and em[1] != 3                            # suppressed while step + i < min_new (index 2)
    em, a, fin = R.accept(lg, [0, 2, 3, 4], 3, step=1, eos=-1, min_new=0, max_new=3)
    assert (em, a, fin) == ([2, 3], 2, True)                    # the clamp at max_new_tokens
    tie = torch.zeros((1, V))
    assert R.accept(tie, [0], 0, 0, -1, 0, 9)[0] == [0] and R.greedy(torch.tensor([1.0, 3.0, 3.0])) == 1


# ------------------------------------------------------------------ (b) the refusals of the engine and the model
def _bare_engine(V=64):
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    eng.lm_head = types.SimpleNamespace(weight=torch.zeros((V, 8)))
    eng._kv_mode, eng._w_mode = "bf16", "bf16"
    eng._call = lambda *a, **k: pytest.fail("device work was reached")
    return eng


def test_engine_refuses_by_name_before_any_device_work():
    eng = _bare_engine()
    emb = torch.zeros((1, 5, 8))
    g = eng.generate_lookup
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_draft_tokens"):
            g(emb, 8, k)
    with pytest.raises(ValueError, match="max_ngram"):
        g(emb, 8, 3, max_ngram=0)
    with pytest.raises(NotImplementedError, match="batch-size 1"):
        g(torch.zeros((2, 5, 8)), 8, 3)
    for k, v in (("sampling", (0.6, 50, 0.9, 1)), ("constraint", object()), ("processors", (1.2, 0, ())), ("return_logprobs", True), ("return_hidden", True)):
        with pytest.raises(NotImplementedError, match=k):
            g(emb, 8, 3, **{k: v})
    for k in ("kv_cache_dtype", "weight_dtype"):
        with pytest.raises(NotImplementedError, match=k):
            g(emb, 8, 3, **{k: "fp8_e4m3"})
    eng._kv_mode = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        g(emb, 8, 3)
    eng._kv_mode, eng._w_mode = "bf16", "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="weight_dtype"):
        g(emb, 8, 3)
    eng._w_mode = "bf16"
    with pytest.raises(ValueError, match="prompt_ids"):
        g(emb, 8, 3, prompt_ids=[1, 2, 3])
    with pytest.raises(TypeError, match="banana"):
        g(emb, 8, 3, banana=1)
    # neutral processors are the call without them: the refusal is not reached, the device work is
    with pytest.raises(pytest.fail.Exception, match="device work"):
        g(emb, 8, 3, processors=(1.0, 0, ()))
    assert ops.LOOKUP_MAX_DRAFT == 15


def _stub():
    calls = []
    eng = types.SimpleNamespace(kv_cache_dtype="bf16", weight_dtype="bf16")

    def generate_lookup(embeds, max_new, k, n, **kw):
        calls.append((tuple(embeds.shape), max_new, k, n, kw))
        res = [torch.zeros((1, 3), dtype=torch.int64)]
        if kw["return_step_logits"]:
            res.append(torch.zeros((1, 3, 11)))
        if kw["return_first_logits"]:
            res.append(torch.zeros((1, 11)))
        res.append({"verify_steps": 1, "drafts_proposed": 2, "drafts_accepted": 2, "tokens_emitted": 2})
        return tuple(res)

    eng.generate_lookup = generate_lookup
    eng.generate = lambda *a, **k: pytest.fail("the plain route was taken")
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), model=types.SimpleNamespace(pad_token_id=None), device="cpu", _engine=eng,
                              _PROCESSOR_ARGS=U._PROCESSOR_ARGS, _BEAM_ARGS=U._BEAM_ARGS, _check_generate_kwargs=U._check_generate_kwargs)
    return m, calls


def test_generate_with_prompt_lookup_reaches_the_lookup_route():
    m, calls = _stub()
    emb = torch.zeros((1, 5, 8))
    out = U.generate(m, inputs_embeds=emb, prompt_lookup_num_tokens=3, max_new_tokens=6)
    assert out.shape == (1, 3)
    (shape, max_new, k, n, kw), = calls
    assert shape == (1, 5, 8) and max_new == 6 and k == 3 and n == 2                  # HF's default max_matching_ngram_size
    assert kw["prompt_ids"] is None and kw["eos_token_id"] == 2 and kw["pad_token_id"] == 2 and kw["return_stats"] is True
    assert m.last_lookup["stats"]["drafts_accepted"] == 2
    out = U.generate(m, inputs_embeds=emb, prompt_lookup_num_tokens=7, max_matching_ngram_size=3, min_new_tokens=2, eos_token_id=[9],
                     output_logits=True, return_dict_in_generate=True)
    kw = calls[-1][4]
    assert calls[-1][2:4] == (7, 3) and kw["min_new_tokens"] == 2 and kw["eos_token_id"] == 9 and kw["return_step_logits"] is True
    assert out.sequences.shape == (1, 3) and len(out.logits) == 3 and out.logits[0].shape == (1, 11)
    # the history comes from batch_input_ids: -1 at the rows of a spliced modality block
    m.prepare_multimodal_inputs = lambda **kw: {"inputs_embeds": torch.zeros((1, 4, 8)), "row_token_ids": torch.tensor([[5, -1, -1, 6]])}
    U.generate(m, batch_input_ids=[torch.tensor([5, 99, 6])], batch_labels=None, batch_X_modals=[{}], batch_task_names=["avqa"], prompt_lookup_num_tokens=2)
    assert calls[-1][4]["prompt_ids"].tolist() == [5, -1, -1, 6]


@pytest.mark.parametrize("kw, name", [
    (dict(do_sample=True), "do_sample"), (dict(num_beams=4), "num_beams"), (dict(guidance_scale=1.5), "guidance_scale"),
    (dict(allowed_sequences=[[3, 4]]), "allowed_sequences"), (dict(repetition_penalty=1.2), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(output_token_logprobs=True), "output_token_logprobs"),
    (dict(eos_token_id=[2, 3]), "eos_token_id"), (dict(kv_cache_dtype="fp8_e4m3"), "kv_cache_dtype"), (dict(weight_dtype="fp8_e4m3"), "weight_dtype"),
    (dict(assistant_model=object()), "assistant_model")])
def test_refused_with_prompt_lookup_by_name(kw, name):
    m, calls = _stub()
    with pytest.raises(NotImplementedError, match=name) as e:
        U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), prompt_lookup_num_tokens=3, **kw)
    assert name == "assistant_model" or "prompt_lookup_num_tokens" in str(e.value)       # both names
    assert not calls


def test_more_than_one_row_and_bad_values_are_refused():
    m, calls = _stub()
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens.*batch"):
        U.generate(m, inputs_embeds=torch.zeros((2, 5, 8)), prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens.*batch"):
        U.generate(m, batch_input_ids=[torch.tensor([1]), torch.tensor([2])], prompt_lookup_num_tokens=3)
    for k in (0, 16):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), prompt_lookup_num_tokens=k)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), prompt_lookup_num_tokens=3, max_matching_ngram_size=0)
    assert not calls


def test_the_other_entry_points_refuse_the_argument_by_name():
    assert U._LOOKUP_ARGS == frozenset(("prompt_lookup_num_tokens",))
    for implemented in (frozenset(), U._PROCESSOR_ARGS | U._WARPER_ARGS):       # what generate_batches / generate_questions / generate_avs* pass
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
            U._check_generate_kwargs(dict(prompt_lookup_num_tokens=3), implemented)
    U._check_generate_kwargs(dict(prompt_lookup_num_tokens=None))
    m = types.SimpleNamespace(_PROCESSOR_ARGS=U._PROCESSOR_ARGS, _check_generate_kwargs=U._check_generate_kwargs)
    for fn, args in ((U.generate_batches, ([],)), (U.generate_questions, ([],)), (U._avs_generate, ([], None))):
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
            if fn is U._avs_generate:
                fn(m, [], None, dict(prompt_lookup_num_tokens=3))
            else:
                fn(m, *args, prompt_lookup_num_tokens=3)


# ------------------------------------------------------------------ (c) the C entry points
def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_attn_verify", "crab_lookup_draft", "crab_lookup_accept"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.crab_abi_version() == 13


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(256), C.c_void_p)
    E_INVALID, E_UNSUPPORTED = -1, -3
    f = C.c_float(0.1)

    def verify(ctx_=h, q=one, ldq=1024, o=one, ldo=1024, B=1, Sq=4, H=2, Hk=2, d=128, Tmax=64, ctx_len=8, word=None):
        return lib.crab_attn_verify(ctx_, None, q, ldq, one, one, o, ldo, B, Sq, H, Hk, d, Tmax, ctx_len, word, f, None)

    assert verify(ctx_=None) == E_INVALID
    for H, Hk, d in ((2, 2, 32), (2, 2, 96), (2, 2, 256), (3, 2, 128), (6, 2, 128), (32, 2, 128), (2, 0, 128)):
        assert verify(H=H, Hk=Hk, d=d) == E_UNSUPPORTED
    assert verify(Sq=0) == E_UNSUPPORTED and verify(Sq=17) == E_UNSUPPORTED
    assert verify(q=None) == E_INVALID and verify(o=None) == E_INVALID and verify(B=0) == E_INVALID and verify(Tmax=0) == E_INVALID
    assert verify(ctx_len=-1) == E_INVALID and verify(ctx_len=62) == E_INVALID          # 62 + Sq - 1 > Tmax with a host position
    assert verify(ldq=1020) == E_INVALID and verify(ldq=128) == E_INVALID and verify(ldo=128) == E_INVALID

    def draft(ctx_=h, hist=one, S=4, step=one, cur=one, k=3, n=2, eos=-1, pad=0, max_new=8, V=16, ids=one, nd=one, fin=one):
        return lib.crab_lookup_draft(ctx_, None, hist, S, step, cur, k, n, eos, pad, max_new, V, ids, nd, fin)

    assert draft(ctx_=None) == E_INVALID
    for bad in (dict(hist=None), dict(step=None), dict(cur=None), dict(ids=None), dict(nd=None), dict(fin=None), dict(S=-1), dict(V=0), dict(max_new=0),
                dict(k=0), dict(k=16), dict(n=0), dict(pad=-1), dict(pad=16)):
        assert draft(**bad) == E_INVALID, bad

    def accept(ctx_=h, logits=one, ldl=16, V=16, k=3, ids=one, nd=one, cur=one, out=one, hist=one, S=4, pos=one, step=one, fin=one, max_new=8,
               stats=one):
        return lib.crab_lookup_accept(ctx_, None, logits, ldl, V, k, ids, nd, cur, out, hist, S, pos, step, fin, -1, 0, 0, max_new, stats, None)

    assert accept(ctx_=None) == E_INVALID
    for bad in (dict(logits=None), dict(ids=None), dict(nd=None), dict(cur=None), dict(out=None), dict(hist=None), dict(pos=None), dict(step=None),
                dict(fin=None), dict(stats=None), dict(S=-1), dict(V=0), dict(ldl=15), dict(max_new=0), dict(k=0), dict(k=16)):
        assert accept(**bad) == E_INVALID, bad
