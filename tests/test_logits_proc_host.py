"""Host side of the logits processors of the decode step (csrc/logits_proc.hip): the CPU restatement the kernels are held to
(tests/logits_proc_ref.py) against transformers' own processors, the ABI, and the argument logic of the engine and the model - no GPU."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder
from crab_amd.unified_llama import UnifiedForCausalLM as U
from tests import logits_proc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(B, V, seed):
    """Random fp32 rows with positive, negative, exactly zero and -inf entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 4
    x[:, ::7] = 0.0
    x[:, 3::11] = -float("inf")
    return x


def _hf():
    try:
        from transformers.generation import logits_process as LP
    except Exception as e:                                       # pragma: no cover
        pytest.skip(f"transformers is not importable here: {e}")
    return LP


@pytest.mark.parametrize("p", [1.3, 0.7, 1.0])
def test_penalty_restatement_equals_hf(p):
    LP = _hf()
    B, V, step = 4, 97, 12
    g = torch.Generator().manual_seed(1)
    raw = _rows(B, V, 2)
    hist = torch.randint(0, 9, (B, step), generator=g)           # few distinct ids: many duplicates, columns 0 / 3 / 7 (zero, -inf) among them
    hist[0, 5] = V - 1
    for s in (0, 1, 5, step):
        want = LP.RepetitionPenaltyLogitsProcessor(penalty=p)(hist[:, :s], raw.clone()) if s else raw
        got = R.edit(raw, hist, s, torch.zeros(B, dtype=torch.int32), R.Params(repetition_penalty=p))
        assert torch.equal(got, want), (p, s)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ngram_restatement_equals_hf(n):
    LP = _hf()
    B, V, step = 4, 53, 15
    g = torch.Generator().manual_seed(3)
    raw = _rows(B, V, 4)
    hist = torch.randint(0, 4, (B, step), generator=g)           # an alphabet of 4: repeated n-grams everywhere
    hist[1] = torch.tensor([5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5])      # an n-gram that overlaps itself
    hist[2, -1] = V - 1
    for s in (0, 1, n - 1, n, n + 1, step):
        if s < 0:
            continue
        want = LP.NoRepeatNGramLogitsProcessor(n)(hist[:, :s], raw.clone())
        got = R.edit(raw, hist, s, torch.zeros(B, dtype=torch.int32), R.Params(no_repeat_ngram_size=n))
        assert torch.equal(got, want), (n, s)


def test_min_new_tokens_with_a_list_of_ids_equals_hf():
    LP = _hf()
    B, V = 3, 41
    raw = _rows(B, V, 5)
    stops = [7, 40, 0]
    hist = torch.randint(0, V, (B, 6), generator=torch.Generator().manual_seed(6))
    for s in (0, 2, 3, 5):
        want = LP.MinNewTokensLengthLogitsProcessor(0, 3, stops)(hist[:, :s], raw.clone())
        got = R.edit(raw, hist, s, torch.zeros(B, dtype=torch.int32), R.Params(stop_ids=stops, min_new_tokens=3))
        assert torch.equal(got, want), s
        assert (s >= 3) == torch.equal(got, raw)


def test_all_three_in_hf_order_and_what_lies_beyond_hf():
    LP = _hf()
    B, V, step = 3, 61, 9
    raw = _rows(B, V, 7)
    hist = torch.randint(0, 5, (B, step), generator=torch.Generator().manual_seed(8))
    prm = R.Params(1.25, 2, (4, 60), 20)
    x = raw.clone()
    for proc in (LP.RepetitionPenaltyLogitsProcessor(penalty=1.25), LP.NoRepeatNGramLogitsProcessor(2), LP.MinNewTokensLengthLogitsProcessor(0, 20, [4, 60])):
        x = proc(hist, x)                                        # the order of GenerationMixin._get_logits_processor
    fin = torch.tensor([0, 1, 0], dtype=torch.int32)
    got = R.edit(raw, hist, step, fin, prm)
    assert torch.equal(got[0], x[0]) and torch.equal(got[2], x[2])
    assert torch.equal(got[1], raw[1]), "a finished row is not edited"
    # ids outside [0, V): never edited, equal to nothing
    bad = hist.clone()
    bad[0, 2], bad[0, 6] = V + 5, -3
    got = R.edit(raw, bad, step, torch.zeros(B, dtype=torch.int32), R.Params(1.25, 2))
    keep = [t for j, t in enumerate(bad[0].tolist()) if 0 <= t < V]
    assert set(torch.nonzero(got[0] != raw[0]).flatten().tolist()) <= set(keep)
    assert R.banned_ngram_tokens([V + 5, 1, V + 5], 2, V) == [] and R.banned_ngram_tokens([2, 1, 2], 2, V) == [1]
    assert R.finished_after(torch.tensor([0, 0, 1]), torch.tensor([60, 5, 5]), prm).tolist() == [1, 0, 1]


def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_logits_edit", "crab_logits_restore"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    _i, _i64, _vp, _f = C.c_int, C.c_int64, C.c_void_p, C.c_float
    assert _lib.SYMBOLS["crab_logits_edit"] == (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _i64, _i, _vp, _vp, _f, _i, _vp, _i, _i, _vp, _vp, _i64])
    assert _lib.SYMBOLS["crab_logits_restore"] == (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i64, _i])
    assert lib.crab_abi_version() == 13


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)

    def edit(logits=one, ldl=8, B=1, V=8, out_ids=one, ld_out=4, n_steps=4, step=one, fin=one, p=1.2, n=0, stops=None, n_stop=0, si=one, sv=one, ld_save=8):
        return lib.crab_logits_edit(h, None, logits, ldl, B, V, out_ids, ld_out, n_steps, step, fin, p, n, stops, n_stop, 0, si, sv, ld_save)

    def restore(logits=one, ldl=8, B=1, V=8, cur=one, fin=one, stops=None, n_stop=0, si=one, sv=one, ld_save=8, n_slots=8):
        return lib.crab_logits_restore(h, None, logits, ldl, B, V, cur, fin, stops, n_stop, si, sv, ld_save, n_slots)

    assert lib.crab_logits_edit(None, None, one, 8, 1, 8, one, 4, 4, one, one, 1.2, 0, None, 0, 0, one, one, 8) == -1
    assert lib.crab_logits_restore(None, None, one, 8, 1, 8, one, one, None, 0, one, one, 8, 8) == -1
    for k in ("logits", "out_ids", "step", "fin", "si", "sv"):
        assert edit(**{k: None}) == -1, k
    assert b"logits_edit" in ctx.raw
    for kw in (dict(B=0), dict(V=0), dict(n_steps=0), dict(p=0.0), dict(p=-1.0), dict(n=-1), dict(n_stop=-1, stops=one), dict(n_stop=9, stops=one),
               dict(n_stop=1), dict(ld_save=7), dict(n_stop=1, stops=one, ld_save=8), dict(ldl=7), dict(ld_out=3)):
        assert edit(**kw) == -1, kw
    assert edit(n_steps=8193, ld_out=8193, ld_save=2 * 8193) == -3, "CRAB_E_UNSUPPORTED past the 8192 history words of the LDS"
    ctx.raw = bytes(len(ctx.raw))
    for k in ("logits", "cur", "fin", "si", "sv"):
        assert restore(**{k: None}) == -1, k
    assert b"logits_restore" in ctx.raw
    for kw in (dict(B=0), dict(V=0), dict(n_stop=-1, stops=one), dict(n_stop=9, stops=one), dict(n_stop=1), dict(n_slots=0), dict(n_slots=9), dict(ldl=7)):
        assert restore(**kw) == -1, kw


def test_check_generate_kwargs_refuses_bare_and_accepts_what_an_entry_point_implements():
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3)):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            U._check_generate_kwargs(kw)
        U._check_generate_kwargs(kw, U._PROCESSOR_ARGS)
        U._check_generate_kwargs(kw, implemented=frozenset(kw))
    with pytest.raises(NotImplementedError, match="num_beams"):
        U._check_generate_kwargs(dict(num_beams=4, repetition_penalty=1.2), U._PROCESSOR_ARGS)
    assert U._UNSUPPORTED["repetition_penalty"] == 1.0 and U._UNSUPPORTED["no_repeat_ngram_size"] == 0


def test_neutral_values_normalise_to_none():
    N = decoder.normalize_processors
    for neutral in (None, (1.0, 0, ()), (1, 0, None), (None, None, []), (1.0, 0, [])):
        assert N(neutral) is None
    assert N((1.2, 0, ())) == (1.2, 0, ()) and N((1.0, 3, None)) == (1.0, 3, ()) and N((1.0, 0, [5, 5, 9, 5])) == (1.0, 0, (5, 9))
    for bad in ((0.0, 0, ()), (-1.0, 0, ()), (1.0, -1, ()), (1.0, 0, [-4])):
        with pytest.raises(ValueError):
            N(bad)
    with pytest.raises(NotImplementedError, match="stop ids"):
        N((1.0, 0, list(range(9))))


def test_refused_combinations_raise_by_name_before_any_device_work():
    chk = decoder.check_processors
    with pytest.raises(NotImplementedError, match="return_logprobs with no_repeat_ngram_size"):
        chk((1.0, 2, ()), 0, False, True)
    with pytest.raises(NotImplementedError, match="return_logprobs with stop_token_ids"):
        chk((1.0, 0, (7,)), 1, False, True)
    with pytest.raises(NotImplementedError, match="constraint with stop_token_ids"):
        chk((1.0, 0, (7,)), 0, True, False)
    with pytest.raises(NotImplementedError, match="constraint with no_repeat_ngram_size"):
        chk((1.0, 2, ()), 0, True, False)
    # the penalty alone combines with everything; stop ids with logprobs while nothing is suppressed
    assert chk((1.3, 0, ()), 4, True, True) == (1.3, 0, ())
    assert chk((1.3, 0, (7,)), 0, False, True) == (1.3, 0, (7,))
    assert chk((1.0, 0, ()), 4, True, True) is None
    # a stop id that repeats eos_token_id is the select's own: the triple is neutral BEFORE the refusals are tried
    assert chk((1.0, 0, [7]), 2, True, True, 7) is None and chk((1.0, 0, [7, 7]), 2, False, True, [7]) is None
    assert chk((1.0, 0, [7, 9]), 0, False, True, 7) == (1.0, 0, (9,))
    with pytest.raises(NotImplementedError, match="return_logprobs with stop_token_ids"):
        chk((1.0, 0, [7, 9]), 2, False, True, 7)
    # the engine's entry points refuse before they look at a tensor: the object below has no weights and no device
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    for call in (lambda **k: eng.generate(None, 4, **k), lambda **k: eng.generate_many(None, 4, **k), lambda **k: eng.generate_shared_prefix(None, None, 4, **k)):
        with pytest.raises(NotImplementedError, match="return_logprobs with no_repeat_ngram_size"):
            call(processors=(1.0, 2, ()), return_logprobs=True)
        with pytest.raises(NotImplementedError, match="constraint with stop_token_ids"):
            call(processors=(1.0, 0, (3,)), constraint=object())


def test_model_arguments_become_one_eos_and_a_triple():
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2))
    f = lambda **kw: U._processors(m, kw)
    assert f() == (2, None) and f(eos_token_id=None) == (None, None)
    assert f(eos_token_id=[5]) == (5, None) and f(eos_token_id=[5, 5]) == (5, None)
    assert f(eos_token_id=[5, 9, 5, 7]) == (5, (1.0, 0, (9, 7)))
    assert f(eos_token_id=torch.tensor([5, 9])) == (5, (1.0, 0, (9,)))
    assert f(repetition_penalty=1.0, no_repeat_ngram_size=0) == (2, None)
    assert f(repetition_penalty=1.1, no_repeat_ngram_size=3, eos_token_id=[4, 6]) == (4, (1.1, 3, (6,)))
    # at the model surface the refusals speak the caller's names
    with pytest.raises(NotImplementedError, match="output_token_logprobs with no_repeat_ngram_size"):
        f(no_repeat_ngram_size=2, output_token_logprobs=True)
    with pytest.raises(NotImplementedError, match="allowed_sequences with eos_token_id"):
        f(eos_token_id=[4, 6], allowed_sequences=[[1, 2]])
    with pytest.raises(NotImplementedError, match="allowed_sequences with no_repeat_ngram_size"):
        f(no_repeat_ngram_size=2, allowed_sequences=[[1, 2]])
    with pytest.raises(NotImplementedError, match="output_token_logprobs with eos_token_id"):
        f(eos_token_id=[4, 6], min_new_tokens=2, output_token_logprobs=True)


def test_trim_and_token_count_stop_at_any_id():
    from crab_amd.unified_llama import _fill_logprob_fields, _stop_ids
    ids = torch.tensor([[4, 8, 9, 9], [5, 6, 9, 2], [7, 7, 7, 8]])
    assert decoder._trim_at_eos(ids, 4, (9, 8)).shape[1] == 4
    assert decoder._trim_at_eos(ids[:2], 4, (9, 8)).shape[1] == 3 and decoder._trim_at_eos(ids[:2], 4, 9).shape[1] == 3
    assert decoder._trim_at_eos(ids, 4, (-1,)).shape[1] == 4 and decoder._trim_at_eos(ids, 3, (9, 8, 7)).shape[1] == 3
    assert decoder._trim_at_eos(ids, 4, (9, 8, 7)).shape[1] == 3
    out = types.SimpleNamespace()
    _fill_logprob_fields(out, ids, torch.zeros(3, 4, 2), _stop_ids(9, (1.0, 0, (8,))))
    assert out.num_tokens.tolist() == [2, 3, 4]
    assert _stop_ids(None, None) == [] and _stop_ids(3, None) == [3]
