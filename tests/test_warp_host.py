"""min_p / epsilon_cutoff / eta_cutoff without a device: crab_sample_select_warped (csrc/sample.hip) is declared, exported, bound and
refuses bad arguments before any HIP call; the argument plumbing of the model surface and the engine (off values are the plain sampling
call, greedy calls ignore the three, the refusals by name); the reference (tests/warp_ref.py) against hand-worked rows and against HF's own
masks; and the cap on the share of grid rows whose classes leave the kernel a choice - tests/test_warp_gpu.py means something only under it."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder, ops
from crab_amd.unified_llama import UnifiedForCausalLM as U
from tests import warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ------------------------------------------------------------------ (a) the C entry point
def test_symbol_is_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    assert re.search(r"^int\s+crab_sample_select_warped\s*\(", txt, flags=re.M)
    assert hasattr(lib, "crab_sample_select_warped") and "crab_sample_select_warped" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["crab_sample_select_warped"][1]) == len(_lib.SYMBOLS["crab_sample_select"][1]) + 5
    assert _lib.SYMBOLS["crab_sample_select_warped"][1][:18] == _lib.SYMBOLS["crab_sample_select"][1]
    assert lib.crab_abi_version() == 13
    assert callable(ops.sample_select_warped)
    assert "sample_select_warped_kernel" in open(os.path.join(ROOT, "crab_amd", "csrc", "sample.hip")).read()       # its kernel has a source


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)

    def call(ctx_=h, logits=one, B=1, V=8, cur=one, out=one, step=one, fin=one, t=0.7, k=0, p=0.9, min_p=0.1, eps=0.0, eta=0.0, kn=None, km=None):
        return lib.crab_sample_select_warped(ctx_, None, logits, 8, B, V, cur, out, 4, step, fin, -1, 0, 0, C.c_float(t), k, C.c_float(p), 1,
                                             C.c_float(min_p), C.c_float(eps), C.c_float(eta), kn, km)

    assert call(ctx_=None) == -1
    for name in ("logits", "cur", "out", "step", "fin"):
        assert call(**{name: None}) == -1, name
    assert b"sample_select_warped" in ctx.raw
    for kw in (dict(B=0), dict(V=0), dict(t=0.0), dict(t=NAN), dict(p=0.0), dict(p=1.5), dict(k=-1)):
        assert call(**kw) == -1, kw
    for name, bad in (("min_p", (-0.1, 1.0001, NAN, math.inf)), ("eps", (-1e-3, 1.0, 2.0, NAN)), ("eta", (-1e-3, 1.0, 2.0, NAN))):
        for v in bad:
            ctx.raw = bytes(len(ctx.raw))
            assert call(**{name: v}) == -1, (name, v)
            assert {"min_p": b"min_p", "eps": b"epsilon_cutoff", "eta": b"eta_cutoff"}[name] in ctx.raw, (name, v)      # the message names the argument


def test_ops_wrapper_checks_its_tensors_before_the_library():
    with pytest.raises(_lib.CrabHipError):
        ops.sample_select_warped(torch.zeros((1, 8)), torch.zeros(1, dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int64),
                                 torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), -1, 0, 0, 0.7, 0, 0.9, 1, min_p=0.1)


# ------------------------------------------------------------------ (b) the kwarg routing
def test_the_three_are_refused_bare_and_pass_with_warper_args():
    assert U._WARPER_ARGS == frozenset(("min_p", "epsilon_cutoff", "eta_cutoff"))
    for name in U._WARPER_ARGS:
        assert name in U._UNSUPPORTED
        with pytest.raises(NotImplementedError, match=name):
            U._check_generate_kwargs({name: 0.1})
        with pytest.raises(NotImplementedError, match=name):
            U._check_generate_kwargs({name: 0.1}, U._PROCESSOR_ARGS | U._BEAM_ARGS | U._GUIDANCE_ARGS)
        U._check_generate_kwargs({name: 0.1}, U._WARPER_ARGS)
    with pytest.raises(NotImplementedError, match="typical_p"):
        U._check_generate_kwargs(dict(typical_p=0.5), U._WARPER_ARGS)


def _stub():
    """A stand-in for the model with a recording engine: (model, plain calls, guided calls, generate_many calls)."""
    plain, guided, many = [], [], []
    eng = types.SimpleNamespace(kv_cache_dtype="bf16", weight_dtype="bf16")
    eng.generate = lambda embeds, max_new, **kw: plain.append((max_new, kw)) or torch.zeros((embeds.shape[0], 3), dtype=torch.int64)
    eng.generate_guided = lambda embeds, neg, scale, max_new, **kw: guided.append((scale, max_new, kw)) or torch.zeros((embeds.shape[0], 3), dtype=torch.int64)
    eng.generate_many = lambda embeds, max_new, **kw: many.append((max_new, kw)) or [torch.zeros((e.shape[0], 3), dtype=torch.int64) for e in embeds]
    eng.generate_beam = lambda *a, **k: pytest.fail("beam mode was reached")
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), model=types.SimpleNamespace(pad_token_id=None), device="cpu", _engine=eng,
                              _PROCESSOR_ARGS=U._PROCESSOR_ARGS, _BEAM_ARGS=U._BEAM_ARGS, _check_generate_kwargs=U._check_generate_kwargs,
                              _sampling=U._sampling, lm_head=types.SimpleNamespace(weight=torch.zeros((64, 8))))
    m._processors = lambda kw: U._processors(m, kw)
    m._constraint = lambda kw, eos=None: U._constraint(m, kw, eos)
    m._generate_beam = lambda *a: U._generate_beam(m, *a)
    m.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    return m, plain, guided, many


EMB = torch.zeros((2, 5, 8))
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=11)


def test_off_values_are_the_plain_sampling_call():
    m, plain, guided, _ = _stub()
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, **SAMPLE)
    base = plain[-1]
    assert base[1]["sampling"] == (0.7, 5, 0.8, 11)
    for off in (dict(min_p=None), dict(min_p=0), dict(min_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0), dict(epsilon_cutoff=None, eta_cutoff=None)):
        U.generate(m, inputs_embeds=EMB, max_new_tokens=4, **SAMPLE, **off)
        assert plain[-1][0] == base[0] and set(plain[-1][1]) == set(base[1]), off
        assert all(plain[-1][1][k] is base[1][k] or plain[-1][1][k] == base[1][k] for k in base[1]), off
    assert not guided


def test_live_values_ride_in_the_sampling_tuple_and_nowhere_else():
    m, plain, guided, many = _stub()
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, **SAMPLE)
    base = set(plain[-1][1])
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, min_p=0.05, eta_cutoff=2e-3, **SAMPLE)
    assert set(plain[-1][1]) == base and plain[-1][1]["sampling"] == (0.7, 5, 0.8, 11, 0.05, 0.0, 2e-3)
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, epsilon_cutoff=3e-4, **SAMPLE)
    assert plain[-1][1]["sampling"] == (0.7, 5, 0.8, 11, 0.0, 3e-4, 0.0)
    # the guided route and generate_batches pass them on in the same place
    U.generate(m, inputs_embeds=EMB, negative_inputs_embeds=EMB[:, :2], guidance_scale=1.5, min_p=0.1, **SAMPLE)
    assert guided[-1][2]["sampling"] == (0.7, 5, 0.8, 11, 0.1, 0.0, 0.0) and not any("min_p" in k for k in guided[-1][2])
    m.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    U.generate_batches(m, [dict(batch_input_ids=EMB, batch_X_modals=None)], min_p=1.0, **SAMPLE)
    assert many[-1][1]["sampling"] == (0.7, 5, 0.8, 11, 1.0, 0.0, 0.0)


def test_without_do_sample_the_call_is_the_plain_greedy_call():
    m, plain, _, _ = _stub()
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4)
    base = plain[-1]
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, min_p=0.3, epsilon_cutoff=0.01, eta_cutoff=0.02)
    assert plain[-1][0] == base[0] and set(plain[-1][1]) == set(base[1]) and plain[-1][1]["sampling"] is None
    U.generate(m, inputs_embeds=EMB, max_new_tokens=4, min_p=0.3, allowed_sequences=[[3, 4]])      # greedy closed-set call: nothing to refuse
    assert plain[-1][1]["sampling"] is None and plain[-1][1]["constraint"] is not None


@pytest.mark.parametrize("name, bad", [("min_p", -0.1), ("min_p", 1.5), ("min_p", NAN), ("epsilon_cutoff", 1.0), ("epsilon_cutoff", -1e-3),
                                       ("epsilon_cutoff", NAN), ("eta_cutoff", 1.0), ("eta_cutoff", 7), ("eta_cutoff", NAN)])
def test_values_out_of_range_raise_by_name(name, bad):
    m, plain, guided, _ = _stub()
    with pytest.raises(ValueError, match=name):
        U.generate(m, inputs_embeds=EMB, **SAMPLE, **{name: bad})
    with pytest.raises(ValueError, match=name):
        U.generate(m, inputs_embeds=EMB, negative_inputs_embeds=EMB[:, :2], guidance_scale=1.5, **SAMPLE, **{name: bad})
    assert not plain and not guided
    idx = 4 + R.STAGES.index(name)
    with pytest.raises(ValueError, match=name):
        decoder.normalize_sampling(tuple(bad if i == idx else v for i, v in enumerate((0.7, 5, 0.8, 11, 0.0, 0.0, 0.0))))


@pytest.mark.parametrize("kw", [dict(min_p=0.1), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)])
def test_closed_set_with_a_live_warper_is_refused_by_name(kw):
    m, plain, _, _ = _stub()
    name, = kw
    with pytest.raises(NotImplementedError, match=r"allowed_sequences[\s\S]*" + name):
        U.generate(m, inputs_embeds=EMB, allowed_sequences=[[3, 4]], **SAMPLE, **kw)
    assert not plain
    # the engine refuses the same pairing on its own, before any device work
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    eng.lm_head = types.SimpleNamespace(weight=torch.zeros((64, 8)))
    eng._constraints = eng._call = lambda *a, **k: pytest.fail("device work was reached")
    smp = (0.7, 5, 0.8, 11, kw.get("min_p", 0.0), kw.get("epsilon_cutoff", 0.0), kw.get("eta_cutoff", 0.0))
    with pytest.raises(NotImplementedError, match=r"constraint[\s\S]*" + name):
        eng.generate(EMB, 4, sampling=smp, constraint=object())
    with pytest.raises(NotImplementedError, match=name):
        eng.generate_many([EMB], 4, sampling=smp, constraint=object())


def test_beam_mode_still_refuses_do_sample_first():
    m, plain, _, _ = _stub()
    with pytest.raises(NotImplementedError, match="do_sample"):
        U.generate(m, inputs_embeds=EMB, num_beams=3, min_p=0.1, **SAMPLE)
    assert not plain


def test_engine_tuples_normalise_and_reseed():
    N = decoder.normalize_sampling
    assert N(None) is None and N((0.7, 5, 0.8, 11)) == (0.7, 5, 0.8, 11)
    assert N((0.7, 5, 0.8, 11, 0, None, 0.0)) == (0.7, 5, 0.8, 11)             # all off: the 4-tuple, so the plain call's state key
    assert N((0.7, 5, 0.8, 11, 0.1, None, 0)) == (0.7, 5, 0.8, 11, 0.1, 0.0, 0.0)
    assert N((0.7, 5, 0.8, 11, 0, 0, 0), constrained=True) == (0.7, 5, 0.8, 11)
    with pytest.raises(ValueError):
        N((0.7, 5, 0.8, 11, 0.1))
    assert decoder.reseed_sampling(None, 5) is None
    assert decoder.reseed_sampling((0.7, 5, 0.8, 11), 5) == (0.7, 5, 0.8, 16)
    assert decoder.reseed_sampling((0.7, 5, 0.8, 11, 0.1, 0.0, 2e-3), 5) == (0.7, 5, 0.8, 16, 0.1, 0.0, 2e-3)


# ------------------------------------------------------------------ (c) the reference against hand-worked rows
ALL = lambda V: torch.ones(V, dtype=torch.bool)
BARE = (1.0, 0, 1.0)


def test_min_p_one_keeps_the_maximum_and_its_ties_only():
    row = torch.tensor([0.5, 3.0, 2.999, 3.0, -1.0, 3.0])
    cls, _ = R.warp_classes(row, ALL(6), BARE, min_p=1.0)
    assert cls.tolist() == [R.DROP, R.KEEP, R.DROP, R.KEEP, R.DROP, R.KEEP]


def test_an_epsilon_above_every_probability_keeps_the_maximum_only():
    row = torch.tensor([1.0, 1.2, 0.9, 1.1, 1.05])               # five close tokens: every p_i < 0.3
    assert float(torch.softmax(row.double(), 0).max()) < 0.3
    cls, _ = R.warp_classes(row, ALL(5), BARE, epsilon_cutoff=0.3)
    assert cls.tolist() == [R.DROP, R.KEEP, R.DROP, R.DROP, R.DROP]
    cls, _ = R.warp_classes(torch.tensor([1.0, 1.2, 0.9, 1.2, 1.05]), ALL(5), BARE, epsilon_cutoff=0.3)
    assert cls.tolist() == [R.DROP, R.KEEP, R.DROP, R.KEEP, R.DROP]          # ... and its exact ties


def test_eta_of_a_uniform_row_by_hand():
    # n equal tokens: p_i = 1 / n, H = ln n, eta = min(eps, sqrt(eps) / n).  With n = 10, eps = 0.64: eta = min(0.64, 0.08) = 0.08 < 0.1 - all stay;
    # eps = 0.9025: eta = min(0.9025, 0.095) < 0.1 - all stay; and were eta above 1 / n they would stay too: all are ties of the maximum.
    for eps in (0.64, 0.9025, 0.99):
        cls, _ = R.warp_classes(torch.zeros(10), ALL(10), BARE, eta_cutoff=eps)
        assert cls.tolist() == [R.KEEP] * 10, eps
    # the uniform row with one token at ln(1 / 2) below: 7 tokens at 2 / 15, one at 1 / 15;
    # H = -(7 * (2 / 15) ln(2 / 15) + (1 / 15) ln(1 / 15)) = 2.0609, exp(-H) = 0.12731
    #   eps = 0.01: eta = min(0.01, 0.1 * 0.12731) = 0.01     < 1 / 15: kept      eps = 0.05: eta = min(0.05, 0.02847) = 0.02847 < 1 / 15: kept
    #   eps = 0.3 : eta = min(0.3, 0.5477 * 0.12731) = 0.06975 > 1 / 15 = 0.06667: removed      eps = 0.9: eta = 0.1208: removed
    row = torch.zeros(8)
    row[0] = math.log(0.5)
    for eps, kept in ((0.01, True), (0.05, True), (0.3, False), (0.9, False)):
        cls, _ = R.warp_classes(row, ALL(8), BARE, eta_cutoff=eps)
        assert cls[1:].tolist() == [R.KEEP] * 7 and int(cls[0]) == (R.KEEP if kept else R.DROP), eps
    H = -(7 * (2 / 15) * math.log(2 / 15) + (1 / 15) * math.log(1 / 15))
    assert abs(math.exp(-H) - 0.12731) < 1e-5


def test_minus_inf_entries_have_no_mass_and_are_never_kept():
    row = torch.tensor([2.0, float("-inf"), 1.0, float("-inf"), -3.0, 0.5])
    for kw in (dict(min_p=0.005), dict(epsilon_cutoff=1e-4), dict(eta_cutoff=1e-4), dict(min_p=0.005, epsilon_cutoff=1e-4, eta_cutoff=1e-4)):
        cls, _ = R.warp_classes(row, ALL(6), BARE, **kw)
        assert cls.tolist() == [R.KEEP, R.DROP, R.KEEP, R.DROP, R.KEEP, R.KEEP], kw
    allowed = ALL(6)
    allowed[0] = False                                            # EOS under min_new_tokens: out, whatever its logit
    cls, _ = R.warp_classes(row, allowed, BARE, min_p=0.5)
    assert cls.tolist() == [R.DROP, R.DROP, R.KEEP, R.DROP, R.DROP, R.KEEP]
    cls, _ = R.warp_classes(torch.full((4,), float("-inf")), ALL(4), BARE, min_p=0.5)
    assert cls.tolist() == [R.EITHER] * 4                         # no finite token: whatever crab_sample_select does today


def test_with_margin_zero_the_classes_are_hf_s_mask_exactly():
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    g = torch.Generator().manual_seed(3)
    for V, (t, k, p), (mp, ec, et) in ((50, (0.8, 0, 1.0), (0.1, 0.0, 0.0)), (300, (0.7, 20, 0.9), (0.05, 0.01, 0.02)), (300, (1.3, 0, 0.95), (0.0, 2e-3, 0.0)),
                                       (2000, (0.6, 50, 0.9), (0.0, 0.0, 0.05)), (2000, (1.0, 0, 1.0), (0.02, 2e-4, 1e-3))):
        row = torch.randn(V, generator=g) * 3
        cls, _ = R.warp_classes(row, ALL(V), (t, k, p), mp, ec, et, exact=True)
        s = TemperatureLogitsWarper(t)(None, row.double()[None])
        if k:
            s = TopKLogitsWarper(k)(None, s)
        if p < 1:
            s = TopPLogitsWarper(R.f32(p))(None, s)
        if mp:
            s = MinPLogitsWarper(R.f32(mp))(None, s)
        if ec:
            s = EpsilonLogitsWarper(R.f32(ec))(None, s)
        if et:
            w = EtaLogitsWarper(0.5)
            w.epsilon = torch.tensor(R.f32(et), dtype=torch.float64)
            s = w(None, s)
        assert not bool((cls == R.EITHER).any())
        assert torch.equal(cls == R.KEEP, torch.isfinite(s[0])), (V, t, k, p, mp, ec, et)


# ------------------------------------------------------------------ (d) the cap
def test_at_most_one_grid_row_in_ten_leaves_the_kernel_a_choice():
    """Over the exact shapes, seeds and parameters of tests/test_warp_gpu.py: the rows with any EITHER token at the end of the chain (a
    superset of those a NEW stage made loose).  A loose row is held to less, so their share is capped; every other row pins the kept set."""
    rows = loose = 0
    per_stage = {}
    for V in R.GRID_V:
        for B in R.GRID_B:
            for front in R.GRID_FRONTS:
                for st in R.GRID_STAGE_NAMES:
                    ref = R.grid_reference(B, V, front, st)
                    n = sum(bool((c == R.EITHER).any()) for c, _ in ref)
                    rows, loose = rows + B, loose + n
                    a = per_stage.setdefault((front, st), [0, 0, 0])
                    a[0], a[1] = a[0] + B, a[1] + n
                    a[2] += sum(int((c == R.KEEP).sum()) < int(torch.isfinite(R.grid_rows(B, V)[b]).sum()) - (b == 0) for b, (c, _) in enumerate(ref))
    print(f"grid rows {rows}, loose {loose}; per (front, stages): {per_stage}")
    assert rows == sum(R.GRID_B) * len(R.GRID_V) * 8 and loose <= R.CAP * rows
    for key, (n, l, cut) in per_stage.items():
        assert l <= R.CAP * n, key
        assert cut >= 0.9 * n, (key, "the stage removes nothing on most rows: the grid would not exercise it")
