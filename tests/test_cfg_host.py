"""Classifier-free guidance without a device: the two C entry points (csrc/cfg.hip) are declared, exported, bound and refuse bad arguments; the
argument plumbing of the model surface (guidance_scale routed by generate() alone, off values a plain call, the refusals by name) and the
refusals of GenerationEngine.generate_guided before any device work; the fp64 reference (tests/cfg_ref.py) against torch's log_softmax form."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder, ops
from crab_amd.unified_llama import UnifiedForCausalLM as U
from tests import cfg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ (a) the C entry points
def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_cfg_mix", "crab_cfg_follow"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.crab_abi_version() == 13
    assert callable(ops.cfg_mix) and callable(ops.cfg_follow)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)
    odd = C.c_void_p(one.value + 2)

    def mix(ctx_=h, logits=one, ldl=8, B=1, V=8, scale=1.5, fin=one, guided=one, ldg=8):
        return lib.crab_cfg_mix(ctx_, None, logits, ldl, B, V, C.c_float(scale), fin, guided, ldg)

    def follow(ctx_=h, cur=one, out=one, ld_out=4, n_steps=4, fin=one, step=one, B=1):
        return lib.crab_cfg_follow(ctx_, None, cur, out, ld_out, n_steps, fin, step, B)

    assert mix(ctx_=None) == -1 and follow(ctx_=None) == -1
    for k in ("logits", "fin", "guided"):
        assert mix(**{k: None}) == -1, k
    assert b"cfg_mix" in ctx.raw
    for kw in (dict(B=0), dict(B=-2), dict(V=0), dict(ldl=7), dict(ldg=7), dict(ldl=-1), dict(logits=odd), dict(guided=odd), dict(scale=float("nan"))):
        assert mix(**kw) == -1, kw
    ctx.raw = bytes(len(ctx.raw))
    for k in ("cur", "out", "fin", "step"):
        assert follow(**{k: None}) == -1, k
    assert b"cfg_follow" in ctx.raw
    for kw in (dict(B=0), dict(n_steps=0), dict(ld_out=3)):
        assert follow(**kw) == -1, kw


# ------------------------------------------------------------------ (b) the kwarg routing
def test_guidance_scale_is_routed_by_generate_alone():
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        U._check_generate_kwargs(dict(guidance_scale=1.5))
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        U._check_generate_kwargs(dict(guidance_scale=1.5), U._PROCESSOR_ARGS)          # what generate_batches / generate_questions / generate_avs* pass
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        U._check_generate_kwargs(dict(guidance_scale=1.5), U._PROCESSOR_ARGS | U._BEAM_ARGS)
    U._check_generate_kwargs(dict(guidance_scale=1.5), U._GUIDANCE_ARGS)
    assert U._GUIDANCE_ARGS == frozenset(("guidance_scale",))
    assert "guidance_scale" in U._UNSUPPORTED and U._UNSUPPORTED["guidance_scale"] is None


def _stub():
    """A stand-in for the model with a recording engine: (model, plain calls, guided calls)."""
    plain, guided = [], []
    eng = types.SimpleNamespace(kv_cache_dtype="bf16", weight_dtype="bf16")
    eng.generate = lambda embeds, max_new, **kw: plain.append((tuple(embeds.shape), max_new, kw)) or torch.zeros((embeds.shape[0], 3), dtype=torch.int64)

    def generate_guided(embeds, neg, scale, max_new, **kw):
        guided.append((tuple(embeds.shape), tuple(neg.shape), scale, max_new, kw))
        ids = torch.zeros((embeds.shape[0], 3), dtype=torch.int64)
        return (ids, torch.arange(2 * embeds.shape[0] * 3 * 5, dtype=torch.float32).view(2 * embeds.shape[0], 3, 5)) if kw["return_step_logits"] else ids

    eng.generate_guided = generate_guided
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), model=types.SimpleNamespace(pad_token_id=None), device="cpu", _engine=eng,
                              _PROCESSOR_ARGS=U._PROCESSOR_ARGS, _BEAM_ARGS=U._BEAM_ARGS, _check_generate_kwargs=U._check_generate_kwargs,
                              _sampling=U._sampling, lm_head=types.SimpleNamespace(weight=torch.zeros((64, 8))))
    m._processors = lambda kw: U._processors(m, kw)
    m._constraint = lambda kw, eos=None: U._constraint(m, kw, eos)
    m.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    return m, plain, guided


def test_off_values_are_the_plain_call_with_no_new_keyword():
    m, plain, guided = _stub()
    emb = torch.zeros((2, 5, 8))
    U.generate(m, inputs_embeds=emb, max_new_tokens=4)
    base = set(plain[-1][2])
    for off in (None, 1, 1.0):
        out = U.generate(m, inputs_embeds=emb, max_new_tokens=4, guidance_scale=off, negative_inputs_embeds=torch.zeros((2, 3, 8)))
        assert out.shape == (2, 3) and set(plain[-1][2]) == base, (off, sorted(set(plain[-1][2]) ^ base))
    assert len(plain) == 4 and not guided
    assert not any("guid" in k or "negative" in k for k in base)


def test_guided_call_reaches_the_engine():
    m, plain, guided = _stub()
    emb, neg = torch.zeros((2, 5, 8)), torch.zeros((2, 3, 8))
    out = U.generate(m, inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=1.5, max_new_tokens=6, min_new_tokens=2, eos_token_id=[9],
                     kv_cache_dtype="fp8_e4m3", max_rows=4)
    assert out.shape == (2, 3) and not plain
    (se, sn, scale, max_new, kw), = guided
    assert se == (2, 5, 8) and sn == (2, 3, 8) and scale == 1.5 and max_new == 6
    assert kw["eos_token_id"] == 9 and kw["pad_token_id"] == 9 and kw["min_new_tokens"] == 2 and kw["sampling"] is None
    assert kw["kv_cache_dtype"] == "fp8_e4m3" and kw["weight_dtype"] is None and kw["max_rows"] == 4 and kw["return_step_logits"] is False
    # the negative prompt as the four generate() arguments: through prepare_multimodal_inputs, like the prompt
    out = U.generate(m, batch_input_ids=emb, negative_inputs=dict(batch_input_ids=neg[:, :2], batch_X_modals=None), guidance_scale=3.0,
                     do_sample=True, temperature=0.7, top_k=5, top_p=0.8, seed=11)
    assert guided[-1][0] == (2, 5, 8) and guided[-1][1] == (2, 2, 8) and guided[-1][2] == 3.0 and guided[-1][4]["sampling"] == (0.7, 5, 0.8, 11)
    # output_logits: the raw logits of the CONDITIONAL rows, step by step
    r = U.generate(m, inputs_embeds=emb, negative_inputs_embeds=neg, guidance_scale=2.0, output_logits=True, return_dict_in_generate=True)
    assert r.sequences.shape == (2, 3) and len(r.logits) == 3 and all(tuple(t.shape) == (2, 5) for t in r.logits)
    assert float(torch.stack(r.logits, 1).max()) == 2 * 3 * 5 - 1                # rows 0 .. B - 1 of the engine's [2B, n, V]


@pytest.mark.parametrize("kw, name", [
    (dict(num_beams=4), "num_beams"), (dict(allowed_sequences=[[3, 4]]), "allowed_sequences"), (dict(output_token_logprobs=True), "output_token_logprobs"),
    (dict(output_first_logits=True), "output_first_logits"), (dict(repetition_penalty=1.2), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(eos_token_id=[2, 3]), "eos_token_id"), (dict(length_penalty=2.0), "length_penalty"),
    (dict(typical_p=0.5), "typical_p")])
def test_refused_with_guidance_by_name(kw, name):
    m, plain, guided = _stub()
    with pytest.raises(NotImplementedError, match=name):
        U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), negative_inputs_embeds=torch.zeros((1, 3, 8)), guidance_scale=1.5, **kw)
    assert not plain and not guided


def test_a_guided_call_needs_one_negative_prompt():
    m, plain, guided = _stub()
    emb, neg = torch.zeros((1, 5, 8)), torch.zeros((1, 3, 8))
    with pytest.raises(ValueError, match="negative_inputs_embeds"):
        U.generate(m, inputs_embeds=emb, guidance_scale=1.5)
    with pytest.raises(ValueError, match="negative_inputs_embeds"):
        U.generate(m, inputs_embeds=emb, guidance_scale=1.5, negative_inputs_embeds=neg, negative_inputs=dict(batch_input_ids=neg))
    assert not plain and not guided


# ------------------------------------------------------------------ (c) the engine's refusals
def _bare_engine(V=64):
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    eng.lm_head = types.SimpleNamespace(weight=torch.zeros((V, 8)))
    eng._kv_mode, eng._w_mode = "bf16", "bf16"
    eng._call = lambda *a, **k: pytest.fail("device work was reached")
    return eng


def test_engine_refuses_by_name_before_any_device_work():
    eng = _bare_engine()
    emb, neg = torch.zeros((2, 5, 8)), torch.zeros((2, 3, 8))
    g = lambda *a, **k: eng.generate_guided(*a, **k)
    for k, v in (("constraint", object()), ("return_logprobs", True), ("processors", (1.2, 0, ())), ("return_hidden", True), ("return_first_logits", True),
                 ("decode_streams", 2)):
        with pytest.raises(NotImplementedError, match=k):
            g(emb, neg, 1.5, 4, **{k: v})
    for scale in (1.0, 0.5, 0.0, -2.0):
        with pytest.raises(NotImplementedError, match="guidance_scale"):
            g(emb, neg, scale, 4)
    with pytest.raises(ValueError, match="negative"):
        g(emb, neg[:1], 1.5, 4)
    with pytest.raises(ValueError, match="negative_embeds"):
        g(emb, neg[..., :4], 1.5, 4)
    with pytest.raises(NotImplementedError, match="eos_token_id"):
        g(emb, neg, 1.5, 4, eos_token_id=[2, 3])
    with pytest.raises(ValueError, match="max_new_tokens"):
        g(emb, neg, 1.5, 0)
    with pytest.raises(ValueError, match="max_rows"):
        g(emb, neg, 1.5, 4, max_rows=1)
    with pytest.raises(TypeError, match="banana"):
        g(emb, neg, 1.5, 4, banana=1)
    # the neutral values of what is refused are the call without them: they reach the (stubbed) entry with an equal request
    reached = []
    eng._call = lambda *a, **k: reached.append(a) or "ran"
    assert g(emb, neg, 1.5, 4, processors=(1.0, 0, ()), decode_streams=1, constraint=None, return_logprobs=False) == "ran"
    assert g(emb, neg, 1.5, 4) == "ran"
    kv, wd, shed, fn, e, n, scale, cap, req = reached[0]
    assert (kv, wd, shed) == (None, None, None) and fn == eng._generate_guided and e is emb and n is neg
    assert scale == 1.5 and req.max_new_tokens == 4 and cap == ops.DECODE_MAX_ROWS // 2
    assert req == reached[1][-1] == decoder._Request(4) and reached[1][:3] + reached[1][4:-1] == reached[0][:3] + reached[0][4:-1]


# ------------------------------------------------------------------ (d) the reference
def test_reference_is_hf_s_formula_and_its_bound_covers_an_fp32_evaluation():
    g_ = torch.Generator().manual_seed(5)
    for V, scale in ((1, 1.5), (5, 7.5), (320, 1.5), (4099, 7.5)):
        z = torch.randn((6, V), generator=g_) * 4
        ref, bound = R.mix_ref(z, 3, scale)
        c, u = torch.log_softmax(z[:3].double(), -1), torch.log_softmax(z[3:].double(), -1)
        hf = scale * (c - u) + u                                  # UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__
        assert float((ref - hf).abs().max()) <= 1e-12 * max(1.0, float(hf.abs().max()))
        c32, u32 = torch.log_softmax(z[:3], -1), torch.log_softmax(z[3:], -1)
        f32 = (scale * (c32 - u32) + u32).double()                # torch's own fp32 evaluation: other steps, the same magnitudes
        assert bool((bound > 0).all()) and bool(((f32 - ref).abs() <= 4 * bound).all())
        assert float(bound.max()) < 2.0 ** -10 * max(1.0, float(ref.abs().max())), "the bound is a few fp32 roundings, not a tolerance"
    z = torch.randn((2, 7), generator=g_)
    z[0, 2] = z[1, 4] = z[0, 6] = z[1, 6] = float("-inf")
    ref, bound = R.mix_ref(z, 1, 1.5)
    assert ref[0, [2, 4, 6]].tolist() == [float("-inf")] * 3 and bound[0, [2, 4, 6]].tolist() == [0.0] * 3 and bool(torch.isfinite(ref[0, [0, 1, 3, 5]]).all())
