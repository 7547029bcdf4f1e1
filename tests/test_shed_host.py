"""shed_finished without a GPU: the two C symbols and their argument checks, the host validation of ops.kv_compact_rows, the ladder policy as a
pure function, every refusal of the engine and of the model surface by name, and the off switch (None / False reach the existing path with
unchanged arguments)."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder, ops
from crab_amd.unified_llama import UnifiedForCausalLM as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ (a) the C entry points
def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_kv_compact_rows", "crab_sample_select_rows"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.crab_abi_version() == 13
    # the documented signatures: (ctx, stream, k, v, layer_stride, L, rows, Hk, Tmax, head_dim, n_live, src_rows, row_off, pos_dev) and
    # crab_sample_select_warped's operands without kept_n / kept_min, + row_ids
    vp, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert _lib.SYMBOLS["crab_kv_compact_rows"] == (i, [vp, vp, vp, vp, i64, i, i, i, i, i, i, vp, vp, vp])
    assert _lib.SYMBOLS["crab_sample_select_rows"] == (i, _lib.SYMBOLS["crab_sample_select_warped"][1][:-2] + [vp])
    m = re.search(r"^int\s+crab_kv_compact_rows\s*\(([^;]*)\);", txt, flags=re.M | re.S)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert names == ["ctx", "stream", "k_cache", "v_cache", "layer_stride", "L", "rows", "Hk", "Tmax", "head_dim", "n_live", "src_rows", "row_off", "pos_dev"]
    m = re.search(r"^int\s+crab_sample_select_rows\s*\(([^;]*)\);", txt, flags=re.M | re.S)
    assert m.group(1).split(",")[-1].split()[-1].lstrip("*") == "row_ids"
    assert list(inspect.signature(ops.kv_compact_rows).parameters) == ["kc", "vc", "src_rows", "pos_dev", "row_off"]


def _aligned(n=64):
    buf = C.create_string_buffer(n + 16)
    a = C.addressof(buf)
    return buf, C.c_void_p(a + (-a % 16))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    keep, one = _aligned()

    def compact(ctx_=h, kc=one, vc=one, stride=None, L=2, rows=4, Hk=2, Tmax=64, d=64, n_live=2, src=one, off=one, pos=one):
        stride = rows * Hk * Tmax * d if stride is None else stride
        return lib.crab_kv_compact_rows(ctx_, None, kc, vc, stride, L, rows, Hk, Tmax, d, n_live, src, off, pos)

    assert compact(ctx_=None) == -1
    for k in ("kc", "vc", "src", "pos"):
        assert compact(**{k: None}) == -1, k
    assert b"kv_compact_rows" in ctx.raw
    for kw in (dict(n_live=0), dict(n_live=5), dict(d=60), dict(d=0), dict(L=0), dict(rows=0, n_live=0), dict(Hk=0), dict(Tmax=0),
               dict(kc=C.c_void_p(one.value + 8)), dict(vc=C.c_void_p(one.value + 2)), dict(stride=4 * 2 * 64 * 64 - 8), dict(stride=4 * 2 * 64 * 64 + 4)):
        assert compact(**kw) == -1, kw
    assert compact(L=40000, Hk=64, Tmax=1024) == -3, "CRAB_E_UNSUPPORTED past 2^31 16-byte units"

    def rows(ctx_=h, logits=one, B=3, V=64, cur=one, out=one, step=one, fin=one, t=0.6, k=50, p=0.9, min_p=0.0, eps=0.0, eta=0.0, ids=one):
        return lib.crab_sample_select_rows(ctx_, None, logits, V, B, V, cur, out, 8, step, fin, 7, 1, 0, t, k, p, 5, min_p, eps, eta, ids)

    ctx.raw = bytes(len(ctx.raw))
    assert rows(ctx_=None) == -1
    for k in ("logits", "cur", "out", "step", "fin", "ids"):
        assert rows(**{k: None}) == -1, k
    assert b"sample_select_rows" in ctx.raw
    for kw in (dict(B=0), dict(V=0), dict(t=0.0), dict(p=0.0), dict(p=1.5), dict(k=-1), dict(min_p=1.5), dict(min_p=-0.1), dict(eps=1.0), dict(eta=1.0),
               dict(eps=float("nan"))):
        assert rows(**kw) == -1, kw
    del keep


# ------------------------------------------------------------------ (b) the host validation of ops.kv_compact_rows
def test_kv_compact_rows_validates_the_indices_on_the_host():
    kc = torch.zeros((2, 6, 2, 64, 64), dtype=torch.bfloat16)    # CPU tensors: the indices are checked before any device is asked for
    pos = torch.zeros((1,), dtype=torch.int32)
    for src, what in (([3, 2, 4], "strictly increasing"), ([1, 1, 2], "repeats"), ([0, 0], "repeats"), ([0, 6], "outside"), ([7], "outside"), ([], "empty"),
                      (torch.tensor([2, 1]), "strictly increasing"), ([-1, 2], "below its destination")):
        with pytest.raises(ValueError, match=what):
            ops.kv_compact_rows(kc, kc, src, pos)
    # src[j] < j cannot be written as a strictly increasing list of non-negative indices, so the contract's third clause is met through the pure checker
    with pytest.raises(ValueError, match="below its destination"):
        ops.check_compact_rows([-1], 6)
    with pytest.raises(ValueError, match="entries for a cache"):
        ops.check_compact_rows(list(range(7)), 6)
    assert ops.check_compact_rows([1, 2, 5], 6) == [1, 2, 5] and ops.check_compact_rows(torch.tensor([0, 3]), 4) == [0, 3]


# ------------------------------------------------------------------ (c) the ladder policy
def test_ladder_policy_is_a_pure_function():
    assert decoder.shed_ladder(None) is None and decoder.shed_ladder(False) is None
    lad = decoder.shed_ladder(True)
    assert lad == decoder.shed_default_ladder() and list(lad) == sorted(set(lad))
    for r in (16, 64, 256, ops.DECODE_MAX_ROWS):                 # the row counts at which the decode step changes kernels
        assert r in lad
    assert all(2 * a <= b for a, b in zip(lad, lad[1:])), "every rung at most half of the next"
    assert decoder.shed_ladder((1, 2, 3, 4, 6)) == (1, 2, 3, 4, 6) and decoder.shed_ladder([16, 24]) == (16, 24)
    for bad in ((4, 2), (2, 2), (0, 4), (-1,), (), (2.5,), "16", 16, (True, 4)):
        with pytest.raises(ValueError, match="shed_finished"):
            decoder.shed_ladder(bad)
    rung = decoder.shed_rung
    assert rung((1, 2, 3, 4, 6), 3, 6) == 3 and rung((1, 2, 3, 4, 6), 5, 6) is None and rung((1, 2, 3, 4, 6), 6, 6) is None
    assert rung((16, 24), 10, 24) == 16 and rung((16, 24), 16, 24) == 16 and rung((16, 24), 17, 24) is None
    assert rung((16, 24), 3, 16) is None, "no shed when B' == B_cur"
    assert rung((4, 16), 100, 512) is None, "no rung holds the live rows"
    assert rung(lad, 1, 512) == lad[0] and rung(lad, 200, 512) == 256 and rung(lad, 257, 512) is None


# ------------------------------------------------------------------ (d) the engine's refusals
def _bare_engine(V=64):
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    eng.lm_head = types.SimpleNamespace(weight=torch.zeros((V, 8)))
    eng._kv_mode, eng._w_mode = "bf16", "bf16"
    eng._tries = {}
    eng._call = lambda *a, **k: pytest.fail("device work was reached")
    return eng


def test_engine_refuses_by_name_before_any_device_work():
    eng = _bare_engine()
    emb = torch.zeros((2, 5, 8))
    for fn, args in ((eng.generate, (emb, 8)), (eng.generate_many, ([emb, emb], 8))):
        extra = {"coalesce": True} if fn == eng.generate_many else {}
        for k, v in (("processors", (1.2, 0, ())), ("return_logprobs", True), ("return_hidden", True)):
            with pytest.raises(NotImplementedError, match="shed_finished with " + k):
                fn(*args, shed_finished=True, **{k: v}, **extra)
        with pytest.raises(NotImplementedError, match='shed_finished with kv_cache_dtype="fp8_e4m3"'):
            fn(*args, shed_finished=True, kv_cache_dtype="fp8_e4m3", **extra)
        with pytest.raises(ValueError, match="shed_every"):
            fn(*args, shed_finished=True, shed_every=0, **extra)
        with pytest.raises(ValueError, match="shed_finished"):
            fn(*args, shed_finished=(4, 2), **extra)
    with pytest.raises(NotImplementedError, match="shed_finished with decode_streams"):
        eng.generate(emb, 8, shed_finished=True, decode_streams=2)
    with pytest.raises(NotImplementedError, match="shed_finished with return_step_logits in the coalesced form"):
        eng.generate_many([emb, emb], 8, coalesce=True, shed_finished=True, return_step_logits=True)
    with pytest.raises(NotImplementedError, match="shed_finished with coalesce=False"):
        eng.generate_many([emb, emb], 8, shed_finished=True)
    eng2 = _bare_engine()
    eng2._kv_mode = "fp8_e4m3"                                   # the engine's own mode counts as the call's
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        eng2.generate(emb, 8, shed_finished=True)
    # constraint: refused by check_shed itself (the engine resolves a trie only after it)
    with pytest.raises(NotImplementedError, match="shed_finished with constraint"):
        decoder.check_shed(True, None, constraint=object())
    for name in ("generate_guided", "generate_beam", "generate_lookup", "generate_shared_prefix"):
        assert "shed_finished" not in inspect.signature(getattr(decoder.GenerationEngine, name)).parameters, name


def test_off_reaches_the_existing_engine_entry_with_unchanged_arguments():
    eng = _bare_engine()
    seen = []
    eng._call = lambda *a, **k: seen.append((a, k)) or "res"
    emb = torch.zeros((2, 5, 8))
    assert eng.generate(emb, 8, eos_token_id=3) == "res"
    for off in (None, False):
        assert eng.generate(emb, 8, eos_token_id=3, shed_finished=off, shed_every=1) == "res"
    # (kv_cache_dtype, weight_dtype, the call's _Shed, fn, embeds, request, decode_streams): no _Shed, and the request of the plain call
    assert len(seen) == 3 and all(s[0][2] is None and s[0][3] == eng._generate and s[0][5].shed is None and not s[1] for s in seen)
    assert all(len(s[0]) == len(seen[0][0]) and s[0][5] == seen[0][0][5] and s[0][6] == seen[0][0][6] for s in seen[1:])
    assert seen[0][0][5] == decoder._Request(8, 3)
    assert eng.generate(emb, 8, eos_token_id=3, shed_finished=(2, 4), shed_every=3) == "res"
    shed = seen[3][0][2]
    assert isinstance(shed, decoder._Shed) and (shed.ladder, shed.every) == ((2, 4), 3) and seen[3][0][5].shed is shed
    assert seen[3][0][5].replace(shed=None) == seen[0][0][5]
    assert decoder.check_shed(None) is None and decoder.check_shed(False, 1, return_logprobs=True) is None
    assert decoder.check_shed(True) == (decoder.shed_default_ladder(), decoder.EOS_CHECK_EVERY) and decoder.check_shed((2, 4), 3) == ((2, 4), 3)


# ------------------------------------------------------------------ (e) the model surface
def _stub():
    calls = []
    eng = types.SimpleNamespace(kv_cache_dtype="bf16", weight_dtype="bf16")
    eng.generate = lambda embeds, max_new, **kw: calls.append(("generate", kw)) or torch.zeros((embeds.shape[0], 3), dtype=torch.int64)
    eng.generate_many = lambda embeds, max_new, **kw: calls.append(("generate_many", kw)) or [torch.zeros((1, 3), dtype=torch.int64)]
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), model=types.SimpleNamespace(pad_token_id=None), device="cpu", _engine=eng,
                              lm_head=types.SimpleNamespace(weight=torch.zeros((64, 8))),
                              _PROCESSOR_ARGS=U._PROCESSOR_ARGS, _BEAM_ARGS=U._BEAM_ARGS, _check_generate_kwargs=U._check_generate_kwargs,
                              _sampling=U._sampling)
    m._processors = types.MethodType(U._processors, m)
    m._constraint = types.MethodType(U._constraint, m)
    m.prepare_multimodal_inputs_many = lambda batches, **kw: [{"inputs_embeds": b["emb"]} for b in batches]
    return m, calls


def test_model_surface_hands_the_arguments_over_and_off_changes_nothing():
    m, calls = _stub()
    emb = torch.zeros((2, 5, 8))
    U.generate(m, inputs_embeds=emb, max_new_tokens=6)
    U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=None)
    U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=False, shed_every=1)
    assert all(c == calls[0] for c in calls[1:]) and "shed_finished" not in calls[0][1] and "shed_every" not in calls[0][1]
    U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=True, shed_every=2)
    U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=(1, 2), do_sample=True, seed=3)
    assert calls[3][1]["shed_finished"] is True and calls[3][1]["shed_every"] == 2
    assert calls[4][1]["shed_finished"] == (1, 2) and calls[4][1]["shed_every"] is None and calls[4][1]["sampling"][3] == 3
    assert {k: v for k, v in calls[3][1].items() if not k.startswith("shed_")} == calls[0][1]
    del calls[:]
    U.generate_batches(m, [{"emb": emb}, {"emb": emb}], coalesce=True, max_new_tokens=6)
    U.generate_batches(m, [{"emb": emb}, {"emb": emb}], coalesce=True, max_new_tokens=6, shed_finished=True)
    assert "shed_finished" not in calls[0][1] and calls[1][1]["shed_finished"] is True and calls[1][1]["coalesce"] is True
    assert "shed_finished" not in U._UNSUPPORTED and "shed_every" not in U._UNSUPPORTED


def test_model_surface_refuses_by_name():
    m, calls = _stub()
    emb = torch.zeros((1, 5, 8))
    g = lambda **kw: U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=True, **kw)
    for k, v in (("num_beams", 2), ("guidance_scale", 1.5), ("prompt_lookup_num_tokens", 3), ("allowed_sequences", [[1, 2]]), ("repetition_penalty", 1.2),
                 ("no_repeat_ngram_size", 2), ("output_token_logprobs", True)):
        with pytest.raises(NotImplementedError, match=r"shed_finished=True, " + k):
            g(**{k: v})
    with pytest.raises(NotImplementedError, match="ONE eos_token_id"):
        g(eos_token_id=[3, 4])
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        g(kv_cache_dtype="fp8_e4m3")
    m._engine.kv_cache_dtype = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        g()
    m._engine.kv_cache_dtype = "bf16"
    with pytest.raises(ValueError, match="shed_finished"):
        U.generate(m, inputs_embeds=emb, max_new_tokens=6, shed_finished=(4, 2))
    with pytest.raises(NotImplementedError, match=r"generate_batches\(coalesce=False\)\(shed_finished"):
        U.generate_batches(m, [{"emb": emb}], max_new_tokens=6, shed_finished=True)
    with pytest.raises(NotImplementedError, match="generate_questions"):
        U.generate_questions(m, [], shed_finished=True)
    with pytest.raises(NotImplementedError, match="generate_avs"):
        U._avs_generate(m, [], None, dict(shed_finished=True))
    assert not calls, "a refused call reached the engine"
