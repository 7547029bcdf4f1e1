"""The opt-in FP8 KV cache, host side (no GPU): bindings and ABI, the engine's byte accounting and refusals, the torch statement of the storage
format (tests/kv_fp8_ref.py), and the softness cap of the token-id test's fixture (tests/test_kv_fp8_gpu.py) checked where it needs no device."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import kv_fp8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def test_bindings_struct_fields_and_abi_version():
    from crab_amd import _lib, ops
    lib = _lib.load()
    for name in ("crab_kv_quant_fp8", "crab_attn_decode_fp8"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert callable(ops.kv_quant_fp8) and callable(ops.attn_decode_fp8)
    names = [f[0] for f in _lib.LlamaIO._fields_]
    assert names[-4:] == ["kv_fp8", "k_scale", "v_scale", "scale_layer_stride"], names[-6:]
    assert C.sizeof(_lib.LlamaIO) == lib.crab_sizeof_llama_io()
    # the version history in csrc/capi.hip names 12 as the parent's ABI (crab_vq_nearest_f32 ...): this feature is 13
    src = open(os.path.join(ROOT, "crab_amd", "csrc", "capi.hip")).read()
    assert re.search(r"\b12: crab_vq_nearest_f32", src) and re.search(r"\b13: the opt-in FP8 KV cache", src)
    assert lib.crab_abi_version() == 13
    # argument validation happens before any HIP call
    assert lib.crab_kv_quant_fp8(None, None, None, None, 0, 0, 0, None, None, 0, None, None, 0, 1, 1, 1, 128, 64, 0, 0, 1, None) < 0
    assert lib.crab_attn_decode_fp8(None, None, None, 0, None, None, None, None, None, None, 0, 1, 1, 1, 128, 64, 0, None, C.c_float(1.0), None) < 0
    io, layer = _lib.LlamaIO(), _lib.LlamaLayer()
    io.kv_fp8 = 1
    assert lib.crab_llama_layers(None, None, C.byref(layer), 1, C.byref(io)) < 0


def _tiny(kv="bf16"):
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    cfg = UnifiedConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=96, pad_token_id=2)
    return get_peft_model(UnifiedForCausalLM(cfg, device="cpu", kv_cache_dtype=kv), LoraConfig())


def test_engine_byte_accounting_switch_and_refusals():
    from crab_amd.decoder import GenerationEngine, _round_up
    um = _tiny().base_model.model
    eng, c = um._engine, um.config
    assert eng.kv_cache_dtype == "bf16"
    L, Hk, d = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    S, new = 702, 256
    Tmax = _round_up(S + new, 64)
    per16 = eng.bytes_per_sequence(S, new)
    assert eng.kv_bytes_per_sequence(Tmax) == 2 * L * Hk * Tmax * d * 2 and eng.staging_bytes(8, S) == 0
    fixed16 = eng.fixed_bytes(8, S)
    eng.kv_cache_dtype = "fp8_e4m3"
    per8 = eng.bytes_per_sequence(S, new)
    assert eng.kv_bytes_per_sequence(Tmax) == 2 * L * Hk * Tmax * (d + 4)                           # codes + one fp32 scale per row
    assert per16 - per8 == 2 * L * Hk * Tmax * (2 * d - (d + 4))                                      # nothing else of a sequence's cost changes
    assert eng.staging_bytes(8, S) == 2 * L * 8 * Hk * _round_up(S, 64) * d * 2                       # the bf16 staging pair of the largest chunk
    assert eng.fixed_bytes(8, S) == fixed16 + eng.staging_bytes(8, S)
    # alloc_cache in fp8 mode: uint8 codes and fp32 scales; persistent per slot; a mode switch replaces the slot's buffers
    kc, vc, ks, vs = eng.alloc_cache(3, 64, slot=0)
    assert kc.dtype == vc.dtype == torch.uint8 and ks.dtype == vs.dtype == torch.float32
    assert tuple(kc.shape) == (L, 3, Hk, 64, d) and tuple(ks.shape) == (L, 3, Hk, 64)
    assert eng.alloc_cache(3, 64, slot=0)[0] is kc
    assert sum(t.numel() * t.element_size() for t in (kc, vc, ks, vs)) == 3 * eng.kv_bytes_per_sequence(64)
    eng.kv_budget_bytes = None
    eng.kv_cache_dtype = "bf16"
    b16 = eng.alloc_cache(3, 64, slot=0)
    assert len(b16) == 2 and b16[0].dtype == BF
    # the switch: two accepted values, per engine and per call
    for bad in ("fp8", "e5m2", "int8", None, 8):
        with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
            GenerationEngine.check_kv_cache_dtype(bad)
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        eng.kv_cache_dtype = "fp8_e5m2"
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        _tiny(kv="fp16")
    emb = torch.zeros(1, 4, c.hidden_size, dtype=BF)
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        eng.generate(emb, 4, kv_cache_dtype="fp8_e4m3fn")
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        um.generate(inputs_embeds=emb, max_new_tokens=4, kv_cache_dtype="FP8")
    assert eng.kv_cache_dtype == "bf16"                                                             # a refused call leaves the engine's mode alone
    # refused by name in fp8 mode: a caller-held cache through forward(), the masked one-token step (key-mask kernel)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        um(inputs_embeds=emb, use_cache=True, kv_cache_dtype="fp8_e4m3")
    kc16 = torch.zeros(L, 1, Hk, 64, d, dtype=BF)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        um(input_ids=torch.zeros(1, 1, dtype=torch.long), past_key_values=(kc16, kc16.clone(), 3), kv_cache_dtype="fp8_e4m3")
    um8 = _tiny(kv="fp8_e4m3").base_model.model
    assert um8._engine.kv_cache_dtype == "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        um8(inputs_embeds=emb, use_cache=True)
    codes = torch.zeros(L, 1, Hk, 64, d, dtype=torch.uint8)
    sc = torch.ones(L, 1, Hk, 64)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype.*crab_attn_decode_keymask"):
        eng._layers(None, 1, 1, codes, codes.clone(), 0, 64, 0, None, None, key_mask=torch.zeros(1, 2, dtype=torch.int32), kv_scales=(sc, sc.clone()))
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        eng._layers(None, 1, 4, codes, codes.clone(), 0, 64, 0, None, torch.zeros(1), kv_scales=(sc, sc.clone()))


def test_the_decode_state_key_separates_the_modes():
    """A captured graph of one mode is never replayed for the other: the mode and both scale pointers are terms of a decode state's key
    (decoder._state_key: real keys from plain values, no device needed), and so is the weight mode."""
    from crab_amd.decoder import _state_key
    base = dict(B=2, Tmax=64, max_new_tokens=8, eos=2, pad=2, min_new_tokens=0, return_hidden=False, ptrs=(11, 12, 13, 14, 15, 16, 17), lora=True,
                sampling=None, ragged=False, kv_mode="bf16", scale_ptrs=(0, 0), w8_key=("bf16",), logprobs=False)
    key = lambda **kw: _state_key(**dict(base, **kw))
    k16, k8 = key(), key(kv_mode="fp8_e4m3", scale_ptrs=(21, 22))
    assert k16 != k8 and "bf16" in k16 and "fp8_e4m3" in k8 and 21 in k8 and 22 in k8 and ("bf16",) in k16
    assert key(kv_mode="fp8_e4m3") != k16                                                         # the mode alone
    assert key(kv_mode="fp8_e4m3", scale_ptrs=(23, 22)) != k8 and key(kv_mode="fp8_e4m3", scale_ptrs=(21, 23)) != k8      # either scale tensor moved
    assert key(kv_mode="fp8_e4m3", scale_ptrs=(21, 22), w8_key=("fp8_e4m3", 31, 32)) != k8       # the weight mode


def test_format_statement_round_trips():
    codes = torch.arange(256, dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    finite = torch.isfinite(vals)
    assert int((~finite).sum()) == 2 and vals[finite].abs().max().item() == 448.0                   # OCP e4m3fn: two NaN codes, no infinities
    # every code times a power-of-two scale is a fixed point: a row that holds all finite codes (so amax = 448 * scale) comes back bit for bit
    row = vals[finite]
    for e in (-20, -3, 0, 5, 40):
        x = row * 2.0 ** e
        c, s = R.quant(x[None])
        assert s.item() == 2.0 ** e and torch.equal(R.dequant(c, s)[0], x)
        assert torch.equal(c[0].view(torch.float8_e4m3fn).float().abs(), row.abs())
    # bf16 rows: quantisation error at most half an e4m3 step of amax-scaled values (2^-4 relative to the element's binade, 2^-9 * scale absolute below it)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 128, generator=g) * 10 ** (torch.rand(64, 1, generator=g) * 8 - 4)).to(BF)
    c, s = R.quant(x)
    err = (R.dequant(c, s) - x.float()).abs()
    assert (err <= torch.maximum(x.float().abs() * 2.0 ** -4, s[:, None] * 2.0 ** -10) * 1.0001).all()
    assert ((R.dequant(c, s).abs().amax(-1) - x.float().abs().amax(-1)).abs() <= x.float().abs().amax(-1) * 2.0 ** -22).all()         # the row maximum is code 448: back up to the division's rounding
    # an all-zero row: scale 1, zero codes
    c, s = R.quant(torch.zeros(2, 64, dtype=BF))
    assert torch.equal(s, torch.ones(2)) and int(c.sum()) == 0
    # rows holding bf16 max / subnormals: finite codes, finite values back
    tiny = torch.finfo(BF).tiny
    rows = torch.zeros(4, 64, dtype=BF)
    rows[0, :] = torch.finfo(BF).max; rows[0, 1] = -torch.finfo(BF).max; rows[0, 2] = 1.0
    rows[1, :] = torch.tensor(tiny / 128).to(BF); rows[1, 3] = -torch.tensor(tiny / 2).to(BF)       # every element a bf16 subnormal
    rows[2, 0] = torch.finfo(BF).max; rows[2, 1] = torch.tensor(tiny / 128).to(BF)                   # max next to the smallest subnormal
    rows[3, 5] = torch.tensor(tiny).to(BF)
    assert rows[1].float().abs().max().item() < tiny and rows[1].float().abs().min().item() > 0
    c, s = R.quant(rows)
    back = R.dequant(c, s)
    assert torch.isfinite(back).all() and torch.isfinite(s).all() and (s > 0).all()
    assert not ((c & 0x7F) == 0x7F).any(), "a NaN code"
    mx = torch.finfo(BF).max
    assert abs(back[0, 0].item() - mx) <= mx * 2.0 ** -22 and abs(back[0, 1].item() + mx) <= mx * 2.0 ** -22
    assert s[1].item() == torch.finfo(torch.float32).tiny                                             # the FLT_MIN floor: 1 / scale stays finite


def test_sharp_fixture_is_not_too_soft_for_the_fp8_token_id_test():
    """tests/test_kv_fp8_gpu.py asserts the reference's greedy id on every step whose recorded margin exceeds twice the fp8-emulated oracle's logit
    distance from fp32.  That rule may exempt at most half of sharp_tiny_llama's steps, or the GPU test would pass vacuously: checked here, where
    the emulation needs no device."""
    from tests.test_kv_fp8_gpu import sharp_exemptions
    exempt, total, worst = sharp_exemptions("sharp_tiny_llama")
    print(f"sharp_tiny_llama: {int(exempt.sum())} of {total} steps exempt; largest per-step fp8-emulation distance {worst:.4f}")
    assert int(exempt.sum()) * 2 <= total, "fixture too soft"


# ------------------------------------------------------------------------------------------------------------------ scripts/fuzz_kv_fp8.py, host side
# The cases the FP8 KV-cache fuzzer generates AT THE COUNT THE GPU SUITE RUNS (scripts/fuzz_all.py at scale 0.5) cover the edges the fuzzer
# exists for - a later cut of the case count that drops one fails here, without a GPU - and its fp64 attention reference agrees with the
# oracle's attention.
import ast
import importlib.util
import math


def _fuzzer():
    spec = importlib.util.spec_from_file_location("fuzz_kv_fp8", os.path.join(ROOT, "scripts", "fuzz_kv_fp8.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _suite_run():
    """(cases, seed) of fuzz_kv_fp8.py in scripts/fuzz_all.py's RUNS, read from its source (importing the file would run the fuzzers)."""
    with open(os.path.join(ROOT, "scripts", "fuzz_all.py")) as f:
        tree = ast.parse(f.read())
    runs = next(ast.literal_eval(n.value) for n in ast.walk(tree) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "RUNS")
    assert runs[-1][0] == "fuzz_kv_fp8.py", "appended last: the other fuzzers keep their seeds and order"
    return runs[-1][1], runs[-1][2]


def _suite_cases():
    cases, seed = _suite_run()
    return _fuzzer().make_cases(max(1, int(cases * 0.5)), seed)        # tests/test_fuzz_gpu.py runs fuzz_all.py at scale 0.5


def test_case_generation_is_deterministic_and_needs_no_gpu():
    F = _fuzzer()
    cases, seed = _suite_run()
    assert F.make_cases(cases // 2, seed) == F.make_cases(cases // 2, seed)
    assert F.make_cases(cases // 2, seed) != F.make_cases(cases // 2, seed + 1)


def test_part_a_covers_the_kernel_edges_at_the_suite_count():
    F = _fuzzer()
    C = _suite_cases()
    attn, quant = C["attn"], C["quant"]
    counts = {n for c in attn for n in c["counts"]}
    assert {n % 64 for n in counts} == set(range(64)), sorted(set(range(64)) - {n % 64 for n in counts})
    assert set(F.BOUNDARY_COUNTS) <= counts, sorted(set(F.BOUNDARY_COUNTS) - counts)
    assert F.BOUNDARY_COUNTS == [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
    assert {c["G"] for c in attn} == {1, 2, 4, 7, 8} and {c["d"] for c in attn} == {64, 128}
    assert {c["Hk"] for c in attn} == {1, 2, 4, 8} and {c["B"] for c in attn} == {1, 2, 3, 8, 40, 130}
    assert {c["pos_form"] for c in attn} == {"pos0", "pos_dev", "both"}
    assert all(c["pos0"] > 0 and c["pos0"] < c["slot"] for c in attn if c["pos_form"] == "both")
    assert any(c["B"] >= 100 for c in attn)
    assert any(c["kv_start"] is not None and 0 in c["counts"][1:] for c in attn), "a row with zero cached keys beside rows that have some"
    assert any(c["kv_start"] is None for c in attn) and any(c["pad_q"] for c in attn) and any(c["pad_o"] for c in attn)
    assert any(t % 64 for t in {c["Tmax"] for c in attn}) and {c["Tmax"] for c in attn} == {64, 128, 200, 960}
    assert {c["new_k"] for c in attn} >= {"dominant", "zero", "subnormal"} and {c["new_v"] for c in attn} >= {"dominant", "zero", "subnormal"}
    for c in attn:                                       # every case stays inside its cache
        assert 0 <= c["slot"] < c["Tmax"] and all(0 <= n <= c["slot"] for n in c["counts"]) and len(c["counts"]) == c["B"]
    assert {c["d"] for c in quant} == {64, 128} and any(c["row_off"] is None for c in quant)
    assert any(c["row_off"] and 0 in c["row_off"] and c["S"] - 1 in c["row_off"] for c in quant)
    assert any((c["L"] * c["Bc"] * c["Hk"] * c["S"]) % (256 // (c["d"] // 8)) for c in quant), "a row total that is not a multiple of the rows per block"
    for c in quant:
        assert c["t0"] + c["S"] <= c["Tsrc"] and c["t_dst"] + c["S"] <= c["Tmax"] and c["b0"] + c["Bc"] <= c["B"]
        assert c["row_off"] is None or all(0 <= o < c["S"] for o in c["row_off"])
    assert len(attn) > len(quant) > len(C["step"]) >= len(C["gen"]), "part A gets the bulk"


def test_parts_b_c_d_cover_their_edges_at_the_suite_count():
    C = _suite_cases()
    step = C["step"]
    assert {c["B"] for c in step} >= {1, 3, 16, 17, 40, 128, 130, 256, 260}, "a batch size in every decode GEMM regime"
    assert any(c["row_off"] for c in step) and any(not c["row_off"] for c in step)
    assert {c["cfg"]["d"] for c in step} == {64, 128} and any(c["cfg"]["qwen"] for c in step) and any(not c["cfg"]["qwen"] for c in step)
    shapes = [s for c in C["gen"] for s in c["shapes"]]
    for k in (1, 7):
        assert any(k in s["chunks"] and s["B"] > k for s in shapes), f"more than one prefill chunk with prefill_chunk={k}"
    assert any(s["B"] // 2 in s["chunks"] and s["B"] // 2 >= 1 and s["B"] >= 2 for s in shapes)
    assert any(s["B"] >= 100 for s in shapes) and any(s["streams2"] for s in shapes)
    assert all(len(set(c["ragged"]["S"])) > 1 for c in C["gen"]), "ragged waves need groups of different prompt lengths"
    calls = C["calls"]
    mode, seen, visited = "bf16", {}, False
    for c in calls:
        mode = c.get("engine") or mode
        if c["kind"] != "generate": continue
        seen.setdefault((c["B"], c["S"], c["n"]), []).append(c["kv"] or mode)
    for modes in seen.values():
        s = "".join("f" if m == "fp8_e4m3" else "b" for m in modes)
        visited = visited or "bfb" in s.replace("bb", "b").replace("ff", "f")
    assert visited, "one shape visited bf16 -> fp8 -> bf16"
    assert any(c.get("engine") == "fp8_e4m3" for c in calls) and any(c["kind"] == "forward" for c in calls) and any(c["kind"] == "batches" for c in calls)
    assert any(c.get("kv") is None and c["kind"] == "generate" for c in calls), "calls that take the engine's mode"


def test_fp64_attention_reference_agrees_with_the_oracle():
    """fuzz_kv_fp8.attention_fp64 (grouped-query heads, a per-sequence visibility mask) against oracle.crab_oracle's softmax attention, sequence
    by sequence over its visible keys; head_rel_err is tests.util.rel_err's measure applied per (sequence, head)."""
    from oracle import crab_oracle as O
    from tests.util import rel_err
    F = _fuzzer()
    g = torch.Generator().manual_seed(3)
    B, Hk, G, d, T = 3, 2, 2, 64, 21
    H = Hk * G
    q, K, V = torch.randn(B, H, d, generator=g), torch.randn(B, Hk, T, d, generator=g), torch.randn(B, Hk, T, d, generator=g) * 3
    first = [0, 5, 20]
    vis = torch.arange(T)[None] >= torch.tensor(first)[:, None]
    got = F.attention_fp64(q, K, V, vis, d ** -0.5)
    assert got.dtype == torch.float64
    for b in range(B):
        kk, vv = (x[b, :, first[b]:].repeat_interleave(G, 0).transpose(0, 1).reshape(1, T - first[b], H * d) for x in (K, V))
        ref = O._mha(q[b].reshape(1, 1, H * d), kk, vv, H, 1.0 / math.sqrt(d))
        assert (got[b].reshape(-1).float() - ref.reshape(-1)).abs().max().item() <= 2e-6 * ref.abs().max().item()
    a, r = torch.randn(2, 3, 8, generator=g), torch.randn(2, 3, 8, generator=g)
    e = F.head_rel_err(a, r)
    for b in range(2):
        for h in range(3):
            assert abs(e[b, h].item() - rel_err(a[b, h], r[b, h])) <= 1e-6 * e[b, h].item()
