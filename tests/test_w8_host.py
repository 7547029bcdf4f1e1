"""The opt-in FP8 decoder weights, host side (no GPU): bindings and ABI, argument validation before any HIP call, the engine's mode switches and
the keys that keep a captured graph inside its mode, the quantised-weight cache of a packed group, and the mixed emulation of the oracle
(tests/w8_ref.py: prefill with W, decode steps with the dequantised weights)."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import w8_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def test_bindings_struct_layout_and_abi_version():
    from crab_amd import _lib, ops
    lib = _lib.load()
    for name in ("crab_weight_quant_fp8", "crab_sizeof_linear_group"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert callable(ops.weight_quant_fp8)
    assert C.sizeof(_lib.GemmDesc) == lib.crab_sizeof_gemm_desc()
    assert C.sizeof(_lib.LinearGroup) == lib.crab_sizeof_linear_group()
    assert C.sizeof(_lib.LlamaLayer) == lib.crab_sizeof_llama_layer()
    # appended: zero-initialised descriptors of existing callers mean "bf16 weights"
    assert [f[0] for f in _lib.GemmDesc._fields_][-3:] == ["B8", "ldb8", "b_scale"]
    assert [f[0] for f in _lib.LinearGroup._fields_][-3:] == ["W8", "ldw8", "w_scale"]
    # crab_llama_io is untouched, and so is the ABI number: the new symbols are additions under 13
    assert [f[0] for f in _lib.LlamaIO._fields_][-4:] == ["kv_fp8", "k_scale", "v_scale", "scale_layer_stride"]
    assert C.sizeof(_lib.LlamaIO) == lib.crab_sizeof_llama_io()
    assert lib.crab_abi_version() == 13
    src = open(os.path.join(ROOT, "crab_amd", "csrc", "capi.hip")).read()
    assert re.search(r"additions under 13.{0,200}crab_weight_quant_fp8", src)
    assert re.search(r"\b12: crab_vq_nearest_f32", src) and re.search(r"\b13: the opt-in FP8 KV cache", src)
    hdr = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for sym in ("crab_weight_quant_fp8", "crab_sizeof_linear_group", "const void* B8; int64_t ldb8; const float* b_scale;",
                "const void* W8; int64_t ldw8; const float* w_scale;"):
        assert sym in hdr, sym


def test_quantiser_refuses_bad_arguments_before_any_hip_call():
    """Every refusal below returns before a launch, so it runs on a machine without a GPU.  crab_ctx_create needs a device; a refusal only
    writes its message into the context (a plain zero-initialised struct, csrc/crab_internal.h), so a zeroed buffer stands in for one."""
    from crab_amd import _lib
    lib = _lib.load()
    q = lib.crab_weight_quant_fp8
    assert q(None, None, None, 0, 0, 0, None, 0, None) < 0                        # no context
    keep = C.create_string_buffer(1 << 16)
    ctx = C.cast(keep, C.c_void_p)
    w = (C.c_uint16 * (4 * 64))()
    codes = (C.c_uint8 * (4 * 64 + 64))()
    sc = (C.c_float * 4)()
    aw, ac, asc = C.addressof(w) + (-C.addressof(w)) % 16, C.addressof(codes) + (-C.addressof(codes)) % 16, C.addressof(sc)

    def call(W=aw, ldw=32, N=3, K=32, cd=ac, ldc=32, s=asc):
        return q(ctx, None, W, ldw, N, K, cd, ldc, s)
    INVALID = -1
    assert call(W=None) == INVALID and call(cd=None) == INVALID and call(s=None) == INVALID
    assert call(N=0) == INVALID and call(K=0) == INVALID
    assert call(K=28) == INVALID                                                   # K % 8
    assert call(ldw=36) == INVALID and call(ldw=24) == INVALID                     # ldw % 8, ldw < K
    assert call(ldc=40) == INVALID and call(ldc=16) == INVALID                     # ld_codes % 16, ld_codes < K
    assert call(W=aw + 2) == INVALID and call(cd=ac + 8) == INVALID                # alignment
    assert b"ld_codes" in lib.crab_last_error(ctx)
    del keep


def _tiny(**kw):
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    cfg = UnifiedConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=96, pad_token_id=2)
    return get_peft_model(UnifiedForCausalLM(cfg, device="cpu", **kw), LoraConfig())


def _cpu_quantiser(monkeypatch):
    """ops.weight_quant_fp8 needs a device; its torch statement stands in for it here (tests/test_w8_gpu.py pins the two to each other)."""
    from crab_amd import ops
    calls = []

    def quant(w, codes=None, scale=None):
        calls.append(w.data_ptr())
        c, s = WR.quant_rows(w)
        return c.contiguous(), s.contiguous()
    monkeypatch.setattr(ops, "weight_quant_fp8", quant)
    return calls


def test_mode_switches_and_refusals():
    from crab_amd.decoder import GenerationEngine, W8_MAX_ROWS
    um = _tiny().base_model.model
    eng, c = um._engine, um.config
    assert eng.weight_dtype == "bf16" and W8_MAX_ROWS == 16
    for bad in ("FP8", "fp8", "e4m3", "int8", None, 8):
        with pytest.raises(ValueError, match="weight_dtype.*'bf16' / 'fp8_e4m3'"):
            GenerationEngine.check_weight_dtype(bad)
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        eng.weight_dtype = "fp8_e5m2"
    with pytest.raises(ValueError, match="'bf16' / 'fp8_e4m3'"):
        _tiny(weight_dtype="FP8")
    emb = torch.zeros(1, 4, c.hidden_size, dtype=BF)
    with pytest.raises(ValueError, match="weight_dtype.*'bf16' / 'fp8_e4m3'"):
        eng.generate(emb, 4, weight_dtype="FP8")
    with pytest.raises(ValueError, match="weight_dtype.*'bf16' / 'fp8_e4m3'"):
        um.generate(inputs_embeds=emb, max_new_tokens=4, weight_dtype="FP8")
    with pytest.raises(ValueError, match="weight_dtype"):
        eng.generate_many([emb], 4, weight_dtype="fp8_e4m3fn")
    # a refused call leaves both modes alone - also when the OTHER argument was acceptable
    with pytest.raises(ValueError, match="weight_dtype"):
        eng.generate(emb, 4, kv_cache_dtype="fp8_e4m3", weight_dtype="FP8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        eng.generate(emb, 4, kv_cache_dtype="FP8", weight_dtype="fp8_e4m3")
    assert eng.weight_dtype == "bf16" and eng.kv_cache_dtype == "bf16"
    um8 = _tiny(weight_dtype="fp8_e4m3", kv_cache_dtype="fp8_e4m3").base_model.model
    assert um8._engine.weight_dtype == "fp8_e4m3" and um8._engine.kv_cache_dtype == "fp8_e4m3"
    assert um8._engine._w8_rows(1) and um8._engine._w8_rows(16) and not um8._engine._w8_rows(17) and not eng._w8_rows(1)
    # weight_dtype is a name of its own: the table of refused HF arguments does not know it
    assert "weight_dtype" not in type(um)._UNSUPPORTED
    # the FP8 weights serve decode steps only: a prefill-shaped or masked pass asking for them is refused by name
    kc = torch.zeros(2, 1, 2, 64, 16, dtype=BF)
    with pytest.raises(NotImplementedError, match="weight_dtype"):
        eng._layers(None, 1, 4, kc, kc.clone(), 0, 64, 0, None, torch.zeros(1), w8=True)
    with pytest.raises(NotImplementedError, match="weight_dtype"):
        eng._layers(None, 17, 1, kc, kc.clone(), 0, 64, 0, None, None, w8=True)


def test_state_key_and_layer_table_fingerprint_separate_the_modes(monkeypatch):
    """A captured graph of one weight mode is never replayed for the other: the mode and the pointers of the codes / scales are part of
    a decode state's key (decoder._state_key over the engine's _w8_key: real keys, no device needed) and of the native sequencer's
    layer-table fingerprint."""
    from crab_amd.decoder import _child_key, _state_key
    _cpu_quantiser(monkeypatch)
    eng = _tiny().base_model.model._engine
    um8 = _tiny(weight_dtype="fp8_e4m3").base_model.model
    eng8 = um8._engine
    base = dict(B=2, Tmax=64, max_new_tokens=8, eos=2, pad=2, min_new_tokens=0, return_hidden=False, ptrs=(11, 12, 13, 14, 15, 16, 17), lora=True,
                sampling=None, ragged=False, kv_mode="bf16", scale_ptrs=(0, 0), logprobs=False)
    key = lambda **kw: _state_key(**dict(base, **kw))
    assert eng._w8_key(2) == ("bf16",) and eng8._w8_key(17) == ("bf16",)         # the bf16 fragment; above 16 rows the FP8 mode steps on bf16 too
    w8k = eng8._w8_key(2)
    quant = [t.data_ptr() for l in um8.model.layers for g in l.groups() for t in g.quantize_fp8()]
    assert w8k == ("fp8_e4m3",) + tuple(quant) and w8k == eng8._w8_key(16)        # the mode, then codes and scales of every group
    k16, k8 = key(w8_key=("bf16",)), key(w8_key=w8k)
    assert k16 != k8 and ("bf16",) in k16 and w8k in k8
    assert key(w8_key=w8k[:-1] + (w8k[-1] + 256,)) != k8                          # a scale tensor that moved: another key
    assert key(w8_key=("bf16",), kv_mode="fp8_e4m3") != k16                      # the KV mode ...
    assert key(w8_key=("bf16",), scale_ptrs=(5, 0)) != k16 and key(w8_key=("bf16",), scale_ptrs=(0, 5)) != k16      # ... and both of its scale pointers
    assert _child_key(k16, 4, w8k) == k16 + ("shed", 4) + w8k                     # a shed child: the root's key, its rows, ITS weight form
    fp16, fp8 = eng._table_fingerprint(False), eng._table_fingerprint(True)
    assert fp16 != fp8 and fp8[:len(fp16)] == fp16 and "fp8_e4m3" in fp8
    n_groups = 4 * len(eng.model.layers)
    assert len(fp8) == len(fp16) + 1 + 2 * n_groups                              # codes and scales of every group
    assert eng._table_fingerprint(True) == fp8                                   # stable while nothing moves
    g = eng.model.layers[0].mlp._down
    old_scale = g.quantize_fp8()[1].clone()
    with torch.no_grad():
        g.linears[0].weight.add_(1.0)                                             # in-place update through the member Parameter: new codes
    eng._table_fingerprint(True)                                                  # (re)quantises what changed
    assert not torch.equal(g.quantize_fp8()[1], old_scale) and torch.equal(g.quantize_fp8()[1], WR.quant_rows(g.W)[1])
    # the native table of the mode carries the pointers; the plain one does not
    t8, t16 = eng._layer_table(True), eng._layer_table(False)
    codes, sc = g.quantize_fp8()
    assert t8[0].down.W8 == codes.data_ptr() and t8[0].down.w_scale == sc.data_ptr() and t8[0].down.ldw8 == codes.stride(0)
    assert not t16[0].down.W8 and not t16[0].down.w_scale and t16[0].down.W == t8[0].down.W


def test_quantised_weight_cache_of_a_group(monkeypatch):
    calls = _cpu_quantiser(monkeypatch)
    um = _tiny().base_model.model
    g = um.model.layers[1].self_attn._qkv
    with torch.no_grad():
        g.W.copy_(torch.randn(g.W.shape).to(BF))
    c0, s0 = g.quantize_fp8()
    assert len(calls) == 1 and c0.dtype == torch.uint8 and tuple(c0.shape) == (g.N, g.K) and s0.dtype == torch.float32 and tuple(s0.shape) == (g.N,)
    assert g.quantize_fp8()[0] is c0 and len(calls) == 1                          # cached
    want_c, want_s = WR.quant_rows(g.W)
    assert torch.equal(c0, want_c) and torch.equal(s0, want_s)
    # an in-place update through a member Parameter (load_state_dict, copy_) invalidates it ...
    with torch.no_grad():
        g.linears[1].weight.mul_(3)
    c1, s1 = g.quantize_fp8()
    assert len(calls) == 2 and not torch.equal(s1, s0)
    k0, k1 = g.row_range(1)
    assert torch.equal(s1[k0:k1], WR.quant_rows(g.W)[1][k0:k1])
    # ... so do rebind() and the engine's invalidate()
    g.rebind()
    assert g._w8 is None
    g.quantize_fp8()
    assert len(calls) == 3
    um._engine.invalidate()
    assert g._w8 is None and all(x._w8 is None for l in um.model.layers for x in l.groups())
    # interleaved gate|up rows: quantised as stored, each row its own scale
    gu = um.model.layers[0].mlp._gu
    with torch.no_grad():
        gu.linears[0].weight.copy_(torch.randn(gu.linears[0].weight.shape).to(BF))
        gu.linears[1].weight.copy_((torch.randn(gu.linears[1].weight.shape) * 100).to(BF))
    _, s = gu.quantize_fp8()
    assert torch.equal(s[0::2], WR.quant_rows(gu.linears[0].weight)[1]) and torch.equal(s[1::2], WR.quant_rows(gu.linears[1].weight)[1])


def test_mixed_oracle_emulation_on_a_tiny_config():
    """Prefill with W, decode steps with dequant(quant(W)): deterministic, equal to the plain oracle at step 0 (prefill is untouched), apart
    from it afterwards by roughly the quantisation noise, and only the seven projections of each layer are replaced."""
    from oracle import crab_oracle as O
    from tests.test_oracle_golden import _full_cfg
    from tests.util import load_fixture, weights_from_table
    meta, A = load_fixture("full_tiny_llama")
    W = O.strip_peft_prefix(weights_from_table(meta))
    cfg = _full_cfg(meta).decoder
    Wq = WR.dequantised_weights(W)
    changed = [k for k in W if not torch.equal(W[k].float(), Wq[k].float())]
    assert changed and all(WR.PROJ.search(k) for k in changed) and len(changed) == 7 * cfg.num_hidden_layers
    for k in changed:                                   # half an e4m3 step of the row's amax-scaled values on top of the bf16 rounding
        w = W[k].to(BF).float()
        assert ((Wq[k] - w).abs() <= torch.maximum(w.abs() * 2.0 ** -4, w.abs().amax(-1, keepdim=True) / 448 * 2.0 ** -10) * 1.0001).all(), k
    emb, ids = A["embeds_bs1"], A["ids_bs1"]
    a = WR.mixed_steps(emb, W, Wq, cfg, ids)
    b = WR.mixed_steps(emb, W, Wq, cfg, ids)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    plain = WR.mixed_steps(emb, W, W, cfg, ids)
    assert torch.equal(a[:, 0], plain[:, 0])
    dev = (a[:, 1:] - plain[:, 1:]).abs().max().item() / plain.abs().max().item()
    print(f"full_tiny_llama bs1: FP8-weight decode steps vs bf16-weight steps, max logit deviation / logit scale = {dev:.3e}")
    assert 0 < dev < 0.25
    ref, bound = WR.mixed_bound(emb, W, cfg, ids)
    assert torch.equal(ref, a) and 0 < bound < 0.1
