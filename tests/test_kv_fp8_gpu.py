"""The opt-in FP8 (e4m3fn) KV cache on the GPU: the quantiser bit for bit against the torch statement of the format (tests/kv_fp8_ref.py), the
fp8 decode-attention kernel against fp32 arithmetic on the dequantised keys, and the engine's fp8 mode end to end."""
import json
import math
import os

import pytest
import torch

from tests import kv_fp8_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the bf16 decode-attention kernels are held to against fp32 arithmetic on the same operands (tests/test_ops_gpu.py TOL_BF16: one bf16
# storage rounding of the output on top of the accumulation order).  The arithmetic after dequantisation is the same fp32 arithmetic.
TOL_BF16 = 6e-3


def _rows_with_spread(n, d, seed, at=3):
    """n bf16 rows of d elements whose amax spans 1e-6 .. 1e4, plus a zero row, a row whose amax is a bf16 subnormal, a row holding bf16 max
    next to subnormals, and a row of one repeated value."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    mag = 10 ** (torch.rand(n, 1, generator=g) * 10 - 6)
    x = (x * mag).to(BF)
    x[at] = 0
    x[at + 1] = (torch.randn(d, generator=g) * 3e-40).to(BF)     # every element a bf16 subnormal (|x| < 1.18e-38)
    x[at + 2] = (torch.randn(d, generator=g) * 1e-39).to(BF)
    x[at + 2, 3] = torch.finfo(BF).max
    x[at + 3] = -0.3359375
    return x


@pytest.mark.parametrize("d,with_off", [(128, False), (128, True), (64, False), (64, True)])
def test_quantiser_equals_the_torch_statement_bit_for_bit(d, with_off):
    """crab_kv_quant_fp8 == kv_fp8_ref.quant: torch.equal on codes and scales, no tolerance.  A bf16 block [L, Bc, Hk, T_src, d] with live rows
    t0 .. t0 + S - 1 goes to sequences b0 .., slots t_dst .. of a larger cache; everything else in the cache (other sequences, other slots, the
    front padding of row_off) keeps its poison."""
    from crab_amd import ops
    L, Bc, Hk, Tsrc, t0, S = 2, 3, 2, 24, 3, 19
    B, Tmax, b0, t_dst = 5, 64, 1, 7
    ks = _rows_with_spread(L * Bc * Hk * Tsrc, d, 1).view(L, Bc, Hk, Tsrc, d)
    vs = _rows_with_spread(L * Bc * Hk * Tsrc, d, 2).flip(0).view(L, Bc, Hk, Tsrc, d).contiguous()
    off = torch.tensor([0, 5, 18], dtype=torch.int32) if with_off else None
    out = {}
    for nm, fill in (("kc", 0xAA), ("vc", 0x55)):
        out[nm] = torch.full((L, B, Hk, Tmax, d), fill, dtype=torch.uint8, device="cuda")
    out["ksc"] = torch.full((L, B, Hk, Tmax), -7.0, dtype=torch.float32, device="cuda")
    out["vsc"] = torch.full((L, B, Hk, Tmax), -9.0, dtype=torch.float32, device="cuda")
    with ops.launch_trace(0) as tr:
        ops.kv_quant_fp8(ks.cuda(), vs.cuda(), out["kc"], out["vc"], out["ksc"], out["vsc"], b0=b0, t0=t0, t_dst=t_dst, S=S,
                         row_off=off.cuda() if with_off else None)
    assert tr.launched(f"kv_quant_fp8_kernel<{d}>") == 1
    for src, cn, sn, cfill, sfill in ((ks, "kc", "ksc", 0xAA, -7.0), (vs, "vc", "vsc", 0x55, -9.0)):
        codes, scale = R.quant(src[:, :, :, t0:t0 + S])
        want_c = torch.full((L, B, Hk, Tmax, d), cfill, dtype=torch.uint8)
        want_s = torch.full((L, B, Hk, Tmax), sfill, dtype=torch.float32)
        for b in range(Bc):
            lo = int(off[b]) if with_off else 0
            want_c[:, b0 + b, :, t_dst + lo:t_dst + S] = codes[:, b, :, lo:]
            want_s[:, b0 + b, :, t_dst + lo:t_dst + S] = scale[:, b, :, lo:]
        got_c, got_s = out[cn].cpu(), out[sn].cpu()
        assert torch.equal(got_s, want_s), f"{sn}: {(got_s != want_s).sum().item()} scales differ"
        bad = (got_c != want_c)
        assert not bad.any(), f"{cn}: {bad.sum().item()} codes differ, first at {bad.nonzero()[0].tolist()}"
        assert torch.isfinite(R.dequant(codes, scale)).all()


def _fp8_cache(B, Hk, Tmax, d, seed):
    """A cache pre-filled through kv_fp8_ref from seeded bf16 rows (every slot: the kernel must not read the ones outside its context - they are
    poisoned below per case)."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(B, Hk, Tmax, d, generator=g) * 0.7).to(BF)
    v = (torch.randn(B, Hk, Tmax, d, generator=g) * 0.7).to(BF)
    v = v * (10 ** (torch.rand(B, Hk, Tmax, 1, generator=g) * 2 - 1)).to(BF)        # row scales that differ by up to 100 x
    kc, ksc = R.quant(k)
    vc, vsc = R.quant(v)
    return kc, ksc, vc, vsc


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("ctx", [1, 2, 15, 16, 17, 33, 830])
@pytest.mark.parametrize("H,Hk,d", [(32, 32, 128), (28, 4, 128), (8, 4, 64)])
def test_fp8_decode_attention_against_fp32_on_the_dequantised_keys(H, Hk, d, ctx, ragged):
    """crab_attn_decode_fp8 on a raw q|k|v row vs fp32 attention over the DEQUANTISED keys (the new row included, quantised by kv_fp8_ref), q and
    k rotated as oracle.apply_rope does, within the bound of the bf16 decode attention.  ctx counts the visible keys, the new one included.  The
    slot the kernel wrote equals kv_fp8_ref.quant of the bf16-rounded rotated k (as the bf16 path stores it: crab_qkv_rope_split) and of v bit
    for bit; every other slot keeps its contents.  launch_trace: the fp8 kernel ran, attn_decode_kernel did not."""
    from crab_amd import ops
    from oracle import crab_oracle as O
    B, Tmax, theta = 3, 896, 10000.0
    off = torch.tensor([0, 5, 40], dtype=torch.int32) if ragged else torch.zeros(B, dtype=torch.int32)
    pos = ctx - 1 + int(off.max())                                 # the append slot, shared by the rows; row b sees pos - off[b] + 1 keys
    assert pos < Tmax
    kc, ksc, vc, vsc = _fp8_cache(B, Hk, Tmax, d, 7 * ctx + H)
    g = torch.Generator().manual_seed(ctx + d)
    qkv = torch.randn(B, (H + 2 * Hk) * d, generator=g).to(BF)
    tab = ops.rope_table(Tmax, d, theta, "cuda")
    # poison what must not be read: slots below row_off and at / beyond pos (NaN codes, huge scales)
    kcp, vcp, kscp, vscp = kc.clone(), vc.clone(), ksc.clone(), vsc.clone()
    for b in range(B):
        for t in (kcp, vcp):
            t[b, :, :int(off[b])] = 0x7F
            t[b, :, pos:] = 0x7F
        for t in (kscp, vscp):
            t[b, :, :int(off[b])] = 3e30
            t[b, :, pos:] = 3e30
    dk, dv, dks, dvs = kcp.cuda(), vcp.cuda(), kscp.cuda(), vscp.cuda()
    o = torch.zeros(B, H * d, dtype=BF, device="cuda")
    pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
    offd = off.cuda() if ragged else None
    with ops.launch_trace(0) as tr:
        ops.attn_decode_fp8(qkv.cuda(), tab, dk, dv, dks, dvs, o, B, H, Hk, d, Tmax, 0, d ** -0.5, pos_dev=pd, kv_start=offd)
    assert tr.launched(f"attn_decode_fp8_kernel<{d}>") == 1
    assert not any(n.startswith("attn_decode_kernel") or n.startswith("attn_decode_gqa") or n.startswith("attn_decode_rope") for n in tr.counts)
    # ---- the appended slot: the bf16 rows the bf16 path stores (HIP rotation, bit-identical by construction of rope_lo / rope_hi), quantised on the CPU
    kb = torch.zeros(B, Hk, Tmax, d, dtype=BF, device="cuda")
    vb = torch.zeros_like(kb)
    ops.qkv_rope_split(qkv.cuda().clone(), tab, kb, vb, None, B, 1, H, Hk, d, Tmax, pos0=0, pos_dev=pd, row_off=offd)
    wk, wks = R.quant(kb[:, :, pos].cpu())
    wv, wvs = R.quant(vb[:, :, pos].cpu())
    gk, gv, gks, gvs = dk.cpu(), dv.cpu(), dks.cpu(), dvs.cpu()
    assert torch.equal(gk[:, :, pos], wk) and torch.equal(gks[:, :, pos], wks), "appended K codes / scale differ from kv_fp8_ref.quant"
    assert torch.equal(gv[:, :, pos], wv) and torch.equal(gvs[:, :, pos], wvs), "appended V codes / scale differ from kv_fp8_ref.quant"
    for got, before in ((gk, kcp), (gv, vcp), (gks, kscp), (gvs, vscp)):
        keep = torch.ones(Tmax, dtype=torch.bool)
        keep[pos] = False
        assert torch.equal(got[:, :, keep], before[:, :, keep]), "a slot other than pos changed"
    # ---- the attention: fp32 on the dequantised keys, rotation by the oracle
    G = H // Hk
    ref = torch.empty(B, H * d)
    for b in range(B):
        lo = int(off[b])
        p_ = torch.tensor([[pos - lo]])
        cos, sin = O.rope_cos_sin(p_, d, theta)
        q = qkv[b, :H * d].float().view(1, H, 1, d)
        k = qkv[b, H * d:(H + Hk) * d].float().view(1, Hk, 1, d)
        v = qkv[b, (H + Hk) * d:].view(1, Hk, 1, d)
        qr, kr = O.apply_rope(q, k, cos, sin)
        knew = R.roundtrip(kr.to(BF))
        vnew = R.roundtrip(v)
        K = torch.cat([R.dequant(kc[b, :, lo:pos], ksc[b, :, lo:pos])[None], knew], 2).repeat_interleave(G, 1)
        V = torch.cat([R.dequant(vc[b, :, lo:pos], vsc[b, :, lo:pos])[None], vnew], 2).repeat_interleave(G, 1)
        a = torch.softmax(torch.matmul(qr.to(BF).float(), K.transpose(2, 3)) * d ** -0.5, -1)
        ref[b] = torch.matmul(a, V).reshape(H * d)
    from tests.util import rel_err
    what = f"fp8 decode attention H={H} Hk={Hk} d={d} ctx={ctx} ragged={ragged}"
    r = rel_err(o, ref, what, TOL_BF16)
    print(f"{what}: rel err {r:.3e} (bound {TOL_BF16:.1e})")
    assert r <= TOL_BF16, f"{what}: relative max err {r:.4g} > {TOL_BF16:.4g}"


# ------------------------------------------------------------------------------------------------------------------ the engine's fp8 mode
FP8 = "fp8_e4m3"
_RECORDS = {}


def _record(key, value):
    """Numbers that are recorded, not asserted: into the parity report and, when CRAB_KV_FP8_PARITY_OUT names a file, into that JSON
    (profiles/kv_fp8_parity.json is such a file from one run)."""
    _RECORDS[key] = value
    print(f"[kv_fp8 record] {key}: {json.dumps(value)}")
    out = os.environ.get("CRAB_KV_FP8_PARITY_OUT")
    if out:
        have = {}
        if os.path.exists(out):
            with open(out) as f:
                have = json.load(f)
        have[key] = value
        with open(out, "w") as f:
            json.dump(have, f, indent=1, sort_keys=True)


def _tiny_model(fixture):
    from tests.util import build_tiny_crab, load_fixture, weights_from_table
    meta, A = load_fixture(fixture)
    model = build_tiny_crab(meta)
    r = model.load_state_dict(weights_from_table(meta), strict=False)
    assert not r.missing_keys, r.missing_keys[:4]
    return meta, A, model


def _oracle_parts(meta):
    from oracle import crab_oracle as O
    from tests.test_oracle_golden import _full_cfg
    from tests.util import stored_params, weights_from_table
    W = O.strip_peft_prefix(weights_from_table(meta))
    return W, stored_params(W), _full_cfg(meta)


def _gen(model, emb, n, **kw):
    r = model.generate(inputs_embeds=emb, use_cache=True, max_new_tokens=n, pad_token_id=2, eos_token_id=None, output_logits=True,
                       return_dict_in_generate=True, **kw)
    return r.sequences.cpu(), torch.stack(r.logits, 1).float().cpu()


@pytest.mark.parametrize("fixture", ["full_tiny_llama", "full_tiny_qwen"])
def test_tiny_generate_in_fp8_mode(fixture):
    """generate(kv_cache_dtype="fp8_e4m3") end to end on the reference-recorded tiny fixtures (bs 1 and the left-padded bs 2):
    (a) step-0 logits torch.equal to the bf16 mode's: prefill is untouched (it runs into the bf16 staging block);
    (b) per-step logits, on the contexts of the fixture's ids (steps up to the first id that departs from them), within
        bounds.FACTOR_VS_EMULATION x the distance between the fp32 oracle and the fp8-KV emulation of the oracle (tests/kv_fp8_emu.py:
        the stack's bf16-storage emulation with the KV rows passed through kv_fp8_ref), measured against that emulation;
    (c) graph replay == plain launches, the Python per-launch sequencer == the native one, a carried engine == a fresh engine, bit for bit;
        bf16 -> fp8 -> bf16 calls on one engine leave the bf16 results torch.equal to an engine that never saw fp8."""
    from crab_amd import decoder, ops
    from tests import bounds as PB
    from tests import kv_fp8_emu as E
    meta, A, model = _tiny_model(fixture)
    W, Ws, ocfg = _oracle_parts(meta)
    n = meta["new_tokens"]
    for key in ("bs1", "bs2"):
        emb = A[f"embeds_{key}"].to(BF).cuda()
        ids16, lg16 = _gen(model, emb, n)
        ids8, lg8 = _gen(model, emb, n, kv_cache_dtype=FP8)
        with ops.launch_trace(0) as tr:
            _gen(model, emb, n, kv_cache_dtype=FP8, use_graph=False)
        d, L = ocfg.decoder.head_dim, ocfg.decoder.num_hidden_layers
        # every decode step attends through the fp8 kernel; the bf16 decode kernel runs ONCE, inside the (bf16) prefill: the last layer's
        # last-row attention over the staging block (crab_llama_io.last_rows_only)
        assert tr.launched(f"attn_decode_fp8_kernel<{d}>") == L * (n - 1) and tr.launched(f"kv_quant_fp8_kernel<{d}>") == 1, tr.counts
        assert sum(v for k, v in tr.counts.items() if k.startswith(("attn_decode_kernel", "attn_decode_gqa", "attn_decode_rope"))) <= 1, tr.counts
        ids16b, lg16b = _gen(model, emb, n)
        assert torch.equal(ids16, ids16b) and torch.equal(lg16, lg16b), "a bf16 call after an fp8 call differs from the one before it"
        assert torch.equal(lg8[:, 0], lg16[:, 0]), "(a) first-token logits differ between the modes"
        assert torch.isfinite(lg8).all()
        # (c)
        ids8e, lg8e = _gen(model, emb, n, kv_cache_dtype=FP8, use_graph=False)
        assert torch.equal(ids8, ids8e) and torch.equal(lg8, lg8e), "HIP-graph replay differs from plain launches (fp8 mode)"
        decoder.NATIVE_LAYERS = False
        try:
            ids8p, lg8p = _gen(model, emb, n, kv_cache_dtype=FP8, use_graph=False)
        finally:
            decoder.NATIVE_LAYERS = True
        assert torch.equal(ids8, ids8p) and torch.equal(lg8, lg8p), "the Python per-launch sequence differs from the native one (fp8 mode)"
        # (b)
        ref_ids = A[f"ids_{key}"]
        ref, emu, dist = E.fp8_yardstick(A[f"embeds_{key}"], W, Ws, ocfg.decoder, ref_ids)
        scale = ref.abs().max().item()
        worst = worst16 = 0.0
        for b in range(ref_ids.shape[0]):
            for s in range(n):
                if s and not torch.equal(ids8[b, :s], ref_ids[b, :s]):
                    break
                worst = max(worst, (lg8[b, s] - emu[b, s]).abs().max().item() / scale)
                worst16 = max(worst16, (lg16[b, s] - ref[b, s]).abs().max().item() / scale)
        from tests.util import record_parity
        record_parity(f"{fixture} {key}: fp8-KV generate, per-step logits vs the fp8-KV emulation of the oracle", worst * scale, scale,
                      PB.FACTOR_VS_EMULATION * dist, emulation_vs_fp32=dist, bf16_mode_vs_fp32=worst16)
        print(f"{fixture} {key}: HIP fp8 vs emulation {worst:.3e}; emulation vs fp32 {dist:.3e}; bound {PB.FACTOR_VS_EMULATION * dist:.3e}; bf16 mode vs fp32 {worst16:.3e}")
        assert worst <= PB.FACTOR_VS_EMULATION * dist, (fixture, key, worst, dist)
    # a fresh engine, fp8 only, and one that never saw fp8
    emb = A["embeds_bs2"].to(BF).cuda()
    carried8 = _gen(model, emb, n, kv_cache_dtype=FP8)
    carried16 = _gen(model, emb, n)
    _, _, fresh = _tiny_model(fixture)
    fresh8 = _gen(fresh, emb, n, kv_cache_dtype=FP8)
    _, _, never = _tiny_model(fixture)
    never16 = _gen(never, emb, n)
    assert torch.equal(carried8[0], fresh8[0]) and torch.equal(carried8[1], fresh8[1]), "carried engine differs from a fresh engine (fp8)"
    assert torch.equal(carried16[0], never16[0]) and torch.equal(carried16[1], never16[1]), "bf16 results changed on an engine that saw fp8"
    # the engine-level switch is the same switch
    um = fresh.base_model.model
    um._engine.kv_cache_dtype = FP8
    again = _gen(fresh, emb, n)
    assert torch.equal(again[0], fresh8[0]) and torch.equal(again[1], fresh8[1])


@pytest.mark.parametrize("fixture", ["full_tiny_llama", "full_tiny_qwen"])
def test_coalesced_batches_in_fp8_mode(fixture):
    """generate_many(coalesce=True, kv_cache_dtype="fp8_e4m3") of groups with different prompt lengths, both prefill forms of a ragged wave (per
    group: the quantiser's t_dst; merged: its row_off): graph replay == plain launches == the Python sequencer bit for bit, and every group
    agrees with its own generate() call in fp8 mode as the bf16 test of that property holds it (tests/test_model_gpu.py
    test_coalesced_batches_match_the_reference_fixture_per_batch): NOT bit for bit in either mode - the rows of a wave go through the
    projection kernels the coalesced M selects (measured here: 5e-3 .. 7e-3 absolute on the logits) - but ids wherever the margin exceeds
    twice the logit difference, and logits within 2 x FACTOR_VS_EMULATION x the fp8-emulation distance (both runs lie within
    FACTOR_VS_EMULATION x that distance of the emulation, test_tiny_generate_in_fp8_mode: triangle inequality)."""
    from crab_amd import decoder
    from tests import bounds as PB
    from tests import kv_fp8_emu as E
    meta, A, model = _tiny_model(fixture)
    W, Ws, ocfg = _oracle_parts(meta)
    dist = max(E.fp8_yardstick(A[f"embeds_{k}"], W, Ws, ocfg.decoder, A[f"ids_{k}"])[2] for k in ("bs1", "bs2"))
    eng = model.base_model.model._engine
    n = meta["new_tokens"]
    e1, e2 = A["embeds_bs1"].to(BF).cuda(), A["embeds_bs2"].to(BF).cuda()
    embeds = [e1, e2, e1[:, 3:].contiguous()]
    assert len({e.shape[1] for e in embeds}) >= 2
    kw = dict(eos_token_id=None, pad_token_id=2, coalesce=True, return_step_logits=True, kv_cache_dtype=FP8)
    solo = [eng.generate(e, n, eos_token_id=None, pad_token_id=2, return_step_logits=True, kv_cache_dtype=FP8) for e in embeds]
    saved = decoder.RAGGED_PAD_MAX
    try:
        for pad_max, form in ((0.0, "per_group"), (0.5, "merged")):
            decoder.RAGGED_PAD_MAX = pad_max
            res = eng.generate_many(embeds, n, **kw)
            assert eng.last_ragged_prefill == form
            res_eager = eng.generate_many(embeds, n, use_graph=False, **kw)
            decoder.NATIVE_LAYERS = False
            try:
                res_py = eng.generate_many(embeds, n, use_graph=False, **kw)
            finally:
                decoder.NATIVE_LAYERS = True
            for g, ((i1, l1), (i2, l2), (i3, l3)) in enumerate(zip(res, res_eager, res_py)):
                assert torch.equal(i1, i2) and torch.equal(l1, l2), "HIP-graph replay of the ragged fp8 step differs from plain launches"
                assert torch.equal(i1, i3) and torch.equal(l1, l3), f"the Python per-launch sequence differs from the native one ({form} prefill, fp8)"
                si, sl = solo[g][0].cpu(), solo[g][1].float().cpu()
                gi, gl = i1.cpu(), l1.float().cpu()
                scale = sl.abs().max().item()
                top2 = sl.topk(2, -1).values
                margin = top2[..., 0] - top2[..., 1]
                worst = 0.0
                for b in range(si.shape[0]):
                    for s_ in range(n):
                        err = (gl[b, s_] - sl[b, s_]).abs().max().item()
                        worst = max(worst, err)
                        if gi[b, s_] != si[b, s_]:
                            assert margin[b, s_] <= 2 * err, (form, g, b, s_, margin[b, s_].item(), err)
                            break
                print(f"{fixture} {form} group {g}: coalesced vs own call, max |dlogit| / scale {worst / scale:.3e} (bound {2 * PB.FACTOR_VS_EMULATION * dist:.3e})")
                assert worst / scale <= 2 * PB.FACTOR_VS_EMULATION * dist, (form, g, worst / scale, dist)
    finally:
        decoder.RAGGED_PAD_MAX = saved
    assert eng.kv_cache_dtype == "bf16"


def _clip_inputs(meta, i):
    from crab_amd import synth
    c, nt = meta["clips"][i], meta["prompt_tokens"][i]
    ids = synth.synth_prompt_ids(nt, meta["base_vocab"], meta["special"], seed=meta["seed"], clip=c)
    mods = [{'<video>': synth.synth_video(meta["t_v"], seed=meta["seed"], clip=c), '<audio>': synth.synth_audio(meta["t_a"], meta["l_a"], seed=meta["seed"], clip=c)}]
    return ids, mods


def _emulated_distances(fixture):
    """Per clip and step: max |fp8-KV emulation of the oracle - fp32 oracle| over the vocabulary, teacher-forced on the reference's ids, on the
    oracle's own inputs_embeds of the clip (CPU only)."""
    from oracle import crab_oracle as O
    from tests import kv_fp8_emu as E
    from tests.util import load_fixture
    meta, A = load_fixture(fixture)
    W, Ws, ocfg = _oracle_parts(meta)
    dist = torch.zeros_like(A["margin"])
    for i in range(len(meta["clips"])):
        ids, mods = _clip_inputs(meta, i)
        emb = O.prepare_multimodal_inputs([ids], mods, W, ocfg)["inputs_embeds"]
        ref, emu, _ = E.fp8_yardstick(emb, W, Ws, ocfg.decoder, A["ids"][i:i + 1])
        dist[i] = (emu - ref).abs().amax(-1)[0]
    return meta, A, dist


def sharp_exemptions(fixture):
    """(exempt [clips, steps] bool, number of steps, largest distance): the steps the margin rule of the token-id test does not hold to the
    reference's id - recorded margin <= 2 x the fp8-emulated oracle's logit distance from fp32 at that step."""
    meta, A, dist = _emulated_distances(fixture)
    return A["margin"] <= 2 * dist, A["margin"].numel(), float(dist.max())


@pytest.mark.parametrize("fixture", ["sharp_tiny_llama", "id_stats_tiny_llama"])
def test_token_ids_in_fp8_mode(fixture):
    """Greedy ids of the reference-recorded clips (sharp_tiny_llama: 8 clips whose margins are >= 10 x the bf16 logit error; id_stats_tiny_llama:
    24 unsearched clips), one clip per generate(), fp8 and bf16 mode side by side.  REPORTED: the share of steps whose greedy id equals the
    reference's.  ASSERTED: every step (on the reference's context) whose recorded margin exceeds twice the fp8-emulated oracle's logit distance
    from fp32 at that step has the reference's id; the rule may exempt at most half of sharp_tiny_llama's steps ("fixture too soft" otherwise)."""
    meta, A, dist = _emulated_distances(fixture)
    exempt = A["margin"] <= 2 * dist
    if fixture == "sharp_tiny_llama":
        assert int(exempt.sum()) * 2 <= exempt.numel(), "fixture too soft"
    _, _, model = _tiny_model(fixture)
    n = meta["new_tokens"]
    same = {"bf16": 0, FP8: 0}
    prefix = {"bf16": 0, FP8: 0}
    for i in range(len(meta["clips"])):
        ids, mods = _clip_inputs(meta, i)
        b = dict(batch_input_ids=[ids], batch_labels=[torch.full_like(ids, -100)], batch_X_modals=mods, batch_task_names=['avqa'])
        for mode in ("bf16", FP8):
            got = model.generate(**b, use_cache=True, max_new_tokens=n, pad_token_id=2, eos_token_id=None, kv_cache_dtype=mode)[0].cpu()
            eq = got == A["ids"][i]
            same[mode] += int(eq.sum())
            k = n if bool(eq.all()) else int((~eq).nonzero()[0])
            prefix[mode] += k
            if mode == FP8 and k < n:                              # step k ran on the reference's context and chose another id
                assert bool(exempt[i, k]), (f"clip {meta['clips'][i]} step {k}: id {int(got[k])} vs the reference's {int(A['ids'][i, k])} although its margin "
                                            f"{A['margin'][i, k].item():.4f} exceeds twice the fp8-emulation distance {dist[i, k].item():.4f}")
    total = exempt.numel()
    _record(f"token_ids/{fixture}", {"steps": total, "exempt_by_margin_rule": int(exempt.sum()),
                                      "share_equal_fp8": round(same[FP8] / total, 4), "share_equal_bf16": round(same["bf16"] / total, 4),
                                      "share_before_first_divergence_fp8": round(prefix[FP8] / total, 4),
                                      "share_before_first_divergence_bf16": round(prefix["bf16"] / total, 4),
                                      "largest_emulated_distance": round(float(dist.max()), 5), "smallest_margin": round(float(A["margin"].min()), 5)})


def test_reference_layer_decode_steps_through_the_fp8_path():
    """llama_layer_wide.npz (a Llama-2-7B-wide hyper-LoRA layer recorded from the reference: y_steps of its cached one-token steps, cache_k /
    cache_v of its last sequence): the prefilled bf16 cache is quantised by crab_kv_quant_fp8 and the reference's decode steps run through the
    fp8 layer path.  RECORDED beside the bf16 path's value and the bf16-operand floor of the same rows: |y - y_ref| / max |y_ref| per step, and
    the distance of the dequantised cache rows from the reference's own, next to kv_fp8_ref's round trip of those reference rows."""
    from crab_amd import ops
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    from oracle import crab_oracle as O
    from tests.util import load_fixture, weights_from_table, wide_layer_inputs
    meta, A = load_fixture("llama_layer_wide")
    c = dict(meta["cfg"])
    c.update(num_hidden_layers=1, vocab_size=320, pad_token_id=2)
    model = get_peft_model(UnifiedForCausalLM(UnifiedConfig(**c), device="cuda"), LoraConfig())
    Wt = weights_from_table(meta)
    model.load_state_dict({"base_model.model." + k_: v for k_, v in Wt.items()}, strict=False)
    eng = model.base_model.model._engine
    x, xs = wide_layer_inputs(meta)
    B, S, D = x.shape
    steps, Tmax = len(xs), S + 8
    seqs = A["step_seqs"]
    scale = A["y_rows"].abs().max().item()
    # the bf16-operand floor of the same steps (oracle on the GPU, fp32 arithmetic)
    torch.backends.cuda.matmul.allow_tf32 = False
    ocfg = O.DecoderConfig(**{**meta["cfg"], "num_hidden_layers": 1, "vocab_size": 320})
    Wd = {k_: v.cuda() for k_, v in Wt.items()}
    cache = O.KVCache()
    O.decoder_layer(x.cuda(), Wd, 0, ocfg, cache, torch.arange(S, device="cuda")[None].expand(B, S), emulate=O.OPERANDS)
    floor = [O.decoder_layer(x1.cuda(), Wd, 0, ocfg, cache, torch.full((B, 1), S + t, device="cuda"), emulate=O.OPERANDS)[seqs.cuda(), 0].cpu()
             for t, x1 in enumerate(xs)]
    del Wd, cache
    kc, vc = eng.alloc_cache(B, Tmax)
    eng.prefill(x.to(BF).cuda(), kc, vc, b0=0, all_logits=True)
    eng.kv_cache_dtype = FP8
    k8, v8, ks, vs = eng.alloc_cache(B, Tmax)
    eng.kv_cache_dtype = "bf16"
    ops.kv_quant_fp8(kc, vc, k8, v8, ks, vs, S=S)
    ws = eng._workspace(B)
    rows = []
    for t in range(steps):
        posd = torch.full((1,), S + t, device="cuda", dtype=torch.int32)
        ops.cast_rows(xs[t][:, 0].to(BF).cuda().contiguous(), ws.x, B, D)
        xo, _ = eng._layers(ws, B, 1, kc, vc, 0, Tmax, 0, posd, None)
        y16 = xo[:B].float()[seqs.cuda()].cpu()
        ops.cast_rows(xs[t][:, 0].to(BF).cuda().contiguous(), ws.x, B, D)
        with ops.launch_trace(0) as tr:
            xo, _ = eng._layers(ws, B, 1, k8, v8, 0, Tmax, 0, posd, None, kv_scales=(ks, vs))
        assert tr.launched("attn_decode_fp8_kernel<128>") == 1 and tr.launched("attn_decode_kernel<128>") == 0, tr.counts
        y8 = xo[:B].float()[seqs.cuda()].cpu()
        assert torch.isfinite(y8).all()
        err = lambda y: (y - A["y_steps"][t]).abs().max().item() / scale
        rows.append({"step": t, "fp8": err(y8), "bf16": err(y16), "bf16_operand_floor": err(floor[t])})
    heads = meta["cache_heads"]
    cache_rows = {}
    for nm, codes, sc, ref in (("K", k8, ks, A["cache_k"]), ("V", v8, vs, A["cache_v"])):
        got = R.dequant(codes[0, B - 1, heads, :S + steps].cpu(), sc[0, B - 1, heads, :S + steps].cpu())
        m = ref.abs().max().item()
        cache_rows[nm] = {"hip_fp8_cache_vs_reference_rows": (got - ref).abs().max().item() / m,
                          "kv_fp8_ref_round_trip_of_reference_rows": (R.roundtrip(ref.to(BF)) - ref).abs().max().item() / m}
    _record("reference_layer/llama_layer_wide", {"decode_steps_rel_err_vs_y_ref": rows, "cache_rows_rel_err": cache_rows, "rows": int(B)})


def test_full_size_fp8_vs_bf16_mode():
    """The 32-layer Llama-2-7B-size hyper-LoRA decoder, 8 sequences of 702 rows, 16 greedy steps, this library's fp8 mode against its bf16 mode:
    the largest per-step logit distance relative to the logit scale over the steps both modes decode on the same context, RECORDED beside the
    bf16-operand floor of this stack (3.4e-3, tests/test_fullsize_gpu.py).  Asserted: finite logits, and the step-0 equality (prefill is
    untouched)."""
    from crab_amd.build_model import build_crab
    crab = build_crab("llama", visual=False, audio=False, conditioned=True)
    um = crab.base_model.model
    g = torch.Generator(device="cuda").manual_seed(41)
    emb = torch.randn(8, 702, um.config.hidden_size, device="cuda", generator=g).to(BF)
    ids16, lg16 = _gen(um, emb, 16)
    ids8, lg8 = _gen(um, emb, 16, kv_cache_dtype=FP8)
    assert torch.isfinite(lg8).all() and torch.isfinite(lg16).all()
    assert torch.equal(lg8[:, 0], lg16[:, 0]) and torch.equal(ids8[:, 0], ids16[:, 0]), "first-token logits differ between the modes"
    scale = lg16.abs().max().item()
    worst, steps = 0.0, 0
    for b in range(8):
        for s in range(16):
            if s and not torch.equal(ids8[b, :s], ids16[b, :s]):
                break
            worst = max(worst, (lg8[b, s] - lg16[b, s]).abs().max().item())
            steps += 1
    _record("full_size/llama_32_layers_8x702_16_steps", {"max_logit_distance_fp8_vs_bf16_mode_rel": worst / scale, "steps_on_the_same_context": steps,
                                                          "steps": 128, "ids_equal": int((ids8 == ids16).sum()), "bf16_operand_floor_rel": 3.4e-3})
    del crab, um
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ fixed points of scripts/fuzz_kv_fp8.py
def _fuzzer():
    """A fresh instance of scripts/fuzz_kv_fp8.py (its failure list is module state): the fixed cases below run through the fuzzer's own checks."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_kv_fp8", os.path.join(ROOT, "scripts", "fuzz_kv_fp8.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fp8_entry_points_refuse_what_they_document():
    """Every documented refusal of crab_kv_quant_fp8 / crab_attn_decode_fp8 and of their wrappers (head_dim 32, H % Hk != 0, pos0 outside the
    cache, misaligned code / source / q|k|v pointers, an odd row stride, t0 + S > T_src, t_dst + S > Tmax, S = 0, b0 outside the cache, wrong
    dtypes and shapes): the call raises with the stated message and codes, scales and output keep their contents.  Host-side checks only."""
    F = _fuzzer()
    F.run_rejections()
    assert not F.bad, F.bad
    assert F.stats["A_reject"] == 21, (F.stats, F.why)
    assert sum(F.why.values()) == 21 and any("position outside the KV cache" in k for k in F.why), F.why


@pytest.mark.parametrize("count", [31, 32, 33, 63, 64, 65, 66, 95, 96, 97, 98, 127, 128, 129, 130])
@pytest.mark.parametrize("Hk,G,d", [(4, 1, 64), (4, 7, 128)])
def test_fp8_decode_attention_at_the_group_and_prefetch_boundaries(Hk, G, d, count):
    """crab_attn_decode_fp8 at the cached-key counts around its structural edges (32 groups, a pair of keys per trip, the two-deep prefetch), one
    MHA and one G = 7 geometry, on a cache whose K row scales spread over 1e-2 .. 1e2 and V row scales over 1e-3 .. 1e3 (the two keys of a pair
    carry very different scales), Tmax = 200, q|k|v and output rows with padded strides, the slot given as pos0 alone / pos_dev alone / both
    non-zero, ragged rows beside the full one: appended codes and scales torch.equal to kv_fp8_ref.quant of the rows crab_qkv_rope_split stores,
    every other slot and every guard unchanged, the output within TOL_BF16 of fp64 attention over the dequantised rows PER (sequence, head)."""
    F = _fuzzer()
    assert F.TOL_BF16 == TOL_BF16
    B, slot = 3, count + (2 if count % 2 else 0)
    ks = [slot - count, 0, min(40, slot)]
    form = F.POS_FORMS[count % 3]
    case = dict(B=B, Hk=Hk, G=G, d=d, Tmax=200, slot=slot, kv_start=ks if any(ks) else None, counts=[slot - k for k in ks], pos_form=form,
                pos0=slot if form == "pos0" else 0 if form == "pos_dev" else 17, pad_q=8 if count % 2 else 0, pad_o=64 if count % 4 < 2 else 0,
                new_k=["plain", "dominant", "zero", "subnormal"][count % 4], new_v=["plain", "zero", "dominant", "subnormal"][(count // 4) % 4], seed=count)
    F.run_attn(case)
    print(f"fp8 decode attention Hk={Hk} G={G} d={d} count={count} {form}: worst rel err per head {F.stats['worst_attn']:.3e} (bound {TOL_BF16:.1e})")
    assert F.stats["A_attn"] == 1 and not F.bad, F.bad


def test_chunked_prefill_fills_the_fp8_cache_like_the_bf16_one():
    """generate(prefill_chunk=2) of 5 sequences in fp8 mode (chunks of 2, 2 and 1 sequences: the staging block reused, the quantiser writing at
    b0 = 2 and 4): first-token logits torch.equal to the bf16 mode's, and afterwards the codes and scales of every prompt slot of every layer and
    sequence torch.equal to kv_fp8_ref.quant of the cache rows the bf16 mode leaves under the same chunking - prefill is the same arithmetic in
    both modes and the quantiser is pinned bit for bit, so a row landing in another sequence / slot / layer shows here."""
    from crab_amd import ops
    F = _fuzzer()
    meta, A, model = _tiny_model("full_tiny_llama")
    eng = model.base_model.model._engine
    e2 = A["embeds_bs2"].to(BF)
    emb = torch.cat([e2, (e2.float() * 0.5).to(BF), -e2[:1]]).cuda()
    assert emb.shape[0] == 5
    n, d = 4, eng.cfg.head_dim
    kw = dict(eos_token_id=None, pad_token_id=2, prefill_chunk=2, return_step_logits=True)
    eng._dec.clear()
    ids16, lg16 = eng.generate(emb, n, kv_cache_dtype="bf16", **kw)
    lg16 = lg16.clone()
    s16 = F.snapshot(eng)
    eng._dec.clear()
    with ops.launch_trace(0) as tr:
        ids8, lg8 = eng.generate(emb, n, kv_cache_dtype=FP8, **kw)
    assert tr.launched(f"kv_quant_fp8_kernel<{d}>") == 3, tr.counts
    s8 = F.snapshot(eng)
    assert torch.equal(lg16[:, 0], lg8[:, 0]), "first-token logits differ between the modes"
    assert list(s16) == [0] and s16[0][0] == emb.shape[1] and len(s8[0][2]) == 4
    assert F.cache_mismatch(s16, s8) is None, F.cache_mismatch(s16, s8)
    # the check sees a row in the wrong sequence: swap two sequences of the fp8 snapshot
    perm = [1, 0, 2, 3, 4]
    swapped = {0: (s8[0][0], s8[0][1], [t[:, perm] for t in s8[0][2]])}
    assert F.cache_mismatch(s16, swapped) is not None
    assert eng.kv_cache_dtype == "bf16"
