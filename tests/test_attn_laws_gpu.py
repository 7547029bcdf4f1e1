"""Every attention kernel under the peaked, sink and shifted score laws of tests/attn_laws.py: an fp64 reference on the same bf16 operands
(fuzz_bounds.attn_ref), EVERY output element held to fuzz_bounds.attn_bound_weighted (whose fp32 slack must itself pass its cap), a second run for
bit equality, and the launch trace naming the instantiation that ran.  No tolerance literal lives here (tests/test_fuzz_bounds_host.py pins that).

Slots a kernel must not read hold NaN.  Two exceptions, both stronger than NaN for what they test: a hidden key that carries the PEAK (the last
key under kv_start, the keys a key_mask hides, the key one past a verify row's limit) holds a real row whose score would dominate and whose V row
is 64 x louder - a kernel that let it in is wrong per element, not merely non-finite; and the hidden V rows of crab_attn_fwd are finite (64 x
louder too): its P.V runs on the matrix pipe over whole tiles, where an exact 0 probability times NaN is NaN by IEEE, not by a defect.

The worst err / bound per kernel and law is printed (pytest -s) and, when CRAB_ATTN_LAWS_OUT names a file, written there as JSON
(profiles/README.md quotes one run); nothing is asserted against those figures."""
import json
import math
import os

import pytest
import torch

from crab_amd import ops
from tests import attn_laws as AL
from tests import fuzz_bounds as FB
from tests import kv_fp8_ref as R8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F64 = torch.bfloat16, torch.float64
SENT, GUARD = 12345.0, 8
WGUARD = 4096                                                       # guard bytes on either side of a workspace
WORST = {}


def _note(kernel, law, ratio):
    key = f"{kernel} {law}"
    if ratio > WORST.get(key, -1.0):
        WORST[key] = ratio
        out = os.environ.get("CRAB_ATTN_LAWS_OUT")
        if out:
            have = {}
            if os.path.exists(out):
                with open(out) as f: have = json.load(f)
            have[key] = max(ratio, have.get(key, 0.0))
            with open(out, "w") as f: json.dump(have, f, indent=1, sort_keys=True)


def _judge(kernel, law, desc, kind, got, q4, k, v, scale, allow, bias=None, gate=None):
    """got / q4 [B, H, Sq, d] against the fp64 reference on (q4, k, v) - k / v clean (no NaN) - every element."""
    ref, bound, rel = FB.attn_bound_weighted(q4, k, v, scale, allow, bias, gate, kind=kind)
    assert rel <= FB.LAW_SLACK_CAP, f"{kernel} {desc}: the derived fp32 slack is {rel / FB.LAW_SLACK_CAP:.3f} of its cap"
    ratio, idx = FB.worst(got, ref, bound)
    _note(kernel, law, ratio)
    assert ratio <= 1.0, f"{kernel} {desc}: err / bound {ratio:.3f} at (b, h, row, e) = {idx}"
    return ratio


def _report(kernel):
    rows = {k: v for k, v in WORST.items() if k.startswith(kernel + " ")}
    print(f"\n{kernel}: worst err / bound per law: " + ", ".join(f"{k[len(kernel) + 1:]} {v:.3f}" for k, v in sorted(rows.items())))


def _inputs(law, R, d, B, H, Hk, Sq, T, vis, loud, seed, t=None, allow=None):
    """q [B, H, Sq, d], k / v [B, Hk, T, d] (bf16, clean) under the law spread over the visible slots vis [B, T] (or the given t [B, T])."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale = d ** -0.5
    t = AL.spread(law, R, vis) if t is None else t
    q, k = AL.plant(AL.draw((B, H, Sq, d), g, DEV), AL.draw((B, Hk, T, d), g, DEV), t[:, None], scale)
    v = AL.draw((B, Hk, T, d), g, DEV).to(BF)
    allow = vis[:, None, None, :] if allow is None else allow
    if loud: v = AL.loud_tail(v, FB.attn_ref(q, k, v, scale, allow)[1])
    return q, k, v, scale, allow


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _slots(B, T):
    return torch.arange(T, device=DEV)[None].expand(B, T)


def _guarded(rows, cols):
    obuf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=BF, device=DEV)
    return obuf, obuf[GUARD:GUARD + rows]


def _guards_ok(obuf, rows):
    return bool((obuf[:GUARD] == SENT).all()) and bool((obuf[GUARD + rows:] == SENT).all())


def _twice(names, run):
    """run() -> output, twice inside one launch trace: the named kernels ran (each once per call, nothing else), the outputs are bit-equal."""
    with ops.launch_trace(0) as tr:
        a = run()
        b = run()
    assert tr.counts == {n: 2 for n in names}, tr.counts
    assert torch.equal(a, b), "a second run differs"
    return a


# ----------------------------------------------------------------------------------------------------- crab_attn_decode / _masked / _keymask
def _decode(names, q, kp, vp, B, H, Hk, d, Tmax, ctx, scale, word, **kw):
    q2 = q.reshape(B, H * d)

    def run():
        obuf, o = _guarded(B, H * d)
        if word: ops.attn_decode(q2, kp, vp, o, B, H, Hk, d, Tmax, 1, scale, ctx_dev=_i32([ctx - 1]), **kw)
        else: ops.attn_decode(q2, kp, vp, o, B, H, Hk, d, Tmax, ctx, scale, **kw)
        torch.cuda.synchronize()
        assert _guards_ok(obuf, B), "a store landed outside the output"
        return o.clone()
    return _twice(names, run).view(B, H, 1, d)


@pytest.mark.parametrize("d", (64, 128))
def test_decode_and_kv_start(d):
    """attn_decode_kernel<d>: B = 3, Hk = 2, G = 1; every law x R at contexts 1, 16, 17, 33, 65, 830; host and device context word; without
    kv_start and with it (the profile runs over the visible keys: its peak is the FIRST visible key under sink / ramp_down); then the peak on the
    LAST HIDDEN key (slot kv_start - 1: a real, dominant, loud row)."""
    B, Hk, H = 3, 2, 2
    name = f"attn_decode_kernel<{d}>"
    i = 0
    for ctx in (1, 16, 17, 33, 65, 830):
        Tmax = (ctx + 8) // 8 * 8
        for R in AL.heights(d):
            for law in AL.NAMES:
                i += 1
                vis = _slots(B, Tmax) < ctx
                ks = None
                if i % 2 and ctx > 1:
                    ks = _i32([0, ctx // 2, ctx - 1])
                    vis = vis & (_slots(B, Tmax) >= ks[:, None])
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, bool(i & 4), i)
                got = _decode([name], q, AL.poison(k, vis), AL.poison(v, vis), B, H, Hk, d, Tmax, ctx, scale, bool(i & 2), kv_start=ks)
                _judge(name, law, f"{law} R={R} ctx={ctx} kv_start={'yes' if ks is not None else 'no'} word={bool(i & 2)}", "decode", got, q, k, v, scale, allow)
        if ctx < 17: continue
        for R in AL.heights(d):
            for law in ("sink", "ramp_up"):
                i += 1
                ks = _i32([1, ctx // 2, ctx - 1])
                sl = _slots(B, Tmax)
                vis = (sl < ctx) & (sl >= ks[:, None])
                hid = sl == ks[:, None] - 1
                t = AL.spread(law, R / 2, vis) + R * hid                                   # the hidden key stands R / 2 above the visible peak
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, False, i, t=t)
                v = torch.where(hid[:, None, :, None], v.float() * AL.LOUD, v.float()).to(BF)
                got = _decode([name], q, AL.poison(k, vis | hid), AL.poison(v, vis | hid), B, H, Hk, d, Tmax, ctx, scale, bool(i & 2), kv_start=ks)
                _judge(name, "hidden_peak", f"peak on the last hidden key, {law} R={R} ctx={ctx}", "decode", got, q, k, v, scale, allow)
    _report(name)


@pytest.mark.parametrize("G", (2, 4, 7, 8))
def test_decode_gqa(G):
    """attn_decode_gqa_kernel<128, G> (taken from B Hk >= 256: B = 64, Hk = 4) at contexts 17, 65, 300: the nine laws in turn over (context, R),
    each law at both R; kv_start on every other case.  The kernel walks the keys in chunks of 512 and rescales once per chunk, so contexts up to
    300 never reach its m_old / m_new step: context 830 does, under the laws whose maximum rises (ramp_up, last) or recurs (two) in the second chunk."""
    B, Hk, d = 64, 4, 128
    H = Hk * G
    name = f"attn_decode_gqa_kernel<128,{G}>"
    i = 0
    for ctx in (17, 65, 300, 830):
        Tmax = (ctx + 8) // 8 * 8
        for R in AL.heights(d) if ctx < 512 else (40,):
            for n in range(3):
                law = AL.NAMES[(i + G) % len(AL.NAMES)] if ctx < 512 else ("ramp_up", "last", "two")[n]
                i += 1
                vis = _slots(B, Tmax) < ctx
                ks = None
                if i % 2:
                    ks = _i32([(7 * b) % ctx for b in range(B)])
                    vis = vis & (_slots(B, Tmax) >= ks[:, None])
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, bool(i & 4), 100 * G + i)
                got = _decode([name], q, AL.poison(k, vis), AL.poison(v, vis), B, H, Hk, d, Tmax, ctx, scale, bool(i & 2), kv_start=ks)
                _judge(name, law, f"{law} R={R} ctx={ctx} kv_start={'yes' if ks is not None else 'no'}", "decode", got, q, k, v, scale, allow)
    _report(name)


@pytest.mark.parametrize("d", (64, 128))
def test_decode_keymask(d):
    """attn_decode_keymask_kernel<d>, context 130: (a) the mask hides the law's peak keys (and a random 30 %): the runner-up takes over; (b) the mask
    hides keys 0 .. 69 - a whole first tile and more - with the sink peak among them; (c) the mask leaves ONE key visible.  Hidden keys inside the
    context are real rows (the profile runs over ALL keys of the context) with loud V rows; slots past the context are NaN."""
    B, Hk, H, ctx, Tmax = 3, 2, 4, 130, 136
    name = "attn_decode_keymask"
    i = 0
    sl = _slots(B, Tmax)
    inctx = sl < ctx
    for R in AL.heights(d):
        for law in AL.NAMES:
            for form in ("peak", "tile", "one"):
                if form != "peak" and law not in ("sink", "ramp_down", "last", "shift_neg"): continue
                i += 1
                g = torch.Generator(device=DEV).manual_seed(i)
                t = AL.spread(law, R, inctx)
                if form == "peak":
                    vis = inctx & (torch.rand(B, Tmax, device=DEV, generator=g) > 0.3) & ~(t >= t.amax(1, keepdim=True))
                    if law in AL.SHIFTS: vis = inctx & (torch.rand(B, Tmax, device=DEV, generator=g) > 0.3)
                    vis[:, 77] = True
                elif form == "tile":
                    vis = inctx & (sl >= 70)
                else:
                    vis = sl == _i32([0, 77, ctx - 1])[:, None]
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, False, 1000 + i, t=t)
                v = torch.where((inctx & ~vis)[:, None, :, None], v.float() * AL.LOUD, v.float()).to(BF)
                word = bool(i & 1)
                got = _decode([name], q, AL.poison(k, inctx), AL.poison(v, inctx), B, H, Hk, d, Tmax, ctx, scale, word, key_mask=ops.pack_key_mask(vis))
                _judge(f"{name}<{d}>", law, f"{law} R={R} mask form {form} word={word}", "decode", got, q, k, v, scale, allow)
    _report(f"{name}<{d}>")


# ------------------------------------------------------------------------------------------------------------------- crab_attn_decode_rope
def _zero_angle_table(Tmax, d):
    tab = torch.zeros((Tmax, d // 2, 2), dtype=torch.float32, device=DEV)
    tab[..., 0] = 1.0                                                                     # cos 1, sin 0: q and the appended k reach the softmax as planted
    return tab


ROPE_GEOM = [  # (d, B, H, Hk, kernel, splits)
    (128, 1, 32, 32, "attn_decode_rope_kernel<128>", 8),
    (128, 8, 32, 8, "attn_decode_rope_kernel<128,32>", 1),       # the dispatcher's two splits run as ONE block of 32 key groups
    (128, 16, 32, 32, "attn_decode_rope_kernel<128>", 1),
    (64, 3, 4, 2, "attn_decode_rope_kernel<64>", 8),
    (64, 16, 32, 8, "attn_decode_rope_kernel<64>", 1),
]


@pytest.mark.parametrize("d,B,H,Hk,name,splits", ROPE_GEOM, ids=[f"d{g[0]}-B{g[1]}-H{g[2]}k{g[3]}" for g in ROPE_GEOM])
def test_decode_rope_splits(d, B, H, Hk, name, splits):
    """crab_attn_decode_rope with a zero-angle rotary table at 8 splits, the 32-group block and one split: laws two, ramp_up, last (the peak is the
    key appended in this very call) and sink at positions 3 (fewer keys than splits: empty splits), 64 and 300, and at position 300 the peak in each
    of the 8 split ranges in turn.  The appended cache rows equal the planted ones; workspace guards and tickets are checked."""
    i = 0
    nb = ops.attn_decode_rope_bytes(B, H, d)
    for pos in (3, 64, 300):
        Tmax = (pos + 9) // 8 * 8
        tab = _zero_angle_table(Tmax, d)
        sl = _slots(B, Tmax)
        vis = sl <= pos
        chunk = (pos + 8) // 8
        cases = [(law, None) for law in ("two", "ramp_up", "last", "sink")] + ([("split_peak", z) for z in range(8)] if pos == 300 else [])
        for R in AL.heights(d):
            for law, z in cases:
                i += 1
                t = None if z is None else R * (sl == min(z * chunk + 5, pos)).to(F64)
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, bool(i & 4) and z is None, 10 * i + d, t=t)
                qkv = torch.cat([q.reshape(B, H * d), k[:, :, pos].reshape(B, Hk * d), v[:, :, pos].reshape(B, Hk * d)], 1).contiguous()
                kp, vp = AL.poison(k, sl < pos), AL.poison(v, sl < pos)
                word = bool(i & 1)

                def run():
                    obuf, o = _guarded(B, H * d)
                    wbuf = torch.full((2 * WGUARD + nb,), 0xA5, dtype=torch.uint8, device=DEV)
                    ws = wbuf[WGUARD:WGUARD + nb]
                    ws.zero_()
                    k2, v2 = kp.clone(), vp.clone()
                    if word: ops.attn_decode_rope(qkv, tab, k2, v2, o, B, H, Hk, d, Tmax, 0, scale, pos_dev=_i32([pos]), workspace=ws)
                    else: ops.attn_decode_rope(qkv, tab, k2, v2, o, B, H, Hk, d, Tmax, pos, scale, workspace=ws)
                    torch.cuda.synchronize()
                    assert _guards_ok(obuf, B), "a store landed outside the output"
                    assert bool((wbuf[:WGUARD] == 0xA5).all()) and bool((wbuf[WGUARD + nb:] == 0xA5).all()), "a store landed outside the workspace"
                    assert int(ws[-B * H * 4:].view(torch.int32).abs().sum()) == 0, "a ticket was left behind"
                    assert bool((k2[:, :, pos].float() == k[:, :, pos].float()).all()) and bool((v2[:, :, pos].float() == v[:, :, pos].float()).all()), "appended rows"
                    same = sl[0] != pos
                    assert torch.equal(k2[:, :, same].view(torch.int16), kp[:, :, same].view(torch.int16)), "another cache slot changed"
                    return o.clone()
                got = _twice([name], run).view(B, H, 1, d)
                _judge(f"{name} splits={splits}", law, f"{law} R={R} pos={pos} z={z} word={word}", "decode", got, q, k, v, scale, allow)
    _report(f"{name} splits={splits}")


# --------------------------------------------------------------------------------------------------------------------------- crab_attn_fwd
def _fwd(names, q4, kp, vp, B, H, Hk, Sq, Skv, d, scale, causal, **kw):
    """q4 [B, H, Sq, d]; kp [B, Hk, Skv, d]; vp [B, Hk, Skv, d] -> the V^T operand [B, Hk, d, Sp] with NaN in its padding columns."""
    q = q4.permute(0, 2, 1, 3).contiguous()
    Sp = (Skv + 7) // 8 * 8
    vt = torch.full((B, Hk, d, Sp), math.nan, device=DEV, dtype=BF)
    vt[..., :Skv] = vp.transpose(2, 3)

    def run():
        obuf, o2 = _guarded(B * Sq, H * d)
        o = o2.view(B, Sq, H * d)
        ops.attn_fwd(q, kp, vt, o, q_strides=(Sq * H * d, d, H * d), k_strides=(Hk * Skv * d, Skv * d, d), vt_strides=(Hk * d * Sp, d * Sp, Sp),
                     o_strides=(Sq * H * d, H * d), B=B, H=H, Hk=Hk, Sq=Sq, Skv=Skv, head_dim=d, scale=scale, causal=causal, **kw)
        torch.cuda.synchronize()
        assert _guards_ok(obuf, B * Sq), "a store landed outside the output"
        return o.clone()
    return _twice(names, run).view(B, Sq, H, d).permute(0, 2, 1, 3)


FWD_KERNELS = [  # (kernel, d, causal, query lengths, (Sq, Skv) -> Skv choices)
    ("attn_fwd32_kernel<128,causal>", 128, True, (65, 300)), ("attn_fwd32_kernel<128>", 128, False, (65, 300)),
    ("attn_fwd32_kernel<64,causal>", 64, True, (65, 300)), ("attn_fwd32_kernel<64>", 64, False, (65, 300)),
    ("attn_fwd_kernel<128,causal>", 128, True, (33,)), ("attn_fwd_kernel<128>", 128, False, (33,)),          # the 64-row kernels take Sq <= 64 without bias
    ("attn_fwd_kernel<64,causal>", 64, True, (33,)), ("attn_fwd_kernel<64>", 64, False, (33,)),
    ("attn_fwd_kernel<32>", 32, False, (65, 300)),
]


@pytest.mark.parametrize("name,d,causal,sqs", FWD_KERNELS, ids=[k[0] for k in FWD_KERNELS])
def test_fwd(name, d, causal, sqs):
    """crab_attn_fwd, B = 2, Hk = 2, G = 1 / 2, Skv = Sq and 600 (150 for the 64-row kernels): every law x R, the modes in turn - no mask;
    kv_start = (70, 3): a first tile wholly hidden, the profile (sink: its peak) starting at the first visible key, and at Skv < 70 a sequence without
    any visible key (zeros); key_mask hiding a random 30 % and, for sequence 0, keys 0 .. 69.  head_dim 32 takes no mask."""
    B, Hk = 2, 2
    i = 0
    for Sq in sqs:
        for Skv in (Sq, 600 if Sq > 64 else 150):
            for R in AL.heights(d):
                for law in AL.NAMES:
                    i += 1
                    H = Hk * (1 + i % 2)
                    mode = ("none", "kv_start", "key_mask")[i % 3] if d != 32 else "none"
                    g = torch.Generator(device=DEV).manual_seed(i)
                    sl = _slots(B, Skv)
                    keyok = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
                    kw = {}
                    if mode == "kv_start":
                        ks = _i32([70, 3])
                        keyok = sl >= ks[:, None]
                        kw["kv_start"] = ks
                    elif mode == "key_mask":
                        keyok = torch.rand(B, Skv, device=DEV, generator=g) > 0.3
                        keyok[0, :70] = False
                        keyok[0, Skv - 1] = True
                        kw["key_mask"] = ops.pack_key_mask(keyok)
                    allow = keyok[:, None, None, :].expand(B, H, Sq, Skv).clone()
                    if causal: allow &= (torch.arange(Skv, device=DEV)[None, :] <= torch.arange(Sq, device=DEV)[:, None] + (Skv - Sq))[None, None]
                    q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, Sq, Skv, keyok, bool(i & 4), 7 * i + d, allow=allow)
                    v = torch.where(keyok[:, None, :, None], v.float(), v.float() * AL.LOUD).to(BF)
                    got = _fwd([name], q, AL.poison(k, keyok), v, B, H, Hk, Sq, Skv, d, scale, causal, **kw)
                    _judge(name, law, f"{law} R={R} H={H} Sq={Sq} Skv={Skv} mask={mode}", "fwd", got, q, k, v, scale, allow)
    _report(name)


@pytest.mark.parametrize("d", (64, 128))
def test_fwd_gated_bias_carries_the_profile(d):
    """attn_fwd_kernel<d,bias>: q, k, v plain 0.7 N(0,1); the profile rides in the fp32 bias [H, Sq, Skv] (+ 0.5 N(0,1) per element) with gate = 1,
    and once with a random gate in [0, 2] on the planted q / k under a small random bias."""
    B, Hk, H = 2, 2, 4
    name = f"attn_fwd_kernel<{d},bias>"
    i = 0
    for Sq, Skv in ((65, 65), (65, 600), (300, 300), (300, 600)):
        for R in AL.heights(d):
            for law in AL.NAMES:
                i += 1
                if (i + Sq + Skv) % 3: continue                                             # a third of the grid per shape: every law x R on some shape
                g = torch.Generator(device=DEV).manual_seed(i + d)
                vis = torch.ones(B, Skv, dtype=torch.bool, device=DEV)
                scale = d ** -0.5
                noise = torch.randn(H, Sq, Skv, device=DEV, generator=g) * 0.5
                if i % 2:
                    q, k, v = (AL.draw((B, h, s, d), g, DEV).to(BF) for h, s in ((H, Sq), (Hk, Skv), (Hk, Skv)))
                    bias = (noise.double() + AL.profile(law, Skv, R, DEV)[None, None]).float().contiguous()
                    gate = torch.ones(B, H, Sq, device=DEV)
                else:
                    q, k, v, scale, _ = _inputs(law, R, d, B, H, Hk, Sq, Skv, vis, False, i)
                    bias, gate = noise.contiguous(), (torch.rand(B, H, Sq, device=DEV, generator=g) * 2).contiguous()
                allow = torch.ones(B, H, Sq, Skv, dtype=torch.bool, device=DEV)
                got = _fwd([name], q, k, v, B, H, Hk, Sq, Skv, d, scale, False, bias=bias, gate=gate)
                _judge(name, law, f"{law} R={R} Sq={Sq} Skv={Skv} profile in {'bias' if i % 2 else 'q.k'}", "fwd", got, q, k, v, scale, allow, bias, gate)
    _report(name)


# ------------------------------------------------------------------------------------------- crab_attn_prefix_partial + crab_attn_own_merge
PREFIX_MODELS = [((2, 2, 128), "attn_own_merge_row_kernel<128>"), ((14, 2, 128), "attn_own_merge_kernel<128>"),
                 ((2, 2, 64), "attn_own_merge_row_kernel<64>"), ((4, 2, 64), "attn_own_merge_kernel<64>")]


@pytest.mark.parametrize("m,merge", PREFIX_MODELS, ids=[f"H{m[0]}k{m[1]}d{m[2]}" for m, _ in PREFIX_MODELS])
def test_prefix_pair(m, merge):
    """Prefix lengths 17, 512, 513 x own 1, 65, two clips of 2 and 1 rows: the peak in the prefix only (in its middle, and on its LAST key: at
    P = 513 that is the one key of the second 512-key chunk, so the chunk rescale of px_attend rises by R), in the own keys only, equal in both
    (two), and ramp_up over the concatenation - the merge weights exp(m - M) are exp(+-R)."""
    H, Hk, d = m
    Gs, B, Cn = (2, 1), 3, 2
    clip_of = torch.tensor([0, 0, 1], device=DEV)
    part = f"attn_prefix_partial_kernel<{d}>"
    scale = d ** -0.5
    tiles, row_clip = ops.prefix_tile_plan(list(Gs), H, Hk)
    tile_rows, row_clip = _i32(tiles).reshape(-1), _i32(row_clip)
    nb = ops.attn_prefix_bytes(B, H, d)
    i = 0
    for P in (17, 512, 513):
        for own in (1, 65):
            for R in AL.heights(d):
                for where in ("prefix", "prefix_tail", "own", "two", "ramp_up"):
                    i += 1
                    kv0 = 3 * (i % 2)
                    Tp, Tmax = (P + 7) // 8 * 8 + 8, (kv0 + own + 8) // 8 * 8
                    g = torch.Generator(device=DEV).manual_seed(i + d)
                    tp = torch.zeros(Cn, Tp, dtype=F64, device=DEV)
                    to = torch.zeros(B, Tmax, dtype=F64, device=DEV)
                    if where in ("prefix", "two"):
                        for c in range(Cn): tp[c, (7 * c + P // 2) % P] = R
                    if where == "prefix_tail": tp[:, P - 1] = R
                    if where in ("own", "two"):
                        for b in range(B): to[b, kv0 + b % own] = R
                    if where == "ramp_up":
                        ramp = AL.profile("ramp_up", P + own, R, DEV)
                        tp[:, :P] = ramp[:P]; to[:, kv0:kv0 + own] = ramp[P:]
                    q, pk = AL.plant(AL.draw((B, H, 1, d), g, DEV), AL.draw((Cn, Hk, Tp, d), g, DEV), tp[:, None], scale)
                    _, kc = AL.plant(AL.draw((1, 1, 1, d), g, DEV), AL.draw((B, Hk, Tmax, d), g, DEV), to[:, None], scale)
                    pv, vc = AL.draw((Cn, Hk, Tp, d), g, DEV).to(BF), AL.draw((B, Hk, Tmax, d), g, DEV).to(BF)
                    pvis = _slots(Cn, Tp) < P
                    ovis = (_slots(B, Tmax) >= kv0) & (_slots(B, Tmax) < kv0 + own)
                    K = torch.cat([pk[clip_of, :, :P], kc[:, :, kv0:kv0 + own]], 2)
                    V = torch.cat([pv[clip_of, :, :P], vc[:, :, kv0:kv0 + own]], 2)
                    qkv = q.reshape(B, H * d)
                    dpk, dpv, dkc, dvc = AL.poison(pk, pvis), AL.poison(pv, pvis), AL.poison(kc, ovis), AL.poison(vc, ovis)
                    word = bool(i & 2)

                    def run():
                        obuf, o = _guarded(B, H * d)
                        wbuf = torch.full((2 * WGUARD + nb,), 0xA5, dtype=torch.uint8, device=DEV)
                        ws = wbuf[WGUARD:WGUARD + nb]
                        ops.attn_prefix_partial(qkv, dpk, dpv, ws, tile_rows, row_clip, B, H, Hk, d, P, scale)
                        ctx = kv0 + own
                        ops.attn_own_merge(qkv, ws, dkc, dvc, o, B, 1, H, Hk, d, Tmax, 1 if word else ctx, scale, ctx_dev=_i32([ctx - 1]) if word else None,
                                           kv_start=_i32([kv0] * B) if kv0 else None)
                        torch.cuda.synchronize()
                        assert _guards_ok(obuf, B), "a store landed outside the output"
                        assert bool((wbuf[:WGUARD] == 0xA5).all()) and bool((wbuf[WGUARD + nb:] == 0xA5).all()), "a store landed outside the workspace"
                        return torch.cat([o.reshape(-1).float(), ws.view(torch.float32)])      # output and partials: both must repeat bit for bit
                    got = _twice([part, merge], run)[:B * H * d].view(B, H, 1, d)
                    allow = torch.ones(B, 1, 1, P + own, dtype=torch.bool, device=DEV)
                    _judge(f"{part} + {merge}", where, f"peak {where} R={R} P={P} own={own} kv_start={kv0} word={word}", "decode", got, q, K, V, scale, allow)
    _report(f"{part} + {merge}")


# ------------------------------------------------------------------------------------------------------------------------ crab_attn_verify
@pytest.mark.parametrize("m", ((2, 2, 128), (14, 2, 128), (8, 2, 128), (4, 2, 64)), ids=lambda m: f"H{m[0]}k{m[1]}d{m[2]}")
def test_verify_row_limits(m):
    """crab_attn_verify, Sq = 4 and 16: the peak is the key ONE PAST row i0's limit (a real, loud row): rows <= i0 must not see it, rows > i0 are
    dominated by it; and ramp_up over the drafted keys (every row's maximum is its own newest key).  17 and 65 common keys keep everything in the
    first 512-key chunk of px_attend; 520 put the drafted keys, the limits and the peak into the second one (Sq = 16: per-row limits in a chunk that
    also rescales)."""
    H, Hk, d = m
    B = 2
    name = f"attn_verify_kernel<{d}>"
    i = 0
    for Sq in (4, 16):
        for common in (17, 65, 520):
            if common == 520 and Sq == 4: continue
            for R in AL.heights(d):
                for i0 in (0, Sq // 2, Sq - 2, None):
                    i += 1
                    kv0 = 3 * (i % 2)
                    ctx = kv0 + common + 1                                                 # query r sees the slots kv0 .. ctx - 1 + r
                    end = ctx + Sq - 1
                    Tmax = (end + 8) // 8 * 8
                    sl = _slots(B, Tmax)
                    live = (sl >= kv0) & (sl < end)
                    t = torch.zeros(B, Tmax, dtype=F64, device=DEV)
                    if i0 is None: t[:, ctx - 1:end] = AL.profile("ramp_up", Sq, R, DEV)
                    else: t[:, ctx + i0] = R
                    lim = ctx - 1 + torch.arange(Sq, device=DEV)
                    allow = ((sl[:, None] >= kv0) & (sl[:, None] <= lim[None, :, None]))[:, None].expand(B, H, Sq, Tmax)
                    q, k, v, scale, allow = _inputs("verify", R, d, B, H, Hk, Sq, Tmax, live, False, i + d, t=t, allow=allow)
                    if i0 is not None: v[:, :, ctx + i0] = (v[:, :, ctx + i0].float() * AL.LOUD).to(BF)
                    qkv = q.permute(0, 2, 1, 3).reshape(B * Sq, H * d).contiguous()
                    kp, vp = AL.poison(k, live), AL.poison(v, live)
                    word = bool(i & 2)

                    def run():
                        obuf, o = _guarded(B * Sq, H * d)
                        ops.attn_verify(qkv, kp, vp, o, B, Sq, H, Hk, d, Tmax, 1 if word else ctx, scale, ctx_dev=_i32([ctx - 1]) if word else None,
                                        kv_start=_i32([kv0] * B) if kv0 else None)
                        torch.cuda.synchronize()
                        assert _guards_ok(obuf, B * Sq), "a store landed outside the output"
                        return o.clone()
                    got = _twice([name], run).view(B, Sq, H, d).permute(0, 2, 1, 3)
                    law = "ramp_up_drafts" if i0 is None else "past_limit"
                    _judge(name, law, f"{law} R={R} Sq={Sq} common={common} i0={i0} kv_start={kv0} word={word}", "decode", got, q, k, v, scale, allow)
    _report(name)


# -------------------------------------------------------------------------------------------------------------------- crab_attn_decode_fp8
@pytest.mark.parametrize("H,Hk,d", [(8, 4, 64), (28, 4, 128)])
def test_decode_fp8(H, Hk, d):
    """crab_attn_decode_fp8 with a zero-angle rotary table under sink, last (the peak is the key quantised and appended in this call) and ramp_up
    at R = 12 and 40.  The cached keys go through ops.kv_quant_fp8; the reference is fp64 attention over the DEQUANTISED rows (code x scale, exact
    in fp64; the new row through tests/kv_fp8_ref.quant).  The bound is attn_bound_weighted on those operands: score = (q . codes) k_scale is a
    d-term dot of exact products (a bf16 times a 4-bit code) and one product with the scalar - the (d + 3) T_j of the bf16 kernels, the row scale
    in the place of the bias product; v_scale rides on p, one more rounding per key, inside the 32 of c(n) that the MFMA tree does not use here."""
    B, Tmax = 3, 72
    name = f"attn_decode_fp8_kernel<{d}>"
    tab = _zero_angle_table(Tmax, d)
    i = 0
    for pos in (16, 64):
        sl = _slots(B, Tmax)
        vis = sl <= pos
        for R in (12, 40):
            for law in ("sink", "last", "ramp_up"):
                i += 1
                q, k, v, scale, allow = _inputs(law, R, d, B, H, Hk, 1, Tmax, vis, False, i + d)
                kc = torch.full((1, B, Hk, Tmax, d), 0x7F, dtype=torch.uint8, device=DEV); vc = kc.clone()          # NaN codes and huge scales outside the cache
                ksc = torch.full((1, B, Hk, Tmax), 3e30, dtype=torch.float32, device=DEV); vsc = ksc.clone()
                ops.kv_quant_fp8(k[None].contiguous(), v[None].contiguous(), kc, vc, ksc, vsc, S=pos)
                qkv = torch.cat([q.reshape(B, H * d), k[:, :, pos].reshape(B, Hk * d), v[:, :, pos].reshape(B, Hk * d)], 1).contiguous()
                word = bool(i & 1)
                kept = {}

                def run():
                    obuf, o = _guarded(B, H * d)
                    c = [x[0].clone() for x in (kc, vc, ksc, vsc)]
                    if word: ops.attn_decode_fp8(qkv, tab, c[0], c[1], c[2], c[3], o, B, H, Hk, d, Tmax, 0, scale, pos_dev=_i32([pos]))
                    else: ops.attn_decode_fp8(qkv, tab, c[0], c[1], c[2], c[3], o, B, H, Hk, d, Tmax, pos, scale)
                    torch.cuda.synchronize()
                    assert _guards_ok(obuf, B), "a store landed outside the output"
                    kept["c"] = [x.cpu() for x in c]
                    return o.clone()
                got = _twice([name], run).view(B, H, 1, d).cpu()
                gk, gv, gks, gvs = kept["c"]
                wk, wks = R8.quant(k[:, :, pos].cpu())
                wv, wvs = R8.quant(v[:, :, pos].cpu())
                assert torch.equal(gk[:, :, pos], wk) and torch.equal(gks[:, :, pos], wks) and torch.equal(gv[:, :, pos], wv) and torch.equal(gvs[:, :, pos], wvs), \
                    "the appended codes / scales differ from kv_fp8_ref.quant"
                K = gk.view(torch.float8_e4m3fn).float().double() * gks.double()[..., None]
                V = gv.view(torch.float8_e4m3fn).float().double() * gvs.double()[..., None]
                keep = vis.cpu()[:, None, :, None]
                K, V = torch.where(keep, K, torch.zeros_like(K)), torch.where(keep, V, torch.zeros_like(V))
                _judge(name, law, f"{law} R={R} pos={pos} word={word}", "decode", got, q.cpu(), K, V, scale, allow.cpu())
    _report(name)
