"""Differential fuzz of the attention entry points (crab_attn_fwd: 64- and 128-row kernels, head_dim 32 / 64 / 128, causal, GQA, gated bias, left-pad
kv_start, general key_mask; crab_attn_decode / _masked / _keymask incl. the grouped-query kernel and device-resident context lengths) against
fp64 attention on the same bf16 operands (on the GPU), every output element held to the derived bound of tests/fuzz_bounds.py: one bf16 store, the
bf16 P of the forward kernels, and an fp32 slack that must itself stay under 2^-12 of sum_j p_j |v_je| (no constant here).
Half of the cases keep that law (q, k, v = 0.7 N(0,1): an almost uniform softmax) and are judged exactly as before; the other half draw a score law of
tests/attn_laws.py (a peak of height R, a ramp, a sink, a uniform shift of -R / +R), R and the V law (plain / loud tail) from a SECOND generator - the
shapes and masks of every case are those of the old fuzzer - and are judged with attn_bound_weighted under its 2^-10 cap.  The worst err / bound
is printed per law.  The laws and their bound live beside the other bounds in tests/ (attn_laws.py, fuzz_bounds.attn_bound_weighted); run against a
tests/ directory that has neither (an older suite driving this script), every case keeps the old law and the script says so.
python scripts/fuzz_attn.py [cases] [seed]"""
import math, os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crab_amd import ops, _lib
from tests import fuzz_bounds as FB
try:
    from tests import attn_laws as AL
except ImportError:
    AL = None
LAWS = AL is not None and hasattr(FB, "attn_bound_weighted")

BF = torch.bfloat16
NCASE = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
rng_law = random.Random(7919 + (int(sys.argv[2]) if len(sys.argv) > 2 else 0))          # the laws: a generator of their own, so that the cases keep their shapes and masks
bad, rejected, done, why = [], 0, 0, {}
run = FB.Run()
law_runs = {}


def judge(desc, kind, o4, q4, k, v, scale, allow, bias=None, gate=None, law=None):
    """o4 / q4 [B, H, Sq, d] against the fp64 reference, every element; the derived fp32 slack must not be able to hide a bf16-level defect."""
    if law is not None:
        ref, bound, rel = FB.attn_bound_weighted(q4, k, v, scale, allow, bias, gate, kind=kind)
        law_runs.setdefault(law, FB.Run()).judge(bad, desc, kind, o4, ref, bound)
        if not rel <= FB.LAW_SLACK_CAP: bad.append(desc + f" -> the derived fp32 slack is {rel / FB.LAW_SLACK_CAP:.3f} of its cap")
        return
    ref, bound, rel = FB.attn_bound(q4, k, v, scale, allow, bias, gate, kind=kind)
    run.judge(bad, desc, kind, o4, ref, bound)
    if not rel <= FB.SLACK_CAP: bad.append(desc + f" -> the derived fp32 slack is {rel / FB.SLACK_CAP:.3f} of its cap")


def draw_law(d):
    """(law or None for the old one, R, loud tail) - always four draws, so that a case's law does not depend on the laws before it."""
    if not LAWS: return None, 0, False
    old, law, R, loud = rng_law.random() < 0.5, rng_law.choice(AL.NAMES), rng_law.choice(AL.heights(d)), rng_law.random() < 0.5
    return (None, 0, False) if old else (law, R, loud)


def reject(e):
    global rejected
    msg = str(e)
    if "error -1:" in msg or "error -3:" in msg:
        rejected += 1
        k = msg.split(":", 2)[-1].strip()[:90]
        why[k] = why.get(k, 0) + 1
        return True
    return False


for case in range(NCASE):
    g = torch.Generator(device="cuda").manual_seed(1000 + case)
    d = rng.choice([32, 64, 64, 128, 128])
    Hk = rng.choice([1, 2, 4])
    G = rng.choice([1, 1, 2, 4, 7])
    H = Hk * G
    B = rng.choice([1, 2, 3, 5])
    decode = rng.random() < 0.4 and d != 32
    if not decode:
        Sq = rng.choice([1, 7, 32, 63, 64, 65, 127, 128, 129, 200, 257, 300, 702])
        causal = rng.random() < 0.6 and d != 32
        Skv = Sq if causal or rng.random() < 0.5 else rng.choice([Sq, 48, 256, 600])
        use_bias = (not causal) and d != 32 and rng.random() < 0.25
        mode = rng.choice(["none", "none", "kv_start", "key_mask"]) if d != 32 and not use_bias else "none"
        q = (torch.randn(B, Sq, H, d, device="cuda", generator=g) * 0.7).to(BF)
        k = (torch.randn(B, Hk, Skv, d, device="cuda", generator=g) * 0.7).to(BF)
        v = (torch.randn(B, Hk, Skv, d, device="cuda", generator=g) * 0.7).to(BF)
        law, R, loud = draw_law(d)
        Sp = (Skv + 7) // 8 * 8
        obuf = torch.full((B * Sq + 2, H * d), 777.0, device="cuda", dtype=BF)          # guard rows above and below the output
        o = obuf[1:B * Sq + 1].view(B, Sq, H * d)
        scale = 1.0 / math.sqrt(d)
        keyok = torch.ones(B, Skv, device="cuda", dtype=torch.bool)
        kw = {}
        if mode == "kv_start":
            ks = torch.tensor([rng.randrange(0, max(1, Skv // 2)) for _ in range(B)], device="cuda", dtype=torch.int32)
            keyok = torch.arange(Skv, device="cuda")[None] >= ks[:, None]
            kw["kv_start"] = ks
        elif mode == "key_mask":
            keyok = torch.rand(B, Skv, device="cuda", generator=g) > 0.3
            kw["key_mask"] = ops.pack_key_mask(keyok)
        bias = gate = None
        if use_bias:
            bias = torch.randn(H, Sq, Skv, device="cuda", generator=g) * 0.5
            gate = torch.rand(B, H, Sq, device="cuda", generator=g) * 2
            kw["bias"], kw["gate"] = bias, gate
        desc = f"case {case}: fwd B={B} H={H} Hk={Hk} Sq={Sq} Skv={Skv} d={d} causal={causal} bias={use_bias} mask={mode}"
        allow = keyok[:, None, None, :].expand(B, H, Sq, Skv).clone()
        if causal: allow &= (torch.arange(Skv, device="cuda")[None, :] <= torch.arange(Sq, device="cuda")[:, None] + (Skv - Sq))[None, None]
        if law is not None:
            desc += f" law={law} R={R} loud={loud}"
            q, k = AL.plant(q.float(), k.float(), AL.spread(law, R, keyok)[:, None], scale)
            if loud: v = AL.loud_tail(v, FB.attn_ref(q.permute(0, 2, 1, 3), k, v, scale, allow, bias, gate)[1])
        vt = torch.zeros(B, Hk, d, Sp, device="cuda", dtype=BF); vt[..., :Skv] = v.transpose(2, 3)
        try:
            ops.attn_fwd(q, k, vt, o, q_strides=(Sq * H * d, d, H * d), k_strides=(Hk * Skv * d, Skv * d, d), vt_strides=(Hk * d * Sp, d * Sp, Sp),
                         o_strides=(Sq * H * d, H * d), B=B, H=H, Hk=Hk, Sq=Sq, Skv=Skv, head_dim=d, scale=scale, causal=causal, **kw)
            torch.cuda.synchronize()
        except _lib.CrabHipError as e:
            if not reject(e): bad.append(desc + " -> " + str(e)[:200])
            continue
        done += 1
        judge(desc, "fwd", o.view(B, Sq, H, d).permute(0, 2, 1, 3), q.permute(0, 2, 1, 3), k, v, scale, allow, bias, gate, law=law)
        if not (bool((obuf[0] == 777.0).all()) and bool((obuf[-1] == 777.0).all())): bad.append(desc + " -> a store landed outside the output")
    else:
        Tmax = rng.choice([64, 128, 960])
        ctx = rng.randrange(1, Tmax + 1)
        Bd = rng.choice([1, 3, 8, 40, 130]) if Hk * 130 <= 600 else rng.choice([1, 3, 8])
        mode = rng.choice(["none", "none", "kv_start", "key_mask"])
        dev_ctx = rng.random() < 0.5
        kc = (torch.randn(Bd, Hk, Tmax, d, device="cuda", generator=g) * 0.7).to(BF)
        vc = (torch.randn(Bd, Hk, Tmax, d, device="cuda", generator=g) * 0.7).to(BF)
        q = (torch.randn(Bd, H * d, device="cuda", generator=g) * 0.7).to(BF)
        law, R, loud = draw_law(d)
        obuf = torch.full((Bd + 2, H * d), 777.0, device="cuda", dtype=BF)
        o = obuf[1:Bd + 1]
        scale = 1.0 / math.sqrt(d)
        keyok = torch.zeros(Bd, Tmax, device="cuda", dtype=torch.bool); keyok[:, :ctx] = True
        kw = {}
        if mode == "kv_start":
            ks = torch.tensor([rng.randrange(0, ctx) for _ in range(Bd)], device="cuda", dtype=torch.int32)
            keyok &= torch.arange(Tmax, device="cuda")[None] >= ks[:, None]
            kw["kv_start"] = ks
        elif mode == "key_mask":
            keyok &= torch.rand(Bd, Tmax, device="cuda", generator=g) > 0.3
            kw["key_mask"] = ops.pack_key_mask(keyok)
        desc = f"case {case}: decode B={Bd} H={H} Hk={Hk} d={d} Tmax={Tmax} ctx={ctx} dev_ctx={dev_ctx} mask={mode}"
        if law is not None:
            desc += f" law={law} R={R} loud={loud}"
            q4, kc = AL.plant(q.float().view(Bd, H, 1, d), kc.float(), AL.spread(law, R, keyok)[:, None], scale)
            q = q4.view(Bd, H * d)
            if loud: vc = AL.loud_tail(vc, FB.attn_ref(q4, kc, vc, scale, keyok[:, None, None, :])[1])
        try:
            if dev_ctx:
                pos = torch.full((1,), ctx - 1, device="cuda", dtype=torch.int32)
                ops.attn_decode(q, kc, vc, o, Bd, H, Hk, d, Tmax, 1, scale, ctx_dev=pos, **kw)
            else:
                ops.attn_decode(q, kc, vc, o, Bd, H, Hk, d, Tmax, ctx, scale, **kw)
            torch.cuda.synchronize()
        except _lib.CrabHipError as e:
            if not reject(e): bad.append(desc + " -> " + str(e)[:200])
            continue
        done += 1
        judge(desc, "decode", o.view(Bd, H, 1, d), q.view(Bd, H, 1, d), kc, vc, scale, keyok[:, None, None, :], law=law)
        if not (bool((obuf[0] == 777.0).all()) and bool((obuf[-1] == 777.0).all())): bad.append(desc + " -> a store landed outside the output")
for k_, v_ in sorted(why.items(), key=lambda kv: -kv[1]): print(f"  rejected x{v_}: {k_}")
for b_ in bad[:40]: print("FAIL", b_)
if not LAWS: print("  NOTE: tests/attn_laws.py or fuzz_bounds.attn_bound_weighted is missing: every case ran under the old law")
for law_, r_ in sorted(law_runs.items()): print(f"  law {law_}: {r_}")
print(f"{done} cases computed, {rejected} rejected by the library, {len(bad)} failures; {run}")
sys.exit(1 if bad else 0)
