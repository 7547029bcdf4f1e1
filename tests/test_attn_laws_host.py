"""tests/attn_laws.py and fuzz_bounds.attn_bound_weighted on the CPU, for every law x R x head size, in the decode form (n = 1, 17, 65, 830 keys)
and the causal forward form (Sq = 65, 300):

cap             max_e slack_e / S_e <= 2^-10 (and <= 2^-12 at R = 12 up to d = 64, 2^-11 at d = 128: a one-key row has e = 131 T there); on the OLD law slack_e <= 1.01 x attn_bound's slack, element by element.
no false alarm  an fp32 online softmax (m = -1e30 start, chunks of 16 and of 32 keys, and 16 interleaved key groups merged by log-sum-exp; P in
                bf16 for kind "fwd") stays within 1 x bound.
caught          four single defects reach err / bound > 2 on every query row they can touch:
                  - the visible key with the second-largest probability is dropped (rows where that key has p >= 2^-8);
                  - group partials are merged without their exp(m_g - M) weights (rows where a key of p >= 2^-8 lies in a group whose
                    maximum is at least ln 2 under the row's: it is counted at least twice);
                  - for the verify form, the key one past a row's limit is read (rows where it would take p >= 2^-8);
                  - one rescale (the largest rise of the running maximum after the first chunk) is applied to acc but not to l.  Its error
                    is delta / (1 + delta) |o_e| on EVERY element, delta the relative growth of the denominator; a p >= 2^-8 rule has no meaning
                    for a defect whose error carries no V row, so the rows asked for follow from the bound's own ceiling: stored(o, f32) is
                    at most 2^-8 |o_e| + 2 f32 with f32 <= (2^-8 + 2^-10) S_e, under 2^-6.6 S_e in all, so on the row's element with the largest
                    rho = |o_e| / S_e the defect reaches 2 bounds wherever delta / (1 + delta) rho >= 2^-5 (all from the reference).
law check       the laws do what tests/attn_laws.py says, so that the GPU tests are not vacuous (see the test's docstring for the cases)."""
import math

import pytest
import torch

from tests import attn_laws as AL
from tests import fuzz_bounds as FB

BF, F64 = torch.bfloat16, torch.float64
NS = (1, 17, 65, 830)
SQS = (65, 300)
P_MIN = 2.0 ** -8
GRID = [(law, R, d) for d in (32, 64, 128) for R in AL.heights(d) for law in AL.NAMES]


def _decode_case(law, R, d, n, loud, seed=0):
    """B = 2, Hk = 1, G = 2 query heads on one key head, n visible keys in a cache of n + 3 slots starting at slot 2."""
    g = torch.Generator().manual_seed(seed + 1000 * n + d)
    B, H, Hk, T = 2, 2, 1, n + 3
    scale = d ** -0.5
    vis = torch.zeros(B, T, dtype=torch.bool); vis[:, 2:2 + n] = True
    q, k = AL.plant(AL.draw((B, H, 1, d), g), AL.draw((B, Hk, T, d), g), AL.spread(law, R, vis)[:, None], scale)
    v = AL.draw((B, Hk, T, d), g).to(BF)
    allow = vis[:, None, None, :]
    if loud: v = AL.loud_tail(v, FB.attn_ref(q, k, v, scale, allow)[1])
    return q, k, v, scale, allow.expand(B, H, 1, T)


def _fwd_case(law, R, d, Sq, loud, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * Sq + d)
    B, H, Hk = 1, 2, 1
    scale = d ** -0.5
    vis = torch.ones(B, Sq, dtype=torch.bool)
    q, k = AL.plant(AL.draw((B, H, Sq, d), g), AL.draw((B, Hk, Sq, d), g), AL.spread(law, R, vis)[:, None], scale)
    v = AL.draw((B, Hk, Sq, d), g).to(BF)
    allow = torch.tril(torch.ones(Sq, Sq, dtype=torch.bool))[None, None].expand(B, H, Sq, Sq)
    if loud: v = AL.loud_tail(v, FB.attn_ref(q, k, v, scale, allow)[1])
    return q, k, v, scale, allow


def emulate(q, k, v, scale, allow, kind, chunk, groups=1, weights=True, skip_l=None):
    """fp32 online softmax with the kernels' storage points.  Key j belongs to group j mod `groups` (16 interleaved key groups, or one); a group
    walks its keys in chunks of `chunk` from m = -1e30, l = 0: mn = max(m, chunk max), a = exp(m - mn), p = exp(s - mn), l = l a + sum p,
    acc = acc a + P v (P = bf16(p) for kind "fwd"), and the groups are merged by log-sum-exp (weights=False: without the exp(m_g - M) weights).
    skip_l [B, H, Sq] (long): the step at which the row's l misses its rescale.  Returns (bf16 output, a of every step [steps, B, H, Sq, groups])."""
    G = q.shape[1] // k.shape[1]
    kk, vv = k.float().repeat_interleave(G, 1), v.float().repeat_interleave(G, 1)
    B, H, Sq, d = q.shape
    T = kk.shape[2]
    s = torch.einsum("bhsd,bhtd->bhst", q.float(), kk) * torch.tensor(scale, dtype=torch.float32)
    s = s.masked_fill(~allow.expand(s.shape), -math.inf)
    step = groups * chunk
    Tp = (T + step - 1) // step * step
    s = torch.nn.functional.pad(s, (0, Tp - T), value=-math.inf).view(B, H, Sq, Tp // groups, groups).transpose(3, 4)    # [B, H, Sq, groups, keys]
    vv = torch.nn.functional.pad(vv, (0, 0, 0, Tp - T)).view(B, H, Tp // groups, groups, d).transpose(2, 3)                # [B, H, groups, keys, d]
    m = torch.full((B, H, Sq, groups), -1e30)
    l = torch.zeros(B, H, Sq, groups)
    acc = torch.zeros(B, H, Sq, groups, d)
    factors = []
    for i, c0 in enumerate(range(0, Tp // groups, chunk)):
        sc = s[..., c0:c0 + chunk]
        mn = torch.maximum(m, sc.max(-1).values)
        a = torch.exp(m - mn)
        p = torch.exp(sc - mn[..., None])
        pn = p.to(BF).float() if kind == "fwd" else p
        al = a if skip_l is None else torch.where((skip_l == i)[..., None], torch.ones_like(a), a)
        l = l * al + p.sum(-1)
        acc = acc * a[..., None] + torch.einsum("bhsgt,bhgtd->bhsgd", pn, vv[:, :, :, c0:c0 + chunk])
        m = mn
        factors.append(a)
    M = m.max(-1, keepdim=True).values
    w = torch.exp(m - M) if weights else torch.ones_like(m)
    L = (l * w).sum(-1)
    O = (acc * w[..., None]).sum(-2)
    out = torch.where(L[..., None] > 0, O / L[..., None], torch.zeros_like(O))
    return out.to(BF), torch.stack(factors)


def _row_ratio(got, ref, bound):
    """err / bound of the worst element of every query row [B, H, Sq]."""
    err = (got.to(F64) - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max(-1).values


def _cases(law, R, d):
    for n in NS:
        yield f"decode n={n}", "decode", _decode_case(law, R, d, n, loud=bool(n & 2))
    for Sq in SQS:
        yield f"fwd Sq={Sq}", "fwd", _fwd_case(law, R, d, Sq, loud=Sq == 300)


WORST = {}


@pytest.mark.parametrize("law,R,d", GRID, ids=[f"{l}-R{R}-d{d}" for l, R, d in GRID])
def test_cap_no_false_alarm_and_defects(law, R, d):
    for what, kind, (q, k, v, scale, allow) in _cases(law, R, d):
        desc = f"{law} R={R} d={d} {what}"
        ref, bound, rel = FB.attn_bound_weighted(q, k, v, scale, allow, kind=kind)
        p = FB.attn_ref(q, k, v, scale, allow)[1]
        # ---- cap
        assert rel <= FB.LAW_SLACK_CAP, f"{desc}: slack {rel / FB.LAW_SLACK_CAP:.3f} of its cap"
        # R = 12: under the old cap as well up to d = 64; the dominant term grows with d + 3, so d = 128 is held to (131 / 67 <) 2 x it
        if R == 12: assert rel <= FB.SLACK_CAP * (2 if d == 128 else 1), f"{desc}: slack {rel / FB.SLACK_CAP:.3f} of the old cap"
        # ---- no false alarm
        for chunk, groups in ((16, 1), (32, 1), (16, 16)):
            got, factors = emulate(q, k, v, scale, allow, kind, chunk, groups)
            r = FB.worst(got, ref, bound)[0]
            WORST["emulation"] = max(WORST.get("emulation", 0.0), r)
            assert r <= 1.0, f"false alarm: {desc} chunk {chunk} groups {groups}: err / bound {r:.3f}"
        # ---- caught: the second-largest key dropped
        if int(allow.sum(-1).min()) >= 2 or kind == "fwd":
            second = p.topk(2, -1).indices[..., 1:] if p.shape[-1] >= 2 else None
            a2 = allow.clone().scatter_(-1, second, False)
            rows = p.gather(-1, second)[..., 0] >= P_MIN
            if rows.any():
                rr = _row_ratio(FB.attn_ref(q, k, v, scale, a2)[0], ref, bound)[rows]
                WORST["dropped"] = min(WORST.get("dropped", math.inf), float(rr.min()))
                assert float(rr.min()) > 2.0, f"missed: second-largest key dropped, {desc}: err / bound {float(rr.min()):.3f}"
        # ---- caught: groups merged without their weights
        got, _ = emulate(q, k, v, scale, allow, kind, 16, 16, weights=False)
        T = p.shape[-1]
        s = FB.attn_ref(q, k, v, scale, allow, detail=True)[2].masked_fill(~allow, -math.inf)
        grp = torch.arange(T) % 16
        mg = torch.stack([s[..., grp == g_].max(-1).values if bool((grp == g_).any()) else torch.full(s.shape[:-1], -math.inf) for g_ in range(16)], -1)
        low = (mg.max(-1, keepdim=True).values - mg) >= math.log(2.0)                        # groups counted at least twice
        rows = ((p >= P_MIN) & low[..., grp]).any(-1)
        if rows.any():
            rr = _row_ratio(got, ref, bound)[rows]
            WORST["unweighted"] = min(WORST.get("unweighted", math.inf), float(rr.min()))
            assert float(rr.min()) > 2.0, f"missed: merge without weights, {desc}: err / bound {float(rr.min()):.3f}"
        # ---- caught: one rescale applied to acc but not to l
        S = torch.einsum("bhst,bhtd->bhsd", p, v.double().repeat_interleave(q.shape[1] // k.shape[1], 1).abs())
        rho = (ref.abs() / S.clamp_min(1e-300)).max(-1).values
        for chunk in (16, 32):
            _, factors = emulate(q, k, v, scale, allow, kind, chunk)
            if factors.shape[0] < 2: continue
            a = factors[1:, ..., 0].double()                                                  # [steps - 1, B, H, Sq]: step 0 rescales nothing (l = 0)
            amin, at = a.min(0)
            at = at + 1
            keys = torch.arange(T)[None, None, None] < (at * chunk)[..., None]                # the keys accumulated before that step
            delta = (p * keys).sum(-1) * (1.0 / amin.clamp_min(1e-300) - 1.0)
            rows = delta / (1 + delta) * rho >= 2.0 ** -5
            if rows.any():
                got, _ = emulate(q, k, v, scale, allow, kind, chunk, skip_l=at)
                rr = _row_ratio(got, ref, bound)[rows]
                WORST["rescale"] = min(WORST.get("rescale", math.inf), float(rr.min()))
                assert float(rr.min()) > 2.0, f"missed: l not rescaled at step {at[rows][0]}, {desc}: err / bound {float(rr.min()):.3f}"


@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("Sq", (4, 16))
def test_verify_form_key_past_the_limit_is_caught(d, Sq):
    """crab_attn_verify's form: query i of Sq sees the keys 0 .. common + i.  The peak is the key one past row i0's limit: rows <= i0 must not see it
    (a kernel that reads one key past the limit on row i0 is dominated by it), rows > i0 are dominated by it."""
    for R in AL.heights(d):
        for common in (1, 17, 65):
            for i0 in (0, Sq // 2, Sq - 2):
                g = torch.Generator().manual_seed(R + common + i0)
                B, H, Hk, T = 1, 2, 1, common + Sq + 1
                scale = d ** -0.5
                t = torch.zeros(B, T, dtype=F64); t[:, common + i0 + 1] = R
                q, k = AL.plant(AL.draw((B, H, Sq, d), g), AL.draw((B, Hk, T, d), g), t[:, None], scale)
                v = AL.draw((B, Hk, T, d), g).to(BF)
                lim = common + torch.arange(Sq)                                               # last visible key of row i
                allow = (torch.arange(T)[None] <= lim[:, None])[None, None].expand(B, H, Sq, T)
                ref, bound, rel = FB.attn_bound_weighted(q, k, v, scale, allow)
                assert rel <= FB.LAW_SLACK_CAP
                for chunk, groups in ((16, 1), (16, 16)):
                    assert FB.worst(emulate(q, k, v, scale, allow, "decode", chunk, groups)[0], ref, bound)[0] <= 1.0
                a2 = allow | (torch.arange(T)[None] == lim[:, None] + 1)[None, None]
                bad, pb = FB.attn_ref(q, k, v, scale, a2)
                rows = pb.gather(-1, (lim + 1).view(1, 1, Sq, 1).expand(B, H, Sq, 1))[..., 0] >= P_MIN
                assert bool(rows[:, :, i0].all())                                            # the planted row is among them
                rr = _row_ratio(bad, ref, bound)[rows]
                WORST["verify"] = min(WORST.get("verify", math.inf), float(rr.min()))
                assert float(rr.min()) > 2.0, (d, Sq, R, common, i0, float(rr.min()))
                p = FB.attn_ref(q, k, v, scale, allow)[1]
                assert float(p[:, :, i0 + 1:, common + i0 + 1].min()) > 0.5 or R == 12        # rows > i0 are dominated by it


def test_weighted_slack_is_within_the_old_one_on_the_old_law():
    """slack_e <= 1.01 x attn_bound's slack, element by element, where both are the whole fp32 term (kind "decode": bound = stored(o, slack) is
    monotone in the slack), on the old law - and the old cap holds for the new function there."""
    for d, n in ((64, 7), (128, 300), (128, 960)):
        g = torch.Generator().manual_seed(d + n)
        q, k, v = (AL.draw((2, h, 1 if h == 4 else n, d), g).to(BF) for h in (4, 2, 2))
        allow = torch.ones(2, 4, 1, n, dtype=torch.bool)
        allow[1, :, :, :n // 3] = False
        o, b_old, rel_old = FB.attn_bound(q, k, v, d ** -0.5, allow)
        o2, b_new, rel_new = FB.attn_bound_weighted(q, k, v, d ** -0.5, allow)
        assert torch.equal(o, o2)
        # stored(o, x) = max(h, x) + x: invert it for the slack of either bound
        h = FB.half_ulp(o)
        s_old = torch.where(b_old > 2 * h, b_old / 2, b_old - h)
        s_new = torch.where(b_new > 2 * h, b_new / 2, b_new - h)
        assert bool((s_new <= 1.01 * s_old * (1 + 1e-12)).all())
        assert rel_new <= 1.01 * rel_old and rel_new <= FB.SLACK_CAP and rel_old <= FB.SLACK_CAP


def test_laws_are_not_degenerate():
    """ramp_up: the chunk maximum of the fp64 scores rises in every chunk of 16 keys, on every row, wherever the profile's rise per chunk
    (16 R / (n - 1)) is above the noise's range (about 3: scores carry O(0.5) of noise, the maximum of 16 of them about 1 +- 0.5): n = 17 and 65
    at R >= 40; at n = 830 the PROFILE rises in every chunk and the scores' running maximum moves in more than half of them.
    last: the rescale factor of the final step is below 2^-15 at R >= 40 (e^-12 is within the noise of 2^-15, so R = 12 is asked for 2^-8).
    R = 90: at least one fp32 exp(s - m) of every row is subnormal or 0.  sink / ramp_down / two / edges / saw: the peak sits where the table
    says; shift_neg / shift_pos: every score is within the noise of -R / +R."""
    for d in (64, 128):
        for R in AL.heights(d):
            for n in (17, 65, 830):
                def scores(law):
                    q, k, v, scale, allow = _decode_case(law, R, d, n, loud=False)
                    s = FB.attn_ref(q, k, v, scale, allow, detail=True)[2]
                    return s[..., 2:2 + n], (q, k, v, scale, allow)
                s, case = scores("ramp_up")
                cm = torch.stack([s[..., c:c + 16].max(-1).values for c in range(0, n, 16)], -1)
                rises = (cm[..., 1:] > cm[..., :-1])
                if R >= 40 and n <= 65: assert bool(rises.all()), (d, R, n)
                run = torch.cummax(cm, -1).values
                assert float((run[..., 1:] > run[..., :-1]).double().mean()) > 0.5, (d, R, n)
                t = AL.profile("ramp_up", n, R)
                tc = torch.stack([t[c:c + 16].max() for c in range(0, n, 16)])
                assert bool((tc[1:] > tc[:-1]).all())
                s, case = scores("last")
                for chunk in (16, 32):
                    a = emulate(*case, "decode", chunk)[1][(n + 1) // chunk]             # the step of the newest key (slot n + 1): it holds the peak, none before it does
                    assert float(a.max()) < (2.0 ** -15 if R >= 40 else 2.0 ** -8), (d, R, n, chunk, float(a.max()))
                assert bool((s.argmax(-1) == n - 1).all())
                s, _ = scores("sink")
                assert bool((s.argmax(-1) == 0).all())
                if R == 90:
                    e = torch.exp((s - s.max(-1, keepdim=True).values).float())
                    assert bool(((e < torch.finfo(torch.float32).tiny).any(-1)).all())
                s, _ = scores("ramp_down")
                assert bool((s[..., 0] - s[..., -1] > R - 4.0).all())
                s, _ = scores("two")
                top = s.topk(2, -1).indices.sort(-1).values
                assert bool((top[..., 0] == n // 3).all()) and bool((top[..., 1] == 2 * n // 3 + 1).all())
                s, _ = scores("edges")
                assert bool(((s.argmax(-1) % 64 == 63) | (s.argmax(-1) % 64 == 0)).all())
                s, _ = scores("saw")
                assert bool((s.argmax(-1) % 17 >= 12).all())
                for law, sign in (("shift_neg", -1), ("shift_pos", 1)):
                    s, _ = scores(law)
                    assert float((s - sign * R).abs().max()) < 4.0 + R * 2.0 ** -8


def test_loud_tail_touches_only_weightless_keys():
    q, k, v, scale, allow = _decode_case("ramp_down", 40, 64, 830, loud=False)
    p = FB.attn_ref(q, k, v, scale, allow)[1]
    v2 = AL.loud_tail(v, p)
    loud = (v2.float() != v.float()).any(-1)[:, 0]                                            # [B, T]
    assert bool(loud.any()) and float(p.amax((1, 2))[loud].max()) < AL.TAIL
    assert torch.equal(v2.float()[loud[:, None].expand(v.shape[:3])], v.float()[loud[:, None].expand(v.shape[:3])] * AL.LOUD)


def test_the_fuzzer_draws_these_laws():
    """scripts/fuzz_attn.py keeps the old law only where tests/ lacks the laws (an older suite driving it); in this tree it must find them."""
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_attn.py")) as f:
        src = f.read()
    assert "from tests import attn_laws as AL" in src and "FB.attn_bound_weighted(" in src and "FB.LAW_SLACK_CAP" in src
    assert hasattr(FB, "attn_bound_weighted") and hasattr(FB, "LAW_SLACK_CAP") and set(AL.NAMES) == set(AL.PEAKED + AL.SHIFTS)
