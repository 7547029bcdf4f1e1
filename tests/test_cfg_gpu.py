"""crab_cfg_mix / crab_cfg_follow (csrc/cfg.hip) on bare logits against the fp64 reference and its derived bound (tests/cfg_ref.py).

Shapes: V in {1, 3, 4, 5} (one element; less than, exactly and just above one 16-byte chunk), 320 and 515 (the tiny models' vocabularies: fewer
chunks than the block has threads, with and without a tail), 4099 (several chunks per thread plus a tail), each with B in {1, 3} pairs; 32000 with
2 pairs (a row that spans many 16-byte loads per thread).  Every shape runs from 16-byte aligned bases with ldl = V and from bases 1, 2 and 3
floats off with ldl > V - the logits and the guided buffer misaligned DIFFERENTLY, so the conditional row, the unconditional row and the
guided row disagree about where a 16-byte chunk starts (scalar head and tail, the 4-byte aligned load form of pass 2).  Scales 1.5 and 7.5.
Rows: normal(0, 4); a pair with a row dominated by one logit; -inf entries in one row and in both; a finished pair.  Around `guided` sit
sentinels, the raw logits must come back bit for bit, and two launches must give the same bits."""
import pytest
import torch

from tests import cfg_ref as R

pytestmark = pytest.mark.gpu
SENT = 777.0
NEG_INF = float("-inf")
WORST = {"ratio": 0.0}


def _view(rows, V, off, pad_ld, fill=SENT):
    """A [rows, V] fp32 device view with row stride V + pad_ld that starts `off` floats into a sentinel-filled buffer: (buffer, view)."""
    ld = V + pad_ld
    buf = torch.full((off + rows * ld + 8,), fill, dtype=torch.float32, device="cuda")
    view = buf[off:off + rows * ld].view(rows, ld)[:, :V]
    assert view.stride(0) == ld and (view.data_ptr() % 16 == 0) == (off % 4 == 0)
    return buf, view


def _logits(B, V, seed):
    """[2B, V] fp32: normal(0, 4); pair 0's unconditional row dominated by one logit (60 above the rest) that its conditional row ranks low;
    with V > 4 a few -inf entries in pair B - 1: one column in the conditional row only, one in the unconditional row only, one in both."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((2 * B, V), generator=g) * 4
    dom = (2 * V) // 3
    z[B, dom] = z[B].max() + 60
    z[0, dom] = z[0].min() - 1
    dead = []
    if V > 4:
        b = B - 1
        one, other, both = V // 5, V // 2 + 1, V - 1
        z[b, one] = z[B + b, other] = z[b, both] = z[B + b, both] = NEG_INF
        dead = [(b, one), (b, other), (b, both)]
    return z, dead


def _mix(z, B, scale, off_l, off_g, pad_ld, finished=None):
    from crab_amd import ops
    V = z.shape[1]
    lbuf, lg = _view(2 * B, V, off_l, pad_ld)
    lg.copy_(z)
    gbuf, gd = _view(B, V, off_g, pad_ld)
    before = lbuf.clone()
    fin = torch.tensor(finished if finished is not None else [0] * B, dtype=torch.int32, device="cuda")
    ops.cfg_mix(lg, gd, B, scale, fin)
    torch.cuda.synchronize()
    assert torch.equal(lbuf.view(torch.int32), before.view(torch.int32)), "the raw logits were written"      # bits: a NaN logit equals itself
    mask = torch.ones_like(gbuf, dtype=torch.bool)
    mask[off_g:off_g + B * (V + pad_ld)].view(B, V + pad_ld)[:, :V] = False
    assert bool((gbuf[mask] == SENT).all()), "a word outside the guided rows was written"
    return gd.cpu().clone(), lg, gd, fin


def _check(B, V, scale, off_l, off_g, pad_ld, seed, finished=None):
    from crab_amd import ops
    what = f"B={B} V={V} scale={scale} logits +{off_l} guided +{off_g} ld=V+{pad_ld}"
    z, dead = _logits(B, V, seed)
    got, lg, gd, fin = _mix(z, B, scale, off_l, off_g, pad_ld, finished)
    ref, bound = R.mix_ref(z, B, scale)
    for b, i in dead:
        assert float(got[b, i]) == NEG_INF and float(ref[b, i]) == NEG_INF, f"{what}: -inf in a row must give -inf at ({b}, {i}), got {float(got[b, i])}"
    live = ref > NEG_INF
    assert bool((got[~live] == NEG_INF).all()) and bool(torch.isfinite(got[live]).all()), f"{what}: the -inf pattern differs"
    err = (got.double() - ref)[live].abs()
    ratio = float((err / bound[live]).max())
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: max |got - ref| {float(err.max()):.3e}, largest ratio to the bound {ratio:.3f} (so far {WORST['ratio']:.3f})")
    assert bool((err <= bound[live]).all()), f"{what}: {float(err.max())} exceeds the bound (ratio {ratio})"
    ops.cfg_mix(lg, gd, B, scale, fin)                           # the second launch, over the first one's output
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu().view(torch.int32), got.view(torch.int32)), f"{what}: two launches differ"
    return got, ref, bound


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1, 3, 4, 5, 320, 515, 4099])
def test_mix_against_fp64(V, B):
    _check(B, V, 1.5, 0, 0, 0, 10 * V + B)                       # everything 16-byte aligned where V % 4 == 0
    for off_l, off_g, scale in ((1, 3, 7.5), (2, 1, 1.5), (3, 2, 7.5)):
        _check(B, V, scale, off_l, off_g, 1 + off_l, 10 * V + B + off_l)


def test_a_row_of_many_chunks_per_thread():
    got, ref, _ = _check(2, 32000, 7.5, 0, 0, 0, 7)
    _check(2, 32000, 1.5, 1, 2, 3, 8)
    # the dominated pair: the unconditional row puts all its mass on one token, which guidance pushes far DOWN, everything else up
    dom = (2 * 32000) // 3
    assert int(got[0].argmin()) == dom and float(got[0, dom]) < -7.5 * 20 and float(got[0].median()) > 0


def test_a_finished_pair_is_computed_like_any_other():
    """The select kernels scan a finished row too (csrc/cfg.hip says why a finished pair is not skipped): its guided row holds this step's
    scores, not what an earlier launch left."""
    a, _, _ = _check(3, 515, 1.5, 1, 2, 2, 21, finished=[0, 1, 0])
    b, _, _ = _check(3, 515, 1.5, 1, 2, 2, 21, finished=[1, 1, 1])
    c, _, _ = _check(3, 515, 1.5, 1, 2, 2, 21)
    assert torch.equal(a, c) and torch.equal(b, c)


def test_edge_rows():
    from crab_amd import ops
    V, B = 37, 2
    g = torch.Generator().manual_seed(3)
    z = torch.randn((2 * B, V), generator=g)
    z[0] = NEG_INF                                               # a conditional row without a finite entry: its pair is -inf throughout
    z[1, 5] = float("nan")                                       # a NaN logit: its row's normaliser is NaN (torch.log_softmax), the pair NaN ...
    z[B + 1, 9] = NEG_INF                                        # ... except where the other row excludes the token
    got, *_ = _mix(z, B, 1.5, 0, 0, 0)
    assert bool((got[0] == NEG_INF).all())
    keep = torch.ones(V, dtype=torch.bool)
    keep[9] = False
    assert bool(torch.isnan(got[1][keep]).all()) and float(got[1, 9]) == NEG_INF
    # shape, dtype and stride are refused by name before the library is asked
    lg = torch.zeros((4, 8), device="cuda")
    fin = torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad_l, bad_g, bad_f, name in ((lg[:3], None, None, "logits"), (lg.double(), None, None, "logits"), (lg[:, ::2], None, None, "logits"),
                                      (None, torch.zeros((2, 7), device="cuda"), None, "guided"), (None, torch.zeros((2, 8), device="cuda").half(), None, "guided"),
                                      (None, torch.zeros((2, 8)), None, "guided"), (None, None, fin[:1], "finished"), (None, None, fin.long(), "finished")):
        with pytest.raises(ValueError, match=name):
            ops.cfg_mix(lg if bad_l is None else bad_l, torch.zeros((2, 8), device="cuda") if bad_g is None else bad_g, 2, 1.5,
                        fin if bad_f is None else bad_f)


def test_follow_copies_the_pairs_words_and_nothing_else():
    from crab_amd import ops
    B, n = 3, 5
    dev = "cuda"
    for step in (0, 3, 4):
        cur = torch.arange(10, 10 + 2 * B, dtype=torch.int64, device=dev)
        base = torch.full((2 * B, n + 2), -7, dtype=torch.int64, device=dev)
        out = base[:, :n]                                         # row stride n + 2
        out[:B] = torch.arange(100, 100 + B * n, dtype=torch.int64, device=dev).view(B, n)
        fin = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.int32, device=dev)
        want_cur, want_out, want_fin = cur.clone(), out.clone(), fin.clone()
        want_cur[B:] = cur[:B]
        want_out[B:, step] = out[:B, step]
        want_fin[B:] = fin[:B]
        ops.cfg_follow(cur, out, fin, torch.tensor([step], dtype=torch.int32, device=dev), B)
        torch.cuda.synchronize()
        assert torch.equal(cur, want_cur) and torch.equal(out, want_out) and torch.equal(fin, want_fin), step
        assert bool(base[:, n:].eq(-7).all()), "a word past the rows' columns was written"
    # step >= n_steps (and a negative one): nothing is written
    for step in (n, n + 3, -1):
        cur = torch.arange(2 * B, dtype=torch.int64, device=dev)
        out = torch.arange(2 * B * n, dtype=torch.int64, device=dev).view(2 * B, n)
        fin = torch.tensor([1, 0, 1, 0, 0, 0], dtype=torch.int32, device=dev)
        c0, o0, f0 = cur.clone(), out.clone(), fin.clone()
        ops.cfg_follow(cur, out, fin, torch.tensor([step], dtype=torch.int32, device=dev), B)
        torch.cuda.synchronize()
        assert torch.equal(cur, c0) and torch.equal(out, o0) and torch.equal(fin, f0), step
    with pytest.raises(ValueError, match="cur_ids"):
        ops.cfg_follow(cur[:B], out, fin, torch.zeros(1, dtype=torch.int32, device=dev), B)
    with pytest.raises(ValueError, match="out_ids"):
        ops.cfg_follow(cur, out.int(), fin, torch.zeros(1, dtype=torch.int32, device=dev), B)
    with pytest.raises(ValueError, match="finished"):
        ops.cfg_follow(cur, out, fin[:B], torch.zeros(1, dtype=torch.int32, device=dev), B)
