"""crab_sample_select_warped (csrc/sample.hip) on bare logits.

(1) all three stages off: cur_ids, out_ids and finished equal crab_sample_select's bit for bit over 8 steps, rows that finish and emit pad
    included.  (2) the stage grid of tests/warp_ref.py - B in {1, 3, 17} x V in {96, 1000, 1025, 32000, 152064}, each stage alone and all three
    together, with and without top-k / top-p in front - against the fp64 classes: kept_n between #KEEP and #KEEP + #EITHER, every KEEP token
    at or above kept_min and every DROP token below it (in the kernel's own fp32 scaled logits, which the test forms bit for bit), the drawn id
    never DROP, EOS under min_new_tokens never drawn.  tests/test_warp_host.py caps the share of rows with any EITHER token at one in ten.
(3) min_p = 1 draws crab_greedy_select's id.  (4) 4096 rows of one 8-token row: a cutoff removes three tokens, which are never drawn, and
    every kept token's count lies within 5 binomial standard deviations of n p_i.
Every launch reads its logits through a row stride larger than V (the last test: stride 0, one row for all) and writes between sentinels."""
import math

import pytest
import torch

from tests import warp_ref as R

pytestmark = pytest.mark.gpu
SENT_I, SENT_F, GUARD = -77, 777.0, 8
PAD = 3


class _Out:
    """The five outputs of one launch, each a view into a sentinel-filled buffer; out_ids with a row stride larger than its width."""

    def __init__(self, B, n_steps, finished=None):
        mk = lambda n, dt, fill: torch.full((n + 2 * GUARD,), fill, dtype=dt, device="cuda")
        self.B, self.n, self.ld = B, n_steps, n_steps + 3
        self.bufs = {"cur": mk(B, torch.int64, SENT_I), "out": mk(B * self.ld, torch.int64, SENT_I), "fin": mk(B, torch.int32, SENT_I),
                     "kn": mk(B, torch.int32, SENT_I), "km": mk(B, torch.float32, SENT_F)}
        v = {k: b[GUARD:b.numel() - GUARD] for k, b in self.bufs.items()}
        self.cur, self.fin, self.kept_n, self.kept_min = v["cur"], v["fin"], v["kn"], v["km"]
        self.out = v["out"].view(B, self.ld)[:, :n_steps]
        self.fin.copy_(torch.tensor(finished if finished is not None else [0] * B, dtype=torch.int32))
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def check_guards(self, what):
        for k, b in self.bufs.items():
            s = SENT_F if k == "km" else SENT_I
            assert bool((b[:GUARD] == s).all()) and bool((b[-GUARD:] == s).all()), f"{what}: a word outside `{k}` was written"
        gaps = self.bufs["out"][GUARD:-GUARD].view(self.B, self.ld)[:, self.n:]
        assert bool((gaps == SENT_I).all()), f"{what}: a word between the rows of out_ids was written"


def _strided(z, pad_ld=5):
    """z [B, V] on the device as a view with row stride V + pad_ld inside a sentinel-filled buffer: (buffer, view)."""
    B, V = z.shape
    buf = torch.full((B * (V + pad_ld) + 4,), SENT_F, dtype=torch.float32, device="cuda")
    view = buf[1:1 + B * (V + pad_ld)].view(B, V + pad_ld)[:, :V]
    view.copy_(z)
    assert view.stride(0) == V + pad_ld
    return buf, view


# ------------------------------------------------------------------ (1) all stages off == crab_sample_select
@pytest.mark.parametrize("V", R.GRID_V)
@pytest.mark.parametrize("front", list(R.GRID_FRONTS))
def test_all_stages_off_is_sample_select_bit_for_bit(front, V):
    from crab_amd import ops
    B, n, seed = 17, 8, 20240 + V
    t, k, p = R.GRID_FRONTS[front]
    g = torch.Generator().manual_seed(V)
    z = torch.randn((n, B, V), generator=g) * 3
    eos = 11
    z[2:, 1, eos] = 40.0                                         # row 1 draws EOS as soon as min_new_tokens lets it, then emits pad
    z[5:, 4, eos] = 40.0
    z[:, 6] = float("-inf")                                      # a row without a finite token: token 0, as crab_sample_select gives it
    fin0 = [0] * B
    fin0[2] = 1                                                  # finished from the start: pad at every step
    a, b, c = _Out(B, n, fin0), _Out(B, n, fin0), _Out(B, n, fin0)      # sample_select; warped with kept_n / kept_min; warped without them
    for s in range(n):
        buf, lg = _strided(z[s])
        before = buf.clone()
        for o in (a, b, c):
            o.step.fill_(s)
        ops.sample_select(lg, a.cur, a.out, a.step, a.fin, eos, PAD, 2, t, k, p, seed)
        ops.sample_select_warped(lg, b.cur, b.out, b.step, b.fin, eos, PAD, 2, t, k, p, seed, 0.0, 0.0, 0.0, b.kept_n, b.kept_min)
        ops.sample_select_warped(lg, c.cur, c.out, c.step, c.fin, eos, PAD, 2, t, k, p, seed)
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the logits were written"
        assert torch.equal(a.cur, b.cur) and torch.equal(a.fin, b.fin) and torch.equal(a.cur, c.cur) and torch.equal(a.fin, c.fin), (front, V, s)
    assert torch.equal(a.out, b.out) and torch.equal(a.out, c.out)
    b.check_guards(f"{front} V={V}")
    c.check_guards(f"{front} V={V}, no kept outputs")
    assert bool((c.bufs["kn"] == SENT_I).all()) and bool((c.bufs["km"] == SENT_F).all())
    out = b.out.cpu()
    assert out[2].tolist() == [PAD] * n and out[6].tolist() == [0] * n
    assert out[1, 2] == eos and out[1, 3:].tolist() == [PAD] * (n - 3) and not bool((out[:, :2] == eos).any())
    assert int(b.fin[1]) == 1 and int(b.fin[4]) == 1


# ------------------------------------------------------------------ (2) the stage grid against the fp64 classes
@pytest.mark.parametrize("V", R.GRID_V)
@pytest.mark.parametrize("B", R.GRID_B)
def test_stage_grid_against_the_reference(B, V):
    from crab_amd import ops
    z = R.grid_rows(B, V)
    buf, lg = _strided(z)
    before = buf.clone()
    for front, (t, k, p) in R.GRID_FRONTS.items():
        xk = R.kernel_scaled(z, t, R.GRID_EOS)                   # what the kernel compares, bit for bit
        for st in R.GRID_STAGE_NAMES:
            mp, ec, et = R.GRID_STAGES[front][st]
            ref = R.grid_reference(B, V, front, st)
            o = _Out(B, 2)
            for s in range(2):                                   # both steps lie under min_new_tokens: two draws from one kept set
                o.step.fill_(s)
                ops.sample_select_warped(lg, o.cur, o.out, o.step, o.fin, R.GRID_EOS, PAD, R.GRID_MIN_NEW, t, k, p, 99 + V + s, mp, ec, et,
                                         o.kept_n, o.kept_min)
            torch.cuda.synchronize()
            what = f"B={B} V={V} {front} {st}"
            o.check_guards(what)
            ids, kn, km = o.out.cpu(), o.kept_n.cpu(), o.kept_min.cpu()
            for b, (cls, _) in enumerate(ref):
                keep, either, drop = cls == R.KEEP, cls == R.EITHER, cls == R.DROP
                nk, ne = int(keep.sum()), int(either.sum())
                print(f"{what} row {b}: KEEP {nk} EITHER {ne} kept_n {int(kn[b])} kept_min {float(km[b]):.6g} ids {ids[b].tolist()}")
                assert nk <= int(kn[b]) <= nk + ne, (what, b)
                assert bool((xk[b][keep] >= km[b]).all()), (what, b, "a KEEP token lies below kept_min")
                assert bool((xk[b][drop] < km[b]).all()), (what, b, "a DROP token lies at or above kept_min")
                for y in ids[b].tolist():
                    assert 0 <= y < V and int(cls[y]) != R.DROP and y != R.GRID_EOS, (what, b, y)
            assert int(o.fin.sum()) == 0
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the logits were written"


# ------------------------------------------------------------------ (3) min_p = 1 is greedy
@pytest.mark.parametrize("V", R.GRID_V)
def test_min_p_one_draws_the_greedy_id(V):
    from crab_amd import ops
    B = 17
    z = R.grid_rows(B, V)
    top2 = torch.topk(z.masked_fill(torch.arange(V) == R.GRID_EOS, float("-inf")), 2, dim=1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "the rows are tie-free at the top"
    _, lg = _strided(z)
    g = _Out(B, 1)
    ops.greedy_select(lg, g.cur, g.out, g.step, g.fin, R.GRID_EOS, PAD, R.GRID_MIN_NEW)
    for front, (t, k, p) in R.GRID_FRONTS.items():
        o = _Out(B, 1)
        ops.sample_select_warped(lg, o.cur, o.out, o.step, o.fin, R.GRID_EOS, PAD, R.GRID_MIN_NEW, t, k, p, 5, 1.0, 0.0, 0.0, o.kept_n, o.kept_min)
        torch.cuda.synchronize()
        assert torch.equal(o.cur, g.cur) and torch.equal(o.out, g.out), (front, V)
        assert o.kept_n.tolist() == [1] * B
        o.check_guards(f"min_p=1 {front} V={V}")


# ------------------------------------------------------------------ (4) the draw's distribution
def test_draws_follow_the_renormalised_distribution_of_the_kept_set():
    from crab_amd import ops
    n = 4096
    probs = torch.tensor([0.015, 0.25, 0.08, 0.3, 0.005, 0.2, 0.03, 0.12], dtype=torch.float64)      # epsilon_cutoff = 0.05 removes 0.015, 0.005, 0.03
    row = probs.log().float()
    cls, _ = R.warp_classes(row, torch.ones(8, dtype=torch.bool), (1.0, 0, 1.0), epsilon_cutoff=0.05)
    assert cls.tolist() == [R.DROP, R.KEEP, R.KEEP, R.KEEP, R.DROP, R.KEEP, R.DROP, R.KEEP]
    pk = R.final_probs(row, cls, 1.0)
    lg = row.cuda()[None].expand(n, 8)                           # one row for all: row stride 0; the streams differ by the row index
    o = _Out(n, 1)
    ops.sample_select_warped(lg, o.cur, o.out, o.step, o.fin, -1, PAD, 0, 1.0, 0, 1.0, 424242, 0.0, 0.05, 0.0, o.kept_n, o.kept_min)
    torch.cuda.synchronize()
    o.check_guards("distribution")
    assert o.kept_n.tolist() == [5] * n
    counts = torch.bincount(o.cur.cpu(), minlength=8).double()
    for i in range(8):
        if int(cls[i]) == R.DROP:
            assert int(counts[i]) == 0, f"token {i} was removed and drawn {int(counts[i])} times"
        else:
            mean, sd = n * float(pk[i]), math.sqrt(n * float(pk[i]) * (1.0 - float(pk[i])))
            print(f"token {i}: drawn {int(counts[i])}, n p = {mean:.1f}, sd = {sd:.1f}: {(float(counts[i]) - mean) / sd:+.2f} sd")
            assert abs(float(counts[i]) - mean) <= 5.0 * sd, (i, int(counts[i]), mean, sd)
