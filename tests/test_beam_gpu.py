"""csrc/beam.hip at kernel level.  crab_kv_beam_reorder bit for bit against index_select on a clone; the step pair crab_beam_row_topk ->
crab_beam_merge driven directly through ops for 12 steps against tests/beam_ref.step, taken from the DEVICE's state before every step - the
check is step-local, so a near-tie (EITHER, tests/beam_ref.py) never propagates.  EITHER steps are skipped and counted; the share of the same
seeded inputs is asserted from the reference alone in tests/test_beam_host.py."""
import pytest
import torch

from crab_amd import ops
from tests import beam_ref as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 0x5A5B


# ------------------------------------------------------------------ crab_kv_beam_reorder
def _patterns(K):
    ident = list(range(K))
    swap = [1, 0] + ident[2:]
    cyc = ([1, 2, 0] + ident[3:]) if K >= 3 else swap
    mixed = [(k * 3 + 1) % K for k in range(K)] if K > 2 else [1, 1]
    mixed[-1] = mixed[0]                                         # a repeat and, for K > 2, a row nobody reads
    return [(ident, [0] * K, swap), (cyc, mixed, swap), (mixed, cyc, [0] * K)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_kv_beam_reorder_equals_index_select(d, K):
    L, C, Hk, Tmax = 2, 3, 2, 64
    rows = C * K
    g = torch.Generator().manual_seed(d + K)
    for pos in (0, 1, 37, 63):
        for n_set, pats in enumerate(_patterns(K)):
            done = 2 if n_set == 2 else -1                       # the last set marks one clip done: skipped whatever its beam_idx says
            kv = []
            for _ in range(2):
                t = torch.randint(-30000, 30000, (L, rows, Hk, Tmax, d), generator=g, dtype=torch.int16)
                t[:, :, :, pos + 1:] = SENTINEL
                kv.append(t)
            idx = torch.tensor([p for pat in pats for p in pat], dtype=torch.int32)
            fin = torch.zeros(rows, dtype=torch.int32)
            if done >= 0:
                fin[done * K:(done + 1) * K] = 1
            want = [t.clone() for t in kv]
            for c in range(C):
                if c == done:
                    continue
                src = torch.tensor([c * K + p for p in pats[c]])
                for t, w in zip(kv, want):
                    w[:, c * K:(c + 1) * K, :, :pos + 1] = t.index_select(1, src)[:, :, :, :pos + 1]
            kc, vc = (t.cuda().view(BF) for t in kv)
            ops.kv_beam_reorder(kc, vc, K, idx.cuda(), fin.cuda(), torch.tensor([pos], dtype=torch.int32).cuda())
            torch.cuda.synchronize()
            for name, t, w in (("k", kc, want[0]), ("v", vc, want[1])):
                got = t.view(torch.int16).cpu()
                assert torch.equal(got, w), f"{name} cache, d={d} K={K} pos={pos} patterns {pats} done clip {done}: {int((got != w).sum())} words differ"
                assert bool((got[:, :, :, pos + 1:] == SENTINEL).all()), "a slot past pos was written"


def test_kv_beam_reorder_first_slot_and_argument_checks():
    L, C, K, Hk, Tmax, d = 1, 1, 2, 1, 64, 64
    t = torch.arange(L * C * K * Hk * Tmax * d, dtype=torch.int32).remainder(30000).to(torch.int16).view(L, C * K, Hk, Tmax, d)
    kc, vc = t.cuda().view(BF), t.flip(1).contiguous().cuda().view(BF)
    idx, fin, pos = torch.tensor([1, 0], dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda(), torch.tensor([9], dtype=torch.int32).cuda()
    ops.kv_beam_reorder(kc, vc, K, idx, fin, pos, first_slot=4)
    want = t.clone()
    want[:, :, :, 4:10] = t.flip(1)[:, :, :, 4:10]
    assert torch.equal(kc.view(torch.int16).cpu(), want)
    with pytest.raises(ValueError):
        ops.kv_beam_reorder(kc, vc[:, :, :, :32], K, idx, fin, pos)
    with pytest.raises(ValueError):
        ops.kv_beam_reorder(kc, vc, K, idx.long(), fin, pos)
    with pytest.raises(Exception):
        ops.kv_beam_reorder(kc.float(), vc.float(), K, idx, fin, pos)


# ------------------------------------------------------------------ the step pair
def _device_state(bs, cur, run_seq, fin):
    st = {k: v.cpu() for k, v in bs.snapshot().items()}
    st.update(cur_ids=cur.cpu(), run_seq=run_seq.cpu(), finished=fin.cpu())
    return st


@pytest.mark.parametrize("c", R.GPU_CASES, ids=lambda c: c.name)
def test_step_pair_equals_the_reference_step_by_step(c):
    p = R.case_params(c)
    K, V, N, clips = c.K, c.V, R.STEPS, R.CLIPS
    rows = clips * K
    dev = "cuda"
    bs = ops.BeamState(clips, K, N, R.PAD, c.lp, c.early, dev)
    cur = torch.zeros(rows, dtype=torch.int64, device=dev)
    run_seq = torch.full((rows, N), R.PAD, dtype=torch.int64, device=dev)
    fin = torch.zeros(rows, dtype=torch.int32, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    init = R.init_state(clips, p)
    first = _device_state(bs, cur, run_seq, fin)
    for f in ("run_score", "hyp_score", "hyp_seq", "hyp_len", "hyp_fin", "unsat", "beam_idx", "run_seq", "finished"):
        assert torch.equal(first[f], init[f]), f"initial {f}"
    hit = live = worst_done = 0
    seen_done_early = False
    for s in range(N):
        before = _device_state(bs, cur, run_seq, fin)
        z = R.case_logits(c, s)
        step_dev.fill_(s)
        ops.beam_row_topk(z.cuda(), bs, step_dev, fin, p.eos, p.min_new)
        ops.beam_merge(bs, V, step_dev, p.eos, cur, run_seq, fin)
        torch.cuda.synchronize()
        got = _device_state(bs, cur, run_seq, fin)
        want, either, tol = R.step(before, z, s, p)
        for cl in range(clips):
            r = slice(cl * K, cl * K + K)
            if int(before["finished"][cl * K]) != 0:
                seen_done_early = seen_done_early or s < N - 1
                for f in got:                                    # a done clip is frozen: bit-identical
                    a, b = (got[f][cl], before[f][cl]) if f == "unsat" else (got[f][r], before[f][r])
                    assert torch.equal(a, b), f"{c.name}: step {s} changed {f} of the done clip {cl}"
                continue
            live += 1
            if either[cl]:
                hit += 1
                continue
            bad = R.compare(got, want, tol, cl, K)
            assert not bad, f"{c.name}: step {s}, clip {cl}:\n  " + "\n  ".join(bad)
    share = hit / max(1, live)
    record_parity(f"beam step pair {c.name}: share of live (clip, step) pairs with a near-tie (EITHER)", share, 1.0, R.EITHER_CAP, live=live)
    print(f"{c.name}: {live} live (clip, step) pairs, {hit} EITHER ({share:.2%})")
    assert share <= R.EITHER_CAP
    end = _device_state(bs, cur, run_seq, fin)
    assert bool(end["finished"].all()), "every clip is done after max_new steps"
    assert bool((end["hyp_fin"].view(clips, K)[:, 0] == 1).all()) and bool((end["hyp_score"].view(clips, K)[:, 0] > -1e8).all())
    hs = end["hyp_score"].view(clips, K)
    assert bool((hs[:, :-1] >= hs[:, 1:]).all()), "hypotheses are kept best first"
    if c.name.startswith("one clip done") or c.name.startswith("early_stopping=True"):
        assert seen_done_early, "no clip was done before the last step: the frozen-state check saw nothing"
    if c.name.startswith("min_new_tokens"):
        assert not bool((end["hyp_len"][end["hyp_fin"] != 0] < 2).any()), "a hypothesis ended below min_new_tokens"
    if c.name.startswith("EOS is the best"):
        assert bool((end["hyp_len"].view(clips, K) == 1).any(1).all()), "the one-token hypothesis of step 0 is kept"
    if c.name.startswith("no EOS"):
        assert bool((end["hyp_len"] == N).all())


def test_wrappers_refuse_misread_tensors():
    bs = ops.BeamState(2, 2, 8, 1, 1.0, False, "cuda")
    z = torch.zeros((4, 64), device="cuda")
    fin, step = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.beam_row_topk(z[:3], bs, step, fin, 7, 0)
    with pytest.raises(ValueError):
        ops.beam_row_topk(z.double(), bs, step, fin, 7, 0)
    with pytest.raises(ValueError):
        ops.beam_row_topk(z, bs, step, fin.long(), 7, 0)
    with pytest.raises(ValueError):
        ops.beam_merge(bs, 64, step, 7, torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros((4, 9), dtype=torch.int64, device="cuda"), fin)
    with pytest.raises(ValueError):
        ops.BeamState(2, 2, 8, 1, 1.0, "sometimes", "cuda")
