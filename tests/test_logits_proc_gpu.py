"""crab_logits_edit / crab_logits_restore (csrc/logits_proc.hip) at kernel level, bit for bit against the CPU restatement of HF's processors
(tests/logits_proc_ref.py, itself held to transformers in tests/test_logits_proc_host.py).  B = 3 rows of V = 1037 logits in a buffer of row
stride V + 3 (the three columns behind every row must survive), 16 steps; row 2 is finished."""
import ctypes as C

import pytest
import torch

from crab_amd import _lib, ops
from tests import logits_proc_ref as R

pytestmark = pytest.mark.gpu
B, V, LDL, NS = 3, 1037, 1037 + 3, 16
INF = float("inf")
STOPS8 = [11, V - 1, 4, 700, V + 9, 300, 5, 8]                   # V - 1, an id in the histories (4, 5, 8) and one outside [0, V)


def _raw():
    g = torch.Generator().manual_seed(20)
    buf = torch.randn(B, LDL, generator=g) * 3
    buf[:, 4] = 0.0                                              # history tokens meet a zero, a -inf, positive and negative values
    buf[:, 5] = -INF
    buf[:, 8], buf[:, 9], buf[:, V - 1] = 2.5, -1.75, 0.625
    buf[:, 100::97] = 0.0
    buf[:, 50::113] = -INF
    return buf


def _history():
    h = torch.empty(B, NS, dtype=torch.int64)
    h[0] = torch.tensor([8, 9, 8, 9, 8, 9, 4, 5, V - 1, 8, 9, 8, 4, 4, 8, 9])               # duplicates, repeated bi- and trigrams
    h[1] = torch.tensor([7, 7, 7, 7, 7, V + 7, 7, 7, -2, 8, 8, 8, 8, 8, 8, 8])              # self-overlapping n-grams, two ids outside [0, V)
    h[2] = torch.tensor([3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3])                   # the finished row
    return h


def _state(n_stop):
    dev = "cuda"
    raw = _raw()
    buf = raw.cuda()
    st = dict(raw=raw, buf=buf, logits=buf[:, :V], out_ids=_history().cuda(), step=torch.zeros(1, dtype=torch.int32, device=dev),
              fin=torch.tensor([0, 0, 1], dtype=torch.int32, device=dev), stops=torch.tensor(STOPS8[:n_stop], dtype=torch.int32, device=dev) if n_stop else None,
              save_idx=torch.full((B, 2 * NS + n_stop), 12345, dtype=torch.int32, device=dev),
              save_val=torch.full((B, 2 * NS + n_stop), 7.0, dtype=torch.float32, device=dev))
    return st


def _edit(st, p, n, min_new):
    ops.logits_edit(st["logits"], st["out_ids"], st["step"], st["fin"], p, n, st["stops"], min_new, st["save_idx"], st["save_val"])


def _restore(st, cur):
    ops.logits_restore(st["logits"], cur, st["fin"], st["stops"], st["save_idx"], st["save_val"])


def _steps(n):
    return sorted({s for s in (0, 1, n - 2, n - 1, n, 15) if s >= 0})


@pytest.mark.parametrize("n_stop", [0, 1, 8])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_edit_equals_the_restatement_and_restore_gives_the_raw_bits_back(n, n_stop):
    min_new = 2
    for p in ((1.3, 0.7) if n in (1, 2) else (1.3, 1.0)):
        st = _state(n_stop)
        prm = R.Params(p, n, STOPS8[:n_stop], min_new)
        hist, fin0 = _history(), torch.tensor([0, 0, 1], dtype=torch.int32)
        for step in sorted(set(_steps(max(n, 1)) + [2, 3])):     # 0 and 1 lie below min_new_tokens, the rest at or above it
            st["step"].fill_(step)
            st["fin"].copy_(fin0)
            want = R.edit(st["raw"][:, :V], hist, step, fin0, prm)
            _edit(st, p, n, min_new)
            got = st["buf"].cpu()
            assert torch.equal(got[:, :V], want), (p, n, n_stop, step, torch.nonzero(got[:, :V] != want)[:8].tolist())
            assert torch.equal(got[:, V:], st["raw"][:, V:]), "the columns behind a row were written"
            assert torch.equal(got[2], st["raw"][2]) and bool((st["save_idx"][2] == -1).all()), "the finished row was edited"
            idx = st["save_idx"].cpu()
            assert bool(((idx >= -1) & (idx < V)).all())
            if n == 1 and p != 1.0 and step == 15:
                both = [c for c in (8, 9, V - 1) if want[0, c] == -INF and st["raw"][0, c] != -INF]
                assert both == [8, 9, V - 1], "columns that are penalised AND banned"
            # the token the select 'chose': row 0 a stop id when there is one, row 1 an ordinary id, row 2 (finished) another stop id
            cur = torch.tensor([STOPS8[n_stop - 1] if n_stop else 6, 6, STOPS8[0]], dtype=torch.int64)
            _restore(st, cur.cuda())
            assert torch.equal(st["buf"].cpu(), st["raw"]), (p, n, n_stop, step)
            want_fin = R.finished_after(fin0, cur, prm)
            assert torch.equal(st["fin"].cpu(), want_fin), (n_stop, st["fin"].tolist(), want_fin.tolist())


def test_neutral_parameters_edit_nothing_and_fill_every_slot():
    st = _state(1)
    st["step"].fill_(9)
    _edit(st, 1.0, 0, 0)
    assert torch.equal(st["buf"].cpu(), st["raw"]) and bool((st["save_idx"] == -1).all()) and bool((st["save_val"] == 0).all())


def test_graph_replay_at_two_steps_gives_the_eager_bits():
    p, n, min_new = 1.3, 2, 4
    prm = R.Params(p, n, STOPS8[:1], min_new)
    eager = {}
    st = _state(1)
    for step in (3, 11):
        st["step"].fill_(step)
        _edit(st, p, n, min_new)
        eager[step] = st["buf"].clone()
        _restore(st, torch.tensor([6, 6, 6], dtype=torch.int64).cuda())
    st = _state(1)
    cur = torch.tensor([STOPS8[0], 6, 6], dtype=torch.int64).cuda()
    snap = torch.zeros_like(st["buf"])

    def launches():
        _edit(st, p, n, min_new)
        snap.copy_(st["buf"])
        _restore(st, cur)

    st["step"].fill_(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launches()                                               # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launches()
    for step in (3, 11, 3):
        st["step"].fill_(step)
        st["fin"].copy_(torch.tensor([0, 0, 1], dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(snap, eager[step]), step
        assert torch.equal(snap[:, :V].cpu(), R.edit(st["raw"][:, :V], _history(), step, torch.tensor([0, 0, 1]), prm))
        assert torch.equal(st["buf"].cpu(), st["raw"]) and st["fin"].tolist() == [1, 0, 1]


def test_error_codes():
    lib, h = _lib.load(), _lib.ctx(0)
    st = _state(1)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    cur = torch.zeros(B, dtype=torch.int64, device="cuda")

    def edit(logits=st["logits"], ldl=LDL, b=B, v=V, out_ids=st["out_ids"], ld_out=NS, n_steps=NS, step=st["step"], fin=st["fin"], p=1.2, n=0,
             stops=st["stops"], n_stop=1, si=st["save_idx"], sv=st["save_val"], ld_save=2 * NS + 1):
        return lib.crab_logits_edit(h, None, P(logits), ldl, b, v, P(out_ids), ld_out, n_steps, P(step), P(fin), p, n, P(stops), n_stop, 0, P(si), P(sv), ld_save)

    def restore(logits=st["logits"], ldl=LDL, b=B, v=V, cur=cur, fin=st["fin"], stops=st["stops"], n_stop=1, si=st["save_idx"], sv=st["save_val"],
                ld_save=2 * NS + 1, n_slots=2 * NS + 1):
        return lib.crab_logits_restore(h, None, P(logits), ldl, b, v, P(cur), P(fin), P(stops), n_stop, P(si), P(sv), ld_save, n_slots)

    INVALID, UNSUPPORTED = -1, -3
    for k in ("logits", "out_ids", "step", "fin", "si", "sv", "stops"):
        assert edit(**{k: None}) == INVALID, k
    for kw in (dict(b=0), dict(v=0), dict(n_steps=0), dict(p=0.0), dict(p=-2.0), dict(n=-1), dict(n_stop=-1), dict(n_stop=9, ld_save=64),
               dict(ld_save=2 * NS), dict(ldl=V - 1), dict(ld_out=NS - 1)):
        assert edit(**kw) == INVALID, kw
    assert edit(n_steps=8193, ld_out=8193, ld_save=2 * 8193 + 1) == UNSUPPORTED
    assert b"8192" in lib.crab_last_error(h)
    for k in ("logits", "cur", "fin", "si", "sv", "stops"):
        assert restore(**{k: None}) == INVALID, k
    for kw in (dict(b=0), dict(v=0), dict(n_stop=-1), dict(n_stop=9), dict(n_slots=0), dict(n_slots=2 * NS + 2), dict(ldl=V - 1)):
        assert restore(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert torch.equal(st["buf"].cpu(), st["raw"]), "a refused call launched something"
    # the bindings: a stride-0 expanded row is refused (the rows are written), and so are the wrong dtypes
    row = st["buf"][0, :V]
    with pytest.raises(ValueError, match="row stride"):
        ops.logits_edit(row.expand(B, V), st["out_ids"], st["step"], st["fin"], 1.2, 0, st["stops"], 0, st["save_idx"], st["save_val"])
    with pytest.raises(ValueError, match="row stride"):
        ops.logits_restore(row.expand(B, V), cur, st["fin"], st["stops"], st["save_idx"], st["save_val"])
    with pytest.raises(ValueError, match="out_ids"):
        ops.logits_edit(st["logits"], st["out_ids"].int(), st["step"], st["fin"], 1.2, 0, st["stops"], 0, st["save_idx"], st["save_val"])
    with pytest.raises(ValueError, match="stop_ids"):
        ops.logits_edit(st["logits"], st["out_ids"], st["step"], st["fin"], 1.2, 0, st["stops"].long(), 0, st["save_idx"], st["save_val"])
    with pytest.raises(ValueError, match="save_idx"):
        ops.logits_edit(st["logits"], st["out_ids"], st["step"], st["fin"], 1.2, 0, st["stops"], 0, st["save_idx"][:, :2 * NS].contiguous(), st["save_val"])
    with pytest.raises(ValueError, match="save_idx"):
        ops.logits_edit(st["logits"], st["out_ids"], st["step"], st["fin"], 1.2, 0, st["stops"], 0, st["save_idx"].cpu(), st["save_val"])
