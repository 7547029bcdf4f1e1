"""crab_kv_compact_rows and crab_sample_select_rows on the GPU (the kernels under shed_finished).

crab_kv_compact_rows: the reference is a row gather on a CPU clone, compared byte for byte.  The caches are views of 6 rows in a 7-row allocation
(layer stride 7 rows) that sits between 0xA5 guard bands; the bands, the 7th row of every layer, the rows >= n_live and the slots > pos must
come back unchanged.  Below a row's row_off the entry point may copy or not ("copying more slots than required is allowed"): there a byte
has to be the destination's old one or the source's.  No test feeds out-of-contract device indices.

crab_sample_select_rows: the existing crab_sample_select / crab_sample_select_warped on all six rows is the reference; the new entry on the
gathered rows (1, 3, 4) with row_ids = (1, 3, 4) must write the same words for them."""
import itertools

import pytest
import torch

from crab_amd import ops

pytestmark = pytest.mark.gpu
GUARD = 64                                                       # int16 elements = 128 bytes on either side
PATTERNS = {"identity": (0, 1, 2, 3, 4, 5), "shift_by_one": (1, 2, 3, 4, 5), "alternate": (0, 2, 4), "tail": (3, 4, 5), "last": (5,)}


def _caches(L, rows, alloc_rows, Hk, Tmax, d, seed):
    """Two bf16 cache views [L, rows, Hk, Tmax, d] of allocations with alloc_rows rows per layer, random bits everywhere inside 0xA5 bands."""
    g = torch.Generator().manual_seed(seed)
    n = L * alloc_rows * Hk * Tmax * d
    out = []
    for _ in range(2):
        flat = torch.full((n + 2 * GUARD,), -23131, dtype=torch.int16)           # 0xA5A5
        flat[GUARD:GUARD + n] = torch.randint(-32768, 32767, (n,), generator=g, dtype=torch.int16)
        dev = flat.cuda()
        view = dev[GUARD:GUARD + n].view(torch.bfloat16).view(L, alloc_rows, Hk, Tmax, d)[:, :rows]
        out.append((flat, dev, view))
    return out


def _check(what, before, after, L, rows, alloc_rows, Hk, Tmax, d, src, pos, off):
    n = L * alloc_rows * Hk * Tmax * d
    assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + n:], before[GUARD + n:]), f"{what}: a guard band changed"
    b = before[GUARD:GUARD + n].view(L, alloc_rows, Hk, Tmax, d)
    a = after[GUARD:GUARD + n].view(L, alloc_rows, Hk, Tmax, d)
    assert torch.equal(a[:, len(src):], b[:, len(src):]), f"{what}: a row >= n_live (or the allocation's padding row) changed"
    assert torch.equal(a[:, :, :, pos + 1:], b[:, :, :, pos + 1:]), f"{what}: a slot above pos changed"
    for j, s in enumerate(src):
        o = 0 if off is None else off[s]
        assert torch.equal(a[:, j, :, o:pos + 1], b[:, s, :, o:pos + 1]), f"{what}: row {j} is not row {s} over the slots {o} .. {pos}"
        low_a, low_d, low_s = a[:, j, :, :o], b[:, j, :, :o], b[:, s, :, :o]
        assert bool(((low_a == low_d) | (low_a == low_s)).all()), f"{what}: row {j} below row_off holds neither its own nor its source's bytes"


def _run(what, L, rows, alloc_rows, Hk, Tmax, d, src, pos, off, seed=0):
    (kb, kd, kc), (vb, vd, vc) = _caches(L, rows, alloc_rows, Hk, Tmax, d, seed)
    pos_dev = torch.tensor([pos], dtype=torch.int32).cuda()
    off_dev = torch.tensor(off, dtype=torch.int32).cuda() if off is not None else None
    ops.kv_compact_rows(kc, vc, list(src), pos_dev, off_dev)
    torch.cuda.synchronize()
    _check(what + " K", kb, kd.cpu(), L, rows, alloc_rows, Hk, Tmax, d, src, pos, off)
    _check(what + " V", vb, vd.cpu(), L, rows, alloc_rows, Hk, Tmax, d, src, pos, off)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_compaction_equals_the_gather_on_a_clone(pattern):
    src = PATTERNS[pattern]
    for Hk, d, Tmax, with_off in itertools.product((2, 3), (64, 128), (64, 128), (False, True)):
        for pos in (0, 37, Tmax - 1):
            # per-row first slots, none beyond pos: 0, pos itself (the row holds one slot), and values in between
            off = [0, pos, min(3, pos), min(11, pos), pos, min(1, pos)] if with_off else None
            _run(f"{pattern} Hk={Hk} d={d} Tmax={Tmax} pos={pos} row_off={'yes' if with_off else 'null'}", 2, 6, 7, Hk, Tmax, d, src, pos, off,
                 seed=Hk * 1000 + d + Tmax + pos)


def test_one_row_cache():
    for pos in (0, 37, 63):
        _run(f"one row pos={pos}", 2, 1, 2, 2, 64, 64, (0,), pos, None)
        _run(f"one row pos={pos} row_off", 2, 1, 2, 2, 64, 64, (0,), pos, [min(5, pos)])


def test_a_larger_cache_and_the_grid_stride_loop(monkeypatch):
    src = tuple(range(1, 40, 2))                                 # alternate rows survive: 20 of 40, three batches of the row walk
    _run("L=4 rows=40", 4, 40, 40, 4, 256, 128, src, 200, None, seed=7)
    _run("L=4 rows=40 row_off", 4, 40, 41, 4, 256, 128, src, 255, [(7 * r) % 200 for r in range(40)], seed=8)
    # more 16-byte positions (5 * 8 * 1024 * 16 = 655360) than the capped grid has threads (2048 * 256): every thread takes a second position
    _run("grid stride", 5, 3, 3, 8, 1024, 128, (1, 2), 1023, None, seed=9)
    # a cache past the entry point's 2^31 units goes layer group by layer group (ops.kv_compact_rows): here groups of two, two and one layers
    per_layer = 7 * 3 * 64 * 128 // 8
    monkeypatch.setattr(ops, "COMPACT_MAX_UNITS", 2 * per_layer + 1)
    _run("layer groups", 5, 6, 7, 3, 64, 128, (1, 3, 5), 63, [0, 5, 0, 63, 0, 9], seed=10)


# ------------------------------------------------------------------ crab_sample_select_rows
ROWS = (1, 3, 4)


def _select_pair(V, step, sampling, eos, min_new, fin0, seed=11):
    """(reference words of rows ROWS, new entry's words): the existing kernel on six rows against the new one on the three gathered rows."""
    g = torch.Generator().manual_seed(1000 * V + step)
    logits = (torch.randn(6, V, generator=g) * 3).cuda()
    n_cols = 9
    step_dev = torch.tensor([step], dtype=torch.int32).cuda()
    cur = torch.full((6,), 5, dtype=torch.int64).cuda()
    out = torch.full((6, n_cols), 5, dtype=torch.int64).cuda()
    fin = torch.tensor(fin0, dtype=torch.int32).cuda()
    idx = torch.tensor(ROWS).cuda()
    cur2, out2, fin2, lg2 = cur[idx].clone(), out[idx].clone(), fin[idx].clone(), logits[idx].clone()
    if len(sampling) == 4:
        ops.sample_select(logits, cur, out, step_dev, fin, eos, 2, min_new, *sampling[:3], seed)
    else:
        ops.sample_select_warped(logits, cur, out, step_dev, fin, eos, 2, min_new, *sampling[:3], seed, *sampling[4:])
    row_ids = torch.tensor(ROWS, dtype=torch.int32).cuda()
    ops.sample_select_rows(row_ids, lg2, cur2, out2, step_dev, fin2, eos, 2, min_new, *sampling[:3], seed, *sampling[4:])
    torch.cuda.synchronize()
    return (cur[idx].cpu(), out[idx].cpu(), fin[idx].cpu()), (cur2.cpu(), out2.cpu(), fin2.cpu())


@pytest.mark.parametrize("V", [1000, 32000])
@pytest.mark.parametrize("sampling", [(0.8, 50, 0.9, 0), (0.8, 50, 0.9, 0, 0.05, 0.0, 0.0), (1.0, 0, 1.0, 0, 0.0, 3e-4, 2e-3)], ids=["plain", "min_p", "cutoffs"])
def test_rows_entry_writes_the_words_of_the_existing_kernels(V, sampling):
    for step in (0, 1, 7):
        ref, got = _select_pair(V, step, sampling, -1, 0, [0] * 6)
        for r, g_, name in zip(ref, got, ("cur_ids", "out_ids", "finished")):
            assert torch.equal(r, g_), f"V={V} step={step}: {name} differ: {r.tolist()} vs {g_.tolist()}"
        picked = ref[0].tolist()
        # a finished row leaves its words alone but for the pad it emits; an EOS that is drawn finishes the row in both
        ref, got = _select_pair(V, step, sampling, picked[0], 0, [0, 0, 0, 1, 0, 0])
        assert all(torch.equal(r, g_) for r, g_ in zip(ref, got)), f"V={V} step={step}: finished row / drawn EOS"
        assert got[2].tolist() == [1, 1, 0] or picked[2] == picked[0], "row 1 drew the EOS, row 3 was finished"
        assert int(got[0][1]) == 2 and int(got[1][1, step]) == 2, "the finished row emits the pad id"
        # min_new_tokens suppresses the EOS in both
        ref, got = _select_pair(V, step, sampling, picked[0], 8, [0] * 6)
        assert all(torch.equal(r, g_) for r, g_ in zip(ref, got)), f"V={V} step={step}: min_new_tokens"
        assert int(got[0][0]) != picked[0] and got[2].tolist() == [0, 0, 0], "the EOS was suppressed"


def test_row_ids_are_the_key_of_the_draw():
    """The same logits under another row id draw another stream: the operand is read (a kernel that ignored it would pass the test above only
    with row_ids = block index)."""
    V, sampling = 32000, (1.0, 0, 1.0, 0)
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(1, V, generator=g) * 0.1).expand(6, V).contiguous().cuda()      # six equal, flat rows: the draw decides
    step_dev = torch.zeros((1,), dtype=torch.int32).cuda()
    cur, out, fin = torch.zeros((6,), dtype=torch.int64).cuda(), torch.zeros((6, 4), dtype=torch.int64).cuda(), torch.zeros((6,), dtype=torch.int32).cuda()
    ops.sample_select(logits, cur, out, step_dev, fin, -1, 2, 0, *sampling[:3], 5)
    cur2, out2, fin2 = torch.zeros_like(cur), torch.zeros_like(out), torch.zeros_like(fin)
    ops.sample_select_rows(torch.tensor([5, 4, 3, 2, 1, 0], dtype=torch.int32).cuda(), logits, cur2, out2, step_dev, fin2, -1, 2, 0, *sampling[:3], 5)
    assert cur2.tolist() == cur.flip(0).tolist() and len(set(cur.tolist())) > 1
