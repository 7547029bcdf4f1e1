"""Host-side logic of the shared-prefix generation (no GPU): tile planning, slot / position arithmetic, the memory plan and the ABI symbols."""
import types

import pytest
import torch

from crab_amd import _lib, ops
from crab_amd.decoder import SUFFIX_PASS_ROWS, GenerationEngine, shared_prefix_layout


def test_tile_plan_never_spans_clips_and_forms_partial_tiles():
    # H == Hk: 16 sibling rows per tile.  Clips of 1, 17 and 5 questions: 1 | 16 + 1 | 5
    tiles, row_clip = ops.prefix_tile_plan([1, 17, 5], 32, 32)
    assert tiles == [(0, 1), (1, 16), (17, 1), (18, 5)]
    assert row_clip == [0] + [1] * 17 + [2] * 5
    # H / Hk = 7: two siblings x 7 heads per tile
    tiles, row_clip = ops.prefix_tile_plan([1, 5, 2], 28, 4)
    assert tiles == [(0, 1), (1, 2), (3, 2), (5, 1), (6, 2)]
    # the suffix prefill: clip c owns G_c * Smax consecutive rows
    tiles, row_clip = ops.prefix_tile_plan([3 * 5, 1 * 5], 2, 2)
    assert tiles == [(0, 15), (15, 5)] and row_clip == [0] * 15 + [1] * 5
    for Gs, H, Hk in (([1, 17, 5], 14, 2), ([16], 2, 2), ([33, 1], 4, 2), ([2, 2, 2], 8, 1)):
        tiles, row_clip = ops.prefix_tile_plan(Gs, H, Hk)
        per = 16 // (H // Hk)
        covered = [r for r0, n in tiles for r in range(r0, r0 + n)]
        assert covered == list(range(sum(Gs))) and len(row_clip) == sum(Gs)
        assert all(1 <= n <= per and len({row_clip[r] for r in range(r0, r0 + n)}) == 1 for r0, n in tiles)
    with pytest.raises(ValueError):
        ops.prefix_tile_plan([1, 0], 2, 2)
    with pytest.raises(ValueError):
        ops.prefix_tile_plan([1], 3, 2)


def test_right_alignment_and_positions():
    # P = 5, questions of 2, 5 and 3 rows, 6 new tokens: Smax = 5, Tmax = 64
    lay = shared_prefix_layout(5, [2, 5, 3], 6)
    assert (lay["Smax"], lay["Tmax"]) == (5, 64)
    assert lay["first_slot"] == [3, 0, 2]
    assert lay["rope_off"] == [-2, -5, -3]
    assert lay["pos_ids"] == [[2, 3, 4, 5, 6], [5, 6, 7, 8, 9], [3, 4, 5, 6, 7]]          # live slots: P, P + 1, ...; padding slots below P
    for b, S in enumerate([2, 5, 3]):
        f, ro = lay["first_slot"][b], lay["rope_off"][b]
        assert [s - ro for s in range(f, 5)] == list(range(5, 5 + S)) == lay["pos_ids"][b][f:]
        assert (5 + 0) - ro == 5 + S                                                   # the first decoded token (slot Smax) continues the sequence
    # a long prefix and a padding longer than it: the clamp keeps padding positions valid
    lay = shared_prefix_layout(1, [1, 4], 60)
    assert lay["Tmax"] == 64 and lay["first_slot"] == [3, 0] and lay["rope_off"] == [2, -1]
    assert lay["pos_ids"] == [[0, 0, 0, 1], [1, 2, 3, 4]]
    assert shared_prefix_layout(800, [30], 128)["Tmax"] == 192
    with pytest.raises(ValueError):
        shared_prefix_layout(0, [1], 1)
    with pytest.raises(ValueError):
        shared_prefix_layout(5, [1, 0], 1)


def _engine():
    eng = GenerationEngine.__new__(GenerationEngine)
    eng.cfg = types.SimpleNamespace(num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=32, head_dim=128, hidden_size=4096,
                                    intermediate_size=11008)
    eng.lm_head = types.SimpleNamespace(weight=torch.empty((32017, 4096), dtype=torch.bfloat16, device="meta"))
    eng._ws, eng._stage, eng._kv_mode, eng._w_mode = {}, None, "bf16", "bf16"
    eng.kv_budget_bytes, eng.last_plan = None, None
    return eng


def test_memory_plan_counts_the_prefix_once_per_clip():
    eng = _engine()
    C, G, P, S, n = 100, 5, 800, 30, 128
    kv_row = 2 * 32 * 32 * 128 * 2                                  # K + V bytes of one cached row
    shared = eng.shared_prefix_bytes(C, P, C * G, S, n)
    separate = C * G * eng.bytes_per_sequence(P + S, n) + eng.fixed_bytes(C * G, P + S)
    # exactly one prefix (round_up(800, 64) = 832 rows) per clip, whatever the number of questions
    rest = C * G * eng.bytes_per_sequence(S, n) + C * G * S * 32 * 130 * 4 + max(eng.fixed_bytes(C, P), eng.fixed_bytes(C * G, S))
    assert shared - rest == C * 832 * kv_row
    assert eng.shared_prefix_bytes(C, P, C * 2 * G, S, n) - 2 * C * G * eng.bytes_per_sequence(S, n) - 2 * C * G * S * 32 * 130 * 4 \
        - max(eng.fixed_bytes(C, P), eng.fixed_bytes(2 * C * G, S)) == C * 832 * kv_row
    assert eng.shared_prefix_bytes(C, P, C * (G + 1), S, n) - shared < C * (eng.bytes_per_sequence(S, n) + S * 32 * 130 * 4) + 1
    assert shared < 0.4 * separate
    # waves of whole clips under the row cap and the budget
    eng.kv_budget_bytes = 1 << 50
    waves = eng.plan_shared_prefix([5] * 150, P, S, n)
    assert [c for w in waves for c in w] == list(range(150)) and all(5 * len(w) <= ops.DECODE_MAX_ROWS for w in waves) and len(waves) == 2
    assert eng.last_plan["shared_prefix"] and sum(eng.last_plan["groups"]) == 750
    eng.kv_budget_bytes = int(eng.shared_prefix_bytes(20, P, 100, S, n) / 0.94) + (1 << 20)
    waves = eng.plan_shared_prefix([5] * 100, P, S, n)
    assert len(waves) > 1 and all(eng.shared_prefix_bytes(len(w), P, 5 * len(w), S, n) <= 0.94 * eng.kv_budget_bytes for w in waves)
    # long questions: the wave also has to fit one suffix prefill pass (rows x S <= SUFFIX_PASS_ROWS), so they make smaller waves, not an error
    eng.kv_budget_bytes = 1 << 50
    waves = eng.plan_shared_prefix([5] * 100, P, 100, n)
    assert len(waves) == 2 and all(5 * len(w) * 100 <= SUFFIX_PASS_ROWS for w in waves) and [c for w in waves for c in w] == list(range(100))
    with pytest.raises(ValueError):
        eng.plan_shared_prefix([5], P, SUFFIX_PASS_ROWS // 4, n)
    eng.kv_budget_bytes = 1 << 20
    with pytest.raises(MemoryError):
        eng.plan_shared_prefix([5, 5], P, S, n)
    with pytest.raises(ValueError):
        eng.plan_shared_prefix([ops.DECODE_MAX_ROWS + 1], P, S, n)


def test_bindings_check_their_raw_pointer_arguments():
    """No device needed: the checks come before the library is touched (meta tensors stand in for device memory)."""
    bf = lambda *sh: torch.empty(sh, dtype=torch.bfloat16, device="meta")
    i32 = lambda n: torch.empty((n,), dtype=torch.int32, device="meta")
    q, pk, kc, o = bf(4, 256), bf(1, 2, 8, 128), bf(4, 2, 8, 128), bf(4, 256)
    ws = torch.empty((4 * 2 * 130 * 4,), dtype=torch.uint8, device="meta")
    good = dict(tile_rows=i32(2), row_clip=i32(4))
    import unittest.mock as mock
    with mock.patch.object(ops, "_dev", return_value=0):
        for bad in (dict(ws=ws.view(torch.float32)), dict(ws=ws[::2]), dict(ws=torch.empty((8,), dtype=torch.uint8)), dict(q=bf(4, 128)), dict(q=bf(3, 256)),
                    dict(tile_rows=i32(3)), dict(tile_rows=i32(10)), dict(tile_rows=torch.empty((2,), dtype=torch.int64, device="meta")), dict(row_clip=i32(3))):
            a = dict(q=q, ws=ws, **good); a.update(bad)
            with pytest.raises(ValueError):
                ops.attn_prefix_partial(a["q"], pk, pk, a["ws"], a["tile_rows"], a["row_clip"], 4, 2, 2, 128, 4, 0.1)
        for bad in (dict(ws=ws.view(torch.int32)), dict(q=bf(4, 128)), dict(o=bf(4, 128)), dict(o=bf(3, 256)), dict(kv_start=torch.empty((4,), dtype=torch.int64, device="meta")),
                    dict(ctx_dev=torch.empty((1,), dtype=torch.int64, device="meta"))):
            a = dict(q=q, ws=ws, o=o, kv_start=None, ctx_dev=None); a.update(bad)
            with pytest.raises(ValueError):
                ops.attn_own_merge(a["q"], a["ws"], kc, kc, a["o"], 4, 1, 2, 2, 128, 8, 1, 0.1, ctx_dev=a["ctx_dev"], kv_start=a["kv_start"])


def test_abi_symbols_exist_in_the_built_library():
    lib = _lib.load()
    for name in ("crab_attn_prefix_workspace", "crab_attn_prefix_partial", "crab_attn_own_merge"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.crab_attn_prefix_workspace(512, 32, 128) == 512 * 32 * 130 * 4
    assert lib.crab_attn_prefix_workspace(0, 32, 128) == 0
    # validation comes before any HIP call: a null context is refused without a device
    assert lib.crab_attn_prefix_partial(None, None, None, 0, None, None, None, 0, None, 0, None, 0, 0, 2, 2, 128, 0, 0, 0.1) < 0
    assert lib.crab_attn_own_merge(None, None, None, 0, None, 0, None, None, None, 0, 0, 0, 2, 2, 128, 0, 0, None, 0.1, None) < 0
