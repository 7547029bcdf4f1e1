"""Host logic of crab_amd/decoder.py that needs no GPU: the one-retry wrapper around generate() / generate_many() (lazy eviction), the
one call entry that applies it, the EOS trim, the wave packing of generate_many(coalesce=True) and the scratch-slot context manager."""
import gc
import types
import weakref

import pytest
import torch

from crab_amd import decoder, ops


class _Engine:
    """The four attributes _retry_after_eviction touches."""

    def __init__(self):
        self._kv, self._dec, self._ws, self.invalidated = {"slot": 1}, {}, {}, 0

    def invalidate(self):
        self.invalidated += 1
        self._kv = {}


class _Big:                       # stands for a tensor a failed attempt still holds in a local
    pass


def test_retry_runs_once_after_dropping_everything_and_outside_the_except_clause():
    eng, calls, held = _Engine(), [], []

    def attempt():
        calls.append(len(calls))
        if len(calls) == 1:
            big = _Big()
            held.append(weakref.ref(big))
            raise torch.cuda.OutOfMemoryError("HIP out of memory (simulated)")     # `big` lives in this frame, the frame in the traceback
        # second attempt: the first attempt's locals must be gone (a retry from INSIDE the except clause would still see them through the traceback)
        gc.collect()
        assert held[0]() is None
        return "ok"

    assert decoder.GenerationEngine._retry_after_eviction(eng, attempt) == "ok"
    assert calls == [0, 1] and eng.invalidated == 1


def test_retry_gives_up_when_nothing_is_cached_and_after_a_second_failure():
    eng = _Engine()
    eng._kv = {}

    def always():
        raise torch.cuda.OutOfMemoryError("HIP out of memory (simulated)")

    with pytest.raises(torch.cuda.OutOfMemoryError):
        decoder.GenerationEngine._retry_after_eviction(eng, always)                # nothing to drop: the caller's error
    assert eng.invalidated == 0
    eng._kv = {"slot": 1}
    with pytest.raises(torch.cuda.OutOfMemoryError):
        decoder.GenerationEngine._retry_after_eviction(eng, always)                # one retry, then the caller's
    assert eng.invalidated == 1


def test_an_out_of_memory_error_in_a_nested_path_is_retried_once_by_the_outermost_call_only():
    """generate_many with a single batch runs generate()'s body.  It used to re-enter the public generate(), whose own retry nested into the
    outer one: a persistent out-of-memory error ran the body four times with three invalidate() calls in between.  One entry (_call), and
    _generate called directly inside the engine: two runs, one invalidate()."""
    eng = object.__new__(decoder.GenerationEngine)
    eng._kv, eng._dec, eng._ws, eng._kv_mode, eng._w_mode, eng._w_used, eng.last_plan = {"slot": 1}, {}, {}, "bf16", "bf16", None, None
    runs, dropped = [], []

    def invalidate():
        dropped.append(1)
        eng._kv = {}

    def body(*a, **k):
        runs.append(1)
        eng._kv = {"slot": 1}                                   # the attempt allocated its cache again before it ran out of memory
        raise torch.cuda.OutOfMemoryError("HIP out of memory (simulated)")

    eng.invalidate, eng._generate = invalidate, body
    with pytest.raises(torch.cuda.OutOfMemoryError):
        eng.generate_many([torch.zeros(1, 3, 8)], 4)
    assert (len(runs), len(dropped)) == (2, 1)
    assert eng._w_mode == "bf16" and eng._kv_mode == "bf16"
    # no method of the engine (nested functions included) so much as names its public entries

    def names(code):
        return set(code.co_names).union(*(names(c) for c in code.co_consts if isinstance(c, types.CodeType)))

    for name, fn in vars(decoder.GenerationEngine).items():
        code = getattr(getattr(fn, "__wrapped__", fn), "__code__", None)
        assert code is None or not names(code) & {"generate", "generate_many"}, f"{name}: the engine re-enters its public entry"


_BUF = [[5, 7, 9, 2, 2, 2, 2, 2], [4, 4, 4, 4, 9, 2, 2, 2]]


@pytest.mark.parametrize("rows, n_done, eos, want", [
    (2, 8, 9, [[5, 7, 9, 2, 2], [4, 4, 4, 4, 9]]),               # cut after the column at which the LAST row finishes
    (2, 8, -1, _BUF),                                            # no stop id
    (2, 3, 9, [[5, 7, 9], [4, 4, 4]]),                           # row 1 has not finished within n_done: no cut
    (1, 8, 9, [[5, 7, 9]]),
    (2, 8, 3, _BUF),                                             # the stop id never appears
])
def test_trim_at_eos(rows, n_done, eos, want):
    buf = torch.tensor(_BUF)[:rows]
    keep = buf.clone()
    out = decoder._trim_at_eos(buf, n_done, eos)
    assert out.tolist() == want[:rows]
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, keep)      # a view of the buffer, which is left alone


@pytest.mark.parametrize("Bs, cap, rows, waves", [
    ([8] * 60, 448, [240, 240], None),                           # even waves, not 448 + 32
    ([8] * 3, 448, [24], None),
    ([1, 2, 1], 2, [1, 2, 1], [[0], [1], [2]]),
    ([5, 600, 3], 448, [5, 600, 3], [[0], [1], [2]]),            # a batch above the cap is a wave of its own
    ([8] * 7, 20, [16, 16, 16, 8], None),                        # four waves although ceil(56 / 20) = 3 sets the target: pinned as it is
])
def test_pack_waves(Bs, cap, rows, waves):
    got = decoder._pack_waves(Bs, cap)
    assert [sum(Bs[g] for g in w) for w in got] == rows
    assert [g for w in got for g in w] == list(range(len(Bs)))  # every batch once, in order
    if waves is not None:
        assert got == waves


def test_ws_slot_is_restored_after_an_exception():
    before = ops.WS_SLOT
    with pytest.raises(RuntimeError):
        with decoder._ws_slot(before + 3):
            assert ops.WS_SLOT == before + 3
            with decoder._ws_slot(before + 1):
                assert ops.WS_SLOT == before + 1
            assert ops.WS_SLOT == before + 3
            raise RuntimeError("a start that fails")
    assert ops.WS_SLOT == before


def test_workspace_queries_are_monotone_so_that_one_buffer_serves_every_smaller_call():
    """r06: callers size ONE workspace for their largest chunk (decoder._Workspace.t for the prefill chunk) and reuse it for the smaller last chunk.
    crab_hyperlora_route_workspace used to return slices(M) * M, which is not monotone (M = 57 344: 5 slices, M = 50 000: 6 -> 5 % more), and
    generate_avs_many with 512 samples failed with "hyperlora_route: workspace too small".  Every query is now non-decreasing in every argument."""
    from crab_amd import _lib
    lib = _lib.load()
    for K in (768, 4096, 11008, 18944):
        prev = 0
        for M in list(range(1, 5000, 7)) + list(range(5000, 400000, 997)):
            w = lib.crab_hyperlora_route_workspace(M, K, 48)
            assert w >= prev, (M, K, w, prev)
            prev = w
        assert lib.crab_hyperlora_route_workspace(50000, K, 48) <= lib.crab_hyperlora_route_workspace(57344, K, 48)
    assert lib.crab_hyperlora_route_workspace(4096, 4096, 48) <= lib.crab_hyperlora_route_workspace(4096, 11008, 48)
    for N in (1, 64, 1000, 16384):
        prev = 0
        for M in range(1, 40000, 13):
            w = lib.crab_vq_nearest_f32_workspace(M, N)
            assert w >= prev, (M, N, w, prev)
            prev = w
    for q, args in ((lib.crab_rowfin_workspace, [(m, 4096) for m in range(1, 17)]), (lib.crab_attn_decode_rope_workspace, [(b, 32, 128) for b in range(1, 64)]),
                    (lib.crab_groupnorm_workspace, [(2, hw, 32) for hw in range(1, 70000, 101)])):
        vals = [q(*a) for a in args]
        assert vals == sorted(vals)
