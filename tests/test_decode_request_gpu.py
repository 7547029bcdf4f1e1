"""A decode state's key is stable: the same call twice on one engine meets the same _DecodeState and the same captured graph.  An unstable
key would capture on every call, which no comparison of outputs can see.  Here for the entry points no other test pins it for:
generate_many (in flight and coalesced), generate_guided and generate_beam.  The others are pinned where they are tested:
  generate                     tests/test_decode_matrix_gpu.py::test_one_option_at_a_time_on_one_engine_equals_a_fresh_engine_and_recaptures_exactly_when_the_key_changes
  generate_shared_prefix       tests/test_shared_prefix_gpu.py::test_captured_graph_is_reused_on_new_inputs_of_the_same_shapes
  generate_lookup              tests/test_lookup_gpu.py::test_graph_replay_is_eager_bit_for_bit_and_the_graph_is_reused
  generate(shed_finished=...)  tests/test_shed_model_gpu.py::test_state_hygiene (the root state and, by shed_captures == 0, every child)"""
import functools
import os
import runpy

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
S, N_NEW = 5, 4


@functools.lru_cache(maxsize=None)
def _engine():
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](False).base_model.model                     # the tiny Llama of the engine-state fuzzer
    return um._engine, um.config.hidden_size


def _emb(B, rows, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, rows, hid, generator=g) * 0.5).to(BF).cuda()


def _flat(r):
    if isinstance(r, torch.Tensor):
        return [r]
    return [t for x in r for t in _flat(x)] if isinstance(r, (tuple, list)) else []


CASES = {
    "many_in_flight": (2, lambda e, h: e.generate_many([_emb(2, S, h, 1), _emb(1, 3, h, 2)], N_NEW, eos_token_id=None, pad_token_id=2,
                                                       return_first_logits=True)),
    "many_coalesced": (1, lambda e, h: e.generate_many([_emb(2, S, h, 1), _emb(1, 3, h, 2)], N_NEW, eos_token_id=None, pad_token_id=2, coalesce=True,
                                                       return_step_logits=True)),
    "guided": (1, lambda e, h: e.generate_guided(_emb(2, S, h, 3), _emb(2, 3, h, 4), 1.5, N_NEW, eos_token_id=None, pad_token_id=2,
                                                 return_step_logits=True)),
    "beam": (1, lambda e, h: e.generate_beam(_emb(2, S, h, 5), 2, N_NEW, eos_token_id=None, pad_token_id=2, return_scores=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_same_call_twice_meets_the_same_state_and_graph(name):
    eng, hid = _engine()
    slots, call = CASES[name]
    eng.invalidate()
    first = [t.clone() for t in _flat(call(eng, hid))]
    sts = [eng._dec[g] for g in range(slots)]
    graphs = [st.graph for st in sts]
    assert len(eng._dec) == slots and all(g is not None for g in graphs), "the call did not decode through captured graphs"
    second = _flat(call(eng, hid))
    assert all(eng._dec[g] is sts[g] and eng._dec[g].graph is graphs[g] for g in range(slots)), "the repeated call built a new state or captured again"
    assert len(first) == len(second) > 0 and all(torch.equal(a, b) for a, b in zip(first, second))
