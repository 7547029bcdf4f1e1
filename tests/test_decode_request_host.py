"""The three places a per-call option of the generation engine lives, on the host (CPU tensors, no device): the request record (_Request),
the key of a decode state (_state_key / stop_words / _child_key) and the collector of what a call returns (_Collect, _join); and the
defaults of _DecodeState."""
import ast
import json
import os

import pytest
import torch

from crab_amd import decoder
from crab_amd.decoder import _Collect, _DecodeState, _Request, _child_key, _join, _state_key, stop_words

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_state_keys.json")

# the arguments of a state as the engine's _state meets them: the caller's eos / pad / processors and the values it reads off its buffers
BASE = dict(B=3, S=5, Tmax=64, max_new_tokens=8, eos_token_id=2, pad_token_id=None, min_new_tokens=0, return_hidden=False,
            ptrs=(1000, 2000, 3000, 4000, 5000, 6000, 7000), lora=True, sampling=None, ragged=False, kv_mode="bf16", scale_ptrs=(0, 0),
            w8_key=("bf16",), logprobs=False, extra_key=(), trie_key=(), processors=None, cfg=None, lookup=None)


def _key(**change):
    """What _state does with its arguments: the one eos id, stop_words, then _state_key."""
    a = dict(BASE, **change)
    eos, proc, pad = stop_words(decoder.one_eos(a.pop("eos_token_id"), "refused"), a.pop("pad_token_id"), a.pop("processors"))
    return _state_key(eos=eos, pad=pad, proc=proc, **a)


# ------------------------------------------------------------------ (a) the key
CHANGES = [dict(B=4), dict(Tmax=128), dict(max_new_tokens=9), dict(eos_token_id=3), dict(eos_token_id=None), dict(pad_token_id=0), dict(min_new_tokens=1),
           dict(return_hidden=True), dict(lora=False), dict(sampling=(0.7, 50, 0.9, 11)), dict(ragged=True), dict(kv_mode="fp8_e4m3"),
           dict(scale_ptrs=(8, 0)), dict(scale_ptrs=(0, 8)), dict(w8_key=("fp8_e4m3", 11, 12)), dict(logprobs=True),
           dict(trie_key=("trie", 21, 22, 23, 40, 41)), dict(processors=(1.3, 0, ())), dict(processors=(1.0, 2, ())), dict(processors=(1.0, 0, (7,))),
           dict(cfg=(2.5, 3)), dict(lookup=(3, 2, False)), dict(extra_key=(5, (2, 1), 101))] + \
          [dict(ptrs=tuple(p + (1 if i == j else 0) for j, p in enumerate(BASE["ptrs"]))) for i in range(7)]


@pytest.mark.parametrize("change", CHANGES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items())[:60])
def test_every_single_change_changes_the_key(change):
    assert _key(**change) != _key()


def test_what_leaves_the_key_alone_and_the_lookup_and_child_forms():
    base = _key()
    assert _key() == base and hash(base) is not None
    for neutral in ((1.0, 0, ()), (None, None, None), (1.0, 0, (2,)), (1, 0, [2, 2])):      # neutral, or only repeating eos: the call without it
        assert _key(processors=neutral) == base, neutral
    assert _key(eos_token_id=[2]) == base and _key(eos_token_id=(2, 2)) == base and _key(pad_token_id=2) == base
    assert _key(S=6) == base, "a plain state meets S through pos_dev alone"
    lk = _key(lookup=(3, 2, True))
    assert _key(lookup=(3, 2, True), S=6) != lk and _key(lookup=(4, 2, True)) != lk and _key(lookup=(3, 1, True)) != lk and _key(lookup=(3, 2, False)) != lk
    assert _key(cfg=(2.5, 4)) != _key(cfg=(2.5, 3)) != _key(cfg=(3.0, 3))
    w8 = ("fp8_e4m3", 11, 12)
    assert _child_key(base, 4, w8) == base + ("shed", 4) + w8 and _child_key(base, 4, ("bf16",)) == base + ("shed", 4, "bf16")
    with pytest.raises(NotImplementedError, match=r"eos_token_id = \[2, 3\]: refused"):
        _key(eos_token_id=[2, 3])
    assert decoder.one_eos([], "x") is None and decoder.one_eos(None, "x") is None and decoder.one_eos(5, "x") == 5


def test_stop_words_and_join_pad_differ_where_they_should():
    assert stop_words(None, None, None) == (-1, None, 0) and stop_words(2, None, None) == (2, None, 2) and stop_words(2, 0, None) == (2, None, 0)
    assert stop_words(None, None, (1.0, 0, (7, 9))) == (-1, (1.0, 0, (7, 9)), 7), "a finished row emits the first further stop id"
    assert stop_words(2, None, (1.2, 0, (2, 7))) == (2, (1.2, 0, (7,)), 2)
    # join_pad: pad -> eos -> 0, and never a further stop id
    assert _Request(8, 2, 0).join_pad == 0 and _Request(8, 2).join_pad == 2 and _Request(8).join_pad == 0
    assert _Request(8, None, None, processors=(1.0, 0, (7, 9))).join_pad == 0


def test_the_new_function_reproduces_the_keys_of_the_expression_it_replaced():
    gold = json.load(open(GOLDEN))
    base = ast.literal_eval(gold["baseline"]["args"])
    assert base == BASE
    assert _key() == ast.literal_eval(gold["baseline"]["key"])
    assert len(gold["variants"]) == 6
    for v in gold["variants"]:
        want = ast.literal_eval(v["key"])
        got = _key(**ast.literal_eval(v["change"]))
        assert got == want and [type(x) for x in got] == [type(x) for x in want], v["name"]


# ------------------------------------------------------------------ (b) the request
def test_request_derives_and_replaces():
    r = _Request(8, 2)
    assert r.graphed and not _Request(2, 2).graphed and not _Request(8, 2, use_graph=False).graphed and _Request(3).graphed
    assert r == _Request(8, 2, None, 0, True, None, None) and r != _Request(8, 3) and hash(r) == hash(_Request(8, 2))
    with pytest.raises(Exception):
        r.eos = 3                                                # frozen
    w = r.replace(sampling=(0.7, 5, 0.8, 16), cfg=(2.5, 3), extra_key=(1, 2))
    assert (w.sampling, w.cfg, w.extra_key, w.max_new_tokens, w.eos) == ((0.7, 5, 0.8, 16), (2.5, 3), (1, 2), 8, 2) and r.cfg is None
    con = decoder._Constraint("dev", [4, 5, 6, 7])
    g = _Request(8, 2, sampling=(0.7, 5, 0.8, 11), constraint=con).rows(1, 3)
    assert g.sampling == (0.7, 5, 0.8, 11) and g.constraint.roots == [5, 6] and g.constraint.dev == "dev"
    assert r.rows(0, 2) is r


# ------------------------------------------------------------------ (c) the collector
V, D_ = 6, 4


def _state(B=3, n_cols=4, eos=9):
    """A stand-in state on CPU tensors: two groups (rows 0-1 and row 2); the first group's rows both emit EOS in column 1."""
    st = _DecodeState()
    st.B, st.eos_all = B, (eos,)
    st.out_ids = torch.tensor([[5, 9, 2, 2], [6, 9, 2, 2], [7, 8, 7, 8]])
    st.logits = torch.zeros((B, V))
    st.hn = torch.zeros((B, D_))
    st.lp = torch.arange(2 * B * n_cols, dtype=torch.float32).reshape(2, B, n_cols)
    return st


def _run(col, st, steps=4):
    """The sink calls of a wave: the first token, then (where something is kept per step) every step."""
    for s in range(steps):
        st.logits.fill_(float(s + 1)); st.hn.fill_(float(-s - 1))
        if s == 0:
            col(st)
        elif col.on_step is not None:
            col.on_step(st)


FLAGS = ("return_step_logits", "return_hidden", "return_first_logits", "return_logprobs")


@pytest.mark.parametrize("flags", [(), ("return_step_logits",), ("return_hidden",), ("return_first_logits",), ("return_logprobs",),
                                   ("return_step_logits", "return_logprobs"), ("return_hidden", "return_logprobs"),
                                   ("return_first_logits", "return_logprobs")], ids=lambda f: "+".join(f) or "ids")
def test_per_group_layout_of_the_coalesced_and_shared_prefix_forms(flags):
    """generate_many (both forms) and generate_shared_prefix: (ids, step logits | hidden | first logits, log-probs last), per group."""
    st, req = _state(), _Request(4, 9, **{f: True for f in flags})
    col = _Collect(req)
    _run(col, st)
    assert (col.on_step is col) == bool({"return_step_logits", "return_hidden"} & set(flags))
    outs = col.groups(st, st.out_ids, [2, 1], 4)
    assert len(outs) == 2
    for (r0, r1, n), r in zip(((0, 2, 2), (2, 3, 4)), outs):
        if not flags:
            assert isinstance(r, torch.Tensor), "a lone ids tensor is not wrapped"
            r = (r,)
        assert isinstance(r, tuple) and len(r) == 1 + len(flags)
        assert torch.equal(r[0], st.out_ids[r0:r1, :n]) and r[0].data_ptr() != st.out_ids.data_ptr()      # trimmed at the GROUP's EOS, and a copy
        if "return_step_logits" in flags:
            assert r[1].shape == (r1 - r0, n, V) and r[1][0, :, 0].tolist() == [float(s + 1) for s in range(n)]
        if "return_hidden" in flags:
            assert r[1].shape == (r1 - r0, n, D_) and r[1][0, :, 0].tolist() == [float(-s - 1) for s in range(n)]
        if "return_first_logits" in flags:
            assert r[1].shape == (r1 - r0, V) and bool((r[1] == 1.0).all()), "the first logits are cloned once, at the first token"
        if "return_logprobs" in flags:
            assert r[-1].shape == (r1 - r0, n, 2) and torch.equal(r[-1], st.lp[:, r0:r1, :n].permute(1, 2, 0))


@pytest.mark.parametrize("flags", [(), ("return_step_logits",), ("return_hidden",), ("return_first_logits",), ("return_logprobs",), FLAGS,
                                   ("return_step_logits", "return_first_logits"), ("return_hidden", "return_first_logits", "return_logprobs")],
                         ids=lambda f: "+".join(f) or "ids")
def test_whole_call_layout_of_generate(flags):
    """generate(): ids, step logits, hidden, first logits, log-probs - in this order, whatever subset is asked for."""
    st, req = _state(eos=-1), _Request(4, None, **{f: True for f in flags})
    col = _Collect(req, 1, 3)
    _run(col, st)
    r = col.whole([st], decoder._trim_at_eos(st.out_ids, 3, st.eos_all))
    if not flags:
        assert isinstance(r, torch.Tensor)
        r = (r,)
    assert len(r) == 1 + len(flags) and torch.equal(r[0], st.out_ids[:, :3]) and r[0].data_ptr() != st.out_ids.data_ptr()
    want = {"return_step_logits": (3, 3, V), "return_hidden": (3, 3, D_), "return_first_logits": (3, V), "return_logprobs": (3, 3, 2)}
    assert [tuple(t.shape) for t in r[1:]] == [want[f] for f in FLAGS if f in flags]
    if "return_hidden" in flags:
        assert float(r[1 + int("return_step_logits" in flags)][0, 0, 0]) == -1.0


def test_the_groups_of_a_split_decode_are_joined_in_row_order():
    """generate(decode_streams = 2): one clone of the first logits per state, not one per step; the scores of all states, in row order."""
    a, b = _state(), _state()
    req = _Request(4, None, return_first_logits=True, return_logprobs=True)
    col = _Collect(req, 2, 6)
    a.logits.fill_(1.0); b.logits.fill_(2.0)
    col(a); col(b); col(a); col(a)
    assert len(col.first) == 2
    ids, first, lp = col.whole([a, b], torch.cat([a.out_ids, b.out_ids], 0))
    assert ids.shape == (6, 4) and first.shape == (6, V) and first[:, 0].tolist() == [1.0] * 3 + [2.0] * 3 and lp.shape == (6, 4, 2)
    # generate_many in flight: every batch is a call of its own with its own collector
    cols = [_Collect(req), _Collect(req)]
    cols[0](a); cols[1](b)
    ra, rb = cols[0].rows(a, a.out_ids, 0, 3, 4), cols[1].rows(b, b.out_ids, 0, 3, 4)
    assert len(ra) == 3 and bool((ra[1] == 1.0).all()) and bool((rb[1] == 2.0).all()) and ra[2].shape == (3, 4, 2)


def test_step_logits_of_a_shed_child_land_under_the_rows_wave_indices():
    req = _Request(6, 9, return_step_logits=True)
    col = _Collect(req, 1, 5)
    root = _state(B=5)
    root.logits = torch.ones((5, V))
    col(root)
    ch = _DecodeState()                                          # a rung of 4 rows that carries the wave's rows 3 and 1 on; two fillers
    ch.B, ch.rows, ch.rows_idx, ch.n_real = 4, torch.tensor([3, 1, -1, -1], dtype=torch.int32), torch.tensor([3, 1]), 2
    ch.logits = torch.tensor([[30.0] * V, [10.0] * V, [77.0] * V, [88.0] * V])
    col.on_step(ch)
    sl = torch.stack(col.steps, 1)
    assert sl.shape == (5, 2, V) and bool((sl[:, 0] == 1.0).all())
    assert sl[:, 1, 0].tolist() == [0.0, 10.0, 0.0, 30.0, 0.0], "real rows under rows_idx, zeros where a row has been shed, no filler"


# ------------------------------------------------------------------ (d) the join
def test_join_pads_the_shorter_parts_and_leaves_the_first_logits_alone():
    ids = lambda B, n, v: torch.full((B, n), v, dtype=torch.int64)
    parts = [(ids(2, 2, 5), torch.ones((2, 2, V)), torch.full((2, V), 3.0), torch.ones((2, 2, 2))),
             (ids(1, 5, 6), torch.ones((1, 5, V)), torch.full((1, V), 4.0), torch.ones((1, 5, 2)))]
    out, sl, first, lp = _join(parts, 7, keep=2)
    assert out.tolist() == [[5, 5, 7, 7, 7]] * 2 + [[6] * 5]
    assert sl.shape == (3, 5, V) and bool((sl[:2, 2:] == 0).all()) and bool((sl[:2, :2] == 1).all()) and bool((sl[2] == 1).all())
    assert first.shape == (3, V) and first[:, 0].tolist() == [3.0, 3.0, 4.0], "first logits have no step axis: never widened"
    assert lp.shape == (3, 5, 2) and bool((lp[:2, 2:] == 0).all())
    assert torch.equal(_join([(ids(2, 3, 1),), (ids(1, 3, 2),)], 7)[0], torch.tensor([[1] * 3] * 2 + [[2] * 3]))
    # V == n_max must not make first logits look like a short per-step tensor either
    short = [(ids(1, 2, 5), torch.full((1, 2), 3.0)), (ids(1, 5, 6), torch.full((1, 2), 4.0))]
    assert _join(short, 0, keep=1)[1].shape == (2, 2)


# ------------------------------------------------------------------ (e) the state's defaults
def test_a_fresh_decode_state_has_every_attribute_the_step_functions_read():
    st = _DecodeState()
    # _decode_step / _lookup_step, _select, _select_token, _capture (crab_amd/decoder.py), and what _run_steps / _shed_to / the sinks read
    read = {"_decode_step": "lookup B ws cur_ids kc vc Tmax pos_dev row_off ks vs w8 prefix logits want_hidden hn step_dev S eos pad finished out_ids min_new",
            "_select": "beam logits step_dev finished eos min_new cur_ids out_ids kc vc pos_dev cfg guided lp lp_norm trie node proc stop_dev save_idx save_val",
            "_select_token": "logits trie sampling node cur_ids out_ids step_dev finished eos pad min_new slot rows",
            "_capture": "graph cur_ids out_ids finished pos_dev step_dev node lookup beam",
            "others": "key eos_all children rows_idx rows_host n_real"}
    for fn, names in read.items():
        for n in names.split():
            assert hasattr(st, n), (fn, n)
    for n in ("graph", "ks", "vs", "row_off", "hn", "sampling", "prefix", "beam", "trie", "node", "lp", "lp_norm", "proc", "save_idx", "save_val", "stop_dev",
              "cfg", "guided", "lookup", "children", "rows", "rows_idx", "rows_host"):
        assert getattr(st, n) is None, n
    assert st.w8 is False and st.want_hidden is False and st.eos == -1 and st.eos_all == (-1,)
    st.alloc("cpu", 3, 4, V, ragged=True)
    assert st.logits.shape == (3, V) and st.out_ids.shape == (3, 4) and st.cur_ids.dtype == st.out_ids.dtype == torch.int64
    assert st.finished.shape == (3,) and st.pos_dev.shape == st.step_dev.shape == (1,) and st.row_off.tolist() == [0, 0, 0]
    assert all(t.dtype == torch.int32 for t in (st.finished, st.pos_dev, st.step_dev, st.row_off))
    lg = torch.zeros((5, V))
    st.alloc("cpu", 1, 4, V, ragged=False, logits=lg[:1])
    assert st.row_off is None and st.logits.data_ptr() == lg.data_ptr()
