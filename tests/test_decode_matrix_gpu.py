"""The options of the device-resident decode step TOGETHER, at the engine, on the tiny models of scripts/fuzz_engine_state.py (Llama V = 320,
Qwen2 V = 515; B <= 4, at most 12 new tokens): shared-prefix KV, the token trie, log-probabilities, the logits processors, the FP8 KV cache and
the FP8 decoder weights, graph and eager, min_new_tokens and EOS - every pair of values that check_processors and _layers do not refuse
(CASES; tests/test_select_chain_host.py holds the table to pairwise coverage), every refused one refused by name before any launch (REFUSALS).

Every case is replayed from THE CALL'S OWN raw step logits through tests/select_chain_ref.walk: no model reference is involved, so the FP8
modes are held as exactly as bf16.  The entry points that return no step logits (generate_many in flight, generate(decode_streams=2)) are
held bit for bit to the generate() calls they are documented to equal, and those are replayed."""
import functools
import itertools
import os
import runpy

import pytest
import torch

from crab_amd import decoder, ops
from crab_amd.constrain import TokenTrie
from tests import select_chain_ref as S
from tests.util import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EOS, PAD, N_NEW, SEED = 1, 2, 12, 77
FP8 = "fp8_e4m3"
EITHER_CAP = 0.05
SAMPLING = (0.9, 40, 0.9)

AXES = dict(entry=["generate", "chunk", "streams", "many", "coalesced", "shared"], select=["greedy", "sample"], trie=[False, True],
            logprobs=[False, True], proc=["none", "penalty", "penalty+ngram", "penalty+stops"], kv=["bf16", "fp8"], w=["bf16", "fp8"],
            graph=[True, False], min_new=[0, 2], eos=[False, True])
PROC = {"none": (1.0, 0, False), "penalty": (1.3, 0, False), "penalty+ngram": (1.3, 2, False), "penalty+stops": (1.3, 0, True)}

# Refused by name.  `axes`: the values that make up the refusal (a pair, once a triple); `engine`: keyword arguments of GenerationEngine's entry
# points, `hf`: the same through the model's surface (None: the surface launches before the engine sees the argument); `match`: the message.
_T = [[7, 8], [9, 10, 11]]
REFUSALS = [
    dict(axes=dict(logprobs=True, proc="penalty+ngram"), engine=dict(return_logprobs=True, processors=(1.3, 2, ())),
         hf=dict(output_token_logprobs=True, repetition_penalty=1.3, no_repeat_ngram_size=2), match="with no_repeat_ngram_size = 2: the banned tokens"),
    dict(axes=dict(logprobs=True, proc="penalty+stops", min_new=2), engine=dict(return_logprobs=True, processors=(1.3, 0, (5, 6)), min_new_tokens=2, eos_token_id=EOS),
         hf=dict(output_token_logprobs=True, repetition_penalty=1.3, eos_token_id=[EOS, 5, 6], min_new_tokens=2), match="the suppressed stop ids"),
    dict(axes=dict(trie=True, proc="penalty+stops"), engine=dict(constraint="trie", processors=(1.3, 0, (5, 6)), eos_token_id=EOS),
         hf=dict(allowed_sequences=_T, repetition_penalty=1.3, eos_token_id=[EOS, 5, 6]), match="a token trie has ONE end-of-sequence edge"),
    dict(axes=dict(trie=True, proc="penalty+ngram"), engine=dict(constraint="trie", processors=(1.3, 2, ()), eos_token_id=EOS),
         hf=dict(allowed_sequences=_T, repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=EOS), match="a ban could empty a trie node's edge set"),
    dict(axes=dict(trie=True, eos=False), engine=None, hf=dict(allowed_sequences=_T, eos_token_id=None), match="ONE EOS id", error=ValueError,
         avs=False),                                             # (generate_avs_many takes no allowed_sequences: nothing to refuse there)
    dict(axes=dict(entry="shared", kv="fp8"), engine=dict(kv_cache_dtype=FP8), hf=None, shared_only=True, match='kv_cache_dtype="fp8_e4m3" with a shared prefix'),
    dict(axes=dict(entry="shared", w="fp8"), engine=dict(weight_dtype=FP8), hf=None, shared_only=True, match='weight_dtype="fp8_e4m3" with a shared prefix'),
]


def refusal(c):
    """The refusal (an entry of REFUSALS) a case meets, or None."""
    for r in REFUSALS:
        if all(c[k] == v for k, v in r["axes"].items()):
            return r
    return None


def engine_refuses(c):
    """What the code says, independent of REFUSALS (the host test holds the two to each other): check_processors, TokenTrie, _layers."""
    p, n, st = PROC[c["proc"]]
    try:
        decoder.check_processors((p, n, (5, 6) if st else ()), c["min_new"], c["trie"], c["logprobs"], EOS if c["eos"] else None)
        if c["trie"] and not c["eos"]:
            TokenTrie([_T], 320, None)
    except (NotImplementedError, ValueError):
        return True
    return c["entry"] == "shared" and FP8[:3] in (c["kv"], c["w"])      # _layers / _generate_shared_prefix: the shared prefix is a bf16 path


# A pairwise covering of the allowed matrix, the nine pairings no other test runs first (penalty x trie greedy and sampled, penalty x trie x
# log-probabilities, processors x FP8 weights, log-probabilities x FP8 weights, both FP8 modes x trie x log-probabilities, stop ids x shared
# prefix, processors x two decode streams, trie x coalesced ragged rows x penalty).
_TABLE = [
    ('generate', 'greedy', True, False, 'penalty', 'bf16', 'bf16', True, 0, True),
    ('generate', 'sample', True, False, 'penalty', 'bf16', 'bf16', True, 2, True),
    ('chunk', 'greedy', True, True, 'penalty', 'bf16', 'bf16', True, 0, True),
    ('generate', 'greedy', False, False, 'penalty+ngram', 'bf16', 'fp8', True, 0, False),
    ('generate', 'greedy', False, True, 'penalty+stops', 'bf16', 'fp8', True, 0, True),
    ('generate', 'sample', True, True, 'penalty', 'fp8', 'fp8', False, 0, True),
    ('shared', 'greedy', False, False, 'penalty+stops', 'bf16', 'bf16', True, 2, True),
    ('streams', 'sample', False, False, 'penalty+ngram', 'bf16', 'bf16', True, 0, True),
    ('coalesced', 'greedy', True, True, 'penalty', 'fp8', 'bf16', True, 0, True),
    ('many', 'sample', False, False, 'none', 'fp8', 'bf16', False, 2, False),
    ('coalesced', 'greedy', False, True, 'none', 'bf16', 'fp8', False, 2, False),
    ('many', 'greedy', True, False, 'none', 'bf16', 'fp8', True, 0, True),
    ('chunk', 'sample', False, False, 'penalty+ngram', 'fp8', 'bf16', False, 2, False),
    ('streams', 'sample', False, True, 'penalty', 'fp8', 'fp8', False, 2, False),
    ('shared', 'sample', False, True, 'penalty+stops', 'bf16', 'bf16', False, 0, False),
    ('coalesced', 'sample', False, False, 'penalty+stops', 'fp8', 'bf16', False, 2, True),
    ('streams', 'greedy', True, True, 'none', 'fp8', 'fp8', True, 0, True),
    ('chunk', 'sample', False, False, 'none', 'bf16', 'fp8', True, 0, False),
    ('many', 'sample', False, True, 'penalty', 'bf16', 'bf16', True, 2, False),
    ('shared', 'sample', True, False, 'penalty', 'bf16', 'bf16', False, 0, True),
    ('generate', 'sample', False, False, 'none', 'fp8', 'bf16', False, 0, True),
    ('coalesced', 'greedy', False, False, 'penalty+ngram', 'bf16', 'bf16', True, 0, True),
    ('many', 'sample', False, False, 'penalty+stops', 'bf16', 'bf16', True, 0, False),
    ('many', 'sample', False, False, 'penalty+ngram', 'fp8', 'fp8', True, 0, True),
    ('chunk', 'greedy', False, False, 'penalty+stops', 'fp8', 'bf16', True, 2, False),
    ('shared', 'greedy', False, True, 'none', 'bf16', 'bf16', False, 2, False),
    ('streams', 'greedy', False, False, 'penalty+stops', 'fp8', 'bf16', True, 2, True),
    ('shared', 'greedy', False, False, 'penalty+ngram', 'bf16', 'bf16', True, 2, True),
]
CASES = [dict(zip(AXES, row)) for row in _TABLE]


def case_id(c):
    return "-".join(f"{k[0]}{int(v)}" if isinstance(v, bool) else str(v) for k, v in c.items())


# ------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def _model(qwen=False):
    ns = runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_engine_state.py"), run_name="lib")
    um = ns["build"](qwen).base_model.model
    return um, um.config.hidden_size, um.lm_head.weight.shape[0]


def _emb(B, S, hid, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()


@functools.lru_cache(maxsize=None)
def _trie(V, which=0):
    """Two answer sets of 2 - 5 tokens with shared prefixes over a small alphabet (so a row's history repeats and the penalty bites); no member is
    shorter than 2 tokens (min_new_tokens = 2 must leave something allowed)."""
    g = torch.Generator().manual_seed(50 + which)
    sets = []
    for s in range(2):
        alphabet = (10 + 40 * s + torch.randperm(40, generator=g)[:5]).tolist()
        sets.append([[alphabet[int(i)] for i in torch.randint(0, 5, (int(torch.randint(2, 6, (1,), generator=g)),), generator=g)] for _ in range(7)])
    return TokenTrie(sets, V, EOS)


def _inputs(um, hid, V, entry):
    """The prompts of one entry point as the list of batches its rows come in, and the set index of every row."""
    if entry in ("many", "coalesced"):
        embs = [_emb(2, 6, hid, 301), _emb(1, 9, hid, 302), _emb(1, 4, hid, 303)]
    elif entry == "shared":
        prefix = _emb(2, 6, hid, 304)
        g = torch.Generator().manual_seed(9)
        qs = [[torch.randint(3, V, (int(s),), generator=g) for s in ss] for ss in ([2], [3, 1, 2])]
        embs = (prefix, [[um.encode_ids(q.cuda()).to(BF) for q in q_] for q_ in qs])
    else:
        embs = [_emb(4 if entry == "streams" else 3, 6, hid, 305)]
    counts = [len(q) for q in embs[1]] if entry == "shared" else [int(e.shape[0]) for e in embs]
    sets, r = [], 0
    for n in counts:
        sets.append([(r + i) % 2 for i in range(n)])
        r += n
    return embs, counts, sets


def _call(eng, c, embs, sets, kw, step_logits=True):
    """One call of the case's entry point -> one (ids, step logits or None, log-probabilities or None) per batch."""
    kw = dict(kw)
    lp = kw.get("return_logprobs", False)
    if c["trie"]:
        kw["constraint"] = (kw["constraint"], sets if c["entry"] in ("many", "coalesced", "shared") else sets[0])
    if c["entry"] == "shared":
        res = eng.generate_shared_prefix(embs[0], embs[1], N_NEW, return_step_logits=True, **kw)
    elif c["entry"] in ("many", "coalesced"):
        co = c["entry"] == "coalesced"
        res = eng.generate_many(embs, N_NEW, coalesce=co, return_step_logits=co, **kw)
    else:
        extra = dict(prefill_chunk=2) if c["entry"] == "chunk" else dict(decode_streams=2) if c["entry"] == "streams" else {}
        res = [eng.generate(embs[0], N_NEW, return_step_logits=step_logits and c["entry"] != "streams", **extra, **kw)]
    out = []
    for r in res:
        r = list(r) if isinstance(r, (tuple, list)) else [r]
        ids = r.pop(0)
        lpv = r.pop() if lp else None
        out.append((ids, r.pop(0) if r else None, lpv))
    return out


def _pick_stop_ids(free, c):
    """EOS and two further stop ids read off the free run (same call, nothing stops it), so that rows stop at different steps and - with
    min_new_tokens - an id is the step's choice while it is still suppressed."""
    rows = free.tolist()
    early = 1 if c["min_new"] else 4
    eos = rows[0][early]
    cand = [rows[-1][0 if c["min_new"] else 6], rows[0][8], rows[-1][9], rows[0][10]]
    stops = tuple(dict.fromkeys(t for t in cand if t not in (eos, PAD)))[:2]
    return eos, stops


def _check_group(batches, counts, sets, o, seed, what):
    """batches: (ids, logits, lp) of the batches that decoded as ONE state, in row order.  Replays them through the composed reference."""
    n = max(int(ids.shape[1]) for ids, _, _ in batches)
    B, V = sum(counts), int(batches[0][1].shape[2])
    ids = torch.full((B, n), o.pad, dtype=torch.int64)
    lg = torch.zeros((B, n, V))
    lp = torch.zeros((2, B, n)) if batches[0][2] is not None else None
    r0 = 0
    for (i_, l_, p_), k in zip(batches, counts):
        m = int(i_.shape[1])
        assert tuple(i_.shape) == (k, m) and tuple(l_.shape) == (k, m, V), f"{what}: shapes {tuple(i_.shape)} {tuple(l_.shape)}"
        assert bool(torch.isfinite(l_).all()), f"{what}: the returned logits are the RAW ones (nothing banned in them)"
        ids[r0:r0 + k, :m], lg[r0:r0 + k, :m] = i_.cpu(), l_.float().cpu()
        if lp is not None:
            assert tuple(p_.shape) == (k, m, 2)
            lp[:, r0:r0 + k, :m] = p_.float().cpu().permute(2, 0, 1)
        r0 += k
    o.set_of = [s for ss in sets for s in ss] if o.trie is not None else None
    walk = S.walk(lg, ids, o)
    share = sum(int(bool((r.classes[b] == S.EITHER).any())) for r in walk.steps for b in range(B)) / float(B * n) if o.sampling is not None else 0.0
    assert share <= EITHER_CAP, f"{what}: {share:.1%} of the (row, step) pairs hold an EITHER token"
    # trim: a batch ends with the first column at which all ITS rows have finished
    fin = torch.zeros((B, n), dtype=torch.bool)
    f = torch.zeros(B, dtype=torch.int32)
    for t in range(n):
        f = walk.steps[t].after(ids[:, t])[2]
        fin[:, t] = f.bool()
    r0 = 0
    for (i_, _, _), k in zip(batches, counts):
        done = torch.nonzero(fin[r0:r0 + k].all(0))
        want = int(done[0]) + 1 if done.numel() else N_NEW
        assert int(i_.shape[1]) == want, f"{what}: a batch of {k} rows returned {int(i_.shape[1])} columns, its rows had all finished after {want}"
        r0 += k
    assert torch.equal(ids, walk.emitted), f"{what}: pad after a row's end, ids inside the trie: {ids.tolist()} vs {walk.emitted.tolist()}"
    if o.sampling is None:
        assert torch.equal(ids, walk.greedy_ids), f"{what}: emitted {ids.tolist()}, the reference {walk.greedy_ids.tolist()}"
    else:
        dev = "cuda"
        cur, out = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, n, dtype=torch.int64, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        up = lambda a: torch.from_numpy(a.copy()).to(dev)
        tr = (up(o.trie.edge_off), up(o.trie.edge_tok), up(o.trie.edge_dst)) if o.trie is not None else None
        t_, k_, p_ = o.sampling
        for t in range(n):
            r = walk.steps[t]
            for b in range(B):
                if not int(r.finished_before[b]) and bool(r.allowed[b].any()):
                    assert int(r.classes[b, int(ids[b, t])]) != S.DROP, f"{what}: step {t} row {b} drew {int(ids[b, t])}, which the fp64 kept set drops"
            step.fill_(t)
            fin_d = r.finished_before.to(dev)
            if tr is not None:
                ops.constrained_select(r.edited.to(dev), *tr, torch.tensor(r.node_before, dtype=torch.int32, device=dev), cur, out, step, fin_d, o.eos, o.pad,
                                       o.min_new, t_, k_, p_, seed)
            else:
                ops.sample_select(r.edited.to(dev), cur, out, step, fin_d, o.eos, o.pad, o.min_new, t_, k_, p_, seed)
            assert torch.equal(cur.cpu(), ids[:, t]), f"{what}: step {t}: the select on the reference's edited rows draws {cur.tolist()}, the call emitted {ids[:, t].tolist()}"
    worst = 0.0
    if lp is not None:
        err = (lp.double() - walk.lp).abs()
        assert bool((err <= walk.bound).all()), f"{what}: log-probabilities off by up to {float(err.max()):.3e}"
        assert bool((lp.permute(1, 2, 0)[~walk.live] == 0).all()), f"{what}: a row that is not live has a log-probability"
        worst = float((err / walk.bound.clamp(min=1e-30))[:, walk.live].max()) if bool(walk.live.any()) else 0.0
    if o.trie is not None:
        for b in range(B):
            row = ids[b].tolist()
            if o.eos in row:
                assert o.trie.is_member(o.set_of[b], row[:row.index(o.eos)]), f"{what}: row {b} {row} is no member of set {o.set_of[b]}"
    return share, worst, walk


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_allowed_pairing_replays_from_its_own_raw_logits(c):
    qwen = c["w"] == "bf16" and CASES.index(c) % 2 == 1
    um, hid, V = _model(qwen)
    eng = um._engine
    eng.invalidate()
    embs, counts, sets = _inputs(um, hid, V, c["entry"])
    p, n, st = PROC[c["proc"]]
    smp = SAMPLING + (SEED,) if c["select"] == "sample" else None
    trie = _trie(V) if c["trie"] else None
    kw = dict(pad_token_id=PAD, sampling=smp, kv_cache_dtype=FP8 if c["kv"] == "fp8" else "bf16", weight_dtype=FP8 if c["w"] == "fp8" else "bf16")
    eos, stops = (EOS if c["trie"] else None), ()
    if (c["eos"] or st) and not c["trie"]:
        free = torch.cat([b[0] for b in _call(eng, c, embs, sets, dict(kw, eos_token_id=None, processors=(p, n, ())), step_logits=False)], 0).cpu()
        assert tuple(free.shape) == (sum(counts), N_NEW)
        e_, stops = _pick_stop_ids(free, c)
        eos, stops = (e_ if c["eos"] else None), (stops if st else ())
        assert not st or len(stops) == 2
    kw.update(eos_token_id=eos, min_new_tokens=c["min_new"], return_logprobs=c["logprobs"], processors=(p, n, stops), use_graph=c["graph"])
    if trie is not None:
        kw["constraint"] = trie
    res = _call(eng, c, embs, sets, kw)
    assert eng.kv_cache_dtype == "bf16" and eng.weight_dtype == "bf16", "a per-call mode outlived its call"
    if c["w"] == "fp8" and isinstance(eng.last_plan, dict):
        assert eng.last_plan.get("weight_dtype_used") == FP8, eng.last_plan
    if c["entry"] != "streams":                                  # (an eager call runs ONE state of all rows, a graphed one two of half the rows: other kernels)
        other = _call(eng, c, embs, sets, dict(kw, use_graph=not c["graph"]))
        for (a, la, pa), (b, lb, pb) in zip(res, other):
            assert torch.equal(a, b) and (la is None or torch.equal(la, lb)) and (pa is None or torch.equal(pa, pb)), "graph and eager runs differ"
    what = case_id(c)
    mk = lambda: S.Opts(eos=eos, pad=PAD, min_new=c["min_new"], penalty=p, ngram=n, stops=stops, sampling=SAMPLING if smp else None, trie=trie)
    groups = []                                                  # (batches, counts, sets, seed) of every decode state
    if c["entry"] in ("many", "streams") and not (c["entry"] == "streams" and not c["graph"]):
        # no step logits on these paths: every state equals the generate() call of its rows (seed + 7919 * slot), bit for bit
        if c["entry"] == "streams":
            B = counts[0]
            parts = [(embs[0][B * g // 2:B * (g + 1) // 2], sets[0][B * g // 2:B * (g + 1) // 2]) for g in range(2)]
        else:
            parts = list(zip(embs, sets))
        solo = []
        for g, (e, ss) in enumerate(parts):
            k = dict(kw, sampling=SAMPLING + (SEED + 7919 * g,) if smp else None)
            if trie is not None:
                k["constraint"] = (trie, ss)
            r = list(eng.generate(e, N_NEW, return_step_logits=True, **k))
            solo.append((r[0], r[1], r[-1] if c["logprobs"] else None))
            groups.append(([solo[-1]], [int(e.shape[0])], [ss], SEED + 7919 * g))
        if c["entry"] == "many":
            for (a, _, pa), (b, _, pb) in zip(res, solo):
                assert torch.equal(a, b) and (pa is None or torch.equal(pa, pb)), "a batch in flight differs from its own generate() call"
        else:
            ids, lpv = res[0][0], res[0][2]
            r0 = 0
            for b, _, pb in solo:                                # the groups are ONE call: trimmed together, a group that ended earlier is padded
                k, m = int(b.shape[0]), int(b.shape[1])
                assert torch.equal(ids[r0:r0 + k, :m], b[:, :ids.shape[1]]) and bool((ids[r0:r0 + k, m:] == PAD).all()), "a stream's group differs from its own generate() call"
                assert pb is None or torch.equal(lpv[r0:r0 + k, :m], pb[:, :ids.shape[1]])
                r0 += k
            assert ids.shape[1] == max(int(b.shape[1]) for b, _, _ in solo)
    elif c["entry"] == "streams":                                # eager: generate() falls back to one state and returns no logits with decode_streams
        r = list(eng.generate(embs[0], N_NEW, return_step_logits=True, **dict(kw, constraint=(trie, sets[0])) if trie is not None else kw))
        assert torch.equal(r[0], res[0][0])
        groups.append(([(r[0], r[1], r[-1] if c["logprobs"] else None)], counts, sets, SEED))
    else:
        groups.append((res, counts, sets, SEED))
    share = worst = 0.0
    ended = 0
    for batches, cnt, ss, seed in groups:
        sh, w, walk = _check_group(batches, cnt, ss, mk(), seed, what)
        share, worst = max(share, sh), max(worst, w)
        ended += int(walk.finished.sum())
    # the case shows what it is about: every constrained row ends its answer, and a stop id read off the free run stops a row
    if c["trie"]:
        assert ended == sum(counts), f"{what}: {ended} of {sum(counts)} constrained rows reached EOS"
    elif (c["eos"] or st) and c["min_new"] == 0:
        assert ended >= 1, f"{what}: no row met EOS or a stop id"
    record_parity(f"decode matrix {what}: share of (row, step) pairs with an EITHER token", share, 1.0, EITHER_CAP, lp_err_over_bound=worst)
    print(f"{what}: either share {share:.2%}, lp error / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ refusals
def _stub_inputs(um):
    um.prepare_multimodal_inputs = lambda batch_input_ids=None, **k: {"inputs_embeds": batch_input_ids}
    um.prepare_multimodal_inputs_many = lambda batches, **k: [{"inputs_embeds": b["batch_input_ids"]} for b in batches]


def _unstub(um):
    del um.prepare_multimodal_inputs, um.prepare_multimodal_inputs_many


@pytest.mark.parametrize("r", REFUSALS, ids=lambda r: "-".join(f"{k}={v}" for k, v in r["axes"].items()))
def test_every_refused_pairing_is_refused_by_name_before_any_launch(r):
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(2, 5, hid, 400)
    err = r.get("error", NotImplementedError)
    trie = TokenTrie([_T], V, EOS)
    q = torch.randint(3, V, (2,), generator=torch.Generator().manual_seed(1)).cuda()
    suffix = [[um.encode_ids(q).to(BF)], [um.encode_ids(q).to(BF)]]
    calls = []
    if r["engine"] is not None:
        kw = dict(r["engine"])
        if kw.get("constraint") == "trie":
            kw["constraint"] = (trie, None)
        lists = dict(kw, constraint=(trie, [[0, 0]])) if "constraint" in kw else kw
        per_clip = dict(kw, constraint=(trie, [[0], [0]])) if "constraint" in kw else kw
        calls.append(("engine.generate_shared_prefix", lambda: eng.generate_shared_prefix(emb, suffix, 4, pad_token_id=PAD, **per_clip)))
        if not r.get("shared_only"):
            calls.append(("engine.generate", lambda: eng.generate(emb, 4, pad_token_id=PAD, **kw)))
            calls.append(("engine.generate_many", lambda: eng.generate_many([emb], 4, pad_token_id=PAD, coalesce=True, **lists)))
    if r["hf"] is not None:
        hf = dict(r["hf"], max_new_tokens=4, pad_token_id=PAD)
        one = dict(batch_input_ids=emb, batch_X_modals=None)
        calls.append(("generate", lambda: um.generate(inputs_embeds=emb, **hf)))
        calls.append(("generate_batches", lambda: um.generate_batches([one], **hf)))
        calls.append(("generate_batches coalesced", lambda: um.generate_batches([one, one], coalesce=True, **hf)))
        calls.append(("generate_questions", lambda: um.generate_questions([dict(batch_input_ids=emb[:1], batch_X_modals=None, question_ids=[q])], **hf)))
        if r.get("avs", True):
            calls.append(("generate_avs_many", lambda: um.generate_avs_many([dict(batch_input_ids=emb[:1], batch_labels=None, batch_X_modals=None, batch_task_names=["avs"])], **hf)))
    assert calls
    modes = (eng.kv_cache_dtype, eng.weight_dtype)
    torch.cuda.synchronize()
    _stub_inputs(um)
    try:
        for name, fn in calls:
            with ops.launch_trace(emb.device.index or 0) as tr:
                with pytest.raises(err, match=r["match"]):
                    fn()
            assert not tr.counts, f"{name}: refused after launching {tr.counts}"
            assert (eng.kv_cache_dtype, eng.weight_dtype) == modes, f"{name}: a refused call changed the engine's modes"
    finally:
        _unstub(um)


# ------------------------------------------------------------------ carried state
def test_one_option_at_a_time_on_one_engine_equals_a_fresh_engine_and_recaptures_exactly_when_the_key_changes():
    um, hid, V = _model()
    eng = um._engine
    emb = _emb(3, 6, hid, 500)
    tA, tB = _trie(V, 0), _trie(V, 1)
    assert tA.key != tB.key
    free = eng.generate(emb, 8, eos_token_id=None, pad_token_id=PAD).cpu()
    stop = int(free[1, 5])
    base = dict(eos_token_id=EOS, pad_token_id=PAD)
    seq = [("plain", dict()),
           ("penalty 1.3", dict(processors=(1.3, 0, ()))),
           ("penalty 1.5", dict(processors=(1.5, 0, ()))),
           ("stop id added", dict(processors=(1.5, 0, (stop,)))),
           ("stop id dropped", dict(processors=(1.5, 0, ()))),
           ("trie A", dict(processors=(1.5, 0, ()), constraint=(tA, [0, 1, 0]))),
           ("trie B", dict(processors=(1.5, 0, ()), constraint=(tB, [0, 1, 0]))),
           ("logprobs on", dict(processors=(1.5, 0, ()), constraint=(tB, [0, 1, 0]), return_logprobs=True)),
           ("logprobs off", dict(processors=(1.5, 0, ()), constraint=(tB, [0, 1, 0]))),
           ("fp8 weights on", dict(processors=(1.5, 0, ()), constraint=(tB, [0, 1, 0]), weight_dtype=FP8)),
           ("fp8 weights off", dict(processors=(1.5, 0, ()), constraint=(tB, [0, 1, 0])))]

    def run(kw):
        r = eng.generate(emb, 8, return_step_logits=True, **base, **kw)
        return [x.clone() for x in r]

    fresh = []
    for _, kw in seq:
        eng.invalidate()
        fresh.append(run(kw))
    assert not torch.equal(fresh[5][0], fresh[6][0]), "the two tries give the same ids: the sequence shows nothing"
    eng.invalidate()
    prev = None
    for (name, kw), want in zip(seq, fresh):
        got = run(kw)
        st = eng._dec[0]
        assert st.graph is not None
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), f"{name}: carried engine state differs from a fresh engine"
        if prev is not None:
            assert st.key != prev[0], f"{name}: the option is no term of the state key - the previous call's graph would be replayed"
            assert st is not prev[1] and st.graph is not prev[2], f"{name}: the key changed and the graph was not rebuilt"
        graph = st.graph
        again = run(kw)                                          # the same call: same key, same state, same captured graph
        assert eng._dec[0] is st and st.graph is graph and all(torch.equal(a, b) for a, b in zip(again, want)), f"{name}: a repeated call did not reuse its graph"
        prev = (st.key, st, graph)
