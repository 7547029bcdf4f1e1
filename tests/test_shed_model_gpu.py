"""GenerationEngine.generate(shed_finished=...) / generate_many(coalesce=True, shed_finished=...) on the tiny Llama and Qwen2 models of
scripts/fuzz_engine_state.py.

The yardstick is the SAME call without the option (the code that existed before it), judged by the rule of tests/test_shared_prefix_gpu.py:
per row, logits within tests/bounds.decoder_bound (teacher-forced along the plain path's ids) of the plain call's at every step at which the
row was live in the plain call; a differing id is accepted only where the plain path's own top-2 margin is below 10 x that bound, and ends the
row's comparison (later steps see another context); at least 75 % of the live (row, step) pairs must actually be compared.  When no row
diverged, the whole result - shape, EOS trim, pad after EOS - has to equal the plain call's.

The EOS id of every case is taken from a free run (no EOS) of the plain path, and the data seed is the first one for which that run meets the
case's need (rows finishing at three or more distinct steps, two or more sheds under the test's ladder - counted by replaying the finish steps
through decoder.shed_rung, the pure policy function).  Every test prints its figures (pytest -s)."""
import functools
import os
import runpy

import pytest
import torch

from crab_amd import decoder as D
from crab_amd import ops
from tests import bounds as PB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 2
LADDER = (1, 2, 3, 4, 6)


@functools.lru_cache(maxsize=None)
def _model(qwen: bool):
    ns = runpy.run_path(os.path.join(ROOT, "scripts", "fuzz_engine_state.py"), run_name="lib")
    return ns["build"](qwen)


def _um(qwen):
    um = _model(qwen).base_model.model
    return um, um._engine, um.config.hidden_size


@functools.lru_cache(maxsize=None)
def _oracle(qwen: bool):
    from oracle import crab_oracle as O
    model = _model(qwen)
    c = model.base_model.model.config
    W = {k: v.detach().float().cpu() for k, v in O.strip_peft_prefix(model.state_dict()).items() if v.dtype.is_floating_point}
    ocfg = O.DecoderConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads, vocab_size=c.vocab_size,
                           rms_norm_eps=c.rms_norm_eps, rope_theta=c.rope_theta, lora_r=8, lora_alpha=16, lora_nums=3)
    return W, ocfg


def _emb(kind: str, B: int, S: int, hid: int, seed: int):
    """rand: B different prompts; same: one prompt B times (the rows finish together); but_last: one prompt B - 1 times and another one;
    ten: one prompt ten times, then different ones."""
    g = torch.Generator().manual_seed(seed)
    e = (torch.randn(B, S, hid, generator=g) * 0.5).to(BF)
    n_same = {"rand": 1, "same": B, "but_last": B - 1, "ten": 10}[kind]
    e[:n_same] = e[0]
    return e.cuda()


@functools.lru_cache(maxsize=None)
def _free(qwen: bool, kind: str, B: int, S: int, N: int, seed: int, sampling=None):
    """The plain path without an EOS, once per case: (embeds, ids [B, N], logits [B, N, V], per-row absolute bound)."""
    um, eng, hid = _um(qwen)
    emb = _emb(kind, B, S, hid, seed)
    ids, lg = eng.generate(emb, N, eos_token_id=None, pad_token_id=PAD, return_step_logits=True, sampling=sampling)
    return emb, ids.cpu(), lg.float().cpu()


@functools.lru_cache(maxsize=None)
def _bounds(qwen: bool, kind: str, B: int, S: int, N: int, seed: int, sampling=None):
    emb, ids, lg = _free(qwen, kind, B, S, N, seed, sampling)
    W, ocfg = _oracle(qwen)
    return tuple(PB.decoder_bound(emb[b:b + 1].cpu(), W, ocfg, ids[b:b + 1]) * lg[b].abs().max().item() for b in range(B))


def _finish_steps(ids, eos):
    out = []
    for row in ids.tolist():
        out.append(row.index(eos) if eos in row else None)
    return out


def _simulate(fin, B, N, ladder, every):
    """The sheds of a call whose rows finish at the steps `fin`, by the pure policy: [(step, rows_before, rows_after)]."""
    cur, sheds = B, []
    for step in range(1, N):
        if step % every:
            continue
        live = sum(1 for f in fin if f is None or f > step)
        if live == 0:
            break
        r = D.shed_rung(ladder, live, cur)
        if r is not None and N - 1 - step >= D.SHED_MIN_STEPS_LEFT:      # no shed within the last steps of a call: it would not pay back
            sheds.append((step, cur, r))
            cur = r
    return sheds


def _spread_case(qwen, B, S, N, ladder, every, sampling=None, kind="rand"):
    """First data seed (and its EOS id) for which the free run's rows finish at >= 3 distinct steps and the ladder sheds at least twice."""
    for seed in range(1, 25):
        emb, ids, lg = _free(qwen, kind, B, S, N, seed, sampling)
        best = None
        for t in sorted(set(ids.flatten().tolist()) - {PAD}):
            fin = _finish_steps(ids, t)
            distinct = len({f for f in fin if f is not None})
            sheds = _simulate(fin, B, N, ladder, every)
            if distinct >= 3 and len(sheds) >= 2 and (best is None or (distinct, len(sheds)) > best[0]):
                best = ((distinct, len(sheds)), t, fin, sheds)
        if best is not None:
            return seed, best[1], best[2], best[3]
    pytest.fail("no data seed in 1 .. 24 lets the plain path finish rows at three distinct steps")


def _compare(what, plain, shed, bnds, eos, sampled=False):
    """plain / shed: (ids [B, n], logits [B, n, V]) of the two calls -> share of the live (row, step) pairs compared."""
    pids, plg = plain[0].cpu(), plain[1].float().cpu()
    sids, slg = shed[0].cpu(), shed[1].float().cpu()
    fin = _finish_steps(pids, eos)
    covered, total, worst, diverged = 0, 0, 0.0, 0
    for b in range(pids.shape[0]):
        last = fin[b] if fin[b] is not None else pids.shape[1] - 1
        total += last + 1
        for s in range(last + 1):
            assert s < sids.shape[1], f"{what}: row {b} is live at step {s} in the plain call, the shedding call returned {sids.shape[1]} columns"
            err = (slg[b, s] - plg[b, s]).abs().max().item()
            worst = max(worst, err / bnds[b])
            assert err <= bnds[b], f"{what}: row {b} step {s}: |dlogit| {err:.4e} above the bound {bnds[b]:.4e}"
            if sids[b, s] != pids[b, s]:
                if sampled:
                    assert not torch.equal(slg[b, s], plg[b, s]), f"{what}: row {b} step {s}: bit-equal logits, ids {sids[b, s]} vs {pids[b, s]}: the draw differs"
                else:
                    top2 = plg[b, s].topk(2).values
                    assert (top2[0] - top2[1]).item() < 10 * bnds[b], \
                        f"{what}: row {b} step {s}: id {sids[b, s]} vs {pids[b, s]} at margin {(top2[0] - top2[1]).item():.4f} >= 10 x bound {bnds[b]:.4e}"
                diverged += 1
                break
            covered += 1
    share = covered / total
    print(f"\n{what}: {covered}/{total} live (row, step) pairs compared ({share:.2f}), {diverged} rows diverged at a sub-margin step, "
          f"worst |dlogit| / bound {worst:.3f}")
    if not diverged:
        assert tuple(sids.shape) == tuple(pids.shape) and torch.equal(sids, pids), f"{what}: the trim / pad layout differs from the plain call's"
    assert share >= 0.75, f"{what}: only {share:.2f} of the live (row, step) pairs were compared"
    return diverged


def _both(eng, emb, N, eos, ladder, every, graph=True, sampling=None, pad=PAD):
    plain = eng.generate(emb, N, eos_token_id=eos, pad_token_id=pad, return_step_logits=True, use_graph=graph, sampling=sampling)
    shed = eng.generate(emb, N, eos_token_id=eos, pad_token_id=pad, return_step_logits=True, use_graph=graph, sampling=sampling,
                        shed_finished=ladder, shed_every=every)
    return plain, shed, dict(eng.last_plan)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_pad_after_eos_without_a_pad_token_id(graph):
    """pad_token_id = None (the engine's default): a finished row emits the EOS id, while the state's buffers start filled with 0.  A row that
    finishes INSIDE a child state - after the first shed - and is left behind at the second one must still hold the EOS id behind its EOS, as the
    plain call writes it at every later step."""
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 24
    seed, eos, fin, want = _spread_case(False, B, S, N, LADDER, 1)
    assert eos != 0 and len(want) >= 2 and any(f is not None and want[0][0] < f <= want[1][0] for f in fin), \
        "the case needs a row that finishes between the first and the second shed"
    emb = _free(False, "rand", B, S, N, seed)[0]
    plain, shed, plan = _both(eng, emb, N, eos, LADDER, 1, graph, pad=None)
    print(f"\npad None: seed {seed} eos {eos}: rows finish at {fin}; sheds {plan['shed']}")
    assert len(plan["shed"]) >= 2
    assert _compare("pad_token_id None", plain, shed, _bounds(False, "rand", B, S, N, seed), eos) == 0
    ids = shed[0].cpu()
    for b, f in enumerate(_finish_steps(ids, eos)):
        if f is not None:
            assert bool((ids[b, f:] == eos).all()), f"row {b}: the EOS id pads the row behind its EOS at step {f}"
    assert torch.equal(ids, plain[0].cpu())


@pytest.mark.parametrize("qwen", [False, True], ids=["llama", "qwen2"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_greedy_wave_sheds_and_equals_the_plain_call(qwen, graph):
    um, eng, hid = _um(qwen)
    B, S, N = 6, 9, 24
    seed, eos, fin, want = _spread_case(qwen, B, S, N, LADDER, 1)
    emb = _free(qwen, "rand", B, S, N, seed)[0]
    plain, shed, plan = _both(eng, emb, N, eos, LADDER, 1, graph)
    print(f"\nseed {seed} eos {eos}: rows finish at {fin}; sheds {plan['shed']} (the policy on the plain path's steps: {want})")
    assert len(plan["shed"]) >= 2 and all(b > a >= 1 for _, b, a, _ in plan["shed"])
    diverged = _compare(f"{'qwen2' if qwen else 'llama'} {'graph' if graph else 'eager'}", plain, shed, _bounds(qwen, "rand", B, S, N, seed), eos)
    assert diverged == 0, "every state of this wave has at most 16 rows and runs the same kernels: the two calls are bit-equal"
    assert [(s, b, a) for s, b, a, _ in plan["shed"]] == want
    # the logits of a row that had been shed are zeros
    fin_p = _finish_steps(plain[0].cpu(), eos)
    step0, _, _, _ = plan["shed"][0]
    gone = [b for b, f in enumerate(fin_p) if f is not None and f <= step0]
    assert gone and all(not bool(shed[1][b, step0 + 1:].any()) for b in gone)
    # return_first_logits: the prefill's, whatever happens later
    ids2, first = eng.generate(emb, N, eos_token_id=eos, pad_token_id=PAD, return_first_logits=True, use_graph=graph, shed_finished=LADDER, shed_every=1)
    assert torch.equal(first, shed[1][:, 0]) and torch.equal(ids2, shed[0])


def test_a_row_whose_first_token_is_the_eos():
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 12
    emb, ids, lg = _free(False, "rand", B, S, N, 3)
    eos = int(ids[2, 0])                                         # row 2 has finished before any decode step
    assert eos != PAD
    plain, shed, plan = _both(eng, emb, N, eos, (1, 2, 3, 4, 5, 6), 1)      # a rung for five rows: one finished row is enough to shed
    fin = _finish_steps(plain[0].cpu(), eos)
    print(f"\nfirst-token EOS: rows finish at {fin}; sheds {plan['shed']}")
    n0 = sum(1 for f in fin if f is not None and f <= 1)
    assert fin[2] == 0 and plan["shed"] and plan["shed"][0][:3] == (1, B, B - n0), "the first look sheds the row"
    assert _compare("first token is the EOS", plain, shed, _bounds(False, "rand", B, S, N, 3), eos) == 0, "at most 16 rows on both sides: bit-equal"


def test_all_rows_but_one_finish():
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 16
    for seed in range(1, 25):
        emb, ids, lg = _free(False, "but_last", B, S, N, seed)
        cand = [int(t) for t in ids[0, 1:].tolist() if int(t) not in ids[B - 1].tolist() and int(t) != PAD]
        if cand:
            break
    else:
        pytest.fail("no seed gives the repeated prompt a token the last row never emits")
    eos = cand[0]
    plain, shed, plan = _both(eng, emb, N, eos, LADDER, 1)
    print(f"\nall but one: seed {seed}, rows finish at {_finish_steps(plain[0].cpu(), eos)}; sheds {plan['shed']}")
    assert len(plan["shed"]) == 1 and plan["shed"][0][1:3] == (B, 1) and plan["shed"][0][3] == 1, "five rows leave at once, the last row moves to the front"
    assert plain[0].shape[1] == N, "the last row runs to max_new_tokens"
    assert _compare("all rows but one", plain, shed, _bounds(False, "but_last", B, S, N, seed), eos) == 0, "at most 16 rows on both sides: bit-equal"


def test_all_rows_finish_at_one_step():
    um, eng, hid = _um(False)
    B, S, N = 4, 9, 12
    emb, ids, lg = _free(False, "same", B, S, N, 5)
    eos = int(ids[0, 3])
    assert eos != PAD
    plain, shed, plan = _both(eng, emb, N, eos, LADDER, 1)
    assert plan["shed"] == [] and plan["shed_captures"] == 0, "nothing is live at the look: the call ends, as without the option"
    assert torch.equal(plain[0], shed[0]) and torch.equal(plain[1], shed[1]) and plain[0].shape[1] <= 4


def test_shed_across_the_16_row_kernel_boundary():
    um, eng, hid = _um(False)
    B, S, N, ladder = 24, 9, 10, (16, 24)
    L = um.config.num_hidden_layers
    for seed in range(1, 25):
        emb, ids, lg = _free(False, "ten", B, S, N, seed)
        # the earliest step >= 1 at which the ten copies emit a token that leaves at least one other row live and at most six of them finished
        picks = [(k, int(ids[0, k])) for k in range(1, N - D.SHED_MIN_STEPS_LEFT)
                 if int(ids[0, k]) != PAD and int(ids[0, k]) not in ids[0, :k].tolist()
                 and 1 <= sum(1 for f in _finish_steps(ids[10:], int(ids[0, k])) if f is None or f > k)]
        if picks:
            break
    else:
        pytest.fail("no seed lets the ten copies finish while another row is live")
    k, eos = picks[0]
    with ops.launch_trace(emb.device.index or 0) as t_plain:
        plain = eng.generate(emb, N, eos_token_id=eos, pad_token_id=PAD, return_step_logits=True, use_graph=False)
    with ops.launch_trace(emb.device.index or 0) as t_shed:
        shed = eng.generate(emb, N, eos_token_id=eos, pad_token_id=PAD, return_step_logits=True, use_graph=False, shed_finished=ladder, shed_every=1)
    plan = dict(eng.last_plan)
    print(f"\n24 -> 16: seed {seed} eos {eos} at step {k}; sheds {plan['shed']}; M <= 16 projection launches {t_plain.launched('gemm_skinny_dma_kernel')} "
          f"plain, {t_shed.launched('gemm_skinny_dma_kernel')} shedding")
    assert len(plan["shed"]) == 1 and plan["shed"][0][1:3] == (24, 16)
    steps_after = shed[0].shape[1] - 1 - plan["shed"][0][0]
    assert steps_after >= 1
    # the M <= 16 projection kernel (csrc/skinny.hip) runs after the shed: at least one launch per layer and step on top of the plain call's
    assert t_shed.launched("gemm_skinny_dma_kernel") >= t_plain.launched("gemm_skinny_dma_kernel") + steps_after * L
    _compare("24 -> 16 rows", plain, shed, _bounds(False, "ten", B, S, N, seed), eos)


def test_coalesced_batches_of_different_lengths():
    um, eng, hid = _um(False)
    Bs, Ss, N = (2, 3, 2), (31, 32, 30), 16
    W, ocfg = _oracle(False)
    for seed in range(1, 25):
        g = torch.Generator().manual_seed(700 + seed)
        embs = [(torch.randn(b, s, hid, generator=g) * 0.5).to(BF).cuda() for b, s in zip(Bs, Ss)]
        free = eng.generate_many(embs, N, eos_token_id=None, pad_token_id=PAD, coalesce=True, return_step_logits=True)
        assert eng.last_ragged_prefill == "merged"
        ids = torch.cat([r[0].cpu() for r in free], 0)
        best = None
        for t in sorted(set(ids.flatten().tolist()) - {PAD}):
            fin = _finish_steps(ids, t)
            sheds = _simulate(fin, sum(Bs), N, (1, 2, 3, 4, 5, 7), 1)
            if len({f for f in fin if f is not None}) >= 3 and len(sheds) >= 2 and (best is None or len(sheds) > best[0]):
                best = (len(sheds), t, fin)
        if best is not None:
            break
    else:
        pytest.fail("no seed lets the coalesced plain path finish rows at three distinct steps")
    _, eos, fin = best
    plain = eng.generate_many(embs, N, eos_token_id=eos, pad_token_id=PAD, coalesce=True)
    shed = eng.generate_many(embs, N, eos_token_id=eos, pad_token_id=PAD, coalesce=True, shed_finished=(1, 2, 3, 4, 5, 7), shed_every=1)
    plan = dict(eng.last_plan)
    print(f"\ncoalesced: seed {seed} eos {eos}, rows finish at {fin}; sheds {plan['shed']}")
    assert len(plan["shed"]) >= 2 and plan.get("coalesced")
    # ids only (the coalesced form keeps no step logits under the option): equal, or differing first at a step where the plain path's own
    # margin (the free run's logits: the same numbers while the row is live) is below 10 x the row's bound
    covered = total = 0
    for e, (fids, flg), p, s in zip(embs, free, plain, shed):
        p, s, fids, flg = p.cpu(), s.cpu(), fids.cpu(), flg.float().cpu()
        same = True
        for b in range(p.shape[0]):
            f = _finish_steps(p[b:b + 1], eos)[0]
            last = f if f is not None else p.shape[1] - 1
            total += last + 1
            for st in range(last + 1):
                if st >= s.shape[1] or s[b, st] != p[b, st]:
                    bnd = PB.decoder_bound(e[b:b + 1].cpu(), W, ocfg, fids[b:b + 1]) * flg[b].abs().max().item()
                    top2 = flg[b, st].topk(2).values
                    assert st < s.shape[1] and (top2[0] - top2[1]).item() < 10 * bnd, f"row {b} step {st}: ids differ at a margin above 10 x the bound"
                    same = False
                    break
                covered += 1
        if same:
            assert torch.equal(p, s), "a batch's trim / pad layout differs from the unshed coalesced call's"
    print(f"coalesced: {covered}/{total} live (row, step) pairs compared")
    assert covered >= 0.75 * total


@pytest.mark.parametrize("sampling", [(0.8, 50, 0.9, 1234), (0.8, 50, 0.9, 1234, 0.05, 0.0, 0.0)], ids=["plain", "min_p"])
def test_sampling_keeps_every_rows_random_stream(sampling):
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 24
    seed, eos, fin, want = _spread_case(False, B, S, N, LADDER, 1, sampling)
    emb = _free(False, "rand", B, S, N, seed, sampling)[0]
    plain, shed, plan = _both(eng, emb, N, eos, LADDER, 1, True, sampling)
    print(f"\nsampling {sampling}: seed {seed} eos {eos}, rows finish at {fin}; sheds {plan['shed']}")
    assert len(plan["shed"]) >= 2
    _compare(f"sampling {len(sampling)}-tuple", plain, shed, _bounds(False, "rand", B, S, N, seed, sampling), eos, sampled=True)


def test_state_hygiene():
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 24
    seed, eos, fin, want = _spread_case(False, B, S, N, LADDER, 1)
    emb = _free(False, "rand", B, S, N, seed)[0]
    eng.invalidate()
    call = lambda **kw: eng.generate(emb, N, eos_token_id=eos, pad_token_id=PAD, return_step_logits=True, **kw)
    before = call()
    root, g0, ws0 = eng._dec[0], eng._dec[0].graph, eng._dec[0].ws
    assert g0 is not None
    first = call(shed_finished=LADDER, shed_every=1)
    plan1 = dict(eng.last_plan)
    assert plan1["shed_captures"] == len({a for _, _, a, _ in plan1["shed"]}) >= 2, "one graph per rung met; the root's graph was there already"
    second = call(shed_finished=LADDER, shed_every=1)
    plan2 = dict(eng.last_plan)
    assert plan2["shed_captures"] == 0 and plan2["shed"] == plan1["shed"]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), "the same shedding call twice"
    after = call()
    assert eng._dec[0] is root and root.graph is g0 and root.ws is ws0, "the parent's state, workspace and graph survive a shedding call"
    assert "shed" not in eng.last_plan
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]), "a plain call after a shedding call"
    assert len(root.children) == plan1["shed_captures"]
    eng.invalidate()
    assert not eng._dec, "invalidate() drops the children with their parent"


def test_model_surface():
    um, eng, hid = _um(False)
    B, S, N = 6, 9, 24
    seed, eos, fin, want = _spread_case(False, B, S, N, LADDER, 1)
    emb = _free(False, "rand", B, S, N, seed)[0]
    direct = eng.generate(emb, N, eos_token_id=eos, pad_token_id=PAD, shed_finished=True, shed_every=1)
    via = um.generate(inputs_embeds=emb, max_new_tokens=N, eos_token_id=eos, pad_token_id=PAD, shed_finished=True, shed_every=1)
    assert torch.equal(direct, via) and eng.last_plan["shed"], "the default ladder sheds a six-row wave to four rows"
    with pytest.raises(NotImplementedError, match="num_beams"):
        um.generate(inputs_embeds=emb, max_new_tokens=4, shed_finished=True, num_beams=2)
