"""Beam search as plain torch on the CPU: one step (`step`) and a whole call (`walk`) of HF's vectorised GenerationMixin._beam_search
(transformers generation/utils.py: _get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams,
_check_early_stop_heuristic, _beam_search_has_unfinished_sequences), restated per clip on the state layout of csrc/beam.hip
(include/crab_hip.h "Beam search"):

    run_score [rows] fp32, run_seq [rows, max_new] int64, hyp_score [rows] fp32, hyp_seq [rows, max_new] int64, hyp_len [rows] int32,
    hyp_fin [rows] int32, unsat [clips] int32, finished [rows] int32, cur_ids [rows] int64, beam_idx [rows] int32       rows = clips x K

HF's torch.topk leaves the order of equal scores open; here (and in the kernels) it is explicit: the higher score first, then the lower index -
the flat index k V + token among continuations, the position in the merged list (kept hypotheses first) in the finalise merge.  One consequence
is used below: a candidate that is NOT finalised carries a score <= -1e9 into the merge and a kept placeholder exactly -1e9, so a placeholder
is never displaced - the hypotheses are real finished ones, then untouched placeholders (pad ids, length 0).  A clip that is done is frozen.

The margin of EITHER - derived from the kernel's arithmetic, never measured from it.  u = 2^-24, one row of V logits z, M = max z:
    d = fl(z - M)                         |d| u                      the argument of one term
    expf(d)                               2 u relative (1 ulp documented, 2 taken) + the argument's |d| u
    a row's sum S                         the terms' errors weigh in by their mass: W u with W = sum e^d |d| / sum e^d, + 2 u;
                                          one thread's serial sum of c = ceil(V / 256) terms (c - 1) u, 6 shuffle levels 6 u, the four
                                          wave partials 2 u               => relative (W + c + 9) u =: eS
    logf(S)                               eS absolute from S, + 2 u |log S|
    lse = fl(M + log S)                   u |lse|
    t = fl(z - lse),  s = fl(run + t)     u |t| + u |s|
    margin(candidate) = eS + u (2 |log S| + |lse| + |t| + |s|)
    f = fl(s / len_tab[n])                margin / len_tab[n] + u |f|      (a true fp32 division by the fp32 table entry)
Two candidates whose fp64 scores differ by less than the sum of their margins have no order the kernel is held to.  A step of a clip is EITHER
when such a pair decides anything: the boundary of the best 2K, the order inside them (the first K are the ones that may be finalised, all of
them may become running beams), the finalise merge among real hypotheses, or the early-stop comparison.  With margin = 0 (`exact`) the
reference is HF's step on tie-free inputs."""
import math
import types

import torch

U = 2.0 ** -24
NEG = -1.0e9


def len_table(max_new: int, length_penalty: float) -> torch.Tensor:
    """n ** length_penalty as HF's Python scalar (a double), rounded to fp32 once; entry 0 unused."""
    return torch.tensor([1.0] + [float(n) ** float(length_penalty) for n in range(1, max_new + 1)], dtype=torch.float64).to(torch.float32)


class Params:
    def __init__(self, K, V, max_new, eos=-1, pad=0, min_new=0, length_penalty=1.0, early_stopping=False):
        self.K, self.V, self.max_new = int(K), int(V), int(max_new)
        self.eos, self.pad, self.min_new = (-1 if eos is None else int(eos)), int(pad), int(min_new)
        self.length_penalty, self.early_stopping = float(length_penalty), early_stopping
        self.len_tab = len_table(self.max_new, self.length_penalty)


def init_state(clips: int, p: Params) -> dict:
    rows, K = clips * p.K, p.K
    run = torch.full((rows,), NEG, dtype=torch.float32)
    run[::K] = 0.0
    return {"run_score": run, "run_seq": torch.full((rows, p.max_new), p.pad, dtype=torch.int64),
            "hyp_score": torch.full((rows,), NEG, dtype=torch.float32), "hyp_seq": torch.full((rows, p.max_new), p.pad, dtype=torch.int64),
            "hyp_len": torch.zeros(rows, dtype=torch.int32), "hyp_fin": torch.zeros(rows, dtype=torch.int32),
            "unsat": torch.ones(clips, dtype=torch.int32), "finished": torch.zeros(rows, dtype=torch.int32),
            "cur_ids": torch.zeros(rows, dtype=torch.int64), "beam_idx": torch.arange(K, dtype=torch.int32).repeat(clips)}


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _add32(a: float, b: float) -> float:
    return float(torch.tensor(a, dtype=torch.float32) + torch.tensor(b, dtype=torch.float32))


def _div32(a: float, b: float) -> float:
    return float(torch.tensor(a, dtype=torch.float32) / torch.tensor(b, dtype=torch.float32))


def row_candidates(z: torch.Tensor, run: float, n: int, eos_masked: int, exact: bool = False):
    """The best n continuations of one row: (fp64 scores, tokens, margins), sorted by (score desc, token asc).  z [V] fp32."""
    V = z.shape[0]
    zd = z.double()
    M = zd.max()
    d = zd - M
    e = torch.exp(d)
    S = e.sum()
    logS = torch.log(S)
    lse = M + logS
    t = zd - lse
    s = run + t
    if eos_masked >= 0:
        s[eos_masked] = -math.inf
    s = torch.where(torch.isnan(s), torch.full_like(s, -math.inf), s)
    top = torch.topk(s, min(n, V)).values[-1]
    idx = torch.nonzero(s >= top)[:, 0]                        # everything tied with the n-th included, in token order
    order = torch.argsort(s[idx], descending=True, stable=True)[:n]
    idx = idx[order]
    if exact:
        return s[idx], idx, torch.zeros(idx.numel(), dtype=torch.float64)
    W = float((e * d.abs()).nan_to_num(0.0).sum() / S) if math.isfinite(float(S)) and float(S) > 0 else 0.0
    eS = (W + -(-V // 256) + 9.0) * U
    fin = lambda x: x.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0)
    m = eS + U * (2.0 * abs(float(logS)) + abs(float(lse)) + fin(t[idx]) + fin(s[idx]))
    return s[idx], idx, m


def step(before: dict, logits: torch.Tensor, step_no: int, p: Params, exact: bool = False):
    """One beam step of every clip from the state `before` and the step's raw logits [rows, V] fp32.  Returns (after, either, tol):
    after - the state the kernels must leave (float fields as fp32 of the fp64 value); either - one bool per clip (module docstring);
    tol - {"run_score", "hyp_score"}: the bound on |device - after| of every entry."""
    K, V, N = p.K, p.V, p.max_new
    rows = logits.shape[0]
    clips = rows // K
    after = {k: v.clone() for k, v in before.items()}
    either = [False] * clips
    tol = {"run_score": torch.zeros(rows, dtype=torch.float64), "hyp_score": torch.zeros(rows, dtype=torch.float64)}
    eos_masked = p.eos if (p.eos >= 0 and step_no < p.min_new) else -1
    last = step_no + 1 >= N
    den = float(p.len_tab[step_no + 1])
    for c in range(clips):
        r0 = c * K
        if int(before["finished"][r0]) != 0:
            continue                                           # frozen
        # ---- c. the clip's best 2K (+ the first one left out) of the K x V continuations
        cs, cf, cm = [], [], []
        for k in range(K):
            s, tok, m = row_candidates(logits[r0 + k], float(before["run_score"][r0 + k]), 2 * K + 1, eos_masked, exact)
            cs.append(s); cf.append(tok + k * V); cm.append(m)
        cs, cf, cm = torch.cat(cs), torch.cat(cf), torch.cat(cm)
        order = sorted(range(cs.numel()), key=lambda i: (-float(cs[i]), int(cf[i])))[:2 * K + 1]
        s2, f2, m2 = cs[order], cf[order], cm[order]
        amb = False
        for i in range(min(2 * K, s2.numel() - 1)):
            if float(s2[i]) - float(s2[i + 1]) < float(m2[i]) + float(m2[i + 1]) and not (float(s2[i]) == -math.inf and float(s2[i + 1]) == -math.inf):
                amb = True
        ts = [float(x) for x in s2[:2 * K]]
        tm = [float(x) for x in m2[:2 * K]]
        tp = [int(x) // V for x in f2[:2 * K]]
        tt = [int(x) % V for x in f2[:2 * K]]
        ts32 = [_f32(x) for x in ts]
        # ---- d. stopping criteria, e. the next running beams
        hit = [last or (p.eos >= 0 and tt[i] == p.eos) for i in range(2 * K)]
        rs = [_add32(ts32[i], NEG) if hit[i] else ts32[i] for i in range(2 * K)]
        if not exact:
            for i in range(2 * K):
                if hit[i] and math.isfinite(ts[i]) and _add32(_f32(ts[i] - tm[i]), NEG) != _add32(_f32(ts[i] + tm[i]), NEG):
                    amb = True                                 # the pushed-down value rounds to a multiple of 64: the kernel's own score may round the other way
        sel = sorted(range(2 * K), key=lambda i: (-rs[i], i))[:K]
        for k, i in enumerate(sel):
            after["run_score"][r0 + k] = rs[i]
            tol["run_score"][r0 + k] = tm[i] + U * abs(rs[i]) if math.isfinite(rs[i]) else 0.0
            after["cur_ids"][r0 + k] = tt[i]
            after["beam_idx"][r0 + k] = tp[i]
            row = before["run_seq"][r0 + tp[i]].clone()
            row[step_no] = tt[i]
            row[step_no + 1:] = p.pad
            after["run_seq"][r0 + k] = row
        # ---- f. finalise: the candidates among the first K that stopped, unless a guard holds; merge with the kept hypotheses
        unsat_old = bool(before["unsat"][c])
        full = p.early_stopping is True and bool(before["hyp_fin"][r0:r0 + K].all())
        merged = [(float(before["hyp_score"][r0 + k]), 0.0, k) for k in range(K)]
        for i in range(2 * K):
            did = hit[i] and i < K
            f = _div32(ts32[i], den)
            for g in (full, not unsat_old, not did):
                if g:
                    f = _add32(f, NEG)
            merged.append((f, tm[i] / den + U * abs(f) if math.isfinite(f) else 0.0, K + i))
        mo = sorted(merged, key=lambda e: (-e[0], e[2]))
        real = [e for e in mo[:K + 1] if e[0] > 0.5 * NEG]
        for a, b in zip(real, real[1:]):
            if a[0] - b[0] < a[1] + b[1] and not (a[2] < K and b[2] < K):
                amb = True
        for j, (f, ftol, src) in enumerate(mo[:K]):
            after["hyp_score"][r0 + j] = f
            tol["hyp_score"][r0 + j] = ftol
            if src < K:
                after["hyp_seq"][r0 + j] = before["hyp_seq"][r0 + src]
                after["hyp_len"][r0 + j] = before["hyp_len"][r0 + src]
                after["hyp_fin"][r0 + j] = before["hyp_fin"][r0 + src]
            else:
                i = src - K
                did = hit[i] and i < K
                row = before["run_seq"][r0 + tp[i]].clone()
                row[step_no] = tt[i]
                row[step_no + 1:] = p.pad
                after["hyp_seq"][r0 + j] = row
                after["hyp_fin"][r0 + j] = int(did)
                after["hyp_len"][r0 + j] = step_no + 1 if did else 0
        # ---- g. the early-stop heuristic and the clip's done flag
        blen = N if (p.early_stopping == "never" and p.length_penalty > 0.0) else step_no + 1
        run0 = float(after["run_score"][r0])
        best = _div32(run0, float(p.len_tab[blen]))
        best_tol = float(tol["run_score"][r0]) / float(p.len_tab[blen]) + U * abs(best) if math.isfinite(best) else 0.0
        hs = [float(x) for x in after["hyp_score"][r0:r0 + K]]
        worst_all = min(hs)
        any_better = False
        for j in range(K):
            w = worst_all if int(after["hyp_fin"][r0 + j]) else NEG
            any_better = any_better or best > w
            wt = max(float(x) for x in tol["hyp_score"][r0:r0 + K]) if int(after["hyp_fin"][r0 + j]) else 0.0
            if abs(best - w) <= best_tol + wt and unsat_old and not exact:
                amb = True
        unsat_new = unsat_old and any_better
        after["unsat"][c] = int(unsat_new)
        all_fin = bool(after["hyp_fin"][r0:r0 + K].all())
        go_on = unsat_new and not (all_fin and p.early_stopping is True) and not all(hit)
        after["finished"][r0:r0 + K] = 0 if go_on else 1
        either[c] = amb and not exact
    return after, either, tol


def walk(logits_fn, clips: int, p: Params, num_return_sequences: int = 1):
    """A whole call: logits_fn(state, step) -> raw logits [rows, V] fp32 of the running beams.  Returns (ids [clips * R, n] - new ids only, best
    hypothesis first per clip, pad after a hypothesis's EOS, n the longest returned -, sequences_scores fp32 [clips * R], EITHER steps seen)."""
    st = init_state(clips, p)
    n_either = 0
    for s in range(p.max_new):
        st, either, _ = step(st, logits_fn(st, s), s, p, exact=False)
        n_either += sum(either)
        if bool(st["finished"].all()):
            break
    K, R = p.K, int(num_return_sequences)
    keep = torch.tensor([c * K + j for c in range(clips) for j in range(R)])
    n = max(1, int(st["hyp_len"][keep].max()))
    return st["hyp_seq"][keep][:, :n], st["hyp_score"][keep], n_either


def compare(dev: dict, after: dict, tol: dict, clip: int, K: int):
    """The mismatches of clip `clip` between a device state and the reference's `after` (both dicts of CPU tensors): a list of strings."""
    r = slice(clip * K, clip * K + K)
    bad = []
    for f in ("run_seq", "hyp_seq", "hyp_len", "hyp_fin", "finished", "cur_ids", "beam_idx"):
        if not torch.equal(dev[f][r].to(after[f].dtype), after[f][r]):
            bad.append(f"{f}: device {dev[f][r].tolist()} vs reference {after[f][r].tolist()}")
    if int(dev["unsat"][clip]) != int(after["unsat"][clip]):
        bad.append(f"unsat: device {int(dev['unsat'][clip])} vs reference {int(after['unsat'][clip])}")
    for f in ("run_score", "hyp_score"):
        d, a = dev[f][r].double(), after[f][r].double()
        same_inf = torch.isinf(d) & torch.isinf(a) & (d == a)
        err = torch.where(same_inf, torch.zeros_like(d), (d - a).abs())
        lim = tol[f][r] + U * a.abs().nan_to_num(0.0, posinf=0.0, neginf=0.0)
        if not bool((err <= lim).all()):
            bad.append(f"{f}: device {d.tolist()} vs reference {a.tolist()} (bound {lim.tolist()})")
    return bad


# ------------------------------------------------------------------ the seeded inputs of the kernel-level GPU test (tests/test_beam_gpu.py)
# Logits randn * 4: at this scale the share of near-tied steps is a fraction of a percent for K <= 8 and V <= 32000 (at scale 1 with K = 8 it
# comes close to the cap).  tests/test_beam_host.py asserts the share from this reference alone; the GPU test counts it again from the device's
# own trajectory.
CLIPS, STEPS, EOS, PAD, SCALE = 3, 12, 7, 1, 4.0
EITHER_CAP = 0.05


def _case(name, V=320, K=4, lp=1.0, early=False, min_new=0, eos=EOS, force=None):
    return types.SimpleNamespace(name=name, V=V, K=K, lp=lp, early=early, min_new=min_new, eos=eos, force=force or {})


# force: {step: (clips or None = all, what added to the EOS column)}
GPU_CASES = [_case(f"V{V} K{K}", V=V, K=K) for V in (320, 515, 32000) for K in (1, 2, 4, 8)] + [
    _case("EOS is the best candidate of the first step", force={0: (None, 40.0)}),
    # "never" with a positive penalty measures the running beams at max length: the clip goes on with the backups K .. 2K after the step
    _case("all of the first K candidates are EOS in one step", early="never", lp=2.0, force={2: (None, 60.0)}),
    _case("early_stopping=True ends a clip when K hypotheses exist", K=2, early=True, force={s: (None, 12.0) for s in range(1, STEPS)}),
    _case('"never" with a positive penalty', early="never", lp=2.0, force={s: (None, 10.0) for s in range(1, STEPS)}),
    _case("length_penalty 0", lp=0.0, force={s: (None, 10.0) for s in range(1, STEPS)}),
    _case("length_penalty -1", lp=-1.0, force={s: (None, 10.0) for s in range(1, STEPS)}),
    _case("min_new_tokens 2", min_new=2, force={s: (None, 40.0) for s in range(0, 4)}),
    _case("no EOS until the last step", eos=None),
    _case("-inf columns", V=515, force={"ninf": (5, 200)}),
    _case("one clip done at step 3 while the others run", K=2, early=True, force={3: ((0,), 60.0)}),
]


def case_params(c) -> Params:
    return Params(c.K, c.V, STEPS, c.eos, PAD, c.min_new, c.lp, c.early)


def case_logits(c, step_no: int) -> torch.Tensor:
    """The raw logits [CLIPS * K, V] fp32 of step `step_no` of a case: seeded, independent of the beams (the kernels are driven directly)."""
    g = torch.Generator().manual_seed(1000 * GPU_CASES.index(c) + step_no + 17)
    z = torch.randn((CLIPS * c.K, c.V), generator=g, dtype=torch.float32) * SCALE
    if "ninf" in c.force:
        lo, hi = c.force["ninf"]
        z[:, lo:hi] = -math.inf
    if step_no in c.force and c.eos is not None:
        clips, add = c.force[step_no]
        for cl in (range(CLIPS) if clips is None else clips):
            z[cl * c.K:(cl + 1) * c.K, c.eos] += add
    return z


def case_either_share(c):
    """(EITHER (clip, step) pairs, live (clip, step) pairs) of a case along the reference's own trajectory."""
    p = case_params(c)
    st = init_state(CLIPS, p)
    hit = live = 0
    for s in range(STEPS):
        live += CLIPS - int(st["finished"][::c.K].sum())
        st, either, _ = step(st, case_logits(c, s), s, p)
        hit += sum(either)
    return hit, live
