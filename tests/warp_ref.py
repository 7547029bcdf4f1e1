"""The kept set of one row under HF's whole sample-mode chain, in fp64, as classes a kernel's kept set can be held to:

    temperature -> top_k -> top_p                      tests/select_chain_ref.kept_classes (nothing of it is restated here)
    -> min_p -> epsilon_cutoff -> eta_cutoff           the INSTALLED transformers' MinPLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper,
                                                       called on float64 scores: the reference is HF's text, not a restatement of it

Every token is `KEEP`, `DROP` or `EITHER` as in select_chain_ref.  A new stage is classified by calling HF's warper twice, with its parameter
moved up and down by the stage's margin: a token is KEEP when the raised threshold still keeps it, DROP when the lowered one still removes
it.  The parameters are rounded to fp32 first - the kernel's arguments are floats.

The margins - derived from the arithmetic of csrc/select_core.h, never measured from it.  Notation of select_chain_ref's docstring:
u = 2^-24, X the largest finite |logit / temperature| of the row, c = ceil(V / 1024); from there

    one term       w_i = __expf(x~_i - mx~)              relative error <= (8 X + 3) u        (w of the maximum: __expf(0) = 1 exactly)
    a mass         Z  = sum of w over the current set    relative error <= (8 X + c + 23) u   (serial sum + the fixed 1024-way tree)

    min_p     the kernel keeps  w_i >= min_p             HF: p_i >= min_p * p_max <=> w_i >= min_p; only the term's error, + 1 u for the
                                                         second-order terms of every product of (1 + d)'s below as well:
                  m = (8 X + 4) u                        relative, on min_p (the raised value stops at 1: the kernel's argument is at
                                                         most 1 and the ties of the maximum, w = 1 exactly, pass it whatever it is)
    epsilon   the kernel keeps  w_i >= fl(eps * Z~)      HF: p_i >= eps <=> w_i >= eps * Z; the term, the mass, the product's rounding:
                  m = (8 X + 3 + 8 X + c + 23 + 1 + 1) u = (16 X + c + 28) u      relative, on eps
    eta       the kernel keeps  w_i >= fminf(fl(eps * Z~), fl(sqrtf(eps) * __expf(fl(S~ / Z~)))),  S = sum w_i d_i,  d_i = x_i - mx <= 0
              HF: eta = min(eps, sqrt(eps) * exp(-H)) and H = ln Z - S / Z, so p_i >= eta <=> w_i >= min(eps * Z, sqrt(eps) * exp(S / Z)).
              first branch: epsilon's margin.  second branch, with A = |S / Z| = sum p_i |d_i| (taken from the fp64 row):
                d~_i                 x~_i and mx~ carry 2 u X each, the subtraction u |d_i| <= 2 u X: absolute error <= 6 X u - and S / Z is a
                                     weighted mean of the d_i, so these add at most 6 X u to it, absolutely
                S~ / Z~              terms of one sign, so relative errors add: w_i (8 X + 3) u, the product w_i d_i 1 u, the sum (c + 20) u,
                                     Z~ (8 X + c + 23) u, the division 1 u: A (16 X + 2 c + 48) u, absolutely
                __expf(a)            a * log2(e) rounds: u |a| = u A on the argument; v_exp_f32 1 ulp = 2 u; an absolute error of the
                                     argument is a relative error of the result
                sqrtf(eps), product  2 u (1 ulp granted) + 1 u
                the term w_i         (8 X + 3) u
                  m = (6 X + A (16 X + 2 c + 48) + A + 2 + 3 + 8 X + 3 + 1) u = (14 X + A (16 X + 2 c + 49) + 9) u
              the stage's margin is the larger of the two branches.  HF takes ONE parameter: eps * (1 +- m)^2 moves the second branch
              (sqrt(eps)) by exactly 1 +- m and the first by more - a wider EITHER band there, never a narrower one.  EtaLogitsWarper keeps
              its epsilon as an fp32 tensor and so takes sqrt in fp32; the reference hands it a float64 tensor of the fp32 argument's value.

An `EITHER` token of an earlier stage moves the Z and H of the later ones.  The kernel's set after any stage is an upper set {x >= t} between
the sure set (KEEP) and the possible set (KEEP + EITHER); a stage is run on EVERY such upper set (the sure set plus the EITHER tokens above
each of their distinct values - a handful), a token is KEEP after the stage only when every one of them keeps it at the raised threshold, and
stays possible when any of them keeps it at the lowered one.  That is kept_classes' treatment of an ambiguous top-k boundary, carried on.
margin = 0 (`exact`) gives exactly HF's mask on tie-free rows.

The module also owns the stage grid of tests/test_warp_gpu.py - shapes, seeds, rows and parameters - so that tests/test_warp_host.py can hold,
on the CPU, the share of rows whose classes leave the kernel any freedom under the cap the GPU test needs to mean something."""
import functools
import math

import torch
from transformers.generation.logits_process import EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper

from tests import select_chain_ref as SC

U = SC.U
DROP, KEEP, EITHER = SC.DROP, SC.KEEP, SC.EITHER
NEG_INF = float("-inf")
STAGES = ("min_p", "epsilon_cutoff", "eta_cutoff")


def f32(v: float) -> float:
    """The value the kernel receives: its arguments are floats."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def stage_margin(stage: str, X: float, V: int, A: float = 0.0) -> float:
    """The derived relative margin (module docstring) of one stage's threshold for a row of V tokens with largest finite |scaled logit| X;
    A = |S / Z| of the set the stage runs on (eta only)."""
    c = -(-V // 1024)
    if stage == "min_p":
        return (8.0 * X + 4.0) * U
    m_eps = (16.0 * X + c + 28.0) * U
    if stage == "epsilon_cutoff":
        return m_eps
    return max(m_eps, (14.0 * X + A * (16.0 * X + 2.0 * c + 49.0) + 9.0) * U)


def hf_keep(scores: torch.Tensor, stage: str, value: float, rel: float = 0.0) -> torch.Tensor:
    """HF's own warper for `stage` on one float64 row (removed tokens at -inf) -> bool [V]: what it keeps.  The threshold parameter is
    value * (1 + rel) - for eta value * (1 + rel)^2 (module docstring) - set on the instance, whose constructor only admits the open range."""
    assert scores.dtype == torch.float64 and scores.dim() == 1
    if stage == "min_p":
        w = MinPLogitsWarper(0.5)
        w.min_p = min(1.0, value * (1.0 + rel))                  # never past 1: above it HF's mask loses the maximum's ties, whose w is exactly 1
    elif stage == "epsilon_cutoff":
        w = EpsilonLogitsWarper(0.5)
        w.epsilon = value * (1.0 + rel)
    else:
        w = EtaLogitsWarper(0.5)
        w.epsilon = torch.tensor(value * (1.0 + rel) ** 2, dtype=torch.float64)
    out = w(None, scores[None].clone())[0]
    return torch.isfinite(out)


def _upper_sets(x, lo, hi):
    """The upper sets S of x with lo <= S <= hi: lo, and lo plus the possible tokens at or above each of their distinct values."""
    amb = hi & ~lo
    sets = [lo] if bool(lo.any()) else []
    if bool(amb.any()):
        sets += [lo | (amb & (x >= v)) for v in torch.unique(x[amb]).tolist()]
    return sets


def warp_classes(row: torch.Tensor, allowed: torch.Tensor, sampling, min_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, exact: bool = False):
    """row [V] fp32, allowed [V] bool (the select's set: all but EOS under min_new_tokens), sampling = (temperature, top_k, top_p), the three
    stage values (0 / None = off).  -> (int8 [V] of DROP / KEEP / EITHER, {stage: the largest margin used}).  exact: margin 0 everywhere."""
    row = row.detach().float().cpu()
    V = row.shape[0]
    cls0, m0 = SC.kept_classes(row, allowed, sampling, exact)
    margins = {"top_p": m0}
    x = (row.double() / sampling[0]).masked_fill(~allowed, NEG_INF)
    fin = torch.isfinite(x)
    if not bool(fin.any()):
        return cls0, margins                                      # no mass at all: kept_classes leaves everything allowed EITHER
    X = float(x[fin].abs().max())
    lo, hi = cls0 == KEEP, cls0 != DROP
    for stage, value in zip(STAGES, (min_p, epsilon_cutoff, eta_cutoff)):
        value = f32(value or 0.0)
        if value == 0.0:
            continue
        new_lo, new_hi, used = lo.clone(), torch.zeros_like(hi), 0.0
        for S in _upper_sets(x, lo, hi):
            scores = x.masked_fill(~S, NEG_INF)
            A = 0.0
            if stage == "eta_cutoff":
                p = torch.softmax(scores, 0)
                A = float((p[S] * (scores[S] - scores[S].max()).abs()).sum())
            m = 0.0 if exact else stage_margin(stage, X, V, A)
            used = max(used, m)
            new_lo &= hf_keep(scores, stage, value, +m)
            new_hi |= hf_keep(scores, stage, value, -m)
        lo, hi, margins[stage] = new_lo, new_hi, used
    cls = torch.zeros(V, dtype=torch.int8)
    cls[hi] = EITHER
    cls[lo] = KEEP
    return cls, margins


def final_probs(row: torch.Tensor, cls: torch.Tensor, temperature: float) -> torch.Tensor:
    """fp64 probabilities of the draw over the KEEP tokens of a row whose classes hold no EITHER: softmax of the scaled logits on that set."""
    assert not bool((cls == EITHER).any())
    return torch.softmax((row.double() / temperature).masked_fill(cls != KEEP, NEG_INF), 0)


# ------------------------------------------------------------------ the stage grid of tests/test_warp_gpu.py
GRID_B = (1, 3, 17)
GRID_V = (96, 1000, 1025, 32000, 152064)          # fewer tokens than threads; a chunk edge (1024) from both sides; Llama (its last 24 threads own nothing); Qwen
GRID_FRONTS = {"bare": (0.8, 0, 1.0), "topk_topp": (0.7, 50, 0.9)}                    # (temperature, top_k, top_p) in front of the new stages
GRID_STAGE_NAMES = ("min_p", "epsilon", "eta", "all")   # each stage alone, all three together: (min_p, epsilon_cutoff, eta_cutoff) per front,
GRID_STAGES = {                                         # chosen so that every stage removes tokens of what the front left
    "bare": {"min_p": (0.05, 0.0, 0.0), "epsilon": (0.0, 3e-4, 0.0), "eta": (0.0, 0.0, 2e-3), "all": (0.02, 2e-4, 1e-3)},
    "topk_topp": {"min_p": (0.2, 0.0, 0.0), "epsilon": (0.0, 0.03, 0.0), "eta": (0.0, 0.0, 0.08), "all": (0.1, 0.02, 0.05)}}
GRID_EOS, GRID_MIN_NEW = 5, 2                     # step 0 < min_new_tokens: EOS is suppressed, and row 0 would otherwise draw it
CAP = 0.1                                         # the share of grid rows that may hold an EITHER token at the end of the chain


@functools.lru_cache(maxsize=None)
def grid_rows(B: int, V: int) -> torch.Tensor:
    """[B, V] fp32 for one grid shape: normal(0, 3); EOS is row 0's largest logit by far (min_new_tokens has to keep it out); the last row
    holds -inf entries (banned tokens), one of them where its maximum stood; with B > 2 row 1 is dominated by one token (a cutoff above
    every other probability: the maximum alone survives)."""
    g = torch.Generator().manual_seed(7919 * B + V)
    z = torch.randn((B, V), generator=g) * 3
    z[0, GRID_EOS] = z[0].max() + 9
    if B > 2:
        z[1, (2 * V) // 3] = z[1].max() + 25
    z[B - 1, int(z[B - 1].argmax())] = NEG_INF
    z[B - 1, V // 7] = z[B - 1, V - 1] = NEG_INF
    return z


def grid_allowed(V: int) -> torch.Tensor:
    a = torch.ones(V, dtype=torch.bool)
    a[GRID_EOS] = False
    return a


@functools.lru_cache(maxsize=None)
def grid_reference(B: int, V: int, front: str, stages: str):
    """[(classes, margins)] for the B rows of one grid case; computed once per process and never changed."""
    z, a = grid_rows(B, V), grid_allowed(V)
    return [warp_classes(z[b], a, GRID_FRONTS[front], *GRID_STAGES[front][stages]) for b in range(B)]


def kernel_scaled(row: torch.Tensor, temperature: float, suppress: int = -1) -> torch.Tensor:
    """The scaled logits as the kernel forms them, bit for bit: fl(z * fl(1 / T)) in fp32, -inf at the suppressed id."""
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    x = row.float() * inv_t
    if suppress >= 0:
        x[..., suppress] = NEG_INF
    return x
