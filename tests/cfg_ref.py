"""Plain torch fp64 statement of the classifier-free-guidance mix of the decode step (csrc/cfg.hip).  Pair b < B is row b (conditional, c) and
row B + b (unconditional, u) of the raw logits [2B, V]:

    guided[b, i] = lu + g * (lc - lu),      lc = c[i] - logsumexp(c),      lu = u[i] - logsumexp(u)

HF's UnbatchedClassifierFreeGuidanceLogitsProcessor: scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond).  An element that
is -inf in either row is -inf (the kernel's stated deviation: HF has NaN where both are), exactly.

Every value comes with the bound the fp32 kernel is held to, derived from its steps; U = 2^-24 is the unit roundoff of fp32, nothing is taken
from an output under test.

The normaliser of a row (lse = max + log S, rounded once to fp32).  A thread adds k = 4 ceil(V / 4096) + 2 terms exp(x - m) in series (its
16-byte chunks of four, one head and one tail element): (k - 1) U on a sum of positive terms whatever the order.  A term carries the rounding
of its exponent, U |x - m| <= U R with R the spread of the row's finite logits, and expf's 1 ulp (2 U).  The running maximum moves at most
once per chunk and once in head and tail, n = ceil(V / 4096) + 2 times; every move rescales the sum by expf(m_old - m_new): 2 U for expf and U for
the product, 3 U per move, and the exponents' roundings add up to at most U R because the moves telescope.  The merge of the 1024 partials,
the log and the sum max + log S are done in double: 1040 additions at 2^-53, below every other term but kept.  So
    rel(S) <= U ((k - 1) + (R + 2) + 3 n + R) + 1040 * 2^-53,      e_lse = rel / (1 - rel) + U |lse|
(a relative error on S is that absolute error on log S; the last term is the one rounding of lse to fp32).

The element.  lc = fl(c_i - lse_c): e_lc = e_lse_c + U |lc|, and the same for lu; d = fl(lc - lu): e_d = e_lc + e_lu + U (|d| + e_lc + e_lu);
out = fma(g, d, lu), one rounding: bound = g e_d + e_lu + U (|out| + g e_d + e_lu)."""
import torch

U32 = 2.0 ** -24
DBL = 2.0 ** -53
NEG_INF = float("-inf")


def lse_ref(row: torch.Tensor):
    """fp64 row -> (logsumexp, the bound on the kernel's fp32 value of it).  A row without a finite entry: (-inf, 0)."""
    V = int(row.shape[0])
    fin = row[row > NEG_INF]
    if fin.numel() == 0:
        return NEG_INF, 0.0
    lse = float(torch.logsumexp(fin, 0))
    spread = float(fin.max() - fin.min())
    chunks = -(-V // 4096)
    k, moves = 4 * chunks + 2, chunks + 2
    rel = U32 * ((k - 1) + (spread + 2) + 3 * moves + spread) + 1040 * DBL
    return lse, rel / (1 - rel) + U32 * abs(lse)


def mix_ref(logits: torch.Tensor, B: int, scale: float):
    """logits [2B, V] (any float dtype, any device) -> (guided fp64 [B, V], bound fp64 [B, V]) on the CPU.  scale: the fp32 value the kernel gets."""
    z = logits.detach().double().cpu()
    assert z.shape[0] == 2 * B
    g = float(torch.tensor(scale, dtype=torch.float32))
    ref = torch.empty((B, z.shape[1]), dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for b in range(B):
        c, u = z[b], z[B + b]
        (lse_c, e_c), (lse_u, e_u) = lse_ref(c), lse_ref(u)
        dead = (c == NEG_INF) | (u == NEG_INF)
        live = ~dead
        ref[b][dead] = NEG_INF
        if not bool(live.any()):
            continue
        lc, lu = c[live] - lse_c, u[live] - lse_u
        e_lc, e_lu = e_c + U32 * lc.abs(), e_u + U32 * lu.abs()
        d = lc - lu
        e_d = e_lc + e_lu + U32 * (d.abs() + e_lc + e_lu)
        out = lu + g * d
        ref[b][live] = out
        bound[b][live] = g * e_d + e_lu + U32 * (out.abs() + g * e_d + e_lu)
    return ref, bound


def choice_margin(ref_row: torch.Tensor, bound_row: torch.Tensor, chosen: int):
    """(how far the chosen token's reference score lies below the reference maximum, the margin a kernel that takes the argmax of scores within
    `bound` of the reference may leave: the bounds of the two elements)."""
    top = int(ref_row.argmax())
    return float(ref_row[top] - ref_row[chosen]), float(bound_row[top] + bound_row[chosen])
