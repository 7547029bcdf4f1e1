"""Score laws for the attention tests (tests/test_attn_laws_host.py, tests/test_attn_laws_gpu.py, scripts/fuzz_attn.py).  Imports only torch; runs on
any device.  Not a test module.

The old law of the suite (q, k = 0.7 N(0,1), scale d^-1/2) gives scores of standard deviation about 0.5: an almost uniform softmax whose running
maximum hardly moves, whose rescale factors exp(m_old - m_new) stay in [e^-2, 1] and whose partial maxima agree to a unit.  The laws here are
rank-one plus noise, so that ONE profile t holds for every query row that shares the keys:

    q, k, v = 0.7 N(0,1);   q[..., 0] = A = 8;   k[..., j, 0] = t_j / (scale A);   everything rounded to bf16

Score (i, j) is then t_j (1 + O(2^-9)) + O(0.5) (the noise of the other d - 1 columns).  Profiles over the n visible keys, peak height R:

    ramp_up    R j / (n - 1)              the maximum rises in every tile, key group and split
    ramp_down  R (1 - j / (n - 1))        maximum at key 0; later probabilities shrink to exact 0
    saw        R (j mod 17) / 16          maxima move between the 16 key groups and between the two keys of a trip
    sink       R at key 0, else 0         the first key dominates; every later tile rescales by 1
    last       R at the newest key        everything accumulated so far is rescaled to about 0 in the last step
    edges      R at j mod 64 in {63, 0}   peaks on both sides of every tile, chunk and prefetch edge
    two        R at n // 3, 2 n // 3 + 1  equal maxima in different groups and splits
    shift_neg  -R on every key            offset against the -1e30 sentinel
    shift_pos  +R on every key            exp range without the maximum subtracted

R is 12 or 40 at every head size and also 90 at d = 32 / 64 (exp(-90) is below the smallest normal fp32; at d = 128 the derived fp32 slack of
tests/fuzz_bounds.attn_bound_weighted passes its 2^-10 cap there, so it is left out).

Two V laws: plain 0.7 N(0,1), and "loud tail": the V row of every key whose reference probability is below 2^-24 on EVERY query row that shares
it is multiplied by 64 (exact in bf16) - a key that should weigh nothing but is given weight then shows.

Slots outside the visible range are NaN for the kernel (poison) and 0 for the fp64 reference (clean): the reference multiplies them by an exact 0."""
import math

import torch

A = 8.0
PEAKED = ("ramp_up", "ramp_down", "saw", "sink", "last", "edges", "two")
SHIFTS = ("shift_neg", "shift_pos")
NAMES = PEAKED + SHIFTS
LOUD = 64.0
TAIL = 2.0 ** -24
BF = torch.bfloat16
F64 = torch.float64


def heights(d):
    return (12, 40, 90) if d in (32, 64) else (12, 40)


def profile(name, n, R, device=None):
    """t [n] (fp64) of the profile over n visible keys, oldest first."""
    j = torch.arange(n, dtype=F64, device=device)
    t = torch.zeros(n, dtype=F64, device=device)
    if n == 0: return t
    if name == "ramp_up": return R * j / max(n - 1, 1)
    if name == "ramp_down": return R * (1 - j / max(n - 1, 1))
    if name == "saw": return R * (j % 17) / 16
    if name == "sink": t[0] = R
    elif name == "last": t[n - 1] = R
    elif name == "edges": t[((j % 64) == 63) | ((j % 64) == 0)] = R
    elif name == "two": t[min(n // 3, n - 1)] = R; t[min(2 * n // 3 + 1, n - 1)] = R
    elif name == "shift_neg": t += -R
    elif name == "shift_pos": t += R
    else: raise ValueError(name)
    return t


def spread(name, R, visible):
    """visible bool [B, T] -> t [B, T] (fp64): the profile over every sequence's visible keys in slot order, 0 elsewhere."""
    t = torch.zeros(visible.shape, dtype=F64, device=visible.device)
    for b in range(visible.shape[0]):
        n = int(visible[b].sum())
        t[b, visible[b]] = profile(name, n, R, visible.device)
    return t


def draw(shape, gen, device=None):
    return torch.randn(shape, generator=gen, device=device) * 0.7


def plant(q, k, t, scale):
    """q [..., d], k [B, Hk, T, d] (fp32, changed in place), t broadcastable to [B, Hk, T]: column 0 carries the profile.  Returns bf16 (q, k)."""
    q[..., 0] = A
    k[..., 0] = (torch.as_tensor(t, dtype=F64, device=k.device) / (scale * A)).to(k.dtype).expand(k.shape[:-1])
    return q.to(BF), k.to(BF)


def loud_tail(v, p):
    """v [B, Hk, T, d] bf16, p [B, H, Sq, T] reference probabilities -> v with the rows of the keys below TAIL on every query row x LOUD."""
    B, Hk, T, _ = v.shape
    top = p.reshape(B, Hk, -1, T).amax(2)                                          # [B, Hk, T]: over the heads of the group and the query rows
    return torch.where((top < TAIL)[..., None], v.float() * LOUD, v.float()).to(BF)


def poison(x, keep):
    """x [B, Hk, T, d], keep bool [B, T]: NaN in every slot the kernel must not read."""
    return torch.where(keep[:, None, :, None], x, torch.full_like(x, math.nan))


def clean(x):
    return x.nan_to_num(0.0)
