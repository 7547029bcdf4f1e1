"""fp64 references and DERIVED per-element error bounds for the differential fuzzers (scripts/fuzz_gemm.py, fuzz_attn.py, fuzz_ops.py,
fuzz_rope_epilogue.py) and tests/test_c_abi_gpu.py.  Imports only torch; runs on any device; restates no kernel: a reference here is the plain
operation in fp64 on the operands the kernel was given, and a bound is the largest error the kernel's arithmetic can legitimately leave on an
element.  No bound is computed from the output under test.  Every number comes from the operands and the fp64 reference, from
U = 2^-9 and U32 = 2^-24, or from TOL_F32 (shared with tests/test_ops_gpu.py).

One bf16 rounding to nearest - half_ulp(y)
    bf16 keeps 8 significant bits: the spacing in the binade [2^e, 2^(e+1)) is 2^(e-7) (2^-7 |y| at the bottom of the binade: "one bf16
    ulp"), so a rounding to nearest moves a value by at most half of it, 2^(e-8) = U * 2^(e+1): U times the TOP of the element's binade.
    That is U |y| only at the top of a binade and 2 U |y| at the bottom (y = 1 + 2^-8 - tiny is stored as 1), so the store term is taken
    exactly, half_ulp(y) = U * 2^(floor(log2 |y|) + 1), never as the product U * |y| (which a correctly rounded store exceeds on about half
    of all elements; tests/test_fuzz_bounds_host.py::test_half_ulp_is_attained_and_sufficient).
    A store rounds the kernel's fp32 value y^, not y.  With |y^ - y| <= delta: if y^ lies in y's binade or a lower one the rounding moves it
    by at most half_ulp(y); if it lies in a higher one, 2^(e+1) is a bf16 number between y and y^, so the rounding moves it by at most delta.
    Hence |bf16(y^) - y| <= max(half_ulp(y), delta) + delta                                                         (stored()).

GEMM (crab_gemm_bf16: csrc/gemm*.hip, skinny.hip, rowfin.hip; epilogue order of gemm_epilogue.h: sums + bias, activation, + residual, store)
    The products of two bf16 numbers are exact in fp32; every kernel adds K + K2 of them in SOME order (MFMA chunks, split-K slices,
    K extension), which leaves at most (K + K2 - 1) U32 A on the sum whatever the order (A the sum of the absolute products).  Bias add,
    residual add and the activation's last rounding: 3 more.  The any-order ceiling of an element is therefore
        ceil_ij = (K + K2 + 4) U32 Lip (|x||w|^T + |x2||w2|^T + |bias| + |residual|)_ij + act_eval_ij
    with Lip the activation's Lipschitz constant (sup of |act'| over the reals: 1 for none / relu, 1.13 gelu, 1.1 silu and quick_gelu)
    and act_eval what evaluating the activation in fp32 at the (already perturbed) argument z adds: x / (1 + __expf(-a x)) has the
    argument's product (U32 |a z|), the exponential (2 U32), the sum and the division (3 U32) on a factor <= 1, erff a few U32 on a factor
    0.5 |z|: act_eval = (8 + 2 |z|) U32 |z|.  (It matters at K = 8 only.)
    An fp32 output must stay under BOTH TOL_F32 max|y| (the level tests/test_ops_gpu.py holds every epilogue to, up to K = 6144) and
    the ceiling: f32_ij = min(TOL_F32 max|y|, ceil_ij).  A bf16 output is that fp32 value with one rounding at the store:
    stored(y_ij, TOL_F32 max|y|).
    swiglu_pair: out = silu(a) b over the column pairs; d_out <= (|b| + d_b)(1.1 d_a + act_eval_a) + |silu(a)| d_b + U32 |out|.

Fused post-norm / RMSNorm (splitk_epilogue_norm_kernel, norm_kernel / norm_f32in_kernel of ops.hip)
    x_hat = x rstd, rstd = rsqrt(sum x^2 / D + eps): a lane adds at most ceil(D / 64) squares (exact products of bf16, one rounding each for
    fp32 rows) in series, then 6 butterfly levels and at most 4 wave partials: (D / 64 + 12) U32 on the sum, half of it on rstd, 2 U32 for
    the division, 2 for rsqrtf, 1 for the product x rstd:  RX = (D / 128 + 11) U32 relative on x_hat.
    fp32 row (no intermediate rounding, LlamaRMSNorm on an fp32 stream): h = bf16(x_hat w): stored(h_ref, (RX + U32) |h_ref|).
    bf16 row: the kernels round x_hat to bf16 BEFORE the weight (modeling_llama.py: weight * x_hat.to(input_dtype)), the reference does the
    same: h_ref = bf16(x_hat) w.  (One rounding of the unrounded form x_hat w, the shorter rule, leaves out this
    rounding: two roundings reach 2^-8 |h| + 2^-8 |h|.)  A rounding is discontinuous: where x_hat (1 - RX) and x_hat (1 + RX) round to
    different bf16 numbers lo != hi the kernel may hold either, which adds |hi - lo| |w| on that element alone.
    LayerNorm: y = bf16((x - mean) rstd w + b), one rounding; mean carries (D / 64 + 8) U32 mean|x|, x - mean one more rounding of |x|.

Router (hyperlora_mix_kernel / lora_mix_reduce_kernel / lora_route_row_kernel; the GEMM's fused router on the stored h)
    t = x [R;A]^T in fp32: d_t = (K + 2) U32 |x||RA|^T (any order).  p = softmax(t_route): the Jacobian's row sums are 2 p (1 - p) <= 1/2
    (Lipschitz <= 1 in the sup norm), evaluation (max, nl exponentials, sum, reciprocal): (2 spread + nl + 6) U32 p with spread the
    route logits' range.  u = bf16(scaling p_i t_j): two products.  f32 = scaling (|t_j| d_p + p_i d_tj) + 2 U32 |u_ref|; stored().
    The GEMM's fused router has TWO legitimate forms of its input row: the split-K reduction and the unfused pair read the normalised row h
    as stored (bf16); the M <= 16 tail (rowfin_apply_kernel / rowfin_norm_mix_kernel) forms t = rstd ((x (.) w) [R;A]^T) from the stored C
    before h is rounded - the same mix of the same row, a bf16 rounding of h apart (found by this bound on the GPU: up to 200 bounds on
    elements near 0).  Each form is held to its own reference with the same rule; an output must lie within one of them as a whole
    (Run.judge_any), so neither rounding can hide anything else.

SwiGLU pass (swiglu_kernel): bf16(silu(g) u): f32 = (9 + 2 |g|) U32 |ref|; stored().

Attention (csrc/attn.hip, attn_decode_core.h).  o_e = sum_j p_j v_je, p = softmax over the visible keys, S_e = sum_j p_j |v_je|.
    score: a d-term dot of exact products in fp32 (MFMA or lane-serial + 16-lane butterfly), the scale and log2(e) multiplies, the bias
    product and add:  d_s_j <= (d + 3) U32 T_j,  T_j = scale sum_d |q_d k_jd| + |gate bias_j|.
    p~_j = exp2(s_j - m): the subtraction and the log2(e) product 2 U32 |s_j - m|, v_exp_f32 one ulp (2 U32), the product p v one more.
    The running maximum m and the rescale factors exp(m_old - m_new) multiply numerator and denominator alike and cancel; what does not
    cancel are the roundings of the running sums: a term passes through at most ceil(n / 16) serial additions (16 key groups, or 16-key
    MFMA chunks) and as many rescale products, 32 more for the MFMA's internal tree, the group / wave merge and the shuffles -
    c(n) = 2 ceil(n / 16) + 32 for the numerator and the same for the denominator; 1 / l and the product: 2 more.  With
    E = max_j visible ((d + 3) T_j + 2 |s_j - m| + 3):
        slack_e = (2 E + 2 c(n) + 2) U32 S_e            (|o_e| <= S_e; n = visible keys of the row)
    Under the fuzz laws (q, k = 0.7 N(0,1), d <= 128, n <= 960) it stays under 2^-12 S_e (asserted on the host and in every fuzz case).
    decode kernels (attn_decode_kernel, _keymask, _gqa): P.V in fp32, one store:     stored(o_e, slack_e).
    forward kernels (crab_attn_fwd): p~ goes to the matrix pipe in bf16 while the row sum keeps the unrounded fp32 p~.  Each p~_j moves by
    at most half a bf16 ulp, up to 2 U p~_j at the bottom of its binade (which binade depends on the running maximum of its tile, so the
    worst place is taken): the numerator moves by sum_j rho_j p_j v_je with |rho_j| <= 2 U, at most 2 U S_e when every rounding falls
    against the sign of its v_je.  (U S_e is the top-of-binade case only: a row of two keys with p~ = (1, 1 + 2^-8 - tiny) / 2 exceeds it
    legitimately, tests/test_fuzz_bounds_host.py.)  Over hundreds of keys that worst case is out of reach and would hide a missing key
    (a one-key defect at 960 keys is about U S_e), so the sum is split into what the roundings have in common and the rest: a common
    rho moves the numerator by rho o_e, at most 2 U |o_e|; the rest are the roundings of unrelated scores, taken as independent with mean 0
    and range 2 U p_j |v_je| - Hoeffding's inequality puts their sum beyond HOEFFDING 2 U ||p (.) v_e||_2 with probability 1e-12 per element
    (HOEFFDING = sqrt(2 ln(2 / 1e-12)) = 7.52; a scale-4 soak judges about 1e9 elements).  The P term is the smaller of the two:
        P_e = 2 U min(S_e, |o_e| + HOEFFDING ||p (.) v_e||_2),        stored(o_e, P_e + slack_e).
    This is the one modelled (not worst-case) term of the module; it equals 2 U S_e on rows of a few keys.
    A row without a visible key is zeros: bound 0.

Attention under a peaked softmax (attn_bound_weighted; the laws of tests/attn_laws.py)
    E above is a maximum over the visible keys.  Under a peaked law it is set by keys of probability about 0 (|s_j - m| = R on a key that weighs
    e^-R) or by the one key that carries T_j = R, and the slack stops meaning anything.  The same terms, kept per key: key j's contribution
    to the numerator, p_j v_je, carries the relative error
        e_j U32,   e_j = (d + 3) T_j + 2 |s_j - m| + 3
    (its score error (d + 3) U32 T_j passes through exp with derivative 1 in relative terms; the subtraction and log2(e) product, v_exp_f32 and
    the product with v as above).  The telescoping argument covers the rescale products: whatever chain of running maxima m_1 <= ... <= m a
    kernel walks between key j's step and the end, the factors multiply to exp(m_1 - m) and their arguments' roundings add up to at most
    U32 (|s_j - m_1| + |m_1 - m_2| + ... ) <= 2 U32 |s_j - m| - what 2 |s_j - m| pays for, once for the key's own exponential and once for
    every rescale after it.  So the numerator N_e = sum_j p_j v_je moves by at most U32 sum_j p_j e_j |v_je| and the denominator (1 after
    normalisation) by U32 sum_j p_j e_j; o_e = N_e / D moves by the first plus |o_e| times the second.  The roundings of the running sums are
    c(n) U32 on each (numerator relative to S_e, denominator relative to 1), and 1 / l with the last product 2 U32 |o_e|:
        slack_e = 1.01 U32 [ sum_j p_j e_j |v_je|  +  |o_e| sum_j p_j e_j  +  c(n) (S_e + |o_e|)  +  2 |o_e| ]
    (1.01 for the second-order terms: every first-order term is below 2^-10.)  With e_j <= E and |o_e| <= S_e each of the four terms is at
    most its counterpart in (2 E + 2 c(n) + 2) U32 S_e, so slack_e <= 1.01 x the slack of attn_bound (asserted on the old law on the host).
    The P_e term of the forward kernels and stored() are unchanged; a row without a visible key keeps bound 0.
    The cap that keeps the slack from hiding a bf16-level defect is max_e slack_e / S_e <= 2^-10 (LAW_SLACK_CAP) under the new laws - at
    R = 12 it stays under the old 2^-12 as well; R = 90 at d = 128 would pass 2^-10 (e_j = 131 x 93 on the key that holds all the weight), which
    is why that pair is not among the laws.

RoPE epilogue, fused against unfused beyond 256 rows (dec2_choose may slice K differently)
    Both forms round the projection sum to bf16, rotate with the same pinned fp32 operations (rope_lo / rope_hi) and round again.  The two
    sums lie within the GEMM ceiling c of the exact y: they can round to different bf16 numbers only where y - c and y + c do, by
    g = bf16(y + c) - bf16(y - c).  Through the rotation (|cos| g_own + |sin| g_partner =: D, at most sqrt(2) max(g)) and the second
    rounding:  |a - b| <= D + 2 (half_ulp(|o_ref| + D)) + 6 U32 (|cos x| + |sin x'|), and 0 (bit-identical) where D = 0.
    (One bf16 ulp of the outputs, 2^-7 max(|a|, |b|), is the second rounding alone; it is not a bound where the rotation cancels.)
"""
import math

import torch

U = 2.0 ** -9
U32 = 2.0 ** -24
TOL_F32 = 3e-6       # fp32 outputs: accumulation order only (worst 1.15e-6 at K = 6144 on MI355X); tests/test_ops_gpu.py imports it from here
SLACK_CAP = 2.0 ** -12
LAW_SLACK_CAP = 2.0 ** -10      # attn_bound_weighted under the laws of tests/attn_laws.py
HOEFFDING = math.sqrt(2.0 * math.log(2.0 / 1e-12))
LIP = {"none": 1.0, "relu": 1.0, "gelu": 1.13, "silu": 1.1, "quick_gelu": 1.1, "swiglu_pair": 1.1}
F64 = torch.float64


def d64(t):
    return None if t is None else t.to(F64)


def bf16_round(x64):
    """fp64 -> the nearest bf16 number (8 significant bits, ties to even), as fp64; in one rounding (a cast through fp32 would round twice).
    Normal range only - no operand or output here comes near bf16's exponent limits."""
    m, e = torch.frexp(x64)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def half_ulp(y64):
    """Half a bf16 ulp at |y|: U times the top of y's binade (module docstring); 0 at 0."""
    a = y64.abs()
    top = torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent)                     # |y| = m 2^e with 1/2 <= m < 1: the top of its binade is 2^e
    return torch.where(a > 0, U * top, torch.zeros_like(a))


def stored(y64, delta):
    """Bound on |bf16(y^) - y| for an fp32 y^ within delta of y."""
    delta = torch.as_tensor(delta, dtype=F64, device=y64.device)
    return torch.maximum(half_ulp(y64), delta) + delta


def worst(got, ref64, bound):
    """(err / bound at the worst element, its index) - the verdict is ratio <= 1.  A bound of 0 asks for equality; a non-finite output is inf."""
    g = got.to(F64)
    err = (g - ref64).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, math.inf))
    if ratio.numel() == 0: return 0.0, ()
    i = flat = int(torch.argmax(ratio))
    idx = []
    for s in reversed(ratio.shape):
        idx.append(i % s); i //= s
    return float(ratio.reshape(-1)[flat]), tuple(reversed(idx))


class Run:
    """The verdicts of one fuzz run: every element of every output against its bound; keeps the worst err / bound and where it was."""

    def __init__(self):
        self.ratio, self.where = 0.0, "none"

    def judge(self, bad, desc, what, got, ref64, bound):
        ratio, idx = worst(got, ref64, bound)
        if ratio > self.ratio: self.ratio, self.where = ratio, f"{desc} [{what} at {idx}]"
        if not ratio <= 1.0: bad.append(desc + f" -> {what}: err / bound {ratio:.3f} at {idx}")
        return ratio

    def judge_any(self, bad, desc, what, got, forms):
        """forms: [(ref64, bound), ...] - the whole output must lie within ONE of them (the smallest of the forms' worst ratios counts)."""
        ratio, idx = min(worst(got, r, b) for r, b in forms)
        if ratio > self.ratio: self.ratio, self.where = ratio, f"{desc} [{what} at {idx}]"
        if not ratio <= 1.0: bad.append(desc + f" -> {what}: err / bound {ratio:.3f} at {idx} (the nearest of {len(forms)} forms)")
        return ratio

    def __str__(self):
        return f"worst err / bound {self.ratio:.3f} ({self.where})"


# ------------------------------------------------------------------------------------------------------------------------------- GEMM
def act64(z, act):
    if act == "gelu": return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752))
    if act == "quick_gelu": return z * torch.sigmoid(1.702 * z)
    if act == "relu": return z.clamp_min(0.0)
    if act == "silu": return z * torch.sigmoid(z)
    if act == "swiglu_pair": return z[:, 0::2] * torch.sigmoid(z[:, 0::2]) * z[:, 1::2]
    return z


def _gemm_parts(x, w, x2, w2, bias, act, residual):
    x, w, x2, w2, bias, residual = d64(x), d64(w), d64(x2), d64(w2), d64(bias), d64(residual)
    z = x @ w.t()
    A = x.abs() @ w.abs().t()
    K = x.shape[1]
    if x2 is not None:
        z = z + x2 @ w2.t(); A = A + x2.abs() @ w2.abs().t(); K += x2.shape[1]
    if bias is not None:
        z = z + bias; A = A + bias.abs()
    y = act64(z, act)
    if residual is not None: y = y + residual
    return z, A, K, y, residual


def gemm_ref(x, w, x2=None, w2=None, bias=None, act="none", residual=None):
    """act(x w^T + x2 w2^T + bias) + residual in fp64."""
    return _gemm_parts(x, w, x2, w2, bias, act, residual)[3]


def gemm_ceiling(x, w, x2=None, w2=None, bias=None, act="none", residual=None):
    """(y64, the any-order fp32 ceiling of every output element) - module docstring."""
    z, A, K, y, r = _gemm_parts(x, w, x2, w2, bias, act, residual)
    dz = (K + 4) * U32 * A
    ev = (8 + 2 * z.abs()) * U32 * z.abs() if act not in ("none", "relu") else torch.zeros_like(z)
    if act == "swiglu_pair":
        a, b = z[:, 0::2], z[:, 1::2]
        sa = a * torch.sigmoid(a)
        c = (b.abs() + dz[:, 1::2]) * (LIP[act] * dz[:, 0::2] + ev[:, 0::2]) + sa.abs() * dz[:, 1::2] + U32 * y.abs()
    else:
        c = LIP[act] * dz + ev
        if r is not None: c = c + (K + 4) * U32 * LIP[act] * r.abs()
    return y, c


def gemm_bound(x, w, x2=None, w2=None, bias=None, act="none", residual=None, out_bf16=False):
    """(y64, bound): fp32 output min(TOL_F32 max|y|, ceiling); bf16 output stored(y, TOL_F32 max|y|)."""
    y, c = gemm_ceiling(x, w, x2, w2, bias, act, residual)
    flat = TOL_F32 * float(y.abs().max()) if y.numel() else 0.0
    if out_bf16: return y, stored(y, flat)
    return y, torch.minimum(c, torch.full_like(c, flat))


# ------------------------------------------------------------------------------------------------------------ norms, SwiGLU, router
def rmsnorm_bound(x, w, eps, round_xhat):
    """(h_ref, bound) of bf16(rmsnorm(x) w).  round_xhat: the bf16-row kernels (x_hat rounded before the weight); False: the fp32-row form."""
    x, w = d64(x), d64(w)
    xh = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    rx = rx_rel(x.shape[-1])
    if not round_xhat:
        h = xh * w
        return h, stored(h, (rx + U32) * h.abs())
    h = bf16_round(xh) * w
    flip = (bf16_round(xh * (1 + rx)) - bf16_round(xh * (1 - rx))).abs() * w.abs()      # 0 unless x_hat sits on a rounding boundary
    return h, flip + stored(h.abs() + flip, U32 * (h.abs() + flip))


def rx_rel(D):
    """Relative fp32 error of x_hat = x rsqrt(mean x^2 + eps) over D columns (module docstring)."""
    return (D / 128.0 + 11) * U32


def layernorm_bound(x, w, b, eps):
    """(ref, bound) of bf16((x - mean) rstd w + b)."""
    x, w, b = d64(x), d64(w), d64(b)
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + eps)
    ref = xc * rstd * w + (b if b is not None else 0.0)
    c = D / 64.0 + 8
    d_xc = U32 * (x.abs() + c * x.abs().mean(-1, keepdim=True) + xc.abs())             # x - mean^: the rounding and the mean's own error
    # rstd: sum of (xc + d_xc)^2 -> relative 2 d_xc / rms on the sum in the worst case, plus the sum's c U32; half of it on rstd; + 4
    rms = xc.pow(2).mean(-1, keepdim=True).sqrt().clamp_min(1e-300)
    r_rstd = d_xc.pow(2).mean(-1, keepdim=True).sqrt() / rms + (c / 2 + 4) * U32
    f32 = (d_xc * rstd + xc.abs() * rstd * r_rstd + 2 * U32 * xc.abs() * rstd) * w.abs() + U32 * ref.abs()
    return ref, stored(ref, f32)


def swiglu_bound(gu):
    """(ref, bound) of bf16(silu(g) u) over gu = [g | u]."""
    gu = d64(gu)
    I = gu.shape[-1] // 2
    g, u = gu[:, :I], gu[:, I:]
    ref = g * torch.sigmoid(g) * u
    return ref, stored(ref, (9 + 2 * g.abs()) * U32 * ref.abs())


def route_bound(x, ra, nproj, nl, r, ucols, scaling, x_rel=0.0):
    """(u_ref [M, ucols], bound) of the hyper-LoRA routing mix of x [R;A]^T; padding columns are zeros (bound 0).  x_rel: relative fp32 error of the
    elements of x where the kernel forms them itself (the M <= 16 tail: x = the unrounded normalised row, rx_rel(N) + 2 U32), 0 for a stored x."""
    x, ra = d64(x), d64(ra)
    M, K = x.shape
    t = x @ ra.t()
    dt = ((K + 2) * U32 + x_rel) * (x.abs() @ ra.abs().t())
    ref = torch.zeros(M, ucols, dtype=F64, device=x.device)
    bnd = torch.zeros_like(ref)
    for p in range(nproj):
        tt, dd = t[:, p * (nl + r):(p + 1) * (nl + r)], dt[:, p * (nl + r):(p + 1) * (nl + r)]
        pr = torch.softmax(tt[:, :nl], -1)
        spread = tt[:, :nl].max(-1, keepdim=True).values - tt[:, :nl].min(-1, keepdim=True).values
        dp = dd[:, :nl].max(-1, keepdim=True).values + (2 * spread + nl + 6) * U32 * pr                 # [M, nl]
        uu = scaling * pr[:, :, None] * tt[:, None, nl:]
        f32 = scaling * (tt[:, None, nl:].abs() * dp[:, :, None] + pr[:, :, None] * dd[:, None, nl:]) + 2 * U32 * uu.abs()
        ref[:, p * nl * r:(p + 1) * nl * r] = uu.reshape(M, nl * r)
        bnd[:, p * nl * r:(p + 1) * nl * r] = stored(uu, f32).reshape(M, nl * r)
    return ref, bnd


# -------------------------------------------------------------------------------------------------------------------------- attention
def attn_ref(q, k, v, scale, allow, bias=None, gate=None, detail=False):
    """q [B, H, Sq, d], k / v [B, Hk, Skv, d] (H a multiple of Hk: grouped heads), allow bool broadcastable to [B, H, Sq, Skv], bias [H, Sq, Skv]
    with gate [B, H, Sq] -> (o64 [B, H, Sq, d], p64 [B, H, Sq, Skv]); a row without a visible key gives zeros.  detail: also (s, T)."""
    q, k, v = d64(q), d64(k), d64(v)
    G = q.shape[1] // k.shape[1]
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = torch.einsum("bhsd,bhtd->bhst", q, kk) * scale
    if bias is not None: s = s + d64(gate)[..., None] * d64(bias)[None]
    allow = allow.expand(s.shape)
    p = torch.softmax(s.masked_fill(~allow, -math.inf), -1).nan_to_num(0.0)
    o = torch.einsum("bhst,bhtd->bhsd", p, vv)
    if not detail: return o, p
    T = torch.einsum("bhsd,bhtd->bhst", q.abs(), kk.abs()) * scale
    if bias is not None: T = T + (d64(gate)[..., None] * d64(bias)[None]).abs()
    return o, p, s, T, vv, allow


def attn_bound(q, k, v, scale, allow, bias=None, gate=None, kind="decode"):
    """(o64, bound [B, H, Sq, d], worst slack_e / S_e of the case) for kind 'decode' (P.V in fp32) or 'fwd' (P in bf16) - module docstring."""
    o, p, s, T, vv, allow = attn_ref(q, k, v, scale, allow, bias, gate, detail=True)
    d = q.shape[-1]
    S = torch.einsum("bhst,bhtd->bhsd", p, vv.abs())
    n = allow.sum(-1, keepdim=True).to(F64)                                           # [B, H, Sq, 1]
    m = s.masked_fill(~allow, -math.inf).max(-1, keepdim=True).values
    E = ((d + 3) * T + 2 * (s - m).abs() + 3).masked_fill(~allow, 0.0).max(-1, keepdim=True).values
    c = 2 * torch.ceil(n / 16) + 32
    rel = (2 * E + 2 * c + 2) * U32                                                     # slack_e / S_e, per row
    slack = rel * S
    f32 = slack
    if kind == "fwd":
        n2 = torch.einsum("bhst,bhtd->bhsd", p * p, vv * vv).sqrt()                     # || p (.) v_e ||_2
        f32 = slack + 2 * U * torch.minimum(S, o.abs() + HOEFFDING * n2)
    bound = torch.where(n > 0, stored(o, f32), torch.zeros_like(o))
    return o, bound, float(rel.masked_fill(n == 0, 0.0).max()) if rel.numel() else 0.0


def attn_bound_weighted(q, k, v, scale, allow, bias=None, gate=None, kind="decode"):
    """attn_bound with the per-key terms weighted by the key's probability (module docstring): (o64, bound [B, H, Sq, d], max_e slack_e / S_e)."""
    o, p, s, T, vv, allow = attn_ref(q, k, v, scale, allow, bias, gate, detail=True)
    d = q.shape[-1]
    S = torch.einsum("bhst,bhtd->bhsd", p, vv.abs())
    n = allow.sum(-1, keepdim=True).to(F64)
    m = s.masked_fill(~allow, -math.inf).max(-1, keepdim=True).values
    pe = p * ((d + 3) * T + 2 * (s - m).abs() + 3).masked_fill(~allow, 0.0)            # p_j e_j; 0 on the hidden keys
    c = 2 * torch.ceil(n / 16) + 32
    slack = 1.01 * U32 * (torch.einsum("bhst,bhtd->bhsd", pe, vv.abs()) + o.abs() * pe.sum(-1, keepdim=True) + c * (S + o.abs()) + 2 * o.abs())
    f32 = slack
    if kind == "fwd":
        n2 = torch.einsum("bhst,bhtd->bhsd", p * p, vv * vv).sqrt()
        f32 = slack + 2 * U * torch.minimum(S, o.abs() + HOEFFDING * n2)
    bound = torch.where(n > 0, stored(o, f32), torch.zeros_like(o))
    rel = torch.where((n > 0) & (S > 0), slack / S.clamp_min(1e-300), torch.zeros_like(S))
    return o, bound, float(rel.max()) if rel.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------- RoPE epilogue pair
def rope_pair_bound(y64, ceil, cos, sin):
    """Bound on |fused - unfused| for one head's rotated block: y64 / ceil [..., d] the exact projection and its GEMM ceiling, cos / sin [..., d / 2]
    (broadcastable) the rotary table entries.  Returns (bound [..., d]); 0 where the two forms must agree bit for bit.  Unrotated blocks
    (v): pass cos = 1, sin = 0."""
    h = y64.shape[-1] // 2
    lo, hi = bf16_round(y64 - ceil), bf16_round(y64 + ceil)
    g = (hi - lo).abs()
    xa = torch.maximum(lo.abs(), hi.abs())
    c, s = cos.to(F64).abs(), sin.to(F64).abs()
    D = torch.cat([c * g[..., :h] + s * g[..., h:], c * g[..., h:] + s * g[..., :h]], -1)
    mag = torch.cat([c * xa[..., :h] + s * xa[..., h:], c * xa[..., h:] + s * xa[..., :h]], -1)
    x = bf16_round(y64)
    o = torch.cat([x[..., :h] * cos - x[..., h:] * sin, x[..., h:] * cos + x[..., :h] * sin], -1)
    b = D + 2 * half_ulp(o.abs() + D) + 6 * U32 * mag
    return torch.where(D > 0, b, torch.zeros_like(b))
