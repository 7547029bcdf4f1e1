"""fp64 references and DERIVED per-element error bounds for the differential fuzzers (scripts/fuzz_gemm.py, fuzz_attn.py, fuzz_ops.py,
fuzz_rope_epilogue.py, fuzz_seg.py), tests/test_c_abi_gpu.py, tests/test_pixel_ops_gpu.py and the kernel tests of tests/test_vqgan.py.  Imports only torch; runs on any device; restates no kernel: a reference here is the plain
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

Pixel path (csrc/seg_ops.hip, csrc/vq_ops.hip).  A scalar argument (scale, eps, alpha, beta) reaches a kernel as a C float: the references take
its fp32 value (f32_arg), the operand the kernel was given.  Operation counts are read off the kernels' loops.

Row softmax (softmax_rows_kernel bf16 out / softmax_rows_f32_kernel), p_j = exp(s_j - m) / l, s = scale x.
    The product scale x_j is rounded once (or not at all where the compiler contracts it into the subtraction): |fp32(s_j) - s_j|, taken exactly
    from the operands (0 for a power-of-two scale).  The maximum is the same rounded value in numerator and denominator and cancels.  The
    subtraction and the log2(e) product of __expf move the argument by 2 U32 |s_j - m|, the exponential itself by one ulp (2 U32):
        a_j = |fp32(s_j) - s_j| + (2 |s_j - m| + 2) U32                                      (relative, on p~_j)
    The row sum moves by sum_k p_k a_k (each term by its own a_k) and by its own roundings: a thread adds ceil(N / 256) terms in series, 6
    butterfly levels, 3 additions of the 4 wave partials; 1 / l and the product p~ / l: 3 more (c = 12).
        f32_j = 1.01 (a_j + sum_k p_k a_k + (ceil(N / 256) + 12) U32) p_j + 2^-126
    (1.01: second order; every a_j that meets a p_j > 0 is below 2^-10.)  The smallest normal is added because an fp32 result below it may be
    flushed to 0: an entry whose exact value underflows is held to 2^-126, not to 0.  bf16 output: stored(p, f32).

In-place activation (act_kernel): bf16(act(x)) with apply_act, the GEMM epilogue's function: stored(act64(x), act_eval(x)).

Previous-mask gate (mask_gate_kernel): src (sigmoid(mean_c prev) + 1).  A lane adds ceil(ncls / 64) bf16 values in series, then 6 butterfly
    levels and the division: d_mean = ((ceil(ncls / 64) + 6) mean|prev| + |mean|) U32.  e = expf(-mean) moves by d_mean + 2 U32 relative;
    sig = 1 / (1 + e): the sum and the reciprocal 3 U32, and e weighs (1 - sig) in it; the + 1 one rounding of g = sig + 1:
        d_g = sig ((1 - sig)(d_mean + 2 U32) + 3 U32) + U32 g;      stored(src g, |src| d_g + U32 |src g|).

Group mean (group_mean_kernel): bf16(scale sum_{k < T} x_k): T - 1 serial additions and the product - stored(ref, (T + 1) U32 |scale| sum|x|).

Row square norms (row_sqnorm_kernel / row_sqnorm_f32_kernel): a lane adds ceil(D / 64) squares in series (exact for bf16 rows, one rounding each
    for fp32 rows), 6 butterfly levels: (ceil(D / 64) + 7) U32 sum e^2, fp32 output.

Dense positional encoding (dense_pe_kernel): [sin a | cos a], a = 2 pi (cx G0 + cy G1), c = 2 (i + 1/2) / n - 1 from the definition in fp64.
    The fp32 coordinate: a division and a subtraction, 3 U32 absolute (|c| <= 1); the two products and the sum U32 (|G0| + |G1|) + U32 |t|; the
    fp32 constant 2 pi and its product 2 U32 |a|:  d_a <= U32 (3 |a| + 8 pi (|G0| + |G1|)) <= 4 U32 (|a| + 2 pi (|G0| + |G1|)).
    sin / cos have slope <= 1 and sinf / cosf are good to 2 ulp of a value <= 1 (4 U32): stored(ref, d_a + 4 U32).

Bilinear resize (bilinear_kernel, align_corners = False): f = (i + 1/2) n_in / n_out - 1/2 clamped at 0, i0 = floor f, i1 = min(i0 + 1, n_in - 1),
    weight l = f - i0, all in fp64 from the definition.  The fp32 f carries the ratio's rounding, the product and the subtraction:
    d_f = 3 U32 (|f| + 1).  The interpolant is continuous and piecewise linear in f, so d_f enters times the slope - of the segment the fp64 f
    lies in or, where f is within d_f of a knot and the kernel lands on the other side, of a neighbouring one: S = the largest |v(k + 1) - v(k)|
    over the segments i0 - 1, i0, i0 + 1 (at the two columns / rows that take part).  The weights 1 - l, four products and three sums:
    6 U32 T, T the sum of the absolute terms.  d_v = 1.01 (d_fy S_y + d_fx S_x + 6 U32 T) (1.01: the cross terms).  out = beta out0 + alpha v:
    two products and a sum - bound = |alpha| d_v + 3 U32 (|beta out0| + |alpha| T); fp32 output, no store rounding.  beta = 0 does not read out0.

GroupNorm (groupnorm_stats_kernel + the three apply kernels; bf16 or fp32 rows, bf16 or fp32 parameters, bf16 or fp32 output).
    Statistics over n = HW C/G values of v = x - k, k the group's first value of the image (the shifted form).  A thread adds rows_per_chunk
    values of a channel in series, one thread then C/G channel sums, the apply pass at most 64 chunk sums: depth L = rows_per_chunk + C/G + chunks
    (chunks = min(64, ceil(HW / 64)), re-derived from the rounded-up rows as the launcher does).  With v's own rounding and the division:
        d_mean = ((L + 2) E|v| + |mean|) U32            (mean = E v + k, one more rounding)
        d_var  = ((L + 3) E v^2 + 2 |E v| (L + 2) E|v| + 2 (E v^2 + (E v)^2)) U32          (var = E v^2 - (E v)^2)
    - relative to E|x - k| and E (x - k)^2, not to E|x| and E x^2: what the unshifted form would owe.  rstd = rsqrtf(var + eps):
    r_rstd = d_var / (2 (var + eps)) + 3 U32.  y = (x - mean) rstd w + b:
        f32 = 1.01 [ ((d_mean + U32 |xc|) rstd + |xc| rstd (r_rstd + 2 U32)) |w| + U32 |y| ]
    swish: LIP f32 + act_eval(y).  fp32 output: f32; bf16 output: stored(y, f32).  Parameters are taken as given (bf16 or fp32, both exact in fp32).

Split-operand GEMM (split3_kernel + crab_gemm_bf16 over 3K): the reference is the exact x w^T; what the form itself leaves out (the lo.lo term and
    the 16-bit split) is |exact - T64| with T64 = hi.hi + lo.hi + hi.lo in fp64, hi = bf16(x), lo = bf16(x - hi); the 3K exact products are added in
    fp32 in some order: bound = |exact - T64| + (3K + 2) U32 A, A the sum of the absolute products of the three terms.

fp32 quantiser (vq_nearest_f32_kernel): d_mn = (|z_m|^2 + |e_n|^2) - 2 z_m . e_n in fp32.  The two square norms: a lane adds ceil(D / 64) squares,
    log2(min(D, 64)) butterfly levels that add non-zero terms, the square's rounding; the dot product D serial FMAs; two more roundings for the
    sum and the difference - at most D + 3 roundings on terms bounded by |z|^2, |e_n|^2 and 2 |z| |e_n| (D >= 4):
        delta_mn = (D + 3) U32 (|z_m|^2 + |e_n|^2 + 2 |z_m| |e_n|).
    Entry n can be returned for row m only if d64_mn - min_n d64_mn <= delta_mn + delta_m,argmin.  A row with one such entry must return it; a
    row with several (EITHER) may return any of THEM, nothing else.  Later copies of an identical codebook row are never a candidate: the kernel
    computes bit-identical distances for them and the first index wins.  The share of EITHER rows of a case is capped (VQ_EITHER_CAP) on cases of
    at least 1 / VQ_EITHER_CAP rows - below that one undecided row exceeds the cap, and such a case holds its rows to their allowed entries only.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -9
U32 = 2.0 ** -24
TOL_F32 = 3e-6       # fp32 outputs: accumulation order only (worst 1.15e-6 at K = 6144 on MI355X); tests/test_ops_gpu.py imports it from here
SLACK_CAP = 2.0 ** -12
LAW_SLACK_CAP = 2.0 ** -10      # attn_bound_weighted under the laws of tests/attn_laws.py
HOEFFDING = math.sqrt(2.0 * math.log(2.0 / 1e-12))
LIP = {"none": 1.0, "relu": 1.0, "gelu": 1.13, "silu": 1.1, "quick_gelu": 1.1, "swiglu_pair": 1.1}
F64 = torch.float64
TINY = 2.0 ** -126                    # the smallest normal fp32 number
VQ_EITHER_CAP = 1.0 / 50             # vq_margin: at most this share of a case's rows may be left to the fp32 arithmetic
                                     # (held on cases of at least 1 / VQ_EITHER_CAP = 50 rows: below that a single undecided row exceeds it; the directed
                                     # edge tests of at most 17 rows print the share and hold every row, undecided ones included, to its allowed entries)
SECOND_ORDER = 1.01                  # the products of two first-order terms, each below 2^-10 where it is used (module docstring: "1.01")


def d64(t):
    return None if t is None else t.to(F64)


def pow2_floor(x64):
    """2^floor(log2 |x|) of a normal fp64 x, from its exponent bits (0 at 0) - exact on every device.  (torch.frexp / torch.ldexp are not: on the
    GPU ldexp's power of two comes out of a pow and is an ulp off for some exponents, which moved bf16_round off the hardware's rounding on up to
    a quarter of the elements of a 0.1 N(0,1) operand; found by split_gemm_bound at K = 8.)"""
    return (x64.abs().contiguous().view(torch.int64) & 0x7FF0000000000000).view(F64)


def bf16_round(x64):
    """fp64 -> the nearest bf16 number (8 significant bits, ties to even), as fp64; in one rounding (a cast through fp32 would round twice).
    Normal range only - no operand or output here comes near bf16's exponent limits."""
    q = pow2_floor(x64) * 2.0 ** -7                                                  # the bf16 spacing in x's binade; x / q and the product are exact
    return torch.where(x64 != 0, torch.round(x64 / q.clamp_min(1e-300)) * q, x64)


def half_ulp(y64):
    """Half a bf16 ulp at |y|: U times the top of y's binade (module docstring); 0 at 0."""
    return U * 2.0 * pow2_floor(y64)                                                   # the top of |y|'s binade is twice its power-of-two floor


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


def act_eval(z, act):
    """What evaluating the activation in fp32 at z adds (module docstring, GEMM): (8 + 2 |z|) U32 |z|; 0 for none / relu (exact)."""
    return (8 + 2 * z.abs()) * U32 * z.abs() if act not in ("none", "relu") else torch.zeros_like(z)


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
    ev = act_eval(z, act)
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
    slack = SECOND_ORDER * U32 * (torch.einsum("bhst,bhtd->bhsd", pe, vv.abs()) + o.abs() * pe.sum(-1, keepdim=True) + c * (S + o.abs()) + 2 * o.abs())
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


# ------------------------------------------------------------------------------------------------------------------------- pixel path
def f32_arg(v):
    """A scalar argument as the kernel receives it (a C float), as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def softmax_rows_bound(x, scale, out_bf16):
    """(p64, bound) of softmax(scale x) over the last dimension of the fp32 block x - module docstring."""
    x = d64(x)
    N = x.shape[-1]
    s = x * f32_arg(scale)                                                              # exact: 24 x 24 bits
    m = s.max(-1, keepdim=True).values
    p = torch.softmax(s, -1)
    a = (s.float().to(F64) - s).abs() + (2 * (s - m).abs() + 2) * U32
    f32 = SECOND_ORDER * (a + (p * a).sum(-1, keepdim=True) + (math.ceil(N / 256) + 12) * U32) * p + TINY
    return p, (stored(p, f32) if out_bf16 else f32)


def act_bound(x, act):
    """(ref, bound) of bf16(act(x)) on bf16 x."""
    x = d64(x)
    return act64(x, act), stored(act64(x, act), act_eval(x, act))


def mask_gate_bound(prev, src):
    """(ref, bound) of bf16(src (sigmoid(mean_c prev) + 1)); prev [M, ncls], src [M, D]."""
    prev, src = d64(prev), d64(src)
    ncls = prev.shape[1]
    mean = prev.mean(1, keepdim=True)
    d_mean = U32 * ((math.ceil(ncls / 64) + 6) * prev.abs().mean(1, keepdim=True) + mean.abs())
    sig = torch.sigmoid(mean)
    g = sig + 1
    d_g = sig * ((1 - sig) * (d_mean + 2 * U32) + 3 * U32) + U32 * g
    ref = src * g
    return ref, stored(ref, src.abs() * d_g + U32 * ref.abs())


def group_mean_bound(x, T, scale):
    """(ref, bound) of bf16(scale sum_{k < T} x[g T + k]); x [G T, D]."""
    x, sc = d64(x), f32_arg(scale)
    xg = x.reshape(x.shape[0] // T, T, x.shape[1])
    ref = sc * xg.sum(1)
    return ref, stored(ref, (T + 1) * U32 * abs(sc) * xg.abs().sum(1))


def sqnorm_bound(e):
    """(ref, bound) of the fp32 row sums of squares of e [N, D] (bf16 or fp32)."""
    e = d64(e)
    ref = (e * e).sum(1)
    return ref, (math.ceil(e.shape[1] / 64) + 7) * U32 * ref


def dense_pe_bound(G, h, w):
    """(ref [h w, 2 F], bound) of the random-Fourier positional encoding of an h x w grid, G fp32 [2, F]."""
    G = d64(G)
    cy = (2 * (torch.arange(h, dtype=F64, device=G.device) + 0.5) / h - 1)[:, None, None]
    cx = (2 * (torch.arange(w, dtype=F64, device=G.device) + 0.5) / w - 1)[None, :, None]
    a = 2 * math.pi * (cx * G[0] + cy * G[1])                                          # [h, w, F]
    d_a = 4 * U32 * (a.abs() + 2 * math.pi * (G[0].abs() + G[1].abs()))
    ref = torch.cat([a.sin(), a.cos()], -1).reshape(h * w, -1)
    f32 = torch.cat([d_a, d_a], -1).reshape(h * w, -1) + 4 * U32
    return ref, stored(ref, f32)


def _bilinear_axis(n_in, n_out, device):
    f = (torch.arange(n_out, dtype=F64, device=device) + 0.5) * (n_in / n_out) - 0.5
    d_f = 3 * U32 * (f.abs() + 1)
    f = f.clamp_min(0.0)
    i0 = f.floor().long().clamp_max(n_in - 1)
    return i0, (i0 + 1).clamp_max(n_in - 1), f - i0, d_f


def _segment_slope(v, dim, i0):
    """The largest |v(k + 1) - v(k)| along dim over the segments i0 - 1, i0, i0 + 1 (absent segments count 0)."""
    n = v.shape[dim]
    dp = F.pad(v.diff(dim=dim).abs(), [0, 0] * (v.dim() - 1 - dim) + [1, 1])          # dp[k + 1] = segment k; n + 1 entries
    return torch.maximum(torch.maximum(dp.index_select(dim, i0), dp.index_select(dim, i0 + 1)), dp.index_select(dim, (i0 + 2).clamp_max(n)))


def bilinear_bound(x, strides, h, w, H, W, alpha, beta, out0):
    """(ref [C, H, W], bound) of beta out0 + alpha resize(v), v(c, y, x) = the element of x's storage at c strides[0] + y strides[1] + x strides[2]
    past x's first element (bf16 or fp32), out0 fp32 [C, H, W] (not read when beta = 0: it may hold anything)."""
    C = out0.shape[0]
    v = d64(x.as_strided((C, h, w), tuple(strides)))
    al, be = f32_arg(alpha), f32_arg(beta)
    y0, y1, ly, d_fy = _bilinear_axis(h, H, v.device)
    x0, x1, lx, d_fx = _bilinear_axis(w, W, v.device)
    ly, d_fy = ly[:, None], d_fy[:, None]

    def interp(t):
        top = (1 - lx) * t[:, y0][:, :, x0] + lx * t[:, y0][:, :, x1]
        bot = (1 - lx) * t[:, y1][:, :, x0] + lx * t[:, y1][:, :, x1]
        return (1 - ly) * top + ly * bot

    val, T = interp(v), interp(v.abs())
    sy = _segment_slope(v, 1, y0)                                                       # [C, H, w]
    sx = _segment_slope(v, 2, x0)                                                       # [C, h, W]
    Sy = torch.maximum(sy[:, :, x0], sy[:, :, x1])
    Sx = torch.maximum(sx[:, y0], sx[:, y1])
    d_v = SECOND_ORDER * (d_fy * Sy + d_fx * Sx + 6 * U32 * T)
    keep = be * d64(out0) if be != 0.0 else torch.zeros_like(val)
    return keep + al * val, abs(al) * d_v + 3 * U32 * (keep.abs() + abs(al) * T)


def groupnorm_chunks(HW):
    """(rows_per_chunk, chunks) as crab_groupnorm_p / crab_groupnorm_f32 launch them."""
    chunks = min(64, -(-HW // 64))
    rows = -(-HW // chunks)
    return rows, -(-HW // rows)


def groupnorm_bound(x, B, HW, G, w, b, eps, swish, out_fp32):
    """(ref [B HW, C], bound) of GroupNorm(G, C) (+ swish) over token-major x [B HW, C] (bf16 or fp32), parameters as given - module docstring."""
    x, e = d64(x), f32_arg(eps)
    C = x.shape[1]
    cpg = C // G
    rows, chunks = groupnorm_chunks(HW)
    L = rows + cpg + chunks
    wg, bg = d64(w).view(G, cpg), d64(b).view(G, cpg)
    xg = x.reshape(B, HW, G, cpg)
    k = xg[:, :1, :, :1]
    v = xg - k
    Ev, Ev2, mv = v.abs().mean((1, 3), keepdim=True), v.pow(2).mean((1, 3), keepdim=True), v.mean((1, 3), keepdim=True)
    mean = mv + k
    xc = xg - mean
    var = xc.pow(2).mean((1, 3), keepdim=True)
    d_mean = U32 * ((L + 2) * Ev + mean.abs())
    d_var = U32 * ((L + 3) * Ev2 + 2 * mv.abs() * (L + 2) * Ev + 2 * (Ev2 + mv * mv))
    rstd = torch.rsqrt(var + e)
    r_rstd = d_var / (2 * (var + e)) + 3 * U32
    y = xc * rstd * wg + bg
    f32 = SECOND_ORDER * (((d_mean + U32 * xc.abs()) * rstd + xc.abs() * rstd * (r_rstd + 2 * U32)) * wg.abs() + U32 * y.abs())
    if swish:
        f32 = LIP["silu"] * f32 + act_eval(y, "silu")
        y = act64(y, "silu")
    y, f32 = y.reshape(B * HW, C), f32.reshape(B * HW, C)
    return y, (f32 if out_fp32 else stored(y, f32))


def split_gemm_bound(x, w):
    """(exact x w^T in fp64, bound) of the split-operand product gemm(split3(x, 0), split3(w, 1)) with fp32 output."""
    x, w = d64(x), d64(w)
    xh, wh = bf16_round(x), bf16_round(w)
    xl, wl = bf16_round(x - xh), bf16_round(w - wh)
    exact = x @ w.t()
    t64 = xh @ wh.t() + xl @ wh.t() + xh @ wl.t()
    A = xh.abs() @ wh.abs().t() + xl.abs() @ wh.abs().t() + xh.abs() @ wl.abs().t()
    return exact, (exact - t64).abs() + (3 * x.shape[1] + 2) * U32 * A


def vq_margin(z, e):
    """(want [M], either [M] bool, allowed [M, N] bool) for the fp32 quantiser of z [M, D] against the codebook e [N, D], from fp64 distances and the
    fp32 margin delta (module docstring): allowed = the entries a row may return; either = rows with more than one; want = the fp64 arg-min
    (first copy of duplicated codebook rows), the only allowed entry of every other row."""
    z, e = d64(z), d64(e)
    N, D = e.shape
    z2, e2 = (z * z).sum(1, keepdim=True), (e * e).sum(1)[None]
    d = z2 + e2 - 2 * z @ e.t()
    delta = (D + 3) * U32 * (z2 + e2 + 2 * z2.sqrt() * e2.sqrt())
    _, inv = torch.unique(e, dim=0, return_inverse=True)
    n = torch.arange(N, device=e.device)
    first = torch.full((int(inv.max()) + 1,), N, device=e.device, dtype=n.dtype).scatter_reduce(0, inv, n, "amin")
    dup = first[inv] != n                                                               # a later copy of an identical row
    d = d.masked_fill(dup[None], math.inf)
    best, want = d.min(1, keepdim=True)
    allowed = (d - best) <= delta + delta.gather(1, want)
    return want[:, 0], allowed.sum(1) > 1, allowed


def vq_verdict(idx, z, e, offset=0):
    """(rows that hold an entry they may not, share of EITHER rows) of the quantiser's ids idx [M] (offset added by the kernel)."""
    want, either, allowed = vq_margin(z, e)
    i = idx.to(want.device).long() - offset
    inside = (i >= 0) & (i < e.shape[0])
    ok = inside & allowed.gather(1, i.clamp(0, e.shape[0] - 1)[:, None])[:, 0]
    return int((~ok).sum()), float(either.double().mean())
