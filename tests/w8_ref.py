"""Pure-torch statement of the opt-in FP8 decoder weights (include/crab_hip.h "FP8 decoder weights") on the CPU: the storage format
(the row format of tests/kv_fp8_ref.py applied to the rows of W), a float64 GEMM on the dequantised operands with the summation bound the GPU
tests hold the kernel to, and the mixed emulation of the oracle (prefill with W, decode steps with dequant(quant(W))).  Not a test module."""
import re

import torch

from tests import kv_fp8_ref as R

BF = torch.bfloat16
FP8 = "fp8_e4m3"
PROJ = re.compile(r"^model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")     # the seven projections of a decoder layer


def quant_rows(W: torch.Tensor):
    """W [N, K] (bf16, or fp32 holding bf16 values) -> (codes uint8 [N, K], scale fp32 [N]): one scale per output row."""
    return R.quant(W)


def dequant_rows(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return R.dequant(codes, scale)


def roundtrip(W: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K]: what a decode step computes with in FP8 mode for the bf16 weights W."""
    return R.roundtrip(W.to(BF))


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def gemm_ref(a, codes, scale, a2=None, b2=None, bias=None, act="none", residual=None, res_scale=1.0, out_bf16=True):
    """float64 on the dequantised operands:  act( scale[n] * sum_k q[n,k] a[m,k] + sum_j b2[n,j] a2[m,j] + bias[n] ) (+ res_scale * residual).
    Returns (y [M, N] float64 - [M, N/2] for act = "swiglu_pair" -, bound [M, N] float64), `bound` being the per-element summation bound of an
    fp32 accumulation of the PRE-activation sum in any order:

        |err| <= 2 (K + K2) 2^-24 (scale[n] sum_k |q a| + sum_j |b2 a2|)

    Products of bf16 values are exact in fp32 (8 x 8 significant bits), so only the fp32 additions err: each of the K + K2 - 1 additions (and the
    one multiplication by the scale) rounds a partial sum no larger than the sum of absolute products by at most 2^-24 relative; the factor 2
    covers the second-order terms and the bias / residual additions of the epilogue.  Callers add one bf16 rounding of the result (2^-8
    relative) where the output is bf16, and propagate the bound through an activation themselves."""
    A = a.cpu().double()
    Q = codes.cpu().view(torch.float8_e4m3fn).double()
    s = scale.cpu().double()
    K, K2 = A.shape[1], (a2.shape[1] if a2 is not None else 0)
    y = (A @ Q.t()) * s[None]
    mag = (A.abs() @ Q.abs().t()) * s[None]
    if a2 is not None:
        y = y + a2.cpu().double() @ b2.cpu().double().t()
        mag = mag + a2.cpu().double().abs() @ b2.cpu().double().abs().t()
    if bias is not None:
        y = y + bias.cpu().double()[None]
        mag = mag + bias.cpu().double().abs()[None]
    bound = 2.0 * (K + K2) * 2.0 ** -24 * mag
    if act == "swiglu_pair":
        y = _silu(y[:, 0::2]) * y[:, 1::2]
    elif act == "silu":
        y = _silu(y)
    elif act not in ("none", None):
        raise ValueError(act)
    if residual is not None:
        y = y + res_scale * residual.cpu().double()
    return y, bound


def swiglu_bound(pre, bound):
    """Bound of silu(g) * u for pre-activation sums pre = [g0, u0, g1, u1, ...] known to `bound`: |d silu / dx| <= 1.1, |silu(g)| <= |g|, plus
    the fp32 evaluation of the epilogue itself (exp, division, product: a few 2^-22 relative)."""
    g, u = pre[:, 0::2].abs(), pre[:, 1::2].abs()
    bg, bu = bound[:, 0::2], bound[:, 1::2]
    return 1.1 * bg * (u + bu) + g * bu + 2.0 ** -20 * g * u


def dequantised_weights(W: dict) -> dict:
    """The checkpoint a decode step of FP8 mode computes with: every projection weight of the decoder layers replaced by
    dequant(quant(bf16(W))) (row scales: packing the rows into groups does not change them); everything else - adapters, biases, norms,
    embeddings, lm_head - as it is."""
    return {k: (roundtrip(v) if PROJ.search(k) else v) for k, v in W.items()}


def mixed_steps(emb, W_prefill, W_decode, cfg, ref_ids, emulate=None):
    """The oracle teacher-forced along ref_ids with TWO checkpoints: the prefill pass on W_prefill, every decode step on W_decode (FP8 mode
    leaves prefill on the bf16 weights).  Returns the last-row logits of every step [B, n, V] (tests/bounds.decoder_bound's run())."""
    from oracle import crab_oracle as O
    cache = O.KVCache()
    logits, _, cache = O.decoder_forward(emb.float(), W_prefill, cfg, cache, last_only=True, emulate=emulate)
    out = [logits[:, -1]]
    for s_ in range(1, ref_ids.shape[1]):
        tok = W_decode["model.embed_tokens.weight"].float()[ref_ids[:, s_ - 1]][:, None]
        logits, _, cache = O.decoder_forward(O._r(tok, emulate), W_decode, cfg, cache, last_only=True, emulate=emulate)
        out.append(logits[:, -1])
    return torch.stack(out, 1)


def mixed_bound(emb, W, cfg, ref_ids, W_stored=None, factor=None):
    """tests/bounds.decoder_bound's construction for the mixed run: (fp32 reference, factor x max(operand floor, storage emulation)), all three
    with the prefill on W and the decode steps on the dequantised weights; relative to max |reference logits|."""
    from oracle import crab_oracle as O
    from tests import bounds as PB
    from tests.util import stored_params
    factor = PB.FACTOR if factor is None else factor
    Ws = W_stored if W_stored is not None else stored_params(W)
    ref = mixed_steps(emb, W, dequantised_weights(W), cfg, ref_ids, None)
    sc = ref.abs().max().item()
    flo = (mixed_steps(emb, W, dequantised_weights(W), cfg, ref_ids, O.OPERANDS) - ref).abs().max().item() / sc
    sto = (mixed_steps(emb, Ws, dequantised_weights(Ws), cfg, ref_ids, BF) - ref).abs().max().item() / sc
    return ref, factor * max(flo, sto)
