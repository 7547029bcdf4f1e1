"""Pure-torch statement of the FP8 KV-cache storage format (include/crab_hip.h "FP8 KV cache"), on the CPU: the reference the
HIP quantiser and the fp8 decode attention are pinned to bit for bit (tests/test_kv_fp8_gpu.py) and the building block of the fp8-KV emulation
of the oracle.  Not a test module.

    amax  = max |x| over the row's d elements (x = the bf16 values the bf16 cache would hold, taken to fp32)
    scale = amax / 448.0f (fp32 division);  1.0f when amax == 0;  FLT_MIN when the quotient is below FLT_MIN
    inv   = 1.0f / scale;   code = e4m3fn_rne(x * inv);   value read back = float(code) * scale

torch's float32 -> float8_e4m3fn conversion on the CPU rounds to nearest even (NaN above 464: never reached, |x * inv| <= 448 up to the rounding
of the product).  The FLT_MIN floor keeps `inv` finite for rows whose amax is below 448 * 2^-126 (bf16 subnormals): without it 1 / scale
overflows and every code of such a row is NaN."""
import torch

E4M3_MAX = 448.0
FLT_MIN = float(torch.finfo(torch.float32).tiny)


def quant(x: torch.Tensor):
    """x [..., d] (bf16 or fp32 holding bf16 values) -> (codes uint8 [..., d], scale fp32 [...])."""
    xf = x.detach().cpu().float()
    amax = xf.abs().amax(-1)
    scale = amax / torch.tensor(E4M3_MAX, dtype=torch.float32)
    scale = torch.clamp(scale, min=FLT_MIN)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    inv = torch.tensor(1.0, dtype=torch.float32) / scale
    codes = (xf * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, scale


def dequant(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 [..., d]: float(code) * scale."""
    return codes.cpu().view(torch.float8_e4m3fn).float() * scale.cpu().float()[..., None]


def roundtrip(x: torch.Tensor) -> torch.Tensor:
    """What a decode step reads back for the bf16 rows x."""
    return dequant(*quant(x))
