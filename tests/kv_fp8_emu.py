"""The fp8-KV emulation of the oracle (not a test module): oracle.crab_oracle.decoder_forward teacher-forced along given ids, with a KVCache whose
k / v lists pass every row through tests/kv_fp8_ref exactly where the FP8 KV cache of crab_amd does (include/crab_hip.h "FP8 KV cache"):
  * a one-row step's appended row is rounded to bf16, quantised and read back BEFORE that step's attention uses it (KVCache.k / .v are plain lists
    and decoder_layer assigns cache.k[i] = cat(old, new), then reads cache.k[i]: a list subclass sees the assignment);
  * the prefill attends its own unquantised rows; they are quantised after the prefill call returns.
oracle/ itself is not edited."""
import torch

from oracle import crab_oracle as O
from tests import kv_fp8_ref as R


class Fp8Rows(list):
    def __setitem__(self, i, v):
        old = self[i]
        if old is not None and v is not None and v.shape[2] == old.shape[2] + 1:          # a one-row decode step appended its row
            v = torch.cat([v[:, :, :-1], R.roundtrip(v[:, :, -1:].to(torch.bfloat16)).to(v.dtype)], 2)
        super().__setitem__(i, v)

    def quantise_all(self):
        for i in range(len(self)):
            if self[i] is not None:
                super().__setitem__(i, R.roundtrip(self[i].to(torch.bfloat16)).to(self[i].dtype))


def teacher_forced_logits(emb, W, cfg, ref_ids, emulate=None, fp8=False):
    """Per-step last-row logits [B, n, V] of the decoder on inputs_embeds `emb`, teacher-forced along ref_ids [B, n] (tests/bounds.decoder_bound's
    loop); emulate: None (fp32) / O.OPERANDS / torch.bfloat16 (storage emulation); fp8: the KV cache holds fp8 rows as described above."""
    cache = O.KVCache(k=Fp8Rows(), v=Fp8Rows()) if fp8 else O.KVCache()
    logits, _, cache = O.decoder_forward(emb.float(), W, cfg, cache, last_only=True, emulate=emulate)
    if fp8:
        cache.k.quantise_all(); cache.v.quantise_all()
    out = [logits[:, -1]]
    for s in range(1, ref_ids.shape[1]):
        tok = W["model.embed_tokens.weight"].float()[ref_ids[:, s - 1]][:, None]
        logits, _, cache = O.decoder_forward(O._r(tok, emulate), W, cfg, cache, last_only=True, emulate=emulate)
        out.append(logits[:, -1])
    return torch.stack(out, 1)


def fp8_yardstick(emb, W, W_stored, cfg, ref_ids):
    """(fp32 logits, emulation logits, distance): the emulation = the bf16-storage emulation of this stack (tests/bounds.py) WITH the fp8 KV
    cache; distance = max |emulation - fp32| over all steps, relative to max |fp32|.  HIP's fp8 mode is held to FACTOR_VS_EMULATION x distance
    from the emulation (the project's rule: the yardstick comes from the oracle, never from the code under test)."""
    ref = teacher_forced_logits(emb, W, cfg, ref_ids)
    emu = teacher_forced_logits(emb, W_stored, cfg, ref_ids, emulate=torch.bfloat16, fp8=True)
    return ref, emu, (emu - ref).abs().max().item() / ref.abs().max().item()
