"""Bounds of the scoring tests, COMPUTED per session from the oracle like tests/bounds.py - in LOG-PROB space: the oracle's decoder runs on the
test's own inputs in fp32, as the bf16-OPERAND FLOOR (emulate=O.OPERANDS: only what a matrix instruction consumes is rounded) and as the
bf16-STORAGE emulation (the parameters as the HIP modules hold them, every storage point rounded), each followed by log-softmax in fp64 at
the shifted labels; a per-token log-prob of the HIP path is held to

        |hip - fp32|  <=  FACTOR x max(floor, storage emulation)        (nats; FACTOR = 1.5 as in tests/bounds.py)

A per-sequence sum of n tokens gets n x that bound, the batch mean loss the bound itself."""
import json
import os

import numpy as np
import torch

from oracle import crab_oracle as O
from tests.bounds import FACTOR
from tests.util import GOLDEN, stored_params

BF = torch.bfloat16


def load_scoring_fixture(name: str = "loss_tiny_llama"):
    z = np.load(os.path.join(GOLDEN, "scoring", name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}


def token_logprobs(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """fp64 log-softmax of logits [B, S, V] at the shifted labels (labels[b, t + 1] != -100), sequence by sequence, position ascending."""
    lp = torch.log_softmax(logits.double(), -1)[:, :-1]
    nxt = labels[:, 1:].long()
    sel = nxt != -100
    return lp[sel].gather(-1, nxt[sel][:, None])[:, 0]


def oracle_logprobs(emb, W, dcfg, labels, positions=None, attention_mask=None, emulate=None) -> torch.Tensor:
    """The oracle's per-token log-probs: an fp32 run takes the inputs as they are, every bf16 execution their bf16 rounding (what the HIP
    entry points receive; scripts/parity_floor.py q())."""
    e = emb.float() if emulate is None else emb.to(BF).float()
    logits, _, _ = O.decoder_forward(e, W, dcfg, positions=positions, attention_mask=attention_mask, emulate=emulate)
    return token_logprobs(logits, labels)


def logprob_bound(emb, W, dcfg, labels, positions=None, attention_mask=None, factor: float = FACTOR):
    """(bound in nats, the fp32 oracle's per-token log-probs, {"floor", "storage_emulation"}) for a decoder stack W (keys without the PEFT prefix)."""
    ref = oracle_logprobs(emb, W, dcfg, labels, positions, attention_mask)
    flo = float((oracle_logprobs(emb, W, dcfg, labels, positions, attention_mask, O.OPERANDS) - ref).abs().max())
    sto = float((oracle_logprobs(emb, stored_params(W), dcfg, labels, positions, attention_mask, BF) - ref).abs().max())
    return factor * max(flo, sto), ref, {"floor": flo, "storage_emulation": sto}


def crab_config(meta) -> "O.CrabConfig":
    """The oracle's configuration of a full tiny model from a fixture's meta (decoder, CLIP, BEATs, Q-Former)."""
    qf = O.QFormerConfig(hidden_size=meta["qf"]["hidden"], num_attention_heads=meta["qf"]["heads"], intermediate_size=meta["qf"]["inter"])
    beats = O.BeatsConfig(**{k: v for k, v in meta["beats"].items() if k in O.BeatsConfig.__dataclass_fields__})
    return O.CrabConfig(decoder=O.DecoderConfig(**meta["dec"]), clip=O.ClipConfig(**meta["clip"], select_layers=tuple(meta["select"])), beats=beats,
                        qformer=qf, base_vocab=meta["base_vocab"], pad_token_id=meta["pad_token_id"])


def multimodal_logprob_bound(meta, ids, mods, labels, W, factor: float = FACTOR):
    """(bound in nats, floor, storage emulation) of the per-token log-prob of the WHOLE multimodal forward (encoders -> splice -> left pad ->
    decoder) on the prompts `ids` with the modal inputs `mods`, at the spliced `labels`; W with the PEFT prefix."""
    cfg = crab_config(meta)
    Wo = O.strip_peft_prefix(W)

    def q(v, e):          # an fp32 run takes the raw inputs, a bf16 execution their bf16 rounding (scripts/parity_floor.py q())
        return v if e is None else {k: t.to(BF).float() for k, t in v.items()}

    def run(Wx, e):
        inp = O.prepare_multimodal_inputs(list(ids), [q(m, e) for m in mods], Wx, cfg, e)
        logits, _, _ = O.decoder_forward(inp["inputs_embeds"], Wx, cfg.decoder, positions=inp["position_ids"], attention_mask=inp["attention_mask"], emulate=e)
        return token_logprobs(logits, labels)
    ref = run(Wo, None)
    flo = float((run(Wo, O.OPERANDS) - ref).abs().max())
    sto = float((run(stored_params(Wo), BF) - ref).abs().max())
    return factor * max(flo, sto), flo, sto
