#!/usr/bin/env python3
"""Generate tests/golden/scoring/loss_tiny_llama.npz by running the REFERENCE's forward(batch_input_ids, batch_labels, batch_X_modals,
batch_task_names) (models/unified_llama.py:129-160 -> models/modeling_llama.py:1261-1274) on the tiny hyper-LoRA Llama of
tests/golden/make_golden.py::golden_full - same configuration, same seeded weights, the two prompts of full_tiny_llama.npz.

Build container only (imports the reference through ref_shims; nothing is copied).  The fixture holds what a scorer needs and nothing of
size rows x vocabulary: the spliced inputs_embeds, attention mask, positions and labels of the left-padded bs-2 batch, the reference's loss
and its per-token log-probs (log_softmax of ITS fp32 logits in fp64, at the shifted labels).

    python tests/golden/scoring/make_golden_scoring.py
"""
from __future__ import annotations

import sys

sys.dont_write_bytecode = True

import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, GOLDEN)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402
import ref_shims  # noqa: E402
from crab_amd import synth  # noqa: E402

TAIL = (6, 5)          # labelled answer-tail tokens of the two samples; -100 elsewhere


def build_model(me):
    """The model of make_golden.golden_full: tiny UnifiedForCausalLM + hyper-LoRA, encoders attached by hand, MM tokenizer, synth weights."""
    model, _cfg = MG.build_full_model(me, MG.TINY_DEC)
    inner = model.get_model()
    inner.pad_token_id = 2
    inner.visual_encoder = MG.build_visual_encoder(me)
    inner.vl_projector = me.VLProjector(hidden_size=128, image_token_nums=256, num_query_token=32, num_hidden_layers=2, d_model=MG.D_MODEL, depth=2)

    class AE(me.AudioEncoder):
        def __init__(self, beats):
            torch.nn.Module.__init__(self)
            self.audio_encoder = beats

    beats = MG.build_beats(MG.TINY_BEATS)
    inner.audio_encoder = AE(beats)
    inner.al_projector = me.ALProjector(hidden_size=128, num_query_token=32, num_hidden_layers=2, d_model=MG.D_MODEL, depth=2)
    tok = MG._Tok(MG.TINY_DEC["vocab_size"] - 17)
    base_vocab = len(tok)
    model.base_model.model.initialize_MM_tokenizer(tok, mask_token_nums=6, use_vqgan=False)
    model.eval()
    alias = [("base_model.model.model.audio_encoder.audio_encoder." + c, ["base_model.model.model.audio_encoder.audio_encoder." + o for o in os_])
             for c, os_ in MG.beats_alias(beats)]
    table = MG.load_synth(model, "", alias_groups=alias)
    return model, base_vocab, table


def main():
    ref_shims.install()
    me = ref_shims.patch_bert_config(lambda: ref_shims.tiny_bert_config(**MG.TINY_QF))
    z = np.load(os.path.join(GOLDEN, "full_tiny_llama.npz"))
    fmeta = json.loads(bytes(z["meta"]).decode())
    model, base_vocab, table = build_model(me)
    assert base_vocab == fmeta["base_vocab"] and [list(t) for t in table] == [list(t) for t in fmeta["table"]], "not the model of full_tiny_llama.npz"
    um = model.base_model.model
    tab = dict(um.SPECIAL_TOKEN_2_IDS)
    p = fmeta["prompts"]
    ids = [synth.synth_prompt_ids(p["n0"], base_vocab, tab, seed=MG.SEED, clip=p["clip0"]),
           synth.synth_prompt_ids(p["n1"], base_vocab, tab, seed=MG.SEED, clip=p["clip1"])]
    assert torch.equal(ids[0], torch.from_numpy(z["ids0"])) and torch.equal(ids[1], torch.from_numpy(z["ids1"]))
    mods = [{'<video>': synth.synth_video(p["t_v"], seed=MG.SEED, clip=c), '<audio>': synth.synth_audio(p["t_a"], p["l_a"], seed=MG.SEED, clip=c)}
            for c in (p["clip0"], p["clip1"])]
    labs = []
    for i, n in zip(ids, TAIL):
        lab = torch.full_like(i, -100)
        lab[-n:] = i[-n:]
        assert int(lab[-n:].min()) >= 3 and int(lab[-n:].max()) < base_vocab          # plain text tokens
        labs.append(lab)
    inp = um.prepare_multimodal_inputs(ids, labs, mods, ['avqa', 'avqa'])
    out = um.forward(batch_input_ids=ids, batch_labels=labs, batch_X_modals=mods, batch_task_names=['avqa', 'avqa'])
    labels = inp["labels"]
    assert int((labels != -100).sum()) == sum(TAIL)
    lp = torch.log_softmax(out.logits.double(), -1)
    sel = labels[:, 1:] != -100
    tok_lp = lp[:, :-1][sel].gather(-1, labels[:, 1:][sel][:, None])[:, 0]      # row-major: sample by sample, position ascending
    loss = float(out.loss)
    assert abs(loss + float(tok_lp.mean())) < 1e-5, (loss, float(tok_lp.mean()))
    counts = sel.sum(1).tolist()
    sums = [float(v.sum()) for v in tok_lp.split(counts)]
    correct = (out.logits[:, :-1][sel].argmax(-1) == labels[:, 1:][sel]).split(counts)
    meta = dict(fmeta, tail=list(TAIL), loss=loss, counts=counts, sum_logprob=sums, num_correct=[int(c.sum()) for c in correct])
    path = os.path.join(HERE, "loss_tiny_llama.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), ids0=ids[0].numpy(), ids1=ids[1].numpy(),
                        labels0=labs[0].numpy(), labels1=labs[1].numpy(), embeds=inp["inputs_embeds"].float().numpy(),
                        mask=inp["attention_mask"].numpy(), pos=inp["position_ids"].numpy(), labels=labels.numpy(),
                        token_logprobs=tok_lp.numpy(), loss=np.float64(loss))
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; loss {loss:.6f}, per-sequence sums {sums}, counts {counts}")


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    main()
