"""UnifiedForCausalLM.generate(prompt_lookup_num_tokens = k) on the tiny Crab fixtures: a synthetic clip (crab_amd/synth.py) through
prepare_multimodal_inputs, the prompt's token ids as the draft history (-1 at the rows of the spliced modality blocks), the ids and the per-step
logits against generate() without the argument under the margin rule of tests/test_shared_prefix_gpu.py (logits within the computed end-to-end
bound, an id may differ only at a step whose top-2 margin is below 10 x that bound)."""
import pytest
import torch

from tests import bounds as PB
from tests import lookup_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fixture", ["full_tiny_llama", "full_tiny_qwen"])
def test_generate_with_prompt_lookup_on_a_synthetic_clip(fixture):
    from crab_amd import synth
    from tests.util import build_tiny_crab, load_fixture, weights_from_table
    meta, A = load_fixture(fixture)
    model = build_tiny_crab(meta, device="cuda:0")
    assert not model.load_state_dict(weights_from_table(meta), strict=False).missing_keys
    um = model.base_model.model
    p = meta["prompts"]
    mods = [{'<video>': synth.synth_video(p["t_v"], seed=meta["seed"], clip=p["clip0"]),
             '<audio>': synth.synth_audio(p["t_a"], p["l_a"], seed=meta["seed"], clip=p["clip0"])}]
    ids0 = A["ids0"]
    n = 8
    kw = dict(batch_input_ids=[ids0], batch_labels=[torch.full_like(ids0, -100)], batch_X_modals=mods, batch_task_names=['avqa'], use_cache=True,
              max_new_tokens=n, pad_token_id=2, eos_token_id=None, output_logits=True, return_dict_in_generate=True)
    plain = model.generate(**kw)
    rid, rlog = plain.sequences.cpu()[0], torch.stack(plain.logits, 1).float().cpu()[0]
    got = model.generate(prompt_lookup_num_tokens=3, **kw)
    ids, logits = got.sequences.cpu()[0], torch.stack(got.logits, 1).float().cpu()[0]
    assert ids.shape == rid.shape == (n,) and logits.shape == rlog.shape

    # the history the engine was given: one entry per prompt row, the text ids in order, -1 where a modality block was spliced in
    hist = um.last_lookup["prompt_ids"].tolist()
    special = set(um.SPECIAL_TOKEN_2_IDS[k] for k in um.KEYS)
    text = [t for t in ids0.tolist() if t not in special]
    assert [t for t in hist if t >= 0] == text and hist.count(-1) > 0 and len(hist) > len(ids0)
    st = um.last_lookup["stats"]
    assert st["tokens_emitted"] == n - 1 and 1 <= st["verify_steps"] <= n - 1 and st["drafts_accepted"] <= st["drafts_proposed"]

    tol = PB.bound(f"{fixture}: end to end") * rlog.abs().max().item()
    top2 = rlog.topk(2, -1).values
    margin = top2[:, 0] - top2[:, 1]
    same = True
    for s in range(n):
        err = (logits[s] - rlog[s]).abs().max().item()
        print(f"\nstep {s}: |dlogit| {err:.4e}, bound {tol:.4e}; id {int(ids[s])} vs {int(rid[s])}, margin {margin[s].item():.4f}")
        assert err <= tol, (s, err, tol)
        if ids[s] != rid[s]:
            assert margin[s].item() < 10 * tol, (s, margin[s].item(), tol)
            same = False
            break
    if same:
        sim = R.simulate(rid.tolist(), hist, 3, 2, None, n)[1]
        assert [st["verify_steps"], st["drafts_proposed"], st["drafts_accepted"], st["tokens_emitted"]] == sim
    # without the dict: the ids alone
    again = model.generate(prompt_lookup_num_tokens=3, **{**kw, "output_logits": False, "return_dict_in_generate": False})
    assert torch.equal(again.cpu()[0], ids)
