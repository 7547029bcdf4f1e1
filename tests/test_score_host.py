"""Teacher-forced scoring, the parts that need no GPU: the host-side row selection against a brute-force restatement, the oracle pinned to the
reference-recorded loss fixture (tests/golden/scoring/loss_tiny_llama.npz: the reference's forward(batch_input_ids, batch_labels, ...)), and
what the public API refuses."""
import numpy as np
import pytest
import torch

from crab_amd import _lib
from crab_amd.decoder import score_rows
from oracle import crab_oracle as O
from tests.score_bounds import load_scoring_fixture, token_logprobs
from tests.util import weights_from_table


def _brute(labels: torch.Tensor):
    """The shift of modeling_llama.py:1265-1266 written out: row t of sequence b scores against labels[b, t + 1] unless that is -100."""
    B, S = labels.shape
    rows, tgt, off = [], [], [0]
    for b in range(B):
        for t in range(S - 1):
            if int(labels[b, t + 1]) != -100:
                rows.append(b * S + t)
                tgt.append(int(labels[b, t + 1]))
        off.append(len(rows))
    return rows, tgt, off


def _check(labels, V):
    r, t, o = score_rows(labels, V)
    rows, tgt, off = _brute(labels)
    assert r.dtype == t.dtype == o.dtype == torch.int32
    assert r.tolist() == rows and t.tolist() == tgt and o.tolist() == off


def test_row_selection_equals_the_brute_force_restatement():
    g = torch.Generator().manual_seed(11)
    V = 97
    for trial in range(40):
        B, S = int(torch.randint(1, 6, (1,), generator=g)), int(torch.randint(1, 40, (1,), generator=g))
        labels = torch.randint(0, V, (B, S), generator=g)
        labels[torch.rand(B, S, generator=g) < 0.6] = -100
        for b in range(B):                                   # left pads: a -100 prefix of random length (what prepare_multimodal_inputs builds)
            labels[b, :int(torch.randint(0, S + 1, (1,), generator=g))] = -100
        if trial % 3 == 0:
            labels[int(torch.randint(0, B, (1,), generator=g))] = -100          # a sequence without any target
        _check(labels, V)
    only0 = torch.full((2, 9), -100)
    only0[0, 0] = 5                                          # position 0 is nobody's next token: it never scores
    r, t, o = score_rows(only0, V)
    assert r.numel() == 0 and t.numel() == 0 and o.tolist() == [0, 0, 0]
    _check(only0, V)
    last = torch.full((1, 4), -100)
    last[0, 3] = V - 1                                       # the largest token id, on the last position: scored by row S - 2
    assert [x.tolist() for x in score_rows(last, V)] == [[2], [V - 1], [0, 1]]
    _check(torch.full((3, 1), 7), V)                         # S = 1: no shifted target at all
    r, t, o = score_rows(np.array([[-100, 3, -100, 4]]), V)  # plain arrays too
    assert r.tolist() == [0, 2] and t.tolist() == [3, 4]


def test_out_of_range_labels_raise():
    ok = torch.tensor([[-100, 1, 2]])
    score_rows(ok, 3)
    for bad in (3, 1000, -101, -1, -99):
        lab = ok.clone()
        lab[0, 2] = bad
        with pytest.raises(ValueError, match="labels"):
            score_rows(lab, 3)
    with pytest.raises(ValueError):
        score_rows(torch.tensor([1, 2, 3]), 5)               # not [B, S]
    with pytest.raises(ValueError):
        score_rows(torch.zeros(2, 3), 5)                     # not integers
    with pytest.raises(ValueError):
        score_rows(ok, 3, shape=(1, 4))                      # not the shape of the embeddings


def test_oracle_reproduces_the_reference_loss_and_token_logprobs():
    """The fixture is the reference's own forward(batch_input_ids, batch_labels, batch_X_modals, batch_task_names) on the golden_full tiny
    model: two samples of different length (left padding), answer-tail labels, -100 elsewhere.  The oracle's fp32 decoder on the recorded
    spliced inputs + log-softmax in fp64 must give the recorded per-token log-probs and loss (5e-4: the oracle-vs-reference tolerance)."""
    meta, A = load_scoring_fixture()
    labels = A["labels"]
    assert tuple(A["embeds"].shape[:2]) == tuple(labels.shape) and labels.shape[0] == 2
    assert int((A["mask"] == 0).sum()) > 0                                         # the shorter sample is left-padded
    assert meta["counts"] == meta["tail"] and int((labels != -100).sum()) == sum(meta["tail"])
    assert bool((labels[A["mask"] == 0] == -100).all())
    W = O.strip_peft_prefix(weights_from_table(meta))
    dcfg = O.DecoderConfig(**meta["dec"])
    logits, _, _ = O.decoder_forward(A["embeds"], W, dcfg, positions=A["pos"], attention_mask=A["mask"])
    lp = token_logprobs(logits, labels)
    assert lp.shape == A["token_logprobs"].shape
    d = float((lp - A["token_logprobs"]).abs().max())
    assert d <= 5e-4, f"per-token log-probs differ from the reference's by {d}"
    assert abs(float(-lp.mean()) - float(A["loss"])) <= 5e-4
    assert abs(float(A["loss"]) - meta["loss"]) < 1e-12
    sums = [float(v.sum()) for v in lp.split(meta["counts"])]
    assert max(abs(a - b) for a, b in zip(sums, meta["sum_logprob"])) <= 5e-4 * max(meta["counts"])
    # the rows score_rows selects are the rows these log-probs belong to
    r, t, o = score_rows(labels, dcfg.vocab_size)
    assert o.tolist() == [0, meta["counts"][0], sum(meta["counts"])] and t.tolist() == labels[:, 1:][labels[:, 1:] != -100].tolist()


def _tiny():
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    cfg = UnifiedConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, vocab_size=96, pad_token_id=2)
    return get_peft_model(UnifiedForCausalLM(cfg, device="cpu"), LoraConfig())


def test_refusals():
    model = _tiny()
    um = model.base_model.model
    emb = torch.zeros(2, 5, 64, dtype=torch.bfloat16)
    lab = torch.full((2, 5), -100)
    um.is_avs_task = True                                    # the AVS forward adds the training-only mask loss: still refused, and so is its score()
    with pytest.raises(NotImplementedError, match="AVS"):
        um(inputs_embeds=emb, labels=lab)
    with pytest.raises(NotImplementedError, match="AVS"):
        um(inputs_embeds=emb)
    with pytest.raises(NotImplementedError, match="AVS"):
        model.score(inputs_embeds=emb, labels=lab)
    um.is_avs_task = False
    for kw in (dict(inputs_embeds=emb, labels=lab[:, :4]), dict(inputs_embeds=emb, labels=lab[:1]), dict(inputs_embeds=emb[0], labels=lab[0]),
               dict(inputs_embeds=emb, labels=lab, attention_mask=torch.ones(2, 4)), dict(inputs_embeds=emb, labels=lab, position_ids=torch.zeros(2, 4)),
               dict(inputs_embeds=emb), dict(labels=lab), dict(batch_input_ids=[torch.zeros(4, dtype=torch.long)]),
               dict(batch_input_ids=[torch.zeros(4, dtype=torch.long)], batch_labels=[torch.zeros(3, dtype=torch.long)])):
        with pytest.raises(ValueError):
            model.score(**kw)
    bad = lab.clone()
    bad[0, 2] = 96                                           # == vocab_size
    with pytest.raises(ValueError, match="labels"):
        model.score(inputs_embeds=emb, labels=bad)
    with pytest.raises(ValueError, match="max_rows"):
        model.score(inputs_embeds=emb, labels=lab, max_rows=0)
    with pytest.raises(ValueError):
        um._engine.score(torch.zeros(2, 5, 32, dtype=torch.bfloat16), lab)      # not the model's width


def test_entry_points_validate_before_any_hip_call():
    lib = _lib.load()
    assert lib.crab_lm_head_xent_workspace(1, 1) == 16 + 16
    assert lib.crab_lm_head_xent_workspace(300, 32017) == 300 * 126 * 16 + 1200          # one 16-byte record per row and 256-column tile + the label logits
    assert lib.crab_lm_head_xent_workspace(0, 5) == 0
    assert lib.crab_lm_head_xent(None, None, None, 0, None, 1, None, 0, 1, 8, None, None, None, None, None, 0) < 0
    assert lib.crab_xent_reduce(None, None, None, None, None, None, 1, None, None, None, None) < 0
    with pytest.raises(_lib.CrabHipError):                   # no CPU fallback
        from crab_amd import ops
        ops.lm_head_xent(torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(16, 8, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int32))
