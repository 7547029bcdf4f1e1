"""Beam search without a device: the CPU restatement (tests/beam_ref.py) against transformers' own _beam_search, the argument plumbing of
the model surface and the engine, the refusals of the three C entry points (csrc/beam.hip), and the EITHER share of the GPU tests' inputs."""
import ctypes as C
import itertools
import os
import re
import types

import pytest
import torch

from crab_amd import _lib, decoder, ops
from crab_amd.unified_llama import UnifiedForCausalLM as U
from tests import beam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ (a) the restatement equals HF
def _table(V, N, seed, eos):
    """Seeded logits indexed by (last token, new tokens so far): [V, N, V] fp32, the EOS column raised so that hypotheses finish."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn((V, N, V), generator=g, dtype=torch.float32) * 4.0
    t[:, :, eos] += 3.0
    return t


def _toy(tab, prompt, K):
    """logits_fn of beam_ref.walk for the table model: the last token is the clip's prompt token at step 0, then the beam's newest id."""
    first = prompt.repeat_interleave(K)
    return lambda st, s: tab[first if s == 0 else st["run_seq"][:, s - 1], s]


def _hf():
    try:
        import transformers
        from transformers import GenerationMixin, PretrainedConfig, PreTrainedModel
        from transformers.modeling_outputs import CausalLMOutput
    except Exception as e:                                       # pragma: no cover
        pytest.skip(f"transformers is not importable here: {e}")
    return types.SimpleNamespace(GenerationMixin=GenerationMixin, PretrainedConfig=PretrainedConfig, PreTrainedModel=PreTrainedModel,
                                 CausalLMOutput=CausalLMOutput)


def _hf_generate(tab, clips, K, N, eos, pad, min_new, lp, early, Rn):
    """HF generate() in beam mode on a GenerationMixin model whose logits are tab[last token, length - 1]; one prompt token per clip.  Returns
    (new ids, sequences_scores)."""
    T = _hf()

    class Cfg(T.PretrainedConfig):
        model_type = "beam_table"

    class Toy(T.PreTrainedModel, T.GenerationMixin):
        config_class = Cfg

        def __init__(self, cfg):
            super().__init__(cfg)
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def forward(self, input_ids=None, **kw):
            return T.CausalLMOutput(logits=tab[input_ids[:, -1], input_ids.shape[1] - 1][:, None, :])

    m = Toy(Cfg(vocab_size=tab.shape[0]))
    prompt = (torch.arange(clips) % tab.shape[0])[:, None]
    if K == 1:                                                   # HF routes num_beams = 1 to its greedy loop: no beam flags, no sequences_scores
        out = m.generate(input_ids=prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=N, eos_token_id=eos, pad_token_id=pad,
                         min_new_tokens=min_new, do_sample=False, use_cache=False)
        return out[:, 1:], None
    out = m.generate(input_ids=prompt, attention_mask=torch.ones_like(prompt), num_beams=K, max_new_tokens=N, eos_token_id=eos, pad_token_id=pad,
                     min_new_tokens=min_new, length_penalty=lp, early_stopping=early, num_return_sequences=Rn, do_sample=False, use_cache=False,
                     return_dict_in_generate=True, output_scores=True)
    return out.sequences[:, 1:], out.sequences_scores


HF_CASES = list(itertools.product((1, 2, 4), (0.0, 1.0, 2.0, -1.0), (False, True, "never"), (0, 2), (False, True)))


def test_walk_equals_hf_beam_search():
    """K x length_penalty x early_stopping x min_new_tokens x num_return_sequences in {1, K}: ids equal, scores to fp32 roundoff.  HF's topk
    leaves ties open: a case in which the reference saw an EITHER step is not held to HF's choice (none is expected with these tables)."""
    _hf()
    V, N, clips, eos, pad = 23, 7, 3, 5, 1
    skipped = 0
    for K, lp, early, min_new, all_k in HF_CASES:
        Rn = K if all_k else 1
        tab = _table(V, N, seed=K * 100 + int(lp * 7) + min_new, eos=eos)
        ids_hf, sc_hf = _hf_generate(tab, clips, K, N, eos, pad, min_new, lp, early, Rn)
        p = R.Params(K, V, N, eos, pad, min_new, lp, early)
        ids, sc, n_either = R.walk(_toy(tab, torch.arange(clips) % V, K), clips, p, Rn)
        what = f"K={K} length_penalty={lp} early_stopping={early!r} min_new_tokens={min_new} num_return_sequences={Rn}"
        if n_either:
            skipped += 1
            continue
        if K == 1 and early == "never" and lp > 0.0:
            continue                                             # one beam is greedy except here: "never" measures the running beam at max length and may go on past an EOS
        assert ids.shape == ids_hf.shape and torch.equal(ids, ids_hf), f"{what}: {ids.tolist()} vs HF {ids_hf.tolist()}"
        if K == 1:
            continue
        assert torch.allclose(sc, sc_hf, rtol=4 * 2.0 ** -23, atol=1e-6), f"{what}: {sc.tolist()} vs HF {sc_hf.tolist()}"
    assert skipped <= len(HF_CASES) // 20, f"{skipped} of {len(HF_CASES)} cases held a near-tie: the pin would be hollow"


def test_exact_mode_is_the_step_with_no_margin():
    c = R.GPU_CASES[0]
    p = R.case_params(c)
    st = R.init_state(R.CLIPS, p)
    a, either, tol = R.step(st, R.case_logits(c, 0), 0, p, exact=True)
    assert not any(either)
    b, _, _ = R.step(st, R.case_logits(c, 0), 0, p)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ (b) the argument plumbing
def _stub(**engine_attrs):
    calls = []
    eng = types.SimpleNamespace(kv_cache_dtype="bf16", weight_dtype="bf16", **engine_attrs)
    eng.generate_beam = lambda embeds, K, max_new, **kw: calls.append((tuple(embeds.shape), K, max_new, kw)) or (
        (torch.zeros((embeds.shape[0] * kw["num_return_sequences"], 3), dtype=torch.int64), torch.zeros(embeds.shape[0] * kw["num_return_sequences"]))
        if kw["return_scores"] else torch.zeros((embeds.shape[0] * kw["num_return_sequences"], 3), dtype=torch.int64))
    eng.generate = lambda *a, **k: pytest.fail("the greedy route was taken")
    m = types.SimpleNamespace(config=types.SimpleNamespace(eos_token_id=2), model=types.SimpleNamespace(pad_token_id=None), device="cpu", _engine=eng,
                              _PROCESSOR_ARGS=U._PROCESSOR_ARGS, _BEAM_ARGS=U._BEAM_ARGS, _check_generate_kwargs=U._check_generate_kwargs)
    m._generate_beam = lambda *a: U._generate_beam(m, *a)
    return m, calls


def test_generate_with_num_beams_reaches_the_beam_route():
    m, calls = _stub()
    emb = torch.zeros((2, 5, 8))
    out = U.generate(m, inputs_embeds=emb, num_beams=4, max_new_tokens=6)
    assert out.shape == (2, 3)
    (shape, K, max_new, kw), = calls
    assert shape == (2, 5, 8) and K == 4 and max_new == 6
    assert kw["eos_token_id"] == 2 and kw["pad_token_id"] == 2 and kw["length_penalty"] == 1.0 and kw["early_stopping"] is False
    assert kw["num_return_sequences"] == 1 and kw["return_scores"] is False
    out = U.generate(m, inputs_embeds=emb, num_beams=3, num_return_sequences=2, length_penalty=0.5, early_stopping="never", min_new_tokens=2,
                     eos_token_id=[9], return_dict_in_generate=True, output_scores=True)
    kw = calls[-1][3]
    assert kw["num_return_sequences"] == 2 and kw["length_penalty"] == 0.5 and kw["early_stopping"] == "never" and kw["min_new_tokens"] == 2
    assert kw["eos_token_id"] == 9 and out.sequences.shape == (4, 3) and out.sequences_scores.shape == (4,)
    out = U.generate(m, inputs_embeds=emb, num_beams=2, return_dict_in_generate=True)
    assert out.sequences.shape == (2, 3) and out.sequences_scores is None


@pytest.mark.parametrize("kw, name", [
    (dict(do_sample=True), "do_sample"), (dict(allowed_sequences=[[3, 4]]), "allowed_sequences"), (dict(repetition_penalty=1.2), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(eos_token_id=[2, 3]), "eos_token_id"),
    (dict(output_token_logprobs=True), "output_token_logprobs"), (dict(output_logits=True, return_dict_in_generate=True), "output_logits"),
    (dict(output_first_logits=True), "output_first_logits"), (dict(kv_cache_dtype="fp8_e4m3"), "kv_cache_dtype"),
    (dict(weight_dtype="fp8_e4m3"), "weight_dtype"), (dict(num_beam_groups=2), "num_beam_groups"), (dict(diversity_penalty=0.5), "diversity_penalty"),
    (dict(constraints=[object()]), "constraints")])
def test_refused_with_beams_by_name(kw, name):
    m, calls = _stub()
    with pytest.raises(NotImplementedError, match=name):
        U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), num_beams=4, **kw)
    assert not calls


def test_what_stays_refused_without_beams_and_elsewhere():
    with pytest.raises(NotImplementedError, match="num_beams"):
        U._check_generate_kwargs(dict(num_beams=4))
    with pytest.raises(NotImplementedError, match="num_beams"):
        U._check_generate_kwargs(dict(num_beams=4), U._PROCESSOR_ARGS)             # what generate_batches / generate_questions / generate_avs* pass
    U._check_generate_kwargs(dict(num_beams=4, length_penalty=2.0, num_return_sequences=3), U._PROCESSOR_ARGS | U._BEAM_ARGS)
    assert U._BEAM_ARGS == frozenset(("num_beams", "length_penalty", "num_return_sequences"))
    m, calls = _stub()
    for kw, name in ((dict(length_penalty=2.0), "length_penalty"), (dict(num_return_sequences=2), "num_return_sequences"),
                     (dict(num_beams=1, length_penalty=0.5), "length_penalty")):
        with pytest.raises(NotImplementedError, match=name):
            U.generate(m, inputs_embeds=torch.zeros((1, 5, 8)), **kw)
    assert not calls


def _bare_engine(V=64):
    eng = decoder.GenerationEngine.__new__(decoder.GenerationEngine)
    eng.lm_head = types.SimpleNamespace(weight=torch.zeros((V, 8)))
    eng._kv_mode, eng._w_mode = "bf16", "bf16"
    eng._call = lambda *a, **k: pytest.fail("device work was reached")
    return eng


def test_engine_refuses_by_name_before_any_device_work():
    eng = _bare_engine()
    emb = torch.zeros((2, 5, 8))
    g = lambda *a, **k: eng.generate_beam(*a, **k)
    with pytest.raises(NotImplementedError, match="num_beams"):
        g(emb, ops.BEAM_MAX + 1, 4)
    with pytest.raises(NotImplementedError, match="num_beams"):
        g(emb, 0, 4)
    with pytest.raises(ValueError, match="num_return_sequences"):
        g(emb, 2, 4, num_return_sequences=3)
    with pytest.raises(ValueError, match="S >= 2"):
        g(emb[:, :1], 2, 4)
    with pytest.raises(NotImplementedError, match="eos_token_id"):
        g(emb, 2, 4, eos_token_id=[2, 3])
    with pytest.raises(NotImplementedError, match="max_new_tokens"):
        g(emb, 2, ops.BEAM_MAX_NEW + 1)
    with pytest.raises(ValueError, match="max_new_tokens"):
        g(emb, 2, 0)
    with pytest.raises(ValueError, match="early_stopping"):
        g(emb, 2, 4, early_stopping="sometimes")
    for k, v in (("sampling", (0.6, 50, 0.9, 1)), ("constraint", object()), ("processors", (1.2, 0, ())), ("return_logprobs", True), ("return_hidden", True)):
        with pytest.raises(NotImplementedError, match=k):
            g(emb, 2, 4, **{k: v})
    for k in ("kv_cache_dtype", "weight_dtype"):
        with pytest.raises(NotImplementedError, match=k):
            g(emb, 2, 4, **{k: "fp8_e4m3"})
    eng._kv_mode = "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        g(emb, 2, 4)
    eng._kv_mode, eng._w_mode = "bf16", "fp8_e4m3"
    with pytest.raises(NotImplementedError, match="weight_dtype"):
        g(emb, 2, 4)
    with pytest.raises(TypeError, match="banana"):
        g(emb, 2, 4, banana=1)


def test_len_table_is_a_double_pow_rounded_once():
    for lp in (0.0, 1.0, 2.0, -1.0, 0.7):
        t = ops.beam_len_table(12, lp)
        assert t.dtype == torch.float32 and t.shape == (13,) and torch.equal(t, R.len_table(12, lp))
        assert all(float(t[n]) == float(torch.tensor(float(n) ** lp, dtype=torch.float64).float()) for n in range(1, 13))
    assert ops.BEAM_MAX == 8 and ops.BEAM_MAX_NEW == _lib.header_const("CRAB_BEAM_MAX_NEW")


# ------------------------------------------------------------------ (c) the C entry points
def test_symbols_are_declared_exported_and_bound_under_abi_13():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "crab_hip.h")).read()
    for name in ("crab_beam_row_topk", "crab_beam_merge", "crab_kv_beam_reorder"):
        assert re.search(r"^int\s+" + name + r"\s*\(", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.crab_abi_version() == 13
    assert lib.crab_beam_max() == ops.BEAM_MAX and lib.crab_beam_max_new() == ops.BEAM_MAX_NEW


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                        # a zeroed block stands in for a context: the refusals are reached without a device
    h = C.cast(ctx, C.c_void_p)
    one = C.cast(C.create_string_buffer(64), C.c_void_p)

    def topk(ctx_=h, logits=one, ldl=64, rows=4, V=64, K=2, run=one, step=one, fin=one, cs=one, ct=one):
        return lib.crab_beam_row_topk(ctx_, None, logits, ldl, rows, V, K, run, step, fin, 7, 0, cs, ct)

    def merge(ctx_=h, rows=4, V=64, K=2, max_new=8, early=0, ld_run=8, ld_hyp=8, **nulls):
        a = dict(cs=one, ct=one, step=one, tab=one, run=one, seq=one, hs=one, hq=one, hl=one, hf=one, un=one, cur=one, bi=one, fin=one)
        a.update(nulls)
        return lib.crab_beam_merge(ctx_, None, a["cs"], a["ct"], rows, V, K, max_new, a["step"], 7, 1, early, 1, a["tab"], a["run"], a["seq"], ld_run,
                                   a["hs"], a["hq"], ld_hyp, a["hl"], a["hf"], a["un"], a["cur"], a["bi"], a["fin"])

    def reorder(ctx_=h, kc=one, vc=one, L=2, rows=4, K=2, Hk=2, Tmax=64, d=64, first=0, pos=one, bi=one, fin=one):
        return lib.crab_kv_beam_reorder(ctx_, None, kc, vc, L, rows, K, Hk, Tmax, d, first, pos, bi, fin)

    assert topk(ctx_=None) == -1 and merge(ctx_=None) == -1 and reorder(ctx_=None) == -1
    for k in ("logits", "run", "step", "fin", "cs", "ct"):
        assert topk(**{k: None}) == -1, k
    assert b"beam_row_topk" in ctx.raw
    for kw in (dict(rows=0), dict(K=0), dict(rows=3), dict(V=3), dict(ldl=-1), dict(V=(1 << 27) + 1)):
        assert topk(**kw) == -1, kw
    assert topk(K=9, rows=9) == -3, "CRAB_E_UNSUPPORTED past CRAB_BEAM_MAX"
    ctx.raw = bytes(len(ctx.raw))
    for k in ("cs", "ct", "step", "tab", "run", "seq", "hs", "hq", "hl", "hf", "un", "cur", "bi", "fin"):
        assert merge(**{k: None}) == -1, k
    assert b"beam_merge" in ctx.raw
    for kw in (dict(rows=0), dict(K=0), dict(rows=3), dict(V=3), dict(max_new=0), dict(ld_run=7), dict(ld_hyp=7), dict(early=3), dict(early=-1)):
        assert merge(**kw) == -1, kw
    assert merge(K=9, rows=9) == -3 and merge(max_new=1025, ld_run=1025, ld_hyp=1025) == -3
    ctx.raw = bytes(len(ctx.raw))
    for k in ("kc", "vc", "pos", "bi", "fin"):
        assert reorder(**{k: None}) == -1, k
    assert b"kv_beam_reorder" in ctx.raw
    for kw in (dict(L=0), dict(rows=0), dict(rows=3), dict(K=0), dict(Hk=0), dict(Tmax=0), dict(first=-1), dict(first=64), dict(d=60), dict(d=0)):
        assert reorder(**kw) == -1, kw
    assert reorder(K=9, rows=9) == -3 and reorder(L=40000, Hk=64, Tmax=1024) == -3, "CRAB_E_UNSUPPORTED past 2^31 16-byte units"


# ------------------------------------------------------------------ (d) the GPU tests' inputs hold few near-ties, by the reference alone
@pytest.mark.parametrize("c", R.GPU_CASES, ids=lambda c: c.name)
def test_either_share_of_the_gpu_inputs_is_under_the_cap(c):
    hit, live = R.case_either_share(c)
    assert live >= R.CLIPS, "the case never ran"
    assert hit <= R.EITHER_CAP * live, f"{c.name}: {hit} of {live} live (clip, step) pairs are EITHER"
