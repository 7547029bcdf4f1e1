"""Llama / Qwen2 decoder stack on the HIP kernels: module containers named like the HF classes the reference
subclasses (transformers LlamaModel / Qwen2Model; in-tree statement models/modeling_llama.py,
models/qwen/modeling_qwen2.py) plus the generation engine (prefill, device-resident greedy decode).

Per layer (modeling_llama.py:805-827):  x += o_proj(attn(rope(qkv(rmsnorm(x)))));  x += down(silu(gate(h))*up(h))
launch sequence, M = batch*seq rows:
  rmsnorm -> [R;A] skinny GEMM -> routing mix -> fused QKV GEMM (K extended by the LoRA segment, +bias for Qwen2)
  -> RoPE + KV-cache scatter (+V^T for the prefill attention) -> flash attention (prefill) | KV-streaming attention
  (decode) -> o_proj GEMM with residual epilogue -> rmsnorm -> gate|up GEMM -> SwiGLU -> down GEMM with residual.
Decode runs the same sequence at M = batch with the step captured once into a HIP graph and replayed; the
token position, step index and finished flags live in device memory, so there is no per-token host sync
(the reference's HF loop syncs every token).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import types
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch import nn

import ctypes as C

from . import _lib, ops
from .peft_hyper import PackedLinearGroup

BF16 = torch.bfloat16
# generate()'s prefill needs one row per sequence after the last layer: its attention / o_proj / MLP run for the last rows only (crab_llama_io.last_rows_only;
# the reference computes all S rows and lm_head drops S - 1 of them, modeling_llama.py:1260).  CRAB_PREFILL_LAST_ROWS=0: every row through every layer (A/B runs).
import os as _os
LAST_ROWS_ONLY = _os.environ.get("CRAB_PREFILL_LAST_ROWS", "1") != "0"
RAGGED_PAD_MAX = 0.06     # a coalesced wave whose batches differ in length is prefilled as ONE padded batch while the padding costs at most this fraction of the prefill rows
WEIGHT_DTYPES = ("bf16", "fp8_e4m3")       # GenerationEngine(weight_dtype=...): bf16 decoder weights | opt-in FP8 (e4m3fn codes + fp32 row scales) for decode steps of <= 16 rows
W8_MAX_ROWS = 16                            # rows up to which a decode step streams the FP8 weights (the regime of gemm_skinny_dma_w8_kernel, csrc/skinny.hip)
KV_CACHE_DTYPES = ("bf16", "fp8_e4m3")     # GenerationEngine(kv_cache_dtype=...): the default bf16 cache | the opt-in FP8 (OCP e4m3fn) cache with fp32 row scales
SHED_MIN_STEPS_LEFT = 4   # shed_finished: a look sheds only while at least this many decode steps remain (the measured break-even is ~3 steps)
EOS_CHECK_EVERY = 16      # decode steps between two host reads of the `finished` flags: the only synchronisation inside the step loop (_run_steps)
ONE_EOS = ("the device-resident decode loop stops on ONE id (pass the chat end token, e.g. <|im_end|>; the reference's own Qwen path never reaches HF "
           "generate, SURVEY.md 2); further stop ids go into processors = (repetition_penalty, no_repeat_ngram_size, stop_token_ids)")      # one_eos: what generate() says
NATIVE_LAYERS = True     # False: issue every launch of a layer from Python (A/B runs and the sequencer-equivalence tests)


@dataclass
class DecoderConfig:
    """Subset of LlamaConfig / Qwen2Config the forward path reads."""
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: Optional[int] = None
    vocab_size: int = 32000
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    attention_bias: bool = False        # True on q/k/v for Qwen2 (modeling_qwen2.py:234-236)
    max_position_embeddings: int = 2048
    pad_token_id: Optional[int] = None
    eos_token_id: Optional[int] = None
    model_type: str = "llama"

    def __post_init__(self):
        if self.num_key_value_heads is None:
            self.num_key_value_heads = self.num_attention_heads

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float, device):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=ops.RMS_DTYPE), requires_grad=False)      # fp32 beside the fp32 residual stream
        self.variance_epsilon = eps


class Attention(nn.Module):
    def __init__(self, cfg: DecoderConfig, device):
        super().__init__()
        D, H, Hk, d = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self._qkv = PackedLinearGroup(["q_proj", "k_proj", "v_proj"], D, [H * d, Hk * d, Hk * d], cfg.attention_bias, device)
        self._o = PackedLinearGroup(["o_proj"], H * d, [D], False, device)
        self._qkv.prof_class = self._o.prof_class = "decoder"
        self.q_proj, self.k_proj, self.v_proj = self._qkv.linears
        self.o_proj = self._o.linears[0]


class MLP(nn.Module):
    def __init__(self, cfg: DecoderConfig, device):
        super().__init__()
        D, I = cfg.hidden_size, cfg.intermediate_size
        # gate / up rows interleaved: the gate|up GEMM epilogue applies SwiGLU itself (no [M, 2I] round trip, one launch less)
        self._gu = PackedLinearGroup(["gate_proj", "up_proj"], D, [I, I], False, device, interleave=True)
        self._down = PackedLinearGroup(["down_proj"], I, [D], False, device)
        self._gu.prof_class = self._down.prof_class = "decoder"
        self.gate_proj, self.up_proj = self._gu.linears
        self.down_proj = self._down.linears[0]


class DecoderLayer(nn.Module):
    def __init__(self, cfg: DecoderConfig, device):
        super().__init__()
        self.self_attn = Attention(cfg, device)
        self.mlp = MLP(cfg, device)
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device)

    def groups(self) -> List[PackedLinearGroup]:
        return [self.self_attn._qkv, self.self_attn._o, self.mlp._gu, self.mlp._down]


class Embedding(nn.Module):
    def __init__(self, n: int, dim: int, device):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n, dim, device=device, dtype=BF16), requires_grad=False)
        self.num_embeddings, self.embedding_dim = n, dim

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        out = ops.embedding(ids, self.weight)
        return out.view(*ids.shape, self.embedding_dim)


class LMHead(nn.Module):
    def __init__(self, dim: int, n: int, device):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n, dim, device=device, dtype=BF16), requires_grad=False)


class DecoderModel(nn.Module):
    """`model.*` of the causal LM: embed_tokens, layers, norm (LlamaModel, modeling_llama.py:989-1124)."""

    def __init__(self, cfg: DecoderConfig, device):
        super().__init__()
        self.config = cfg
        self.embed_tokens = Embedding(cfg.vocab_size, cfg.hidden_size, device)
        self.layers = nn.ModuleList([DecoderLayer(cfg, device) for _ in range(cfg.num_hidden_layers)])
        self.norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device)


class _Workspace:
    """Caller-owned activation buffers for M rows (allocated once per shape through torch's allocator)."""

    def __init__(self, cfg: DecoderConfig, M: int, device, t_cols: int, u_cols: int):
        D, I = cfg.hidden_size, cfg.intermediate_size
        H, Hk, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        e = lambda *s, dt=BF16: torch.empty(s, device=device, dtype=dt)
        self.M = M
        self.x = e(M, D, dt=ops.RES_DTYPE)       # the residual stream: fp32 (ops.RESIDUAL_FP32), read / written by the o_proj / down_proj epilogues
        self.h = e(M, D)
        self.qkv = e(M, (H + 2 * Hk) * d)
        self.att = e(M, H * d)
        self.act = e(M, I)
        self.t = torch.empty((max(ops.hyperlora_route_workspace(M, max(D, I), max(t_cols, 16)), 16),), device=device, dtype=torch.uint8)
        self.u = e(M, max(u_cols, 32))
        self.u2 = e(M, max(u_cols, 32))       # router output produced ahead by a fused post-norm epilogue
        # small batches (M * H blocks cannot fill the chip): scratch of the fused RoPE + append + split-context decode attention; its
        # tickets start at zero and the kernel leaves them zero
        self.attn_ws = ops.attn_decode_rope_workspace(M, H, d, device) if M * H < ops.ATTN_SPLIT_BELOW and d in (64, 128) else None


@contextlib.contextmanager
def _ws_slot(slot: int):
    """ops.WS_SLOT = slot for the launches issued (or captured) inside; the previous value is back on any exit."""
    saved, ops.WS_SLOT = ops.WS_SLOT, slot
    try:
        yield
    finally:
        ops.WS_SLOT = saved


def _trim_at_eos(out_ids: torch.Tensor, n_done: int, eos) -> torch.Tensor:
    """The first n_done columns of out_ids [B, n], cut after the first column at which EVERY row has emitted `eos` (HF stops a call as soon as
    all of its rows have finished; the columns behind it were produced between two checks).  eos < 0: no stop id; a tuple of ids (a state's
    eos_all: eos_token_id and the stop_token_ids of its processors): any of them stops a row.  A view: callers clone."""
    out = out_ids[:, :n_done]
    ids = [int(e) for e in (eos if isinstance(eos, (tuple, list)) else (eos,)) if int(e) >= 0]
    if ids:
        hit = out == ids[0]
        for e in ids[1:]:
            hit = hit | (out == e)
        idx = torch.nonzero((hit.int().cumsum(1) > 0).all(0))
        if idx.numel():
            out = out[:, : int(idx[0].item()) + 1]
    return out


def normalize_processors(processors):
    """The `processors` argument of the generate entry points - (repetition_penalty, no_repeat_ngram_size, stop_token_ids) or None - as
    (float, int, tuple of distinct ints in the order given) or None when every value is neutral (1.0, 0, no ids): a neutral call is the
    call without the argument (same state key, same graph, same launches).  stop_token_ids are the stop ids BEYOND eos_token_id."""
    if processors is None:
        return None
    p, n, stops = processors
    p = 1.0 if p is None else float(p)
    n = 0 if n is None else int(n)
    stops = tuple(dict.fromkeys(int(e) for e in (stops or ())))
    if not p > 0:                                           # HF: RepetitionPenaltyLogitsProcessor - "`penalty` has to be a strictly positive float"
        raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {p}")
    if n < 0:                                               # HF: NoRepeatNGramLogitsProcessor - "`ngram_size` has to be a strictly positive integer" (0 = off)
        raise ValueError(f"`no_repeat_ngram_size` has to be a positive integer or 0 (off), but is {n}")
    if any(e < 0 for e in stops):
        raise ValueError(f"stop_token_ids must be token ids >= 0, got {list(stops)}")
    if len(stops) > ops.LOGITS_PROC_MAX_STOP:
        raise NotImplementedError(f"stop_token_ids = {list(stops)}: the decode step takes at most {ops.LOGITS_PROC_MAX_STOP} stop ids beyond eos_token_id")
    return None if (p == 1.0 and n == 0 and not stops) else (p, n, stops)


def check_processors(processors, min_new_tokens: int = 0, constrained: bool = False, return_logprobs: bool = False, eos_token_id=None,
                     names=("return_logprobs", "constraint", "stop_token_ids")):
    """eos_token_id: the select's own stop id - a stop_token_id equal to it drops out first, so a triple that only repeats it is neutral.
    names: what the caller's surface calls the three arguments in the messages (the model passes its HF-side names).
    normalize_processors + the combinations the decode step refuses BY NAME, before any device work: each would need a change to a kernel
    the processors leave alone (crab_logprob_norm sums plane 1 over "every token but EOS" or the trie's edges, the trie has one EOS edge).
    The repetition penalty alone combines with everything."""
    proc = normalize_processors(processors)
    if isinstance(eos_token_id, (list, tuple)) and len(set(int(e) for e in eos_token_id)) == 1:
        eos_token_id = eos_token_id[0]                          # a one-id list is that id (_state)
    if proc is not None and isinstance(eos_token_id, int):
        proc = normalize_processors((proc[0], proc[1], tuple(e for e in proc[2] if e != int(eos_token_id))))
    if proc is None:
        return None
    p, n, stops = proc
    lp_name, con_name, stop_name = names
    if return_logprobs and n > 0:
        raise NotImplementedError(f"{lp_name} with no_repeat_ngram_size = {n}: the banned tokens would have to leave the set token_logprobs_allowed is "
                                  "normalised over (crab_logprob_norm); the repetition penalty alone is fine")
    if return_logprobs and stops and int(min_new_tokens) > 0:
        raise NotImplementedError(f"{lp_name} with {stop_name} = {list(stops)} and min_new_tokens = {min_new_tokens}: the suppressed stop ids would "
                                  "have to leave the set token_logprobs_allowed is normalised over (crab_logprob_norm knows one EOS)")
    if constrained and stops:
        raise NotImplementedError(f"{con_name} with {stop_name} = {list(stops)}: a token trie has ONE end-of-sequence edge (pass one eos_token_id)")
    if constrained and n > 0:
        raise NotImplementedError(f"{con_name} with no_repeat_ngram_size = {n}: a ban could empty a trie node's edge set, which crab_constrained_select "
                                  "reads from the trie alone")
    return proc


def normalize_sampling(sampling, constrained: bool = False):
    """The `sampling` argument of the generate entry points: None (greedy), (temperature, top_k, top_p, seed) or, with HF's further truncation
    warpers, (temperature, top_k, top_p, seed, min_p, epsilon_cutoff, eta_cutoff) - 0 or None = that stage is off (csrc/sample.hip).
    A 7-tuple whose three stages are all off comes back as the 4-tuple: that call is the plain sampling call (same state key, same graph,
    same launches).  Values outside min_p in [0, 1] / the cutoffs in [0, 1), NaN included, raise ValueError by name; a live stage with a
    token trie (constrained) is refused by name - crab_constrained_select is a kernel of its own.  All before any device work."""
    if sampling is None or len(sampling) == 4:
        return sampling
    if len(sampling) != 7:
        raise ValueError(f"sampling must be (temperature, top_k, top_p, seed) or those four + (min_p, epsilon_cutoff, eta_cutoff), got {sampling!r}")
    w = []
    for name, v, hi_ok in (("min_p", sampling[4], True), ("epsilon_cutoff", sampling[5], False), ("eta_cutoff", sampling[6], False)):
        v = 0.0 if v is None else float(v)
        if not (0.0 <= v <= 1.0) or (v == 1.0 and not hi_ok):
            raise ValueError(f"`{name}` has to be a float in " + ("[0, 1]" if hi_ok else "[0, 1)") + f" (0 = off), but is {v}")
        w.append(v)
    if not any(w):
        return tuple(sampling[:4])
    if constrained:
        live = ", ".join(f"{n} = {v}" for n, v in zip(("min_p", "epsilon_cutoff", "eta_cutoff"), w) if v)
        raise NotImplementedError(f"constraint with {live}: the truncation warpers beyond top_p are not implemented under a token trie "
                                  "(crab_constrained_select is a kernel of its own; temperature, top_k and top_p are)")
    return tuple(sampling[:4]) + tuple(w)


def reseed_sampling(sampling, offset: int):
    """The sampling tuple (of either length) of a later wave or group of one call: its seed moved by `offset`, everything else kept."""
    return None if sampling is None else tuple(sampling[:3]) + (sampling[3] + offset,) + tuple(sampling[4:])


def shed_default_ladder():
    """The row counts a shedding wave (shed_finished=True) steps down through: the powers of two from 4 to ops.DECODE_MAX_ROWS.  They contain the
    counts at which the decode step changes kernels - 16 (the M <= 16 projections), 64 (CRAB_DEC_MIN_ROWS), 256 and ops.DECODE_MAX_ROWS - and
    every rung is half of the next: a wave that has lost half of its rows always finds a rung, and the rows a call moves over all of its
    sheds are bounded by a geometric series (< 2 x the rows of its first shed).  Below 4 rows a step is a latency chain that no row count
    shortens.  A decision, not a measured optimum."""
    top = int(ops.DECODE_MAX_ROWS)
    return tuple(sorted({r for r in (4, 8, 16, 32, 64, 128, 256) if r < top} | {top}))


def shed_ladder(shed_finished):
    """The `shed_finished` argument as a ladder: None / False -> None (the option is off: the call is the call without the argument), True ->
    shed_default_ladder(), a tuple / list of row counts -> that tuple, which has to be strictly increasing and positive (ValueError by name)."""
    if shed_finished is None or shed_finished is False:
        return None
    if shed_finished is True:
        return shed_default_ladder()
    if not isinstance(shed_finished, (tuple, list)) or not shed_finished or any(isinstance(r, bool) or not isinstance(r, int) for r in shed_finished):
        raise ValueError(f"`shed_finished` has to be None, a bool or a sorted tuple of row counts, but is {shed_finished!r}")
    lad = tuple(int(r) for r in shed_finished)
    if any(r < 1 for r in lad):
        raise ValueError(f"`shed_finished` = {lad}: every rung has to be a positive row count")
    if any(b <= a for a, b in zip(lad, lad[1:])):
        raise ValueError(f"`shed_finished` = {lad}: the rungs have to be sorted (strictly increasing)")
    return lad


def shed_rung(ladder, n_live: int, B_cur: int) -> Optional[int]:
    """The row count a state of B_cur rows with n_live unfinished ones sheds to: the smallest rung >= n_live when that is below B_cur, else None
    (no rung holds the live rows, or the state already is that small: nothing happens)."""
    for r in ladder:
        if r >= n_live:
            return r if r < B_cur else None
    return None


def check_shed(shed_finished, shed_every=None, constraint=None, processors=None, return_logprobs: bool = False, return_hidden: bool = False,
               decode_streams: int = 1, kv_cache_dtype: str = "bf16", return_step_logits: bool = False, coalesced: bool = False):
    """shed_ladder + what a shedding call refuses BY NAME, before any device work (the style of check_lookup).  A shed gathers the per-row words a plain greedy / sampling step owns and moves bf16 cache rows; every option below
    owns further per-row device state that would have to move with them.  Returns (ladder, steps between looks) or None when the option is off."""
    s_name, e_name, c_name, p_name, lp_name, h_name, d_name, sl_name = ("shed_finished", "shed_every", "constraint", "processors", "return_logprobs",
                                                                         "return_hidden", "decode_streams", "return_step_logits")
    lad = shed_ladder(shed_finished)
    if lad is None:
        return None
    every = EOS_CHECK_EVERY if shed_every is None else int(shed_every)
    if every < 1:
        raise ValueError(f"`{e_name}` has to be a strictly positive number of steps, but is {shed_every}")
    if constraint is not None:
        raise NotImplementedError(f"{s_name} with {c_name}: the trie node of every row (crab_constrained_select) would have to follow its row")
    if normalize_processors(processors) is not None:
        raise NotImplementedError(f"{s_name} with {p_name}: the save area of crab_logits_edit / crab_logits_restore is laid out per row of the wave")
    if return_logprobs:
        raise NotImplementedError(f"{s_name} with {lp_name}: the log-probability planes are laid out per row of the wave")
    if return_hidden:
        raise NotImplementedError(f"{s_name} with {h_name}: the hidden rows are kept per row of the wave")
    if int(decode_streams) > 1:
        raise NotImplementedError(f"{s_name} with {d_name} = {decode_streams}: the groups of a split wave step in lockstep on their own streams")
    if kv_cache_dtype == "fp8_e4m3":
        raise NotImplementedError(f'{s_name} with kv_cache_dtype="fp8_e4m3": crab_kv_compact_rows moves the bf16 cache (the fp8 row scales would have to move too)')
    if coalesced and return_step_logits:
        raise NotImplementedError(f"{s_name} with {sl_name} in the coalesced form: the per-step logits of a shedding wave are kept by generate() only")
    return lad, every


class _Shed:
    """One shedding call: the ladder, the steps between looks, and what the call records - log: (step, rows_before, rows_after, rows_moved) per
    shed; captures: HIP graphs captured by this call.  out: the result buffer of the wave in progress (_run_steps)."""

    def __init__(self, ladder, every: int):
        self.ladder, self.every = tuple(ladder), int(every)
        self.log, self.captures = [], 0
        self.out = None


def _pack_waves(Bs: List[int], cap: int) -> List[List[int]]:
    """generate_many(coalesce=True): the batches (Bs[g] rows each), in order, as waves of at most `cap` rows and about equal size - 60 batches
    of 8 at cap 448 run as 240 + 240, not 448 + 32.  A batch larger than the cap is a wave of its own.  Returns the batch indices per wave."""
    total = sum(Bs)
    n_waves = max(1, -(-total // cap))
    target = -(-total // n_waves)
    waves, cur, rows = [], [], 0
    for g, b in enumerate(Bs):
        if cur and rows + b > min(cap, max(target, b)):
            waves.append(cur)
            cur, rows = [], 0
        cur.append(g)
        rows += b
    if cur:
        waves.append(cur)
    return waves


def one_eos(eos_token_id, what: str):
    """HF accepts a list of stop ids (Qwen2-7B-Instruct's generation_config holds two); the device loop carries ONE: a list of one distinct id
    is that id, an empty list is None, several ids are refused - `what` is the caller's half of the message.  THE rule of every entry point."""
    if not isinstance(eos_token_id, (list, tuple)):
        return eos_token_id
    if len(set(int(e) for e in eos_token_id)) > 1:
        raise NotImplementedError(f"eos_token_id = {list(eos_token_id)}: {what}")
    return eos_token_id[0] if len(eos_token_id) else None


@dataclass(frozen=True)
class _Request:
    """The per-call options of a generate entry point, normalised ONCE by it (after its check_* / normalize_* calls): every private method takes
    (tensors ..., req) and what is genuinely its own.  eos: the single stop id (one_eos) or None; pad_token_id: as given; shed: the call's
    _Shed.  The last four fields vary per wave or group of a call, through replace(): the wave's _Constraint, cfg = (guidance_scale, pairs),
    lookup = (k, max_ngram, keep step logits), extra_key = what else the captured step bakes in (prefix buffers, beam parameters).
    A new option is a field here, a term of _state_key, a line of _Collect if it returns something, and its launch in _select / _decode_step."""
    max_new_tokens: int
    eos: Optional[int] = None
    pad_token_id: Optional[int] = None
    min_new_tokens: int = 0
    use_graph: bool = True
    sampling: Optional[tuple] = None
    processors: Optional[tuple] = None
    return_step_logits: bool = False
    return_hidden: bool = False
    return_first_logits: bool = False
    return_logprobs: bool = False
    prefill_chunk: int = 0
    shed: Optional[_Shed] = None
    constraint: Optional["_Constraint"] = None
    cfg: Optional[tuple] = None
    lookup: Optional[tuple] = None
    extra_key: tuple = ()

    replace = dataclasses.replace                # the per-wave variation: req.replace(sampling=..., constraint=..., cfg=..., extra_key=...)

    @property
    def graphed(self) -> bool:                   # the steps are captured and replayed: with one or two tokens there is none (or one) to replay
        return bool(self.use_graph and self.max_new_tokens > 2)

    @property
    def join_pad(self) -> int:
        """What fills the ids of a group or wave that stopped before the longest (_join): pad -> eos -> 0.  NOT a state's pad word (stop_words),
        which also falls back to the first further stop id: that is what a finished row emits INSIDE the step (HF's list-valued eos_token_id
        makes its first id the pad); a join fills columns behind a whole group's end, and has always stopped at eos."""
        return int(self.pad_token_id) if self.pad_token_id is not None else (int(self.eos) if self.eos is not None else 0)

    def rows(self, b0: int, b1: int) -> "_Request":
        """The request of rows b0 .. b1 of the call's batch: the constraint's roots of those rows."""
        return self if self.constraint is None else self.replace(constraint=self.constraint.rows(b0, b1))


def stop_words(eos, pad_token_id, processors):
    """(eos, proc, pad) as a decode state holds them.  eos: -1 for None.  proc: the triple normalised against eos - a stop id equal to eos is
    the select's own, and a triple that is neutral after that is None: the call meets the key, graph and launches of a call without it.
    pad: what a finished row emits - pad_token_id, else eos, else the first further stop id (HF: the first id of a list-valued eos), else 0."""
    eos = -1 if eos is None else int(eos)
    proc = normalize_processors(processors)
    if proc is not None:
        proc = normalize_processors((proc[0], proc[1], tuple(e for e in proc[2] if e != eos)))
    stops = proc[2] if proc is not None else ()
    pad = int(pad_token_id) if pad_token_id is not None else (eos if eos >= 0 else (stops[0] if stops else 0))
    return eos, proc, pad


def _state_key(B, Tmax, max_new_tokens, eos, pad, min_new_tokens, return_hidden, ptrs, lora, sampling, ragged, kv_mode, scale_ptrs, w8_key,
               logprobs, extra_key=(), trie_key=(), proc=None, cfg=None, lookup=None, S=0):
    """The key of a decode state: everything its captured HIP graph bakes in, as plain values - a state (and its graph) serves exactly the
    calls whose key is equal.  ptrs: K cache, V cache, id of the workspace, RoPE table, lm_head, embedding, first q|k|v weight, as ints;
    scale_ptrs: the FP8 cache's two row-scale pointers (0, 0 in bf16 mode); w8_key: _w8_key; eos / pad / proc: stop_words; S: with lookup only."""
    return (B, Tmax, max_new_tokens, eos, pad, int(min_new_tokens), bool(return_hidden)) + tuple(ptrs) + \
        (bool(lora), sampling, bool(ragged), kv_mode) + tuple(scale_ptrs) + (w8_key, bool(logprobs)) + tuple(extra_key) + tuple(trie_key) + \
        (("proc",) + proc if proc is not None else ()) + \
        (("cfg", float(cfg[0]), int(cfg[1])) if cfg is not None else ()) + \
        (("lookup", int(lookup[0]), int(lookup[1]), bool(lookup[2]), int(S)) if lookup is not None else ())


def _child_key(root_key, Bp: int, w8_key):
    """The Bp-row child of a wave that sheds rows (_shed_to): the root's key stands for all the child bakes in but its rows and weight form."""
    return tuple(root_key) + ("shed", Bp) + tuple(w8_key)


def _join(parts, pad: int, keep=None):
    """Groups or waves of one call that ran one after the other, joined along the rows (parts[i]: the tuple of tensors of part i).  A part that
    stopped early (EOS) is widened to the longest: its ids (element 0) with `pad`, its per-step tensors with zeros; never element `keep`
    (the first logits [B, V]: no step axis)."""
    n_max = max(q[0].shape[1] for q in parts)
    res = []
    for j in range(len(parts[0])):
        cols = []
        for q in parts:
            t = q[j]
            if j != keep and t.dim() >= 2 and t.shape[1] < n_max:
                fill = torch.full((t.shape[0], n_max - t.shape[1]) + tuple(t.shape[2:]), pad if j == 0 else 0, device=t.device, dtype=t.dtype)
                t = torch.cat([t, fill], 1)
            cols.append(t)
        res.append(torch.cat(cols, 0))
    return tuple(res)


class GenerationEngine:
    """Prefill + greedy decode over a DecoderModel + lm_head.  Owns KV caches / workspaces (torch allocator)."""

    def __init__(self, model: DecoderModel, lm_head: LMHead, kv_cache_dtype: str = "bf16", weight_dtype: str = "bf16"):
        """weight_dtype: "bf16" (default) or "fp8_e4m3" - the opt-in FP8 decoder weights (include/crab_hip.h "FP8 decoder weights"): the DECODE
        steps of generate() / generate_many() with at most 16 rows stream the four projection groups of every layer as e4m3fn codes with one
        fp32 scale per output row (PackedLinearGroup.quantize_fp8; activations, adapters and biases stay bf16).  Out of scope, all on the bf16
        weights: prefill (the first token's logits equal the bf16 mode's bit for bit), decode batches above 16 rows (the 17-128 row
        register-direct kernel and beyond), lm_head, forward() and score().  Also settable per call: generate(..., weight_dtype=...).
        kv_cache_dtype: "bf16" (default) or "fp8_e4m3" - the opt-in FP8 KV cache of generate() / generate_many() (include/crab_hip.h "FP8 KV
        cache": e4m3fn codes + one fp32 scale per cached row and KV head; prefill runs in bf16 into a staging block that crab_kv_quant_fp8 moves
        over, decode attends the fp8 rows through crab_attn_decode_fp8).  Also settable per call: generate(..., kv_cache_dtype=...)."""
        self.model, self.lm_head = model, lm_head
        self._stage = None             # fp8 mode: the bf16 staging pair a prefill chunk runs into (flat, grow-only)
        self.kv_cache_dtype = kv_cache_dtype
        self.weight_dtype = weight_dtype
        self._w_used = None            # weight dtype the decode states of the call in progress were built for (last_plan["weight_dtype_used"])
        self.cfg = model.config
        self._rope = None
        self._ws = {}
        self._kv = {}
        self._dec = {}                 # slot -> persistent decode state (+ captured graph)
        self._prefix = None            # generate_shared_prefix: the persistent buffers of the last wave shape (_shared_prefix_buffers: two _SharedPrefix forms)
        self._tries = {}               # TokenTrie.key -> device copies of its CSR arrays (constrained generation; dropped by invalidate())
        self._attn_ws = {}             # B -> scratch of the fused small-batch attention for calls that run in the SHARED prefill workspace (_attn_scratch)
        self.kv_budget_bytes = None    # None: ask the device (hipMemGetInfo); an int caps what generate() may plan with (tests)
        self.last_plan = None          # what the last generate() decided: {"B", "groups", "bytes_per_seq", "budget"}

    # ------------------------------------------------------------------ helpers
    @property
    def device(self):
        return self.lm_head.weight.device

    @staticmethod
    def check_kv_cache_dtype(v) -> str:
        if v not in KV_CACHE_DTYPES:
            raise ValueError(f"kv_cache_dtype must be one of {' / '.join(repr(k) for k in KV_CACHE_DTYPES)}, got {v!r}")
        return v

    @property
    def kv_cache_dtype(self) -> str:
        """The mode of the call in progress (a per-call kv_cache_dtype argument overrides the engine's own for that call), else the engine's."""
        return self._kv_mode

    @kv_cache_dtype.setter
    def kv_cache_dtype(self, v):
        self._kv_mode = self.check_kv_cache_dtype(v)

    @property
    def _fp8(self) -> bool:
        return getattr(self, "_kv_mode", "bf16") == "fp8_e4m3"

    @staticmethod
    def check_weight_dtype(v) -> str:
        if v not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype must be one of {' / '.join(repr(k) for k in WEIGHT_DTYPES)}, got {v!r}")
        return v

    @property
    def weight_dtype(self) -> str:
        """The weight mode of the call in progress (a per-call weight_dtype argument overrides the engine's own for that call), else the engine's."""
        return self._w_mode

    @weight_dtype.setter
    def weight_dtype(self, v):
        self._w_mode = self.check_weight_dtype(v)

    def _w8_rows(self, B: int) -> bool:
        """True when a decode step of B rows streams the FP8 weights under the mode that holds."""
        return getattr(self, "_w_mode", "bf16") == "fp8_e4m3" and B <= W8_MAX_ROWS

    def _w8_key(self, B: int) -> tuple:
        """The weight form of a B-row decode step as a state key holds it: ("bf16",), or the mode and the pointers of every group's codes and
        row scales - the FP8 forms are (re)built here (_quantized), which has to happen before a step can be captured."""
        return ("fp8_e4m3",) + tuple(t.data_ptr() for pair in self._quantized() for t in pair) if self._w8_rows(B) else ("bf16",)

    def _with_kv_mode(self, kv_cache_dtype, fn, *a, **k):
        """Run fn under the per-call mode (None: whatever holds - the engine's, or the enclosing call's for the calls generate() makes itself)."""
        if kv_cache_dtype is None:
            return fn(*a, **k)
        saved, self._kv_mode = self._kv_mode, self.check_kv_cache_dtype(kv_cache_dtype)
        try:
            return fn(*a, **k)
        finally:
            self._kv_mode = saved

    def _call(self, kv_cache_dtype, weight_dtype, shed, fn, *a):
        """The one entry of every generate method: fn under both per-call modes (both values are checked before either is set, so a
        refused call changes nothing) and under the one retry (_retry_after_eviction), then last_plan is stamped with the weight dtype the
        call's decode states ran with ("bf16" when a decode batch exceeded 16 rows).  Nothing inside the engine comes back here - a single
        batch of generate_many, a lone coalesced wave and the groups of a split batch call _generate - so there is one verdict and one retry
        per call by construction.  shed: the _Shed of a shedding call (the one its request carries) or None - every attempt starts its
        record again (a retry after an eviction runs the call anew), and last_plan is stamped with what it recorded."""
        if kv_cache_dtype is not None:
            self.check_kv_cache_dtype(kv_cache_dtype)
        saved = self._w_mode
        if weight_dtype is not None:
            self._w_mode = self.check_weight_dtype(weight_dtype)
        self._w_used = None

        def run():
            if shed is not None:
                shed.log, shed.captures = [], 0
            return fn(*a)

        try:
            res = self._with_kv_mode(kv_cache_dtype, self._retry_after_eviction, run)
            if isinstance(self.last_plan, dict):
                self.last_plan["weight_dtype_used"] = self._w_used or "bf16"
                if shed is not None:
                    self.last_plan["shed"], self.last_plan["shed_captures"] = list(shed.log), shed.captures
            return res
        finally:
            self._w_mode = saved

    def _staging(self, n: int, S: int):
        """fp8 mode: the bf16 block [L, n, Hk, round_up(S, 64), d] x 2 one prefill chunk runs into before crab_kv_quant_fp8 moves it into the
        fp8 cache - views of ONE persistent pair per engine, sized by the largest chunk seen."""
        c = self.cfg
        shape = (c.num_hidden_layers, n, c.num_key_value_heads, _round_up(S, 64), c.head_dim)
        need = math.prod(shape)
        if self._stage is None or self._stage[0].numel() < need or self._stage[0].device != self.device:
            self._stage = None
            self._stage = (torch.empty((need,), device=self.device, dtype=BF16), torch.empty((need,), device=self.device, dtype=BF16))
        return self._stage[0][:need].view(shape), self._stage[1][:need].view(shape)

    def staging_bytes(self, B: int, S: int) -> int:
        """Bytes of the staging pair a generate() of B sequences of S rows needs in fp8 mode (0 in bf16 mode)."""
        if not self._fp8:
            return 0
        c = self.cfg
        n = min(B, max(1, 32768 // max(S, 1)))
        return 2 * c.num_hidden_layers * n * c.num_key_value_heads * _round_up(S, 64) * c.head_dim * 2

    def invalidate(self):
        self._stage = None
        self._dec = {}
        self._ws = {}
        self._kv = {}
        self._attn_ws = {}
        self._tries = {}
        self._prefix = None
        self._table = None
        self._table8 = None
        for l in self.model.layers:                 # the FP8 forms of the packed weights (weight_dtype = "fp8_e4m3"): rebuilt on the next use
            for g in l.groups():
                g.drop_fp8()

    def _rope_tab(self, need: int) -> torch.Tensor:
        if self._rope is None or self._rope.shape[0] < need or self._rope.device != self.device:
            n = max(need, 1024)
            self._rope = ops.rope_table(n, self.cfg.head_dim, self.cfg.rope_theta, self.device)
        return self._rope

    def _attn_scratch(self, ws: _Workspace, B: int):
        """Scratch (split-context partials + arrival counters) of the fused RoPE + append + attention launch of a B-row step, or None when B rows
        do not take that launch.  A decode workspace is made for exactly its B rows and owns its scratch (captured graphs bake the pointer).  The
        SHARED prefill workspace - which forward()'s one-token shortcut runs in - is grow-only and serves any B <= its M, and the launch places its
        counters right behind the partials of ITS B: r06 (scripts/fuzz_engine_state.py) - (1) whether the step fused depended on how large an
        earlier prefill had made that workspace (state, not shape: a 1-ulp difference in the logits, and at the real width never fused at all), and
        (2) a 4-row step followed by a 2-row step in the same buffer would have found the 4-row partials where its zeroed counters belong.  Such
        calls get a zero-filled scratch per B from the engine instead."""
        c = self.cfg
        H, d = c.num_attention_heads, c.head_dim
        if B * H >= ops.ATTN_SPLIT_BELOW or d not in (64, 128):
            return None
        if ws.M == B and ws.attn_ws is not None:
            return ws.attn_ws
        buf = self._attn_ws.get(B)
        if buf is None or buf.device != self.device:
            buf = self._attn_ws[B] = ops.attn_decode_rope_workspace(B, H, d, self.device)
        return buf

    def _workspace(self, M: int, slot: int = 0, decode: bool = False) -> _Workspace:
        """Activation buffers for M rows.
        decode = False: ONE grow-only buffer set shared by every prefill / forward() pass (they are sequential on the stream);
        callers slice [:M].  The prompt length varies per batch in a real evaluation, so a set per distinct M (1.7 GB at
        35 x 702 rows) would pin tens of GB next to the KV cache over a long run.
        decode = True: the buffers a decode state (and its captured HIP graph) keeps; `slot` separates the groups that
        decode concurrently on different streams.  max(4, live groups + 1) sets are kept here (a live _DecodeState holds its own reference)."""
        if not decode:
            ws = self._ws.get("prefill")
            if ws is None or ws.M < M or ws.x.device != self.device:
                self._ws.pop("prefill", None)                 # free the smaller set before allocating the bigger one
                ws = None
                tc, uc = self._ws_cols()
                self._ws["prefill"] = ws = _Workspace(self.cfg, M, self.device, tc, uc)
            return ws
        key = ("decode", M, slot)
        ws = self._ws.pop(key, None)
        if ws is None or ws.x.device != self.device:
            tc, uc = self._ws_cols()
            ws = _Workspace(self.cfg, M, self.device, tc, uc)
        self._ws[key] = ws                                    # most recently used last
        dec_keys = [k for k in self._ws if k != "prefill"]
        keep = max(4, len(self._dec) + 1, slot + 1)           # every live decode group keeps its set (decode_streams > 4 included)
        for k in dec_keys[:-keep]:
            del self._ws[k]
        return ws

    def _ws_cols(self):
        tc = uc = 0
        for g in self.model.layers[0].groups():
            if g.RA is not None:
                tc, uc = max(tc, g.t_cols), max(uc, g.u_cols)
        return tc, uc

    def plan_prefill_chunks(self, B: int, S: int, max_rows: int = 32768) -> List[int]:
        """Split B sequences of S rows into prefill chunks whose projection GEMMs fill whole rounds of 256x256 output tiles
        over the device's CUs.  One block owns a CU, so a GEMM costs ceil(tiles / CUs) rounds of K; a chunk that leaves
        the last round mostly empty pays for it in every projection of every layer (16 x 702 rows: 8.25 -> 9 rounds for
        q|k|v, 2.75 -> 3 for o / down = 5.7 % of the decoder GEMM time).  Exact DP over the chunk sizes <= max_rows / S."""
        cmax = max(1, min(B, max_rows // max(S, 1)))
        if B * S < 2048:                                   # below the ring-GEMM regime the rounds model does not apply
            return [B]
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        shapes = [(g.W.shape[0], g.W.shape[1]) for g in self.model.layers[0].groups()]

        def cost(c):
            tr = -(-(c * S) // 256)
            return sum(-(-(tr * -(-n // 256)) // cus) * k for n, k in shapes)

        per_chunk = 0.002 * cost(cmax)                     # weights re-read + launches: prefer fewer chunks on ties
        best, prev = [0.0] + [float("inf")] * B, [0] * (B + 1)
        costs = [0.0] + [cost(c) + per_chunk for c in range(1, cmax + 1)]
        for n in range(1, B + 1):
            for c in range(1, min(n, cmax) + 1):
                v = best[n - c] + costs[c]
                if v < best[n]:
                    best[n], prev[n] = v, c
        out, n = [], B
        while n:
            out.append(prev[n])
            n -= prev[n]
        return sorted(out, reverse=True)

    # ------------------------------------------------------------------ capacity planning
    def bytes_per_sequence(self, S: int, max_new_tokens: int) -> int:
        """Device bytes ONE more sequence costs a generate() call: its KV-cache rows (2 x L x Hk x Tmax x d bf16), its row of the
        decode workspace / logits / output ids, its share of the prefill V^T scratch."""
        c = self.cfg
        Tmax = _round_up(S + max_new_tokens, 64)
        kv = self.kv_bytes_per_sequence(Tmax)
        D, I = c.hidden_size, c.intermediate_size
        H, Hk, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        xb = 2 if ops.RESIDUAL_FP32 else 0                    # the fp32 residual row costs 2 more bytes per element
        dec_row = (2 * D + (H + 2 * Hk) * d + H * d + I + 3 * 128) * 2 + D * xb + self.lm_head.weight.shape[0] * 4 + D * 2 + max_new_tokens * 8 + 64
        return kv + dec_row

    def kv_bytes_per_sequence(self, Tmax: int) -> int:
        """KV-cache bytes of one sequence: 2 L Hk Tmax d bf16, or in fp8 mode 2 L Hk Tmax (d + 4) (one byte per element + one fp32 scale per row)."""
        c = self.cfg
        rows = 2 * c.num_hidden_layers * c.num_key_value_heads * Tmax
        return rows * (c.head_dim + 4) if self._fp8 else rows * c.head_dim * 2

    def fixed_bytes(self, B: int, S: int) -> int:
        """Batch-size independent scratch of a generate(): the prefill activation set of the largest chunk (<= 32768 rows) + its V^T."""
        c = self.cfg
        D, I = c.hidden_size, c.intermediate_size
        H, Hk, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        rows = min(B, max(1, 32768 // max(S, 1))) * S
        per_row = (2 * D + (H + 2 * Hk) * d + H * d + I + 3 * 128) * 2 + Hk * d * 2 + (D * 2 if ops.RESIDUAL_FP32 else 0)
        have = self._ws.get("prefill")
        have_bytes = have.M * per_row if have is not None else 0
        stage = 0
        if self._fp8:                                          # the bf16 staging pair of the fp8 mode's prefill (grow-only, like the prefill workspace)
            stage = max(self.staging_bytes(B, S) - (2 * self._stage[0].numel() * 2 if self._stage is not None else 0), 0)
        return max(rows * per_row - have_bytes, 0) + stage + (256 << 20)           # + split-K / router workspaces, allocator slack

    def _drop_stale_slots(self, keep_slots: int):
        """Free the persistent KV buffers, decode states (+ graphs) and decode workspaces of the slots >= keep_slots: what an earlier
        generate_many / decode_streams > 1 call left behind and the upcoming call (which uses slots 0 .. keep_slots-1) will not reuse.
        alloc_cache(slot=g) only ever replaces the buffer of the slot it is asked for, so without this those tens of GB would neither be
        reclaimable by the new call nor counted correctly by memory_budget()."""
        stale = [k for k in self._kv if k[0] >= keep_slots]
        for k in stale:
            del self._kv[k]
        for g in [g for g in self._dec if g >= keep_slots]:
            del self._dec[g]
        for k in [k for k in self._ws if k != "prefill" and k[2] >= keep_slots]:
            del self._ws[k]
        if stale:
            torch.cuda.empty_cache()

    def memory_budget(self, B: int, Tmax: int, slots: int = 1) -> int:
        """Bytes generate() may still claim on this device: what the driver reports free (hipMemGetInfo) + what torch's caching
        allocator holds but has not handed out + the engine's own persistent KV buffers - those of the slots the upcoming call re-allocates
        (alloc_cache drops a slot's old buffers before allocating the new shape) AND those of the other slots, which an earlier
        generate_many / decode_streams > 1 call left behind: alloc_cache evicts them (_drop_stale_slots) the moment a new cache would not fit
        beside them, so they count as reclaimable.  A pure query: nothing is freed here (a loop that alternates generate_many(G > 1) with
        generate() keeps its caches and captured graphs as long as the memory is not needed).  `kv_budget_bytes` overrides it."""
        if self.kv_budget_bytes is not None:
            return int(self.kv_budget_bytes)
        self._live_slots = max(1, int(slots))                  # what alloc_cache may NOT evict during the call being planned
        free, _total = torch.cuda.mem_get_info(self.device)
        cached = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        own = sum(t.numel() * t.element_size() for bufs in self._kv.values() for t in bufs)
        px = getattr(self, "_prefix", None)                    # the shared-prefix buffers of an earlier wave shape are replaced, not kept beside the new ones
        if px is not None:
            own += sum(t.numel() * t.element_size() for t in (px.decode.pk, px.decode.pv, px.decode.ws))
        return int(free + cached + own)

    def _evict_for(self, need_bytes: int, slot: int, slack: int = 4 << 30) -> bool:
        """Lazy eviction: the KV caches, decode states and graphs of slots the running call does not use (left by an earlier generate_many /
        decode_streams > 1) are released only when `need_bytes` (+ slack for workspaces) would not fit beside them - memory_budget() counted
        them as reclaimable.  Returns whether anything was dropped."""
        free, _t = torch.cuda.mem_get_info(self.device)
        cached = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if need_bytes + slack <= free + cached:
            return False
        keep = max(getattr(self, "_live_slots", 1), slot + 1)
        had = any(k[0] >= keep for k in self._kv)
        self._drop_stale_slots(keep)
        return had

    def plan_batch(self, B: int, S: int, max_new_tokens: int, slots: int = 1) -> List[int]:
        """Split B sequences into groups that are generated one after the other when their KV cache + scratch would not fit the device
        (the reference's max_new_tokens = 500 at S = 766: 0.66 MB of KV per token per clip -> 0.67 GB per clip, B = 384 does not fit
        288 GB next to the weights; scripts/quick_start.py:36-41).  Returns the group sizes (a single [B] when everything fits)."""
        per = self.bytes_per_sequence(S, max_new_tokens)
        budget = self.memory_budget(B, _round_up(S + max_new_tokens, 64), slots)
        room = int(0.94 * budget) - self.fixed_bytes(B, S)
        fit = max(1, room // per)
        if B <= fit:
            groups = [B]
        else:
            n = -(-B // fit)
            base, extra = divmod(B, n)                        # even groups: the same decode shapes (graphs) repeat
            groups = [base + (1 if i < extra else 0) for i in range(n)]
        self.last_plan = {"B": B, "groups": groups, "bytes_per_seq": per, "budget": budget}
        return groups

    def alloc_cache(self, B: int, Tmax: int, slot: Optional[int] = None):
        """KV cache [L, B, Hk, Tmax, d] x 2; in fp8 mode (kv_cache_dtype = "fp8_e4m3") FOUR tensors: uint8 codes x 2 and fp32 row scales
        [L, B, Hk, Tmax] x 2.  slot = None: fresh zero-filled tensors (callers that keep the cache, e.g.
        forward(use_cache=True)).  slot = g: the engine's persistent buffers for decode group g, reused by every generate()
        of the same shape - rows at or beyond the live context are never read, so they need no clearing, and a 2 x 65 GB
        re-allocation per call (allocator splitting / hipFree retries: the second generate() of a process measured ~0.9 s
        slow) is avoided."""
        c = self.cfg
        shape = (c.num_hidden_layers, B, c.num_key_value_heads, Tmax, c.head_dim)
        fp8 = self._fp8
        if slot is None:
            if fp8:
                return (torch.zeros(shape, device=self.device, dtype=torch.uint8), torch.zeros(shape, device=self.device, dtype=torch.uint8),
                        torch.ones(shape[:4], device=self.device, dtype=torch.float32), torch.ones(shape[:4], device=self.device, dtype=torch.float32))
            return torch.zeros(shape, device=self.device, dtype=BF16), torch.zeros(shape, device=self.device, dtype=BF16)
        key = (slot,)
        hit = self._kv.get(key)
        if hit is None or hit[0].shape != shape or hit[0].device != self.device or (len(hit) == 4) != fp8:
            self._kv.pop(key, None)                  # drop the old buffers before allocating the new shape ...
            hit = None
            if self._dec.pop(slot, None) is not None:    # ... and the decode state (+ graph) that still references them: at
                torch.cuda.empty_cache()                 # 256 clips the old and new caches (2 x ~65 GB each) do not fit together
            if self.device.type == "cuda":
                self._evict_for(B * self.kv_bytes_per_sequence(Tmax), slot)
            if fp8:
                # fp8 mode: (k codes, v codes, k scales, v scales) - uint8 [L, B, Hk, Tmax, d] and fp32 [L, B, Hk, Tmax]
                self._kv[key] = (torch.empty(shape, device=self.device, dtype=torch.uint8), torch.empty(shape, device=self.device, dtype=torch.uint8),
                                 torch.empty(shape[:4], device=self.device, dtype=torch.float32), torch.empty(shape[:4], device=self.device, dtype=torch.float32))
            else:
                self._kv[key] = (torch.empty(shape, device=self.device, dtype=BF16), torch.empty(shape, device=self.device, dtype=BF16))
        return self._kv[key]

    # ------------------------------------------------------------------ the layer table of the native sequencer
    def _quantized(self):
        """weight_dtype = "fp8_e4m3": (codes, scale) of every packed group, built (or rebuilt after a weight update) OUTSIDE any graph capture -
        _state() calls this before a decode step can be captured."""
        return [g.quantize_fp8() for l in self.model.layers for g in l.groups()]

    def _table_fingerprint(self, w8: bool = False):
        """Everything a layer table bakes in: the weight mode and every pointer (the FP8 codes and scales included)."""
        layers = self.model.layers
        fp = tuple(t.data_ptr() if t is not None else 0 for l in layers for g in l.groups() for t in (g.W, g.RA, g.B2, g.bias)) + \
            tuple(w.data_ptr() for l in layers for w in (l.input_layernorm.weight, l.post_attention_layernorm.weight)) + \
            (self.model.norm.weight.data_ptr(),)
        if w8:
            fp += ("fp8_e4m3",) + tuple(t.data_ptr() for pair in self._quantized() for t in pair)
        return fp

    def _layer_table(self, w8: bool = False):
        """crab_llama_layer[n_layers] (include/crab_hip.h) over the packed groups: borrowed pointers, rebuilt when a buffer moved.  w8: the
        table of the FP8-weight decode steps - every group also carries its codes and row scales (crab_linear_group.W8); prefill, forward()
        and score() always run on the plain table."""
        layers = self.model.layers
        fp = self._table_fingerprint(w8)
        slot_name = "_table8" if w8 else "_table"
        hit = getattr(self, slot_name, None)
        if hit is not None and hit[0] == fp:
            return hit[1]
        c = self.cfg
        tab = (_lib.LlamaLayer * len(layers))()

        def fill(dst, g: PackedLinearGroup):
            dst.W, dst.ldw, dst.N, dst.K = g.W.data_ptr(), g.W.stride(0), g.N, g.K
            dst.bias = g.bias.data_ptr() if g.bias is not None else None
            if g.RA is not None:
                dst.RA, dst.ldra, dst.B2, dst.ldb2 = g.RA.data_ptr(), g.RA.stride(0), g.B2.data_ptr(), g.B2.stride(0)
                dst.nproj, dst.nl, dst.r, dst.tcols, dst.ucols, dst.scaling = len(g.names), g.nl, g.r, g.t_cols, g.u_cols, g.scaling
            if w8:
                codes, wsc = g.quantize_fp8()
                dst.W8, dst.ldw8, dst.w_scale = codes.data_ptr(), codes.stride(0), wsc.data_ptr()
        for i, l in enumerate(layers):
            e = tab[i]
            fill(e.qkv, l.self_attn._qkv); fill(e.o, l.self_attn._o); fill(e.gu, l.mlp._gu); fill(e.down, l.mlp._down)
            e.post_attention_norm_w = l.post_attention_layernorm.weight.data_ptr()
            last = i + 1 == len(layers)
            e.next_norm_w = (self.model.norm.weight if last else layers[i + 1].input_layernorm.weight).data_ptr()
            if not last:
                e.next_qkv = C.pointer(tab[i + 1].qkv)
            e.H, e.Hk, e.d, e.rms_eps = c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.rms_norm_eps
            e.norm_w_fp32 = 1 if l.post_attention_layernorm.weight.dtype == torch.float32 else 0
        setattr(self, slot_name, (fp, tab))
        return tab

    def _layers_native(self, ws: _Workspace, B: int, S: int, kc: torch.Tensor, vc: torch.Tensor, b0: int, Tmax: int, pos0: int,
                       pos_dev: Optional[torch.Tensor], vt: Optional[torch.Tensor], t0: int = 0, row_off: Optional[torch.Tensor] = None,
                       pos_ids: Optional[torch.Tensor] = None, kv_start: Optional[torch.Tensor] = None, last_rows: bool = False,
                       kv_scales=None, w8: bool = False):
        """The whole stack through ONE C call (crab_llama_layers, csrc/llama_layer.hip): the same launches in the same order as the
        per-launch Python sequence below, which is kept for the runs that time individual kernels (ops.PROFILER)."""
        io = _lib.LlamaIO()
        io.x, io.h, io.qkv, io.att, io.act, io.u, io.u2 = (t.data_ptr() for t in (ws.x, ws.h, ws.qkv, ws.att, ws.act, ws.u, ws.u2))
        io.ldx, io.ldh, io.ldqkv, io.ldatt, io.ldact, io.ldu = (t.stride(0) for t in (ws.x, ws.h, ws.qkv, ws.att, ws.act, ws.u))
        io.route_ws, io.route_ws_bytes = ws.t.data_ptr(), ws.t.numel()
        sk = ops._splitk_workspace(self.device)
        io.splitk_ws, io.splitk_ws_bytes = sk.data_ptr(), sk.numel()
        io.rope_tab = self._rope_tab(Tmax).data_ptr()
        shift = t0 * kc.stride(3) * kc.element_size()              # a prefill into a right-aligned cache starts at slot t0 of every head's rows
        io.k_cache, io.v_cache, io.cache_layer_stride = kc[0, b0].data_ptr() + shift, vc[0, b0].data_ptr() + shift, kc.stride(0)
        io.row_off = row_off.data_ptr() if row_off is not None else None
        if pos_ids is not None:                                    # prefill under forward()'s position_ids / left-pad mask (the ragged prefill of _start_ragged)
            io.pos_ids, io.ld_pos = pos_ids.data_ptr(), pos_ids.stride(0)
        io.kv_start = kv_start.data_ptr() if kv_start is not None else None
        if vt is not None:
            io.vt, io.vt_ld = vt.data_ptr(), vt.stride(-2)
        io.pos_dev = pos_dev.data_ptr() if pos_dev is not None else None
        aw = self._attn_scratch(ws, B) if vt is None else None
        if aw is not None:
            io.attn_ws, io.attn_ws_bytes = aw.data_ptr(), aw.numel()
        io.B, io.S, io.Tmax, io.pos0, io.u_qkv_ready = B, S, Tmax, pos0, 0
        io.x_fp32 = 1 if ws.x.dtype == torch.float32 else 0
        io.last_rows_only = 1 if last_rows else 0
        if kv_scales is not None:                                  # the FP8 KV cache (decode): kc / vc hold codes (byte strides), one fp32 scale per row beside them
            ks, vs = kv_scales
            io.kv_fp8, io.k_scale, io.v_scale, io.scale_layer_stride = 1, ks[0, b0].data_ptr(), vs[0, b0].data_ptr(), ks.stride(0)
        ops.llama_layers(self._layer_table(w8), len(self.model.layers), io, self.device)

    # ------------------------------------------------------------------ one pass over the layers
    def _layers(self, ws: _Workspace, B: int, S: int, kc: torch.Tensor, vc: torch.Tensor, b0: int, Tmax: int, pos0: int,
                pos_dev: Optional[torch.Tensor], vt: Optional[torch.Tensor], pos_ids: Optional[torch.Tensor] = None,
                kv_start: Optional[torch.Tensor] = None, key_mask: Optional[torch.Tensor] = None, t0: int = 0,
                row_off: Optional[torch.Tensor] = None, last_rows: bool = False, kv_scales=None, w8: bool = False, prefix=None,
                verify: bool = False):
        """x (ws.x[:B*S]) -> x after all layers.  w8 (decode steps of generate() only, <= 16 rows): the projections stream the FP8 weights.  Prefill when vt is given (S rows per sequence, positions pos0..),
        decode otherwise (S == 1, position read from pos_dev).  kc/vc: [L, Btot, Hk, Tmax, d]; rows b0..b0+B.
        The RAGGED decode batch (generate_many(coalesce=True)): sequences of different prompt lengths are right-aligned in one cache - a
        prefill writes its rows to slots t0 .. t0 + S - 1 (rotary positions still 0 .. S - 1: only the cache pointers move), a decode step
        gets row_off (int32 [B]: first slot of every sequence) = per-row rotary offset + first visible key.
        last_rows (prefill): the caller reads ONE row per sequence after the last layer (generate()): the returned h then holds, in its first
        B rows, rmsnorm(last row of sequence b) * model.norm - the last layer ran its attention / o_proj / MLP for those rows only
        (crab_llama_io.last_rows_only; _last_layer_last_rows is the per-launch form) - and x is not updated for the last layer.
        pos_ids (int32 [B, S]) / kv_start (int32 [B]) / key_mask (int32 [B, words], ops.pack_key_mask): forward()'s position_ids and
        attention_mask (unified_llama.py:149-160) - explicit rotary positions, a per-sequence first visible key (left padding) or a
        visibility bit per key (any other mask); they select the per-launch sequence below (RoPE as its own pass), which is not the
        benchmarked path.
        kv_scales = (k_scale, v_scale) fp32 [L, Btot, Hk, Tmax]: kc / vc are the uint8 codes of the FP8 KV cache (decode steps only): the
        projection leaves its raw row and crab_attn_decode_fp8 rotates, quantises, appends and attends (row_off = its first visible key).
        prefix (_SharedPrefix; generate_shared_prefix): the B rows are questions about prefix.pk.shape[1] clips whose first prefix.P positions live
        once per clip in prefix.pk / prefix.pv [L, C, Hk, Tp, d]; kc / vc hold the rows' own keys only.  Per-launch sequence; the attention is
        crab_attn_prefix_partial + crab_attn_own_merge.  Decode step (vt None, S == 1): row_off = first own slot of every row (the first visible
        key), prefix.rope_off = that minus P (the rotary offset: slot - rope_off = position, a NEGATIVE word - crab_qkv_rope_split_ragged only
        subtracts it).  Suffix prefill (vt None, S > 1): pos_ids = the rotary positions, kv_start = the first own slot; query s sees the own
        slots kv_start[b] .. pos0 + s.
        verify (generate_lookup): the verify step of prompt-lookup decoding - vt None, S = k + 1 <= 16 rows of ONE sequence at the slots
        pos_dev + pos0 + s: the M <= 16 projection kernels, crab_qkv_rope_split with S rows and the device position word, then
        crab_attn_verify (row s sees the slots 0 .. pos_dev + pos0 + s).  Per-launch sequence, bf16 cache and weights."""
        c = self.cfg
        H, Hk, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        M = B * S
        if w8 and (vt is not None or S != 1 or M > W8_MAX_ROWS or pos_ids is not None or kv_start is not None or key_mask is not None):
            raise NotImplementedError('weight_dtype="fp8_e4m3" serves the decode steps of generate() with at most 16 rows; prefill, forward() and larger batches run on the bf16 weights')
        if kv_scales is not None:
            if vt is not None or S != 1:
                raise NotImplementedError('kv_cache_dtype="fp8_e4m3": a prefill runs in bf16 into the staging block (GenerationEngine._prefill_chunk), the fp8 cache takes decode steps only')
            if pos_ids is not None or kv_start is not None or key_mask is not None:
                raise NotImplementedError('kv_cache_dtype="fp8_e4m3": the masked one-token step of forward() (position_ids / attention_mask; crab_attn_decode_keymask) has no fp8 form')
            if kc.dtype != torch.uint8 or not (kc.is_contiguous() and vc.is_contiguous() and kv_scales[0].is_contiguous() and kv_scales[1].is_contiguous()):
                raise ValueError("fp8 KV cache: contiguous uint8 codes and fp32 scales expected")
        if prefix is not None:
            if kv_scales is not None or self._fp8:
                raise NotImplementedError('kv_cache_dtype="fp8_e4m3" with a shared prefix (generate_shared_prefix) is not implemented: the prefix cache and its attention kernels are bf16')
            if w8:
                raise NotImplementedError('weight_dtype="fp8_e4m3" with a shared prefix (generate_shared_prefix) is not implemented')
            if vt is not None or key_mask is not None or t0 or b0 or last_rows or (S == 1) != (row_off is not None) or (S > 1) != (pos_ids is not None and kv_start is not None):
                raise ValueError("prefix=: a decode step takes row_off, the suffix prefill pos_ids and kv_start; rows 0 .. B - 1, no V^T, no key mask")
        if verify and (vt is not None or pos_dev is None or not 1 <= S <= 16 or prefix is not None or kv_scales is not None or w8 or row_off is not None
                       or pos_ids is not None or kv_start is not None or key_mask is not None or last_rows or t0):
            raise ValueError("verify=: S <= 16 rows per sequence at pos_dev + pos0 + s, bf16 cache and weights, no masks, no prefix")
        x, h, qkv, att, act = ws.x[:M], ws.h[:M], ws.qkv[:M], ws.att[:M], ws.act[:M]
        tab = self._rope_tab(Tmax if prefix is None else prefix.P + Tmax)
        scale = 1.0 / math.sqrt(d)
        ldq = qkv.stride(0)
        layers = self.model.layers
        ops.rmsnorm(x, layers[0].input_layernorm.weight, c.rms_norm_eps, out=h)
        timed = ops.per_launch_profiling() and not torch.cuda.is_current_stream_capturing()
        masked = pos_ids is not None or kv_start is not None or key_mask is not None
        if row_off is not None and (vt is not None or masked) and prefix is None:
            raise ValueError("row_off is a decode-step argument (no masks / position ids next to it)")
        contig = kc.is_contiguous() and vc.is_contiguous()
        # the native sequencer takes a prefill's rotary positions / first visible keys as well (crab_llama_io.pos_ids / kv_start); a general key
        # mask and the masked one-token step of forward() stay on the per-launch sequence below
        for nm, t in (("kv_start", kv_start), ("row_off", row_off)):
            # the kernels read these as int32 [B] through a raw pointer: an int64 or strided tensor would be misread silently
            if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < B or not t.is_contiguous() or t.device != x.device):
                raise ValueError(f"{nm} must be a contiguous int32 [B] tensor on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        native_ok = key_mask is None and (not masked or (vt is not None and pos_dev is None and
                                                         (pos_ids is None or (pos_ids.dtype == torch.int32 and pos_ids.stride(1) == 1))))
        last_rows = bool(last_rows) and vt is not None and S > 1 and key_mask is None and pos_dev is None
        # the sequencer takes the layer stride on its own (io.cache_layer_stride): the first rows of every layer of a larger allocation - the
        # cache of a wave that shed rows (_shed_to) - are a cache to it as long as the rows of a layer are packed
        packed = contig or (kc.dim() == 5 and kc.stride() == vc.stride() and kc[0].is_contiguous() and vc[0].is_contiguous())
        if prefix is None and not verify and NATIVE_LAYERS and not timed and native_ok and packed and (vt is not None or S == 1):
            self._layers_native(ws, B, S, kc, vc, b0, Tmax, pos0, pos_dev, vt, t0, row_off, pos_ids, kv_start, last_rows, kv_scales, w8)
            return x, h
        u_qkv = None                                   # router output for the q|k|v group when a producer epilogue made it
        # small batch: the projection leaves its raw row, ONE launch does RoPE + KV append + split-context attention (as csrc/llama_layer.hip)
        aw = self._attn_scratch(ws, B) if (vt is None and S == 1 and not masked and row_off is None and contig and kv_scales is None and prefix is None
                                           and not verify) else None
        fuse_attn = aw is not None and aw.numel() >= ops.attn_decode_rope_bytes(B, H, d)
        for li, layer in enumerate(layers):
            a, m = layer.self_attn, layer.mlp
            kcl, vcl = kc[li, b0:b0 + B], vc[li, b0:b0 + B]
            lcontig = kcl.is_contiguous()
            if t0:                                         # same strides, first slot t0: the kernels take the pointer and Tmax
                kcl, vcl = kcl[:, :, t0:], vcl[:, :, t0:]
            if last_rows and li + 1 == len(layers):
                self._last_layer_last_rows(ws, layer, B, S, kcl, vcl, lcontig, Tmax, pos0, vt, pos_ids, kv_start, u_qkv)
                return x, h
            if prefix is not None:
                # RoPE + KV append as their own pass: the rotary offset (prefix.rope_off) is not the first visible key (row_off) here
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv)
                ops.qkv_rope_split(qkv, tab, kcl, vcl, None, B, S, H, Hk, d, Tmax, pos0=pos0, pos_dev=pos_dev, pos_ids=pos_ids,
                                   row_off=prefix.rope_off if S == 1 else None)
            elif fuse_attn or kv_scales is not None:
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv, fp8=w8)
            elif verify:
                # the k + 1 rows of a verify step: RoPE + KV append as their own pass (slot = pos_dev + pos0 + s)
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv)
                ops.qkv_rope_split(qkv, tab, kcl, vcl, None, B, S, H, Hk, d, Tmax, pos0=pos0, pos_dev=pos_dev)
            elif vt is None and S == 1 and lcontig and not masked:
                # decode: RoPE + KV append ride on the q|k|v projection (fused into its split-K reduction when it has one)
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv, rope=(tab, kcl, vcl, H, Hk, d, Tmax, pos0, pos_dev), rope_row_off=row_off, fp8=w8)
            elif vt is not None and pos_dev is None and lcontig:
                # prefill: q and k rotate (and k lands in the cache) in the projection's epilogue when the library says so; the v columns
                # (cache append + V^T) are then all that is left for the split pass
                gi = {}
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv, rope=(tab, kcl, vcl, H, Hk, d, Tmax, pos0, None, S, pos_ids, vt), info=gi)
                if gi.get("fused_prefill_rope") == 2:
                    pass                                          # v-cache append and V^T written by the projection's epilogue as well
                elif gi.get("fused_prefill_rope") == 1:
                    ops.qkv_rope_split(qkv, None, None, vcl, vt, B, S, H, Hk, d, Tmax, pos0=pos0)
                else:
                    ops.qkv_rope_split(qkv, tab, kcl, vcl, vt, B, S, H, Hk, d, Tmax, pos0=pos0, pos_dev=pos_dev, pos_ids=pos_ids)
            else:
                a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv, fp8=w8)
                ops.qkv_rope_split(qkv, tab, kcl, vcl, vt, B, S, H, Hk, d, Tmax, pos0=pos0, pos_dev=pos_dev, pos_ids=pos_ids, row_off=row_off)
            if prefix is not None:
                ops.attn_prefix_partial(qkv, prefix.pk[li], prefix.pv[li], prefix.ws, prefix.tile_rows, prefix.row_clip, M, H, Hk, d, prefix.P, scale)
                ops.attn_own_merge(qkv, prefix.ws, kcl, vcl, att, B, S, H, Hk, d, Tmax, pos0 + 1, scale, ctx_dev=pos_dev,
                                   kv_start=row_off if S == 1 else kv_start)
            elif verify:
                ops.attn_verify(qkv, kcl, vcl, att, B, S, H, Hk, d, Tmax, pos0 + 1, scale, ctx_dev=pos_dev)
            elif vt is not None:
                Sp = vt.shape[-1]
                ops.attn_fwd(qkv, kcl, vt, att, q_strides=(S * ldq, d, ldq), k_strides=(Hk * Tmax * d, Tmax * d, d),
                             vt_strides=(Hk * d * Sp, d * Sp, Sp), o_strides=(S * H * d, H * d), B=B, H=H, Hk=Hk, Sq=S,
                             Skv=pos0 + S, head_dim=d, scale=scale, causal=True, kv_start=kv_start, key_mask=key_mask)
            elif kv_scales is not None:
                ops.attn_decode_fp8(qkv, tab, kcl, vcl, kv_scales[0][li, b0:b0 + B], kv_scales[1][li, b0:b0 + B], att, B, H, Hk, d, Tmax, pos0, scale,
                                    pos_dev=pos_dev, kv_start=row_off)
            elif fuse_attn:
                ops.attn_decode_rope(qkv, tab, kcl, vcl, att, B, H, Hk, d, Tmax, pos0, scale, pos_dev=pos_dev, workspace=aw)
            else:
                ops.attn_decode(qkv, kcl, vcl, att, B, H, Hk, d, Tmax, pos0 + 1, scale, ctx_dev=pos_dev,
                                kv_start=kv_start if row_off is None else row_off, key_mask=key_mask)
            # x += o_proj(att); h = rmsnorm(x) * post_attention_layernorm  (norm fused into the GEMM epilogue for small M)
            # (decode regime) the row-owning epilogue that produces h also evaluates the router of the group that consumes h
            ahead_gu = m._gu.routes_ahead(M)
            a._o(att, residual=x, out=x, t_buf=ws.t, u_buf=ws.u, post_norm=(layer.post_attention_layernorm.weight, c.rms_norm_eps, h),
                 route_next=(m._gu, ws.u2) if ahead_gu else None, fp8=w8)
            m._gu(h, out=act, t_buf=ws.t, u_buf=ws.u, act="swiglu_pair", u_ready=ws.u2 if ahead_gu else None, fp8=w8)   # silu(gate(h)) * up(h)
            # x += down(act); h = rmsnorm(x) * (next layer's input_layernorm | the final model.norm)
            last = li + 1 == len(layers)
            nxt = self.model.norm.weight if last else layers[li + 1].input_layernorm.weight
            nq = None if last else layers[li + 1].self_attn._qkv
            ahead_q = nq is not None and nq.routes_ahead(M)
            m._down(act, residual=x, out=x, t_buf=ws.t, u_buf=ws.u, post_norm=(nxt, c.rms_norm_eps, h),
                    route_next=(nq, ws.u2) if ahead_q else None, fp8=w8)
            u_qkv = ws.u2 if ahead_q else None
        return x, h

    def _last_layer_last_rows(self, ws, layer, B, S, kcl, vcl, lcontig, Tmax, pos0, vt, pos_ids, kv_start, u_qkv):
        """Per-launch form of crab_llama_io.last_rows_only (csrc/llama_layer.hip, same launches, same buffers): q|k|v for all rows, then the last
        row of every sequence through attention (one query row over the S cached keys), o_proj, the MLP and model.norm -> ws.h[0:B]."""
        c = self.cfg
        H, Hk, d = c.num_attention_heads, c.num_key_value_heads, c.head_dim
        D = c.hidden_size
        M = B * S
        a, m = layer.self_attn, layer.mlp
        h, qkv = ws.h[:M], ws.qkv[:M]
        tab = self._rope_tab(Tmax)
        ldq = qkv.stride(0)
        if lcontig:
            gi = {}
            a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv, rope=(tab, kcl, vcl, H, Hk, d, Tmax, pos0, None, S, pos_ids, vt), info=gi)
            if gi.get("fused_prefill_rope") == 1:
                ops.qkv_rope_split(qkv, None, None, vcl, None, B, S, H, Hk, d, Tmax, pos0=pos0)
            elif gi.get("fused_prefill_rope") != 2:
                ops.qkv_rope_split(qkv, tab, kcl, vcl, None, B, S, H, Hk, d, Tmax, pos0=pos0, pos_ids=pos_ids)
        else:
            a._qkv(h, out=qkv, t_buf=ws.t, u_buf=ws.u, u_ready=u_qkv)
            ops.qkv_rope_split(qkv, tab, kcl, vcl, None, B, S, H, Hk, d, Tmax, pos0=pos0, pos_ids=pos_ids)
        ql = ws.act[:B]
        ops.copy_rows(qkv[S - 1:], ql, B, H * d, lds=S * ldq)                      # the rotated q of the last rows
        attl = ws.att[:B]
        ops.attn_decode(ql, kcl, vcl, attl, B, H, Hk, d, Tmax, pos0 + S, 1.0 / math.sqrt(d), kv_start=kv_start)
        # the residual rows of the last tokens, gathered into qkv's storage
        x = ws.x[:M]
        words = 2 * D if x.dtype == torch.float32 else D
        xl = ws.qkv.view(-1)[: B * words].view(B, words)                          # bf16 words: [B, D] fp32 rows when the stream is fp32
        ops.copy_rows(x.view(BF16)[S - 1:], xl, B, words, lds=S * x.view(BF16).stride(0))
        xl = xl.view(x.dtype) if x.dtype == torch.float32 else xl
        hl, actl = ws.h[:B], ws.act[:B]
        ahead = m._gu.routes_ahead(B)
        a._o(attl, residual=xl, out=xl, t_buf=ws.t, u_buf=ws.u, post_norm=(layer.post_attention_layernorm.weight, c.rms_norm_eps, hl),
             route_next=(m._gu, ws.u2) if ahead else None)
        m._gu(hl, out=actl, t_buf=ws.t, u_buf=ws.u, act="swiglu_pair", u_ready=ws.u2 if ahead else None)
        m._down(actl, residual=xl, out=xl, t_buf=ws.t, u_buf=ws.u, post_norm=(self.model.norm.weight, c.rms_norm_eps, hl))

    # ------------------------------------------------------------------ prefill
    def prefill(self, embeds: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, b0: int = 0, all_logits: bool = False,
                logits_out: Optional[torch.Tensor] = None, hn_out: Optional[torch.Tensor] = None,
                pos_ids: Optional[torch.Tensor] = None, kv_start: Optional[torch.Tensor] = None, key_mask: Optional[torch.Tensor] = None,
                t0: int = 0, want_logits: bool = True):
        """embeds [B,S,D] bf16 -> (fp32 logits, post-final-norm hidden) of the LAST row ([B,V], [B,D]), or of all
        rows with all_logits ([B,S,V], [B,S,D]); fills cache rows b0..b0+B.  The reference computes lm_head on all
        S rows and discards S-1 of them (modeling_llama.py:1260); generate() only needs the last row
        (SURVEY.md appendix A.2).  want_logits = False (last-row form only): the caller wants the cache alone (the shared prefix of
        generate_shared_prefix) - no lm_head product, logits is None."""
        c = self.cfg
        B, S, D = embeds.shape
        Tmax = kc.shape[3]
        if S + t0 > Tmax:
            raise ValueError("prompt longer than the KV cache")
        M = B * S
        ws = self._workspace(M)
        ops.cast_rows(embeds.reshape(M, D), ws.x, M, D)          # bf16 inputs_embeds -> the (fp32) residual stream
        Sp = (S + 7) // 8 * 8
        vt = torch.empty((B, c.num_key_value_heads, c.head_dim, Sp), device=self.device, dtype=BF16)
        last_rows = (LAST_ROWS_ONLY and not all_logits and S > 1 and key_mask is None and
                     c.intermediate_size >= c.num_attention_heads * c.head_dim and c.intermediate_size % 8 == 0)      # (the q rows are staged in act's first B rows)
        x, hfin = self._layers(ws, B, S, kc, vc, b0, Tmax, 0, None, vt, pos_ids=pos_ids, kv_start=kv_start, key_mask=key_mask, t0=t0,
                               last_rows=last_rows)                       # hfin = model.norm(x): all rows, or the B last rows in hfin[0:B]
        if last_rows:
            hn = hn_out if hn_out is not None else torch.empty((B, D), device=self.device, dtype=BF16)
            ops.copy_rows(hfin, hn, B, D)
            logits = ops.gemm(hn, self.lm_head.weight, out=logits_out, out_fp32=True) if want_logits else None
            return logits, hn
        if all_logits:
            hn = hfin.clone()
            logits = ops.gemm(hn, self.lm_head.weight, out_fp32=True, prof_class="head")
            return logits.view(B, S, -1), hn.view(B, S, D)
        hn = hn_out if hn_out is not None else torch.empty((B, D), device=self.device, dtype=BF16)
        ops.copy_rows(hfin[S - 1:], hn, B, D, lds=S * D)                  # hn[b] = hfin[b*S + S-1]
        logits = ops.gemm(hn, self.lm_head.weight, out=logits_out, out_fp32=True) if want_logits else None
        return logits, hn

    # ------------------------------------------------------------------ teacher-forced scoring
    def key_visibility(self, attention_mask, B: int, T: int, width: int):
        """2-D attention_mask [B, T] over ALL keys (cached + new) -> (kv_start, key_mask) for the attention kernels, at most one of them set:
        nothing masked -> (None, None); left padding (zeros, then ones: what prepare_multimodal_inputs builds, unified_arch.py:344-348) ->
        int32 [B] index of the first visible key per sequence (whole key tiles below it are skipped); any other mask (holes anywhere: HF's
        mask utilities AND the padding mask with the causal one whatever its shape) -> int32 [B, ceil(width / 32)] visibility words
        (ops.pack_key_mask), `width` >= T bits wide (the cache capacity for the decode shortcut, whose context length travels as a device word).
        The one classification of a mask: forward() and score() both come here."""
        if attention_mask is None:
            return None, None
        m = attention_mask.to(torch.bool).reshape(B, -1)
        if m.shape[1] != T:
            raise ValueError(f"attention_mask covers {m.shape[1]} keys, expected {T} (cached + new tokens)")
        if bool(m.all()):
            return None, None
        start = (~m).sum(1)
        if bool((m == (torch.arange(T, device=m.device)[None] >= start[:, None])).all()):
            return start.to(device=self.device, dtype=torch.int32), None
        full = torch.zeros(B, max(width, T), dtype=torch.bool, device=m.device)
        full[:, :T] = m
        return None, ops.pack_key_mask(full).to(self.device)

    def rotary_positions(self, position_ids, B: int, S: int):
        """position_ids [B | 1, S] -> (contiguous int32 [B, S] on the device, the largest position: the caller grows the RoPE table to cover it)."""
        p = position_ids.reshape(-1, S)
        if p.shape[0] not in (1, B):
            raise ValueError(f"position_ids has {p.shape[0]} rows for a batch of {B}")
        lo, hi = int(p.min()), int(p.max())
        if lo < 0:
            raise ValueError("negative position_ids")
        return p.expand(B, S).to(device=self.device, dtype=torch.int32).contiguous(), hi

    def _xent_rows(self, h2d: torch.Tensor, row_idx: torch.Tensor, tgt: torch.Tensor, logprob, lse, argmax, r0: int, r1: int, ws):
        """The fused head over the labelled rows r0 .. r1 of the compacted problem: h2d[row_idx[r]] . lm_head^T against tgt[r]."""
        ops.lm_head_xent(h2d, self.lm_head.weight, tgt[r0:r1], row_idx=row_idx[r0:r1], logprob=logprob[r0:r1], lse=lse[r0:r1],
                         argmax=argmax[r0:r1], workspace=ws)

    def xent_from_hidden(self, hn: torch.Tensor, labels) -> "ScoreOutput":
        """The language-model loss of forward(labels=...) (modeling_llama.py:1261-1274) from the post-final-norm states hn [B, S, D] the logits
        were made from: shift by one, ignore -100, mean over all labelled tokens of the batch - through crab_lm_head_xent, no second logits pass
        in PyTorch."""
        B, S, D = hn.shape
        row_idx, tgt, seq_off = score_rows(labels, self.lm_head.weight.shape[0], (B, S))
        n = int(row_idx.shape[0])
        dev = self.device
        logprob = torch.empty((n,), device=dev, dtype=torch.float32)
        lse = torch.empty((n,), device=dev, dtype=torch.float32)
        argmax = torch.empty((n,), device=dev, dtype=torch.int32)
        tgt_d, seq_d = tgt.to(dev), seq_off.to(dev)
        if n:
            self._xent_rows(hn.reshape(B * S, D), row_idx.to(dev), tgt_d, logprob, lse, argmax, 0, n, None)
        s, nt, nc, mean = ops.xent_reduce(logprob, tgt_d, argmax, seq_d)
        return ScoreOutput(mean.reshape(()), s, nt, nc, None)

    def score(self, embeds: torch.Tensor, labels, attention_mask=None, position_ids=None, max_rows: Optional[int] = None,
              return_token_logprobs: bool = False) -> "ScoreOutput":
        """Teacher-forced scoring of embeds [B, S, D] against labels [B, S] (HF convention: unshifted, -100 ignored - the target of row t is
        labels[t + 1], so position 0 never scores): the prefill of forward() (every row through every layer on a scratch bf16 cache, the
        left-pad mask / position_ids honoured), then crab_lm_head_xent over the LABELLED rows of the final hidden states only.  Sequences are
        prefilled in chunks (plan_prefill_chunks under the device's memory budget; max_rows caps the rows of a chunk); nothing proportional to
        rows x vocabulary is allocated.  Returns ScoreOutput(loss = mean NLL over all labelled tokens (NaN when there is none), sum_logprob [B],
        num_tokens [B], num_correct [B] (argmax == label), token_logprobs = per sequence [n_i] fp32 when asked)."""
        return self._with_kv_mode("bf16", self._retry_after_eviction, self._score, embeds, labels, attention_mask, position_ids, max_rows,
                                  return_token_logprobs)

    def _score(self, embeds, labels, attention_mask, position_ids, max_rows, return_token_logprobs):
        c = self.cfg
        if embeds.dim() != 3 or embeds.shape[2] != c.hidden_size:
            raise ValueError(f"embeds must be [B, S, {c.hidden_size}], got {tuple(embeds.shape)}")
        B, S, D = embeds.shape
        V = self.lm_head.weight.shape[0]
        row_idx, tgt, seq_off = score_rows(labels, V, (B, S))
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError("max_rows must be positive")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        dev = self.device
        n = int(row_idx.shape[0])
        offs = seq_off.tolist()
        logprob = torch.empty((n,), device=dev, dtype=torch.float32)
        lse = torch.empty((n,), device=dev, dtype=torch.float32)
        argmax = torch.empty((n,), device=dev, dtype=torch.int32)
        tgt_d, seq_d = tgt.to(dev), seq_off.to(dev)
        if n:
            embeds = embeds.to(device=dev, dtype=BF16)
            Tmax = _round_up(S, 64)
            kv_start, key_mask = self.key_visibility(attention_mask, B, S, S)
            pos_ids = None
            if position_ids is not None:
                pos_ids, hi = self.rotary_positions(position_ids, B, S)
                self._rope_tab(max(hi + 1, Tmax))
            Hk, d, L = c.num_key_value_heads, c.head_dim, c.num_hidden_layers
            Sp = (S + 7) // 8 * 8
            # chunk rows: the caller's cap, then what the scratch cache + V^T of a chunk may claim of the device next to the activation set
            per_seq = self.kv_bytes_per_sequence(Tmax) + Hk * d * Sp * 2
            room = int(0.94 * self.memory_budget(B, Tmax)) - self.fixed_bytes(B, S)
            cap = min(int(max_rows) if max_rows is not None else 32768, max(1, room // per_seq) * S)
            chunks = self.plan_prefill_chunks(B, S, max(cap, S))
            cmax = max(1, min(B, cap // S))
            if max(chunks) > cmax:                            # below the ring-GEMM regime the planner answers with one chunk: the cap still holds
                chunks = [cmax] * (B // cmax) + ([B % cmax] if B % cmax else [])
            cmax = max(chunks)
            bounds = [0]
            for n_c in chunks:
                bounds.append(bounds[-1] + n_c)
            # chunk-local row indices (row b * S + t of the batch is row (b - b0) * S + t of its chunk), uploaded once
            local = row_idx.numpy().copy()
            for b0, b1 in zip(bounds, bounds[1:]):
                local[offs[b0]:offs[b1]] -= b0 * S
            local_d = torch.from_numpy(local).to(dev)
            kv = torch.empty((2, L * cmax * Hk * Tmax * d), device=dev, dtype=BF16)       # rows at or beyond the context are never read
            vt_buf = torch.empty((cmax * Hk * d * Sp,), device=dev, dtype=BF16)
            n_max = max(offs[b1] - offs[b0] for b0, b1 in zip(bounds, bounds[1:]))
            xws = torch.empty((ops.lm_head_xent_bytes(n_max, V),), device=dev, dtype=torch.uint8)
            for b0, b1 in zip(bounds, bounds[1:]):
                r0, r1 = offs[b0], offs[b1]
                if r0 == r1:
                    continue                                  # no labelled token in these sequences: nothing to prefill
                n_c = b1 - b0
                M = n_c * S
                shape = (L, n_c, Hk, Tmax, d)
                kc, vc = kv[0][:math.prod(shape)].view(shape), kv[1][:math.prod(shape)].view(shape)
                vt = vt_buf[:n_c * Hk * d * Sp].view(n_c, Hk, d, Sp)
                ws = self._workspace(M)
                ops.cast_rows(embeds[b0:b1].reshape(M, D), ws.x, M, D)
                _x, hfin = self._layers(ws, n_c, S, kc, vc, 0, Tmax, 0, None, vt,
                                        pos_ids=pos_ids[b0:b1] if pos_ids is not None else None,
                                        kv_start=kv_start[b0:b1] if kv_start is not None else None,
                                        key_mask=key_mask[b0:b1] if key_mask is not None else None)
                self._xent_rows(hfin, local_d, tgt_d, logprob, lse, argmax, r0, r1, xws)
        s, nt, nc, mean = ops.xent_reduce(logprob, tgt_d, argmax, seq_d)
        toks = [logprob[offs[b]:offs[b + 1]] for b in range(B)] if return_token_logprobs else None
        return ScoreOutput(mean.reshape(()), s, nt, nc, toks)

    # ------------------------------------------------------------------ decode
    def _constraints(self, constraint, counts: List[int], eos_token_id, min_new_tokens: int, flat: bool = False):
        """The `constraint` argument of generate() / generate_many() / generate_shared_prefix - (TokenTrie, set indices) or None - as one
        _Constraint per group of `counts` rows.  The set indices come as the rows come: one list per group, or (flat) one list for the one group
        (None: set 0 everywhere, an error when the trie holds several sets).  eos_token_id / min_new_tokens are checked against the trie (ValueError by
        name).  The device copies of the CSR arrays are made once per trie CONTENT and kept until invalidate(), so repeated calls with the same
        sets meet the same pointers and reuse the captured graph."""
        if constraint is None:
            return [None] * len(counts)
        from .constrain import TokenTrie, rows_of
        trie, sets = constraint if isinstance(constraint, (tuple, list)) else (constraint, None)
        if not isinstance(trie, TokenTrie):
            raise ValueError("constraint must be (TokenTrie, set indices) - crab_amd.constrain.as_trie builds one from id sequences")
        trie.check(eos_token_id, min_new_tokens, self.lm_head.weight.shape[0])
        if sets is not None and flat:
            sets = [sets]
        if sets is not None and len(sets) != len(counts):
            raise ValueError(f"allowed_set: {len(sets)} lists of set indices for {len(counts)} groups of rows")
        cache = self.__dict__.setdefault("_tries", {})
        dev = cache.get(trie.key)
        if dev is None or dev.edge_off.device != self.device:
            up = lambda a: torch.from_numpy(a.copy()).to(self.device)
            dev = types.SimpleNamespace(edge_off=up(trie.edge_off), edge_tok=up(trie.edge_tok), edge_dst=up(trie.edge_dst), n_nodes=trie.n_nodes,
                                        n_edges=trie.n_edges)
            dev.key = ("trie", dev.edge_off.data_ptr(), dev.edge_tok.data_ptr(), dev.edge_dst.data_ptr(), dev.n_nodes, dev.n_edges)
            cache[trie.key] = dev
        out = []
        for g, n in enumerate(counts):
            idx = rows_of(trie, None if sets is None else sets[g], n)
            out.append(_Constraint(dev, [int(trie.roots[i]) for i in idx]))
        return out

    def _decode_step(self, st: "_DecodeState"):
        """One greedy step entirely on device: embed(cur_ids) -> layers -> norm -> lm_head -> greedy select -> advance."""
        if st.lookup is not None:
            return self._lookup_step(st)
        c = self.cfg
        B = st.B
        ws = st.ws
        ops.embedding(st.cur_ids, self.model.embed_tokens.weight, out=ws.x[:B])
        x, hfin = self._layers(ws, B, 1, st.kc, st.vc, 0, st.Tmax, 0, st.pos_dev, None, row_off=st.row_off,
                               kv_scales=(st.ks, st.vs) if st.ks is not None else None, w8=st.w8, prefix=st.prefix)
        ops.gemm(hfin, self.lm_head.weight, out=st.logits)
        if st.want_hidden:
            ops.copy_rows(hfin, st.hn, B, hfin.shape[1])
        self._select(st)
        ops.advance(st.pos_dev, st.step_dev)

    def _lookup_step(self, st: "_DecodeState"):
        """One verify step of prompt-lookup decoding (generate_lookup), entirely on device: draft k tokens from the history -> embed
        [current ; drafts] -> layers over the k + 1 rows -> lm_head -> accept (1 .. k + 1 tokens emitted; pos / step advance by that many).
        A finished state runs the same launches and changes nothing, so the step loop and its EOS check are _run_steps' own."""
        lk = st.lookup
        M = lk.k + 1
        V = lk.logits.shape[1]
        ops.lookup_draft(lk.hist, st.S, st.step_dev, st.cur_ids, lk.k, lk.max_ngram, st.eos, st.pad, lk.max_new, V, lk.ids, lk.n_draft, st.finished)
        ops.embedding(lk.ids, self.model.embed_tokens.weight, out=st.ws.x[:M])
        x, hfin = self._layers(st.ws, 1, M, st.kc, st.vc, 0, st.Tmax, 0, st.pos_dev, None, verify=True)
        ops.gemm(hfin, self.lm_head.weight, out=lk.logits)
        ops.lookup_accept(lk.logits, lk.ids, lk.n_draft, st.cur_ids, st.out_ids, lk.hist, st.S, st.pos_dev, st.step_dev, st.finished, st.eos, st.pad,
                          st.min_new, lk.max_new, lk.stats, lk.step_logits)

    def _select(self, st: "_DecodeState"):
        """Next token of every row from st.logits: greedy (argmax) or, with st.sampling = (temperature, top_k, top_p, seed), HF's sample
        mode (temperature -> top-k -> top-p -> draw) - both device-resident, so the step stays capturable.  A sampling tuple that goes on with
        (min_p, epsilon_cutoff, eta_cutoff), at least one of them live, takes those three stages between top-p and the draw
        (ops.sample_select_warped); the values are part of the tuple and so of the state key.  A state with a token trie (st.trie:
        closed-set generation) takes both among the out-edges of every row's node instead (ops.constrained_select; st.node follows the edge).
        A state with st.lp (return_logprobs) also records the log-probability of the chosen token: the normalisers of the raw logits are taken
        BEFORE the select (it sets `finished` and moves st.node), the token's logit is gathered AFTER it (ops.logprob_norm / logprob_gather); the
        select itself is the same launch either way.
        A state with st.proc (processors: repetition penalty, n-gram ban, further stop ids) has the few logits they touch edited in place
        between the two (ops.logits_edit) and written back right after the select (ops.logits_restore, which also marks a row that emitted a
        further stop id as finished): the select chooses from the edited row, everything else - the logits a caller gets, both log-probability
        planes - sees the raw one.
        A state with st.beam (generate_beam) takes none of these: its select is the beam step (csrc/beam.hip).
        A state with st.cfg (generate_guided) takes none of these either: the select runs on the guided scores of its pairs (csrc/cfg.hip)."""
        if st.beam is not None:
            # beam search (generate_beam): the select is the beam step - the rows' best 2K continuations, the clip's merge (HF's steps c-g), then
            # the own cache rows follow their parents; `finished` carries the clip's done flag, so the EOS check of _run_steps works unchanged
            bs = st.beam
            ops.beam_row_topk(st.logits, bs, st.step_dev, st.finished, st.eos, st.min_new)
            ops.beam_merge(bs, st.logits.shape[1], st.step_dev, st.eos, st.cur_ids, st.out_ids, st.finished)
            ops.kv_beam_reorder(st.kc, st.vc, bs.K, bs.beam_idx, st.finished, st.pos_dev)
            return
        if st.cfg is not None:
            # classifier-free guidance (generate_guided; csrc/cfg.hip): rows 0 .. B - 1 are the conditional prompts, rows B .. 2B - 1 their
            # unconditional ones.  The guided scores of the pairs go to st.guided (the raw logits stay what the lm_head wrote), the ordinary
            # select runs on those B rows - a sampled row's stream is keyed by the clip's row index - and the unconditional rows take their
            # pair's token, so both embed it at the next step
            scale, Bc = st.cfg
            ops.cfg_mix(st.logits, st.guided, Bc, scale, st.finished)
            self._select_token(st, st.guided)
            ops.cfg_follow(st.cur_ids, st.out_ids, st.finished, st.step_dev, Bc)
            return
        if st.lp is not None:
            tr = st.trie
            ops.logprob_norm(st.logits, st.step_dev, st.finished, st.eos, st.min_new, st.lp_norm, tr.edge_off if tr is not None else None,
                             tr.edge_tok if tr is not None else None, st.node)
        if st.proc is not None:
            p, n, _ = st.proc
            ops.logits_edit(st.logits, st.out_ids, st.step_dev, st.finished, p, n, st.stop_dev, st.min_new, st.save_idx, st.save_val)
        self._select_token(st)
        if st.proc is not None:
            ops.logits_restore(st.logits, st.cur_ids, st.finished, st.stop_dev, st.save_idx, st.save_val)
        if st.lp is not None:
            ops.logprob_gather(st.logits, st.cur_ids, st.step_dev, st.lp_norm, st.lp)

    def _select_token(self, st: "_DecodeState", logits=None):
        """logits: the scores to choose from when they are not st.logits - a guided state's st.guided, whose B rows are the FIRST rows of the
        state: the select then writes those rows' words."""
        logits = st.logits if logits is None else logits
        if st.trie is not None:
            t, k, p_, seed = st.sampling if st.sampling is not None else (0.0, 0, 1.0, 0)      # never a 7-tuple: normalize_sampling refuses it
            ops.constrained_select(logits, st.trie.edge_off, st.trie.edge_tok, st.trie.edge_dst, st.node, st.cur_ids, st.out_ids, st.step_dev,
                                   st.finished, st.eos, st.pad, st.min_new, t, k, p_, seed + 7919 * st.slot)
        elif st.sampling is None:
            ops.greedy_select(logits, st.cur_ids, st.out_ids, st.step_dev, st.finished, st.eos, st.pad, st.min_new)
        elif st.rows is not None:
            # the child state of a wave that shed rows (_shed_to): every row draws under the index it had in the whole wave, so the random
            # stream is the unshed call's; one entry for both tuple forms (it picks the plain or the warped pipeline itself)
            t, k, p_, seed = st.sampling[:4]
            ops.sample_select_rows(st.rows, logits, st.cur_ids, st.out_ids, st.step_dev, st.finished, st.eos, st.pad, st.min_new, t, k, p_,
                                   seed + 7919 * st.slot, *st.sampling[4:])
        elif len(st.sampling) == 4:
            t, k, p_, seed = st.sampling
            ops.sample_select(logits, st.cur_ids, st.out_ids, st.step_dev, st.finished, st.eos, st.pad, st.min_new, t, k, p_, seed + 7919 * st.slot)
        else:
            # a live min_p / epsilon_cutoff / eta_cutoff (normalize_sampling: a 7-tuple holds at least one): csrc/sample.hip
            t, k, p_, seed, min_p, eps, eta = st.sampling
            ops.sample_select_warped(logits, st.cur_ids, st.out_ids, st.step_dev, st.finished, st.eos, st.pad, st.min_new, t, k, p_,
                                     seed + 7919 * st.slot, min_p, eps, eta)

    def _state(self, B: int, S: int, req: _Request, slot: int = 0, ragged: bool = False) -> "_DecodeState":
        """The persistent decode state of `slot` for B sequences whose (longest) prompt has S rows: KV cache, per-row words, logits and the HIP
        graph captured over them.  Kept per slot and reused by every call whose shapes, flags and buffers are the same: the key (_state_key)
        holds everything the captured launches bake in (pointers included).  ragged: the state of a coalesced batch
        (generate_many(coalesce=True)) - it owns a row_off word per row (first cache slot of the row's sequence) that the captured decode step
        reads.  The fields of `req` it reads, beside the plain ones:  extra_key: what else a caller's captured step bakes in
        (generate_shared_prefix: the prefix cache, its length, the tile plan and the workspace).  constraint: the rows' _Constraint (closed-set
        generation) - the trie's device pointers enter the key, so a captured graph never crosses tries, and every call puts the rows back on
        their roots.  return_logprobs: the state owns st.lp [2, B, max_new_tokens] fp32 (plane 0: log-probability of every emitted token over the
        whole vocabulary, plane 1: within the allowed set; zeroed by every call like out_ids) and st.lp_norm [B, 4], and _select fills them;
        the flag is part of the key, so a graph captured without the two launches is never replayed for a call that wants them.
        processors: (repetition_penalty, no_repeat_ngram_size, stop_token_ids) or None - a non-neutral triple owns st.save_idx / st.save_val
        (the save area of crab_logits_edit / crab_logits_restore) and st.stop_dev, and its values enter the key in the same way.
        cfg: (guidance_scale, pairs) or None - classifier-free guidance (generate_guided): the B = 2 * pairs rows are the conditional rows and
        then their unconditional ones, the state owns st.guided [pairs, V] fp32 (the scores the select reads, crab_cfg_mix) and _select
        takes the guided route.  The scale is baked into the captured launch, so both values enter the key; st.guided is born with the
        state and dies with it.
        lookup: (k, max_ngram, keep step logits) or None - prompt-lookup decoding (generate_lookup, B == 1): a verify step appends k + 1 cache rows
        and runs k + 1 rows through the layers, so Tmax = round_up(S + max_new_tokens + k, 64), the decode workspace is made for k + 1 rows and
        the logits buffer holds k + 1 rows (st.logits, what the prefill and the first select use, is its first row).  The state owns st.lookup
        (_Lookup: history, draft ids, counters).  All three values enter the key, and so does S: the history is sized S + max_new_tokens and the
        captured draft / accept launches bake S in as a host integer (a plain state meets S only through pos_dev; Tmax alone would let two
        prompt lengths of one 64-row bucket share a state)."""
        max_new_tokens, constraint, cfg, lookup = req.max_new_tokens, req.constraint, req.cfg, req.lookup
        if int(max_new_tokens) < 1:                             # HF: GenerationConfig.validate() - "`max_new_tokens` must be greater than 0"; here the first token's slot would not exist
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new_tokens}.")
        dev = self.device
        lk_rows = (int(lookup[0]) + 1) if lookup is not None else 1
        Tmax = _round_up(S + max_new_tokens + lk_rows - 1, 64)
        kv = self.alloc_cache(B, Tmax, slot=slot)
        kc, vc = kv[0], kv[1]
        ks, vs = (kv[2], kv[3]) if len(kv) == 4 else (None, None)          # fp8 mode: the row scales beside the codes
        V = self.lm_head.weight.shape[0]
        # the pad word falls back to the first further stop id as well (stop_words): NOT _Request.join_pad, which says why the two differ
        eos, proc, pad = stop_words(req.eos, req.pad_token_id, req.processors)
        stops = proc[2] if proc is not None else ()
        if proc is not None and int(max_new_tokens) > ops.LOGITS_PROC_MAX_STEPS:
            raise NotImplementedError(f"processors with max_new_tokens = {max_new_tokens}: crab_logits_edit holds at most {ops.LOGITS_PROC_MAX_STEPS} generated tokens")
        ws = self._workspace(B * lk_rows, slot, decode=True)
        tab = self._rope_tab(Tmax)
        # the weight mode of this state's decode steps; the FP8 forms are (re)built here, before any capture, and their pointers enter the key
        w8, w8_key = self._w8_rows(B), self._w8_key(B)
        self._w_used = "bf16" if (not w8 or self._w_used == "bf16") else "fp8_e4m3"
        qkv0 = self.model.layers[0].self_attn._qkv
        key = _state_key(B, Tmax, max_new_tokens, eos, pad, req.min_new_tokens, req.return_hidden,
                         (kc.data_ptr(), vc.data_ptr(), id(ws), tab.data_ptr(), self.lm_head.weight.data_ptr(),
                          self.model.embed_tokens.weight.data_ptr(), qkv0.W.data_ptr()), qkv0.RA is not None, req.sampling, ragged, self._kv_mode,
                         (ks.data_ptr(), vs.data_ptr()) if ks is not None else (0, 0), w8_key, req.return_logprobs, req.extra_key,
                         constraint.dev.key if constraint is not None else (), proc, cfg, lookup, S)
        st = self._dec.get(slot)
        if st is None or st.key != key:
            st = _DecodeState()
            st.key = key
            st.B, st.Tmax, st.kc, st.vc, st.slot, st.ws = B, Tmax, kc, vc, slot, ws
            st.ks, st.vs = ks, vs
            st.w8 = w8
            if lookup is not None:
                st.lookup = _Lookup(dev, S, int(max_new_tokens), int(lookup[0]), int(lookup[1]), V, bool(lookup[2]))
            st.alloc(dev, B, max_new_tokens, V, ragged, logits=st.lookup.logits[:B] if lookup is not None else None)
            st.hn = torch.empty((B, self.cfg.hidden_size), device=dev, dtype=BF16)
            st.eos, st.pad, st.min_new, st.want_hidden = eos, pad, int(req.min_new_tokens), bool(req.return_hidden)
            st.sampling = req.sampling
            if constraint is not None:
                st.trie, st.node = constraint.dev, torch.empty((B,), device=dev, dtype=torch.int32)
            if req.return_logprobs:
                st.lp = torch.empty((2, B, max_new_tokens), device=dev, dtype=torch.float32)
                st.lp_norm = torch.zeros((B, 4), device=dev, dtype=torch.float32)
            # processors: the save area of crab_logits_edit / crab_logits_restore and the device copy of the further stop ids.  The buffers are
            # born with the state and die with it, so the values in the key stand for their pointers as well
            st.proc, st.eos_all = proc, (eos,) + stops
            if proc is not None:
                n_slots = 2 * int(max_new_tokens) + len(stops)
                st.save_idx = torch.full((B, n_slots), -1, device=dev, dtype=torch.int32)
                st.save_val = torch.zeros((B, n_slots), device=dev, dtype=torch.float32)
            st.stop_dev = torch.tensor(stops, dtype=torch.int32).to(dev) if stops else None
            if cfg is not None:
                st.cfg, st.guided = (float(cfg[0]), int(cfg[1])), torch.empty((int(cfg[1]), V), device=dev, dtype=torch.float32)
            # shed_finished: the child states of this state, (rows, weight form) -> _DecodeState (_shed_to).  They live and die with their
            # parent - its key stands for everything theirs bake in - so invalidate() and a changed key drop them with it
            st.children = {}
            self._dec[slot] = st
        st.S = S
        st.cur_ids.zero_(); st.out_ids.fill_(req.pad_token_id if req.pad_token_id is not None else 0); st.finished.zero_()
        st.pos_dev.fill_(S - 1); st.step_dev.zero_()
        if st.lp is not None:
            st.lp.zero_()
        if st.lookup is not None:
            st.lookup.reset(pad)
        if constraint is not None:
            assert len(constraint.roots) == B, "one trie root per row"
            st.node.copy_(torch.tensor(constraint.roots, dtype=torch.int32))
        return st

    def _prefill_chunk(self, st: "_DecodeState", emb: torch.Tensor, b0: int, t0: int = 0, pos_ids=None, kv_start=None):
        """Prefill the sequences b0 .. b0 + n of a decode state (first logits / hidden rows into st.logits / st.hn).  bf16 mode: straight into the
        cache at slots t0 ...  fp8 mode: exactly the same prefill into the bf16 staging block (slots 0 ..; the first token's logits equal the
        bf16 mode's bit for bit), then crab_kv_quant_fp8 moves the rows to slots t0 .. of the fp8 cache; kv_start (the front padding of a merged
        ragged wave) doubles as the quantiser's row_off: the padded rows are neither read nor written."""
        n, S = emb.shape[0], emb.shape[1]
        lo, hn = st.logits[b0:b0 + n], st.hn[b0:b0 + n]
        if st.ks is None:
            self.prefill(emb, st.kc, st.vc, b0=b0, logits_out=lo, hn_out=hn, pos_ids=pos_ids, kv_start=kv_start, t0=t0)
            return
        sk, sv = self._staging(n, S)
        self.prefill(emb, sk, sv, b0=0, logits_out=lo, hn_out=hn, pos_ids=pos_ids, kv_start=kv_start)
        ops.kv_quant_fp8(sk, sv, st.kc, st.vc, st.ks, st.vs, b0=b0, t0=0, t_dst=t0, S=S, row_off=kv_start)

    def _start(self, embeds: torch.Tensor, req: _Request, slot: int = 0, sink=None) -> "_DecodeState":
        """Allocate the decode state of one group of sequences, prefill it and select its first token."""
        B, S, D = embeds.shape
        st = self._state(B, S, req, slot)
        # ---- prefill in chunks of sequences (bounds activation memory, keeps GEMM M in the MFMA-efficient range)
        prefill_chunk = req.prefill_chunk
        chunks = self.plan_prefill_chunks(B, S) if not prefill_chunk else [prefill_chunk] * (B // prefill_chunk) + \
            ([B % prefill_chunk] if B % prefill_chunk else [])
        b0 = 0
        for n in chunks:
            self._prefill_chunk(st, embeds[b0:b0 + n], b0)
            b0 += n
        return self._first_token(st, sink)

    def _first_token(self, st: "_DecodeState", sink=None) -> "_DecodeState":
        """The tail of every start: the prefill's logits / hidden rows to the sink, then the first token selected from them."""
        if sink is not None:
            sink(st)
        self._select(st)
        ops.advance(st.pos_dev, st.step_dev)           # pos: S-1 -> S (the slot of the token just selected; Smax-1 -> Smax in a ragged state), step: 0 -> 1
        return st

    def _prefill_groups(self, st, embeds_list, Bs, Ss, Smax):
        """Per-group prefill into the right-aligned cache: spans of consecutive groups with the same prompt length share one chunk plan (whole
        rounds of 256 x 256 tiles, plan_prefill_chunks); the cache pointers are advanced by the span's offset (t0), nothing else changes."""
        g = 0
        b0 = 0
        while g < len(embeds_list):
            g1 = g
            while g1 + 1 < len(embeds_list) and Ss[g1 + 1] == Ss[g]:
                g1 += 1
            span = embeds_list[g:g1 + 1]
            n_span = sum(Bs[g:g1 + 1])
            starts = [0]
            for e in span:
                starts.append(starts[-1] + e.shape[0])
            c0 = 0
            for n in self.plan_prefill_chunks(n_span, Ss[g]):
                pieces = []
                for j, e in enumerate(span):                  # the rows c0 .. c0 + n of the span, from whichever groups hold them
                    lo, hi = max(c0, starts[j]), min(c0 + n, starts[j + 1])
                    if lo < hi:
                        pieces.append(e[lo - starts[j]:hi - starts[j]])
                emb = pieces[0] if len(pieces) == 1 else torch.cat(pieces, 0)
                self._prefill_chunk(st, emb, b0 + c0, t0=Smax - Ss[g])
                c0 += n
            b0 += n_span
            g = g1 + 1

    def _start_ragged(self, embeds_list: List[torch.Tensor], req: _Request, sink=None) -> "_DecodeState":
        """The decode state of SEVERAL generate() calls coalesced into one batch.  Group g = [B_g, S_g, D] is one call of the eval loop: its
        own prompt length and left padding, positions 0 .. S_g - 1 (unified_llama.py:262-267).  All rows share one KV cache [L, sum B_g, Hk,
        Tmax, d] in which every group is RIGHT-ALIGNED at Smax = max S_g: group g's prompt occupies slots Smax - S_g .. Smax - 1, so the token
        decoded at step t lands in slot Smax + t - 1 for every row (one device-resident append index, one captured graph), while row_off[row]
        = Smax - S_g gives the decode kernels the row's rotary offset and its first visible key.  Prefill: groups of ONE length are prefilled
        exactly as generate() prefills them (shared chunks, the cache pointers advanced by row_off: _prefill_groups); groups of different
        lengths as one front-padded batch under forward()'s left-pad mask + position_ids (merged form below) unless the padding would cost
        more than RAGGED_PAD_MAX of the rows."""
        Bs = [int(e.shape[0]) for e in embeds_list]
        Ss = [int(e.shape[1]) for e in embeds_list]
        Bt, Smax = sum(Bs), max(Ss)
        st = self._state(Bt, Smax, req, 0, ragged=True)
        st.row_off.copy_(torch.tensor([Smax - S for B, S in zip(Bs, Ss) for _ in range(B)], dtype=torch.int32), non_blocking=False)
        waste = sum(B * (Smax - S) for B, S in zip(Bs, Ss)) / max(1, sum(B * S for B, S in zip(Bs, Ss)))
        if len(set(Ss)) > 1 and waste <= RAGGED_PAD_MAX:
            # MERGED prefill (batches of different lengths, the normal case of a real question set): every sequence is padded IN FRONT to Smax
            # rows (zero rows: never attended, their outputs never read), its real tokens keep the rotary positions 0 .. S_g - 1 (pos_ids) and
            # see no key below their own first row (kv_start = row_off) - forward()'s left-pad mask + position_ids, which both prefill kernels
            # take (crab_llama_io.pos_ids / kv_start) - so the chunks are planned over ALL rows of the wave (whole rounds of 256 x 256 tiles,
            # as for one large generate()) instead of per batch of 8 (22 row tiles: 4.1 / 1.4 / 7.4 rounds).  The cache rows land right-aligned
            # by construction.  Cost: the (Smax - S_g) padded rows, `waste` of the prefill work (a few % at most, else the per-group form below).
            D = embeds_list[0].shape[2]
            emb = torch.zeros((Bt, Smax, D), device=self.device, dtype=BF16)
            r0 = 0
            for e, B, S in zip(embeds_list, Bs, Ss):
                emb[r0:r0 + B, Smax - S:] = e
                r0 += B
            pos_ids = (torch.arange(Smax, device=self.device, dtype=torch.int32)[None] - st.row_off[:, None]).clamp_(min=0).contiguous()
            self._rope_tab(st.Tmax)
            b0 = 0
            for n in self.plan_prefill_chunks(Bt, Smax):
                self._prefill_chunk(st, emb[b0:b0 + n], b0, pos_ids=pos_ids[b0:b0 + n], kv_start=st.row_off[b0:b0 + n])
                b0 += n
            del emb
            self.last_ragged_prefill = "merged"
        else:
            self.last_ragged_prefill = "per_group"
            self._prefill_groups(st, embeds_list, Bs, Ss, Smax)
        return self._first_token(st, sink)

    def _retry_after_eviction(self, fn, *a, **k):
        """memory_budget() counts the KV caches of stale slots (left by an earlier generate_many / decode_streams > 1) as reclaimable, but
        only a KV allocation evicts them (_evict_for); a later allocation planned against that budget - prefill workspace, logits, the merged
        ragged `emb` - could run out of memory beside them.  One retry: on an out-of-memory error every slot, decode state, graph and workspace is
        dropped (the call rebuilds what it needs) and the call runs once more; a second failure is the caller's."""
        try:
            return fn(*a, **k)
        except torch.cuda.OutOfMemoryError:
            if not (self._kv or self._dec or self._ws):
                raise
        # the retry runs OUTSIDE the except clause: inside it the exception's traceback keeps the failed attempt's frames - and the tensors they hold - alive
        import gc
        self.invalidate()
        gc.collect()
        torch.cuda.empty_cache()
        return fn(*a, **k)

    @torch.no_grad()
    def generate(self, embeds: torch.Tensor, max_new_tokens: int, eos_token_id: Optional[int] = None,
                 pad_token_id: Optional[int] = None, min_new_tokens: int = 0, prefill_chunk: int = 0, use_graph: bool = True,
                 return_step_logits: bool = False, return_hidden: bool = False, decode_streams: int = 1,
                 return_first_logits: bool = False, sampling=None, kv_cache_dtype: Optional[str] = None, weight_dtype: Optional[str] = None,
                 constraint=None, return_logprobs: bool = False, processors=None, shed_finished=None, shed_every: Optional[int] = None):
        """kv_cache_dtype / weight_dtype: "bf16" / "fp8_e4m3" for this call (None: the engine's); see _generate for the rest.
        shed_finished (opt-in; None / False: off, the call is the call without the argument): a wave stops carrying the rows that have
        emitted EOS.  True: the default ladder (shed_default_ladder), a sorted tuple of row counts: that ladder.  Every shed_every steps
        (default EOS_CHECK_EVERY) the EOS check reads the `finished` vector; when the unfinished rows fit a smaller rung B', their cache rows
        move to the front in place (crab_kv_compact_rows) and a child state of B' rows steps on (_shed_to) - the attention stops reading the
        finished rows' keys and the projections run at B' rows.  The result is the unshed call's: same shape, trimming and padding; the
        surviving rows run the kernels B' selects, so ids / logits agree within the decoder's bf16 bound, not bit for bit (the rule of
        coalesce and decode_streams); sample mode keeps every row's random stream (crab_sample_select_rows).  return_step_logits holds zeros
        where a row had been shed.  last_plan["shed"] = [(step, rows_before, rows_after, rows_moved)], last_plan["shed_captures"] = graphs
        captured by the call.  Refused by name (check_shed): constraint, processors, return_logprobs, return_hidden, decode_streams > 1,
        kv_cache_dtype="fp8_e4m3".
        processors = (repetition_penalty, no_repeat_ngram_size, stop_token_ids) or None: HF's RepetitionPenaltyLogitsProcessor and
        NoRepeatNGramLogitsProcessor over the GENERATED tokens (generate() with inputs_embeds starts HF from an empty input_ids, so the prompt
        never enters them) and stop ids BEYOND eos_token_id (HF's list-valued eos_token_id: any of them finishes a row, min_new_tokens
        suppresses all of them, finished rows emit pad_token_id - by default eos_token_id, the first id).  Applied inside the decode step
        (csrc/logits_proc.hip: the touched logits are edited in place before the select and restored after it), greedy and sample mode alike
        (sample mode: before the warpers, HF's order); return_step_logits and return_logprobs keep reporting the RAW logits.  Neutral values
        (1.0, 0, no ids) are the call without the argument.  Refused by name (check_processors): return_logprobs with no_repeat_ngram_size or
        with stop_token_ids under min_new_tokens, constraint with stop_token_ids or no_repeat_ngram_size.
        constraint = (TokenTrie, one set index per row or None): closed-set generation (crab_amd/constrain.py) - every row's ids, cut at EOS,
        are a member of the row's answer set; greedy and sample mode both choose among the trie's edges on the device, everything else (KV and
        weight modes, EOS trim, padding of finished rows) is unchanged.  A row that max_new_tokens cuts in the middle of an answer holds a
        proper prefix of a member, as HF's constrained decode does.
        return_logprobs: the result gains, as its LAST element, an fp32 tensor [B, n, 2] beside the ids [B, n]: [..., 0] the log-probability of every
        emitted token over the whole vocabulary (raw logits: no EOS suppression, no temperature, no trie - the number score() gives teacher-forced
        on the same ids), [..., 1] the same within the set the step chose from (all but EOS while min_new_tokens holds; the trie's edges in a
        constrained call) - HF's compute_transition_scores(normalize_logits=True) of a greedy call.  0.0 where the row emitted no token
        (padding after its EOS; the EOS column itself is a token).  Sample mode: the warpers are a drawing device and enter neither number
        (HF's warped `scores` are not reproduced).  Written inside the decode step (csrc/logprob.hip): no host sync, nothing of size B x V kept."""
        sampling = normalize_sampling(sampling, constraint is not None)
        proc = check_processors(processors, min_new_tokens, constraint is not None, return_logprobs, eos_token_id)      # refused before any device work
        plan = check_shed(shed_finished, shed_every, constraint, proc, return_logprobs, return_hidden, decode_streams,
                          self._kv_mode if kv_cache_dtype is None else self.check_kv_cache_dtype(kv_cache_dtype))
        cons, = self._constraints(constraint, [int(embeds.shape[0])], eos_token_id, min_new_tokens, flat=True)
        req = _Request(max_new_tokens, one_eos(eos_token_id, ONE_EOS), pad_token_id, min_new_tokens, use_graph, sampling, proc, return_step_logits,
                       return_hidden, return_first_logits, return_logprobs, prefill_chunk, _Shed(*plan) if plan is not None else None, cons)
        return self._call(kv_cache_dtype, weight_dtype, req.shed, self._generate, embeds, req, decode_streams)

    def _run_steps(self, sts: List["_DecodeState"], req: _Request, side_streams: bool, retire: bool, on_step=None, sampled_step=None):
        """The decode steps 1 .. max_new_tokens - 1 of started states (step 0, the first token, is _start's): THE step loop of the engine.
        req.graphed: every state's step is captured under its own scratch slot (or its graph reused, _capture) and replayed; else the step runs
        eagerly.  side_streams: every state steps on a HIP stream of its own, forked from the current stream before the first step and joined
        to it after the last; else all steps go to the current stream.  The loop holds no host synchronisation but the EOS check: every
        EOS_CHECK_EVERY steps (a lookup state: every step) the `finished` flags are read, and
          retire = True:  a state whose rows have all finished stops stepping (generate_many: HF stops that call);
          retire = False: every state keeps stepping until ALL of them have finished (generate(decode_streams > 1): the groups are one call,
                          their buffers are joined column by column).
        on_step(sts[0]) runs after every step.  sampled_step(step, sts[0]) is asked before every graphed step of the FIRST state and returns
        True when it has run that step itself (bench.py's roofline sampling); the state is device-resident, so replays continue after it.
        req.shed (shed_finished; ONE state on the current stream): the EOS check reads the `finished` vector instead of its .all() - still the
        loop's only synchronisation, every shed.every steps - and when the unfinished rows fit a smaller rung of the ladder, sts[0] is
        replaced IN THE LIST by the child state that carries them on (_shed_to).  The ids of the whole wave are then in shed.out."""
        max_new_tokens, graphed, shed = req.max_new_tokens, req.graphed, req.shed
        main = torch.cuda.current_stream()
        graphs, streams = [], []
        if shed is not None:
            assert len(sts) == 1 and not side_streams and sts[0].lookup is None, "a shedding wave is one state on the current stream"
            shed.out, root = None, sts[0]
        for st in sts:
            with _ws_slot(st.slot):
                if shed is not None and graphed and st.graph is None:
                    shed.captures += 1
                graphs.append(self._capture(st) if graphed else None)
            streams.append(torch.cuda.Stream() if side_streams else main)
        if side_streams:
            for sg in streams:
                sg.wait_stream(main)
        eos_on = any(e >= 0 for e in sts[0].eos_all) or sts[0].lookup is not None      # a lookup state finishes early by max_new_tokens as well
        # a verify step of a lookup state emits up to k + 1 tokens, so the call can end at ANY step, and every step past its end is a whole
        # (k + 1)-row pass over the weights that changes nothing: such a state is read after every step (one 4-byte read against a >= 4 ms step)
        check_every = 1 if sts[0].lookup is not None else (shed.every if shed is not None else EOS_CHECK_EVERY)
        live = list(range(len(sts)))
        for step in range(1, max_new_tokens):
            for g in live:
                with torch.cuda.stream(streams[g]):
                    if graphs[g] is None:
                        with _ws_slot(sts[g].slot):
                            self._decode_step(sts[g])
                    elif not (g == 0 and sampled_step is not None and sampled_step(step, sts[0])):
                        graphs[g].replay()
            if on_step is not None:
                on_step(sts[0])
            if eos_on and step % check_every == 0 and shed is not None:
                fin = sts[0].finished.tolist()                 # the one read of this look (the fillers of a rung are finished by construction)
                rows_live = [i for i, f in enumerate(fin) if not f]
                if not rows_live:
                    break
                Bp = shed_rung(shed.ladder, len(rows_live), sts[0].B)
                # a shed costs about three steps of what it saves per step: near the end of the call it is pure loss
                if Bp is not None and max_new_tokens - 1 - step >= SHED_MIN_STEPS_LEFT:
                    if shed.out is None:
                        shed.out = torch.empty_like(root.out_ids)
                    sts[0] = self._shed_to(root, sts[0], rows_live, Bp, shed, step)
                    with _ws_slot(sts[0].slot):
                        if graphed and sts[0].graph is None:
                            shed.captures += 1
                        graphs[0] = self._capture(sts[0]) if graphed else None
            elif eos_on and step % check_every == 0:
                still = []
                for g in live:
                    if still and not retire:
                        break                                  # one unfinished state keeps all of them stepping: the others need not be read
                    with torch.cuda.stream(streams[g]):
                        if not bool(sts[g].finished.all().item()):
                            still.append(g)
                if not still:
                    break
                if retire:
                    live = still
        if shed is not None and sts[0].rows is not None:
            self._shed_flush(sts[0], shed, 0)                  # the rows that stepped to the end
        if side_streams:
            for sg in streams:
                main.wait_stream(sg)

    def _generate(self, embeds: torch.Tensor, req: _Request, decode_streams: int = 1):
        """Greedy generation from inputs_embeds only, as UnifiedForCausalLM.generate drives HF generate
        (unified_llama.py:262-267): positions 0..S-1 (left pads attended), returns ONLY new ids.

        sampling = (temperature, top_k, top_p, seed): HF sample mode instead of greedy (what the reference actually runs with a Llama-2-chat
        checkpoint, whose generation_config sets do_sample); None = greedy.  With three more entries,
        (..., seed, min_p, epsilon_cutoff, eta_cutoff), HF's further truncation warpers run between top-p and the draw (normalize_sampling;
        0 / None = off, all three off is the 4-tuple's call; refused by name with a constraint).

        return_first_logits: also return the fp32 last-row logits of the prefill ([B, V], one clone per call: what the multi-GPU
        eval gathers next to the ids, crab_amd/parallel.py) without keeping every step's logits.

        decode_streams > 1 splits the batch into that many groups whose decode steps (one HIP graph each) replay on
        separate HIP streams: the HBM-bound KV-cache attention of one group overlaps the MFMA-bound projections of
        another.  Rows never interact, so the split only changes which M the projection kernels see."""
        B, S, D = embeds.shape
        groups = self.plan_batch(B, S, req.max_new_tokens, slots=max(1, decode_streams))
        if len(groups) > 1:
            return self._generate_split(groups, embeds, req)
        G = decode_streams if (decode_streams > 1 and req.graphed and B >= decode_streams and
                               not req.return_step_logits and not req.return_hidden) else 1
        sink = _Collect(req, G, B)

        def sampled_step(step, st):
            # roofline sampling (bench.py): this step runs the same launches eagerly with HIP events around the decode-attention kernel
            prof = ops.PROFILER
            if prof is None or not prof.decode_every or step % prof.decode_every != prof.decode_every // 2:
                return False
            with _ws_slot(st.slot):
                prof.decode_eager, prof.decode_ctx = True, S + step
                self._decode_step(st)
                prof.decode_eager = False
            return True

        sts = []
        for g in range(G):
            with _ws_slot(g):
                b0, b1 = B * g // G, B * (g + 1) // G
                sts.append(self._start(embeds[b0:b1], req.rows(b0, b1), g, sink))
        if ops.PROFILER is not None:
            ops.PROFILER.mark("prefill_end")
        # the groups are ONE call: all of them step until all have finished (a retired group's buffer would hold the fill value, not its pad id)
        self._run_steps(sts, req, G > 1, False, sink, sampled_step)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("decode_end")
        n_done = int(sts[0].step_dev.item())
        if req.shed is not None and req.shed.out is not None:         # the wave shed rows: its ids were assembled under the rows' original indices
            ids = req.shed.out
        else:
            ids = sts[0].out_ids if G == 1 else torch.cat([st.out_ids for st in sts], 0)
        return sink.whole(sts, _trim_at_eos(ids, n_done, sts[0].eos_all))

    @torch.no_grad()
    def generate_many(self, embeds_list: List[torch.Tensor], max_new_tokens: int, eos_token_id: Optional[int] = None,
                      pad_token_id: Optional[int] = None, min_new_tokens: int = 0, use_graph: bool = True, sampling=None,
                      return_first_logits: bool = False, coalesce: bool = False, max_rows: Optional[int] = None,
                      return_step_logits: bool = False, return_hidden: bool = False, kv_cache_dtype: Optional[str] = None,
                      weight_dtype: Optional[str] = None, constraint=None, return_logprobs: bool = False, processors=None, shed_finished=None,
                      shed_every: Optional[int] = None):
        """kv_cache_dtype / weight_dtype: "bf16" / "fp8_e4m3" for this call (None: the engine's); see _generate_many for the rest.
        shed_finished / shed_every (coalesce=True only): as in generate(), for every ragged wave of the call - a batch's result is still what
        its rows produced, trimmed per batch from the assembled buffer.  Refused by name as in generate(), and with return_step_logits.
        processors = (repetition_penalty, no_repeat_ngram_size, stop_token_ids) or None, as in generate(): every row's own generated tokens
        are its history, wherever the row decodes (in-flight states, ragged waves).
        return_logprobs: every batch's result gains a LAST element, fp32 [B_g, n_g, 2], as in generate(); a row's scores follow the row into the
        in-flight states and the ragged waves.
        constraint = (TokenTrie, one list of set indices per batch or None): closed-set generation as in generate(); the set indices follow
        their rows into the in-flight states and the ragged waves."""
        sampling = normalize_sampling(sampling, constraint is not None)
        proc = check_processors(processors, min_new_tokens, constraint is not None, return_logprobs, eos_token_id)
        plan = check_shed(shed_finished, shed_every, constraint, proc, return_logprobs, return_hidden, 1,
                          self._kv_mode if kv_cache_dtype is None else self.check_kv_cache_dtype(kv_cache_dtype), return_step_logits, coalesced=True)
        if plan is not None and not coalesce:
            raise NotImplementedError("shed_finished with coalesce=False: the batches in flight are states of their own that retire as a whole "
                                      "(use coalesce=True, or generate() per batch)")
        cons = self._constraints(constraint, [int(e.shape[0]) for e in embeds_list], eos_token_id, min_new_tokens) if constraint is not None else None
        req = _Request(max_new_tokens, one_eos(eos_token_id, ONE_EOS), pad_token_id, min_new_tokens, use_graph, sampling, proc, return_step_logits,
                       return_hidden, return_first_logits, return_logprobs, shed=_Shed(*plan) if plan is not None else None)
        return self._call(kv_cache_dtype, weight_dtype, req.shed, self._generate_many, embeds_list, req, cons, coalesce, max_rows)

    def _generate_many(self, embeds_list: List[torch.Tensor], req: _Request, constraints=None, coalesce: bool = False,
                       max_rows: Optional[int] = None):
        """Several INDEPENDENT batches in flight: each element of `embeds_list` ([B_i, S_i, D], its own prompt length and left padding, i.e.
        exactly what one generate() call of the reference's eval loop gets) becomes one decode group with its own KV cache, decode state
        and captured HIP graph; the groups are prefilled one after the other and their decode steps are replayed on separate HIP streams.
        At the reference's batch of 8 a decode step is latency-bound (a chain of dependent launches that uses a third of the HBM
        bandwidth), so the chains of 2-4 batches overlap: 8 clips / 4.6 ms alone, 16 / 6.8 ms, 24 / 8.7 ms, 32 / 11.3 ms in flight
        (profiles/README.md r03) - per-batch RESULTS are those of separate generate() calls (rows never interact, every group runs
        the kernels its own M selects).  Returns a list of id tensors (each trimmed like generate() trims it; with return_first_logits a list
        of (ids, first-step logits)).  Sample mode: batch g draws with seed + 7919 g (_select), i.e. what generate(seed = seed + 7919 g) draws for it.

        coalesce = True: the batches decode as ONE ragged batch instead (_start_ragged: right-aligned in one KV cache, per-row rotary offset and
        first visible key), so a decode step streams the 13 GB of weights once for all of them - the eval loop's batches of 8
        (scripts/finetune/inference_hyper_lora.py:1466-1479) then run at the throughput of one large generate() instead of G latency-bound
        M = 8 chains (6.6-9.6 clips/s -> the headline's regime).  Every batch keeps the semantics of its own call (own left padding,
        positions from 0, stops contributing once all ITS rows have finished; ids trimmed per batch); the rows go through the kernels the
        coalesced M selects, so ids / logits agree with separate calls within the bf16 tolerance of the decoder, not bit for bit.  At most
        max_rows (default ops.DECODE_MAX_ROWS) rows decode together; more are run as consecutive waves of about equal size.  Sample mode
        draws per (seed, step, row of the wave): a different random stream than separate calls.
        return_step_logits (coalesce only; parity audits): every batch's result becomes (ids, fp32 logits of every step [B_g, n_g, V]).
        return_hidden (coalesce only; the pixel tasks, generate_avs): every batch's result becomes (ids, post-final-norm hidden state of every
        step [B_g, n_g, D]) - what generate(return_hidden=True) returns for that batch."""
        if not embeds_list:
            return []
        G = len(embeds_list)
        cons = constraints if constraints is not None else [None] * G      # one _Constraint per batch
        per_step = req.return_step_logits or req.return_hidden
        if per_step and (not coalesce or req.return_first_logits or (req.return_step_logits and req.return_hidden)):
            raise NotImplementedError("generate_many: return_step_logits / return_hidden are options of the coalesced form, one at a time (use generate() per batch otherwise)")
        if coalesce and (G > 1 or per_step):
            return self._generate_coalesced(embeds_list, req, cons, max_rows)
        if G == 1:
            return [self._generate(embeds_list[0], req.replace(constraint=cons[0]))]
        max_new_tokens = req.max_new_tokens
        need = sum(e.shape[0] * self.bytes_per_sequence(e.shape[1], max_new_tokens) for e in embeds_list) + self.fixed_bytes(max(e.shape[0] for e in embeds_list),
                                                                                                                            max(e.shape[1] for e in embeds_list))
        budget = self.memory_budget(0, 0, slots=G)
        if need > 0.94 * budget:
            raise MemoryError(f"generate_many: {G} batches need {need / 2**30:.1f} GiB of KV cache and scratch, {budget / 2**30:.1f} GiB available: put fewer in flight")
        self._rope_tab(max(_round_up(e.shape[1] + max_new_tokens, 64) for e in embeds_list))    # grown ONCE: every group's launches bake its pointer
        sts, sinks = [], [_Collect(req) for _ in embeds_list]      # every batch is a call of its own: its own first logits
        for g, emb in enumerate(embeds_list):
            with _ws_slot(g):
                sts.append(self._start(emb, req.replace(constraint=cons[g]), g, sinks[g]))
        self._run_steps(sts, req, True, True)
        return [sinks[g].rows(st, st.out_ids, 0, st.B, int(st.step_dev.item())) for g, st in enumerate(sts)]

    def _generate_coalesced(self, embeds_list, req: _Request, cons, max_rows):
        """generate_many(coalesce=True): pack the batches, in order, into waves of at most `cap` rows (the weight-streaming regime of the decode
        projections, and what the device's memory holds at the longest prompt), run every wave as one ragged batch."""
        Bs = [int(e.shape[0]) for e in embeds_list]
        Smax = max(int(e.shape[1]) for e in embeds_list)
        cap = min(int(max_rows), ops.DECODE_MAX_ROWS) if max_rows else ops.DECODE_MAX_ROWS
        per = self.bytes_per_sequence(Smax, req.max_new_tokens)
        budget = self.memory_budget(0, 0, slots=1)
        fit = (int(0.94 * budget) - self.fixed_bytes(min(sum(Bs), cap), Smax)) // per
        waves = _pack_waves(Bs, max(1, min(cap, fit)))
        plan = {"B": sum(Bs), "groups": [sum(Bs[g] for g in w) for w in waves], "bytes_per_seq": per, "budget": budget, "coalesced": True}
        outs = [None] * len(embeds_list)
        for w in waves:
            if len(w) == 1:                                    # a lone batch (or one larger than the cap: _generate plans its own split)
                outs[w[0]] = self._generate(embeds_list[w[0]], req.replace(constraint=cons[w[0]]))
                continue
            # the rows of the wave are the rows of its batches in wave order: so are their trie roots
            wc = _Constraint(cons[w[0]].dev, [r for g in w for r in cons[g].roots]) if cons[w[0]] is not None else None
            res = self._ragged_wave([embeds_list[g] for g in w], req.replace(constraint=wc))
            for g, r in zip(w, res):
                outs[g] = r
        self.last_plan = plan
        return outs

    def _ragged_wave(self, embeds_list, req: _Request):
        sink = _Collect(req)
        with _ws_slot(0):
            st = self._start_ragged(embeds_list, req, sink)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("prefill_end")
        sts = [st]
        self._run_steps(sts, req, False, True, sink.on_step)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("decode_end")
        n_done = int(sts[0].step_dev.item())                   # a wave that shed rows ends in a child state: the counters went with it
        shed = req.shed
        ids = shed.out if (shed is not None and shed.out is not None) else st.out_ids      # ... and its ids were assembled in shed.out
        # every batch gets what its own generate() call returns: HF stops a call as soon as all of ITS rows have finished
        return sink.groups(st, ids, [int(e.shape[0]) for e in embeds_list], n_done)

    # ------------------------------------------------------------------ classifier-free guidance: a clip's two prompts as two rows of one wave
    @torch.no_grad()
    def generate_guided(self, embeds: torch.Tensor, negative_embeds: torch.Tensor, guidance_scale: float, max_new_tokens: int,
                        eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, min_new_tokens: int = 0, use_graph: bool = True,
                        sampling=None, return_step_logits: bool = False, kv_cache_dtype: Optional[str] = None, weight_dtype: Optional[str] = None,
                        max_rows: Optional[int] = None, **refused):
        """Classifier-free guidance (HF's UnbatchedClassifierFreeGuidanceLogitsProcessor; with a negative prompt that is the question without
        its clip, "visual contrastive decoding"): embeds [B, S, D] are the conditional prompts, negative_embeds [B, Sn, D] the unconditional
        ones, and every token is chosen from
            lu + guidance_scale * (lc - lu),    lc / lu = log_softmax of the conditional / unconditional logits,
        greedy or, with sampling = (temperature, top_k, top_p, seed[, min_p, epsilon_cutoff, eta_cutoff]), in HF's sample mode (the guided
        scores go through the warpers, HF's order).  HF runs a second model forward per step from a Python callback; here the two prompts of a clip are two ROWS of one ragged
        wave (_start_ragged: conditional rows first, unconditional rows after, each group with its own length, right-aligned in one KV cache),
        so the weights stream once per step for both and the step stays one captured graph: crab_cfg_mix -> the ordinary select on the B
        guided rows -> crab_cfg_follow (csrc/cfg.hip), which hands the unconditional row its pair's token.  An 800-row clip prompt beside a
        30-row text prompt takes the per-group prefill form by the RAGGED_PAD_MAX rule.
        A wave holds at most min(max_rows, ops.DECODE_MAX_ROWS) // 2 clips and as many as the memory plan admits; more clips run as
        successive waves of about equal size, a pair is never split (sample mode then draws per (seed, step, row of the wave)).
        Returns the NEW ids of the conditional rows [B, n], trimmed like generate() trims them; with return_step_logits also the RAW step
        logits [2B, n, V] fp32 (conditional rows, then unconditional rows): what the lm_head wrote, not the guided scores.
        Deviation from HF: a token whose logit is -inf in either row scores -inf (HF: NaN where both are).
        Refused by name before any device work: constraint, return_logprobs, processors, return_hidden, return_first_logits,
        decode_streams > 1, several eos ids, guidance_scale <= 1 (HF treats 1 as off: that is the caller's plain generate())."""
        for name, v in refused.items():
            if name not in ("constraint", "return_logprobs", "processors", "return_hidden", "return_first_logits", "decode_streams"):
                raise TypeError(f"generate_guided() got an unexpected keyword argument {name!r}")
            if name == "decode_streams":
                if v is not None and int(v) > 1:
                    raise NotImplementedError(f"generate_guided(decode_streams={v}): a guided wave is one decode state (a pair's rows step together)")
            elif name == "processors":
                if normalize_processors(v) is not None:
                    raise NotImplementedError("generate_guided(processors=...): not implemented with guidance (the edits would have to be applied to the guided scores)")
            elif v is not None and v is not False:
                raise NotImplementedError(f"generate_guided({name}=...): not implemented with guidance")
        g = float(guidance_scale)
        if not g > 1.0:
            raise NotImplementedError(f"guidance_scale = {guidance_scale}: guidance needs a scale > 1 (HF treats 1 as off - call generate())")
        if embeds.dim() != 3 or negative_embeds.dim() != 3 or embeds.shape[2] != negative_embeds.shape[2]:
            raise ValueError(f"generate_guided: embeds [B, S, D] and negative_embeds [B, Sn, D] expected, got {tuple(embeds.shape)} and "
                             f"{tuple(negative_embeds.shape)}")
        if embeds.shape[0] != negative_embeds.shape[0] or embeds.shape[0] < 1:
            raise ValueError(f"generate_guided: {embeds.shape[0]} prompts and {negative_embeds.shape[0]} negative prompts - one negative prompt per row")
        eos = one_eos(eos_token_id, "a guided call stops on ONE id")
        if int(max_new_tokens) < 1:
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new_tokens}.")
        cap = (min(int(max_rows), ops.DECODE_MAX_ROWS) if max_rows else ops.DECODE_MAX_ROWS) // 2
        if cap < 1:
            raise ValueError(f"max_rows = {max_rows}: a pair needs two rows")
        req = _Request(int(max_new_tokens), eos, pad_token_id, int(min_new_tokens), use_graph, normalize_sampling(sampling),
                       return_step_logits=return_step_logits)
        return self._call(kv_cache_dtype, weight_dtype, None, self._generate_guided, embeds, negative_embeds, g, cap, req)

    def _generate_guided(self, embeds, negative_embeds, scale, cap, req: _Request):
        """Plan the waves - whole pairs, at most `cap` per wave and what the device's memory holds - run them, join them as _generate_split
        joins the groups of a split batch (_join: a wave that stopped early is padded with pad ids / zero logits)."""
        embeds = embeds.to(device=self.device, dtype=BF16)
        negative_embeds = negative_embeds.to(device=self.device, dtype=BF16)
        B = int(embeds.shape[0])
        Smax = max(int(embeds.shape[1]), int(negative_embeds.shape[1]))
        per = 2 * self.bytes_per_sequence(Smax, req.max_new_tokens) + self.lm_head.weight.shape[0] * 4       # both rows sit in one cache of Smax rows; + the guided row
        budget = self.memory_budget(0, 0, slots=1)
        fit = (int(0.94 * budget) - self.fixed_bytes(2 * min(B, cap), Smax)) // per
        n_waves = -(-B // max(1, min(cap, fit)))
        sizes = [B // n_waves + (1 if i < B % n_waves else 0) for i in range(n_waves)]
        plan = {"B": B, "groups": sizes, "bytes_per_seq": per, "budget": budget, "guided": True}
        parts, b0 = [], 0
        for n in sizes:
            parts.append(self._guided_wave(embeds[b0:b0 + n], negative_embeds[b0:b0 + n],
                                           req.replace(sampling=reseed_sampling(req.sampling, 104729 * b0), cfg=(scale, n))))
            b0 += n
        self.last_plan = plan
        res = _join(parts, req.join_pad)
        # the raw step logits of the whole call: every wave's conditional rows, then every wave's unconditional rows
        return (res[0], torch.cat(res[1:], 0)) if req.return_step_logits else res[0]

    def _guided_wave(self, embeds, negative_embeds, req: _Request):
        """One wave of whole pairs (req.cfg = (scale, pairs)): a ragged state of two groups.  Returns fresh (ids of the conditional rows
        [B, n],) and, with return_step_logits, the raw step logits [B, n, V] of the conditional and of the unconditional rows."""
        B = int(embeds.shape[0])
        sink = _Collect(req)
        with _ws_slot(0):
            st = self._start_ragged([embeds, negative_embeds], req, sink)
        self._run_steps([st], req, False, True, sink.on_step)
        out = _trim_at_eos(st.out_ids[:B], int(st.step_dev.item()), st.eos_all).clone()
        if not req.return_step_logits:
            return (out,)
        sl = torch.stack(sink.steps, 1)[:, : out.shape[1]]
        return out, sl[:B], sl[B:]

    # ------------------------------------------------------------------ several questions per clip on one prefix KV
    def shared_prefix_bytes(self, C: int, P: int, B: int, S: int, max_new_tokens: int) -> int:
        """Device bytes of one generate_shared_prefix wave - the sibling of B * bytes_per_sequence(P + S, ...): the prefix rows are counted ONCE PER
        CLIP (C x the KV bytes of round_up(P, 64) rows), every one of the B questions pays only for its own round_up(S + max_new_tokens, 64) cache
        rows and its decode row, plus the fp32 partials of the prefix attention (B x S query rows in the suffix prefill) and the prefill scratch."""
        c = self.cfg
        partials = B * max(S, 1) * c.num_attention_heads * (c.head_dim + 2) * 4
        return C * self.kv_bytes_per_sequence(_round_up(P, 64)) + B * self.bytes_per_sequence(S, max_new_tokens) + partials + \
            max(self.fixed_bytes(C, P), self.fixed_bytes(B, S))

    def plan_shared_prefix(self, Gs: List[int], P: int, S: int, max_new_tokens: int, max_rows: Optional[int] = None) -> List[List[int]]:
        """plan_batch's sibling for generate_shared_prefix: the clips (Gs[c] questions each, prefix of P rows, longest question S rows), in order,
        as waves of whole clips with at most min(max_rows, ops.DECODE_MAX_ROWS) rows that fit the memory budget (shared_prefix_bytes: the prefix
        counted once per clip).  The row cap is halved until every wave fits; a single clip that does not fit raises MemoryError."""
        cap = min(int(max_rows), ops.DECODE_MAX_ROWS) if max_rows else ops.DECODE_MAX_ROWS
        # the questions of a wave are prefilled in ONE front-padded pass of rows x S rows: at most SUFFIX_PASS_ROWS of them (the row cap of a
        # prefill chunk, plan_prefill_chunks), so long questions make smaller waves instead of being refused
        cap = max(1, min(cap, SUFFIX_PASS_ROWS // max(int(S), 1)))
        if max(Gs) > cap:
            raise ValueError(f"generate_shared_prefix: a clip with {max(Gs)} questions of up to {S} rows exceeds the {cap} rows of a wave "
                             f"({ops.DECODE_MAX_ROWS} per decode step, {SUFFIX_PASS_ROWS} rows per suffix prefill pass); split its questions")
        budget = self.memory_budget(0, 0, slots=1)
        while True:
            waves = _pack_waves(list(Gs), cap)
            need = max(self.shared_prefix_bytes(len(w), P, sum(Gs[c] for c in w), S, max_new_tokens) for w in waves)
            if need <= 0.94 * budget:
                break
            if all(len(w) == 1 for w in waves):
                raise MemoryError(f"generate_shared_prefix: one clip needs {need / 2**30:.1f} GiB, {budget / 2**30:.1f} GiB available")
            cap = max(max(Gs), cap // 2)
        self.last_plan = {"B": sum(Gs), "groups": [sum(Gs[c] for c in w) for w in waves], "bytes": need, "budget": budget, "shared_prefix": True}
        return waves

    def _shared_prefix_buffers(self, C: int, P: int, Gs: List[int], Smax: int):
        """The persistent device side of a wave, kept while (C, P, Gs, Smax) repeat so that a captured decode step stays valid: prefix cache
        [L, C, Hk, round_up(P, 64), d] x 2, the partials workspace, the per-row rotary offsets and the two tile plans (ops.prefix_tile_plan):
        .decode - clip c owns Gs[c] consecutive query rows - and .prefill - Gs[c] * Smax rows (question-major)."""
        c = self.cfg
        L, H, Hk, d = c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim
        key = (C, P, tuple(Gs), Smax, str(self.device))
        px = self._prefix
        if px is None or px.shape_key != key:
            self._prefix = px = None
            dev, B = self.device, sum(Gs)
            px = types.SimpleNamespace(shape_key=key)
            shape = (L, C, Hk, _round_up(P, 64), d)
            pk, pv = torch.empty(shape, device=dev, dtype=BF16), torch.empty(shape, device=dev, dtype=BF16)
            ws = torch.empty((ops.attn_prefix_bytes(B * Smax, H, d),), device=dev, dtype=torch.uint8)
            rope_off = torch.zeros((B,), device=dev, dtype=torch.int32)
            forms = []
            for rows in (list(Gs), [G * Smax for G in Gs]):
                tiles, row_clip = ops.prefix_tile_plan(rows, H, Hk)
                forms.append(_SharedPrefix(pk, pv, P, ws, rope_off, torch.tensor(tiles, dtype=torch.int32).reshape(-1).to(dev),
                                           torch.tensor(row_clip, dtype=torch.int32).to(dev)))
            px.decode, px.prefill = forms
            # what a captured decode step bakes in beyond _state's own key
            px.key = (P, tuple(Gs), pk.data_ptr(), pv.data_ptr(), ws.data_ptr(), rope_off.data_ptr(), px.decode.tile_rows.data_ptr(),
                      px.decode.row_clip.data_ptr())
            self._prefix = px
        return px

    @torch.no_grad()
    def generate_shared_prefix(self, prefix_embeds: torch.Tensor, suffix_embeds, max_new_tokens: int, eos_token_id: Optional[int] = None,
                               pad_token_id: Optional[int] = None, min_new_tokens: int = 0, use_graph: bool = True, sampling=None,
                               return_first_logits: bool = False, return_step_logits: bool = False, kv_cache_dtype: Optional[str] = None,
                               weight_dtype: Optional[str] = None, max_rows: Optional[int] = None, constraint=None, return_logprobs: bool = False,
                               processors=None):
        """Several questions per clip on ONE prefix KV.  prefix_embeds [C, P, D] bf16: the shared part of C clips (everything up to the question
        text; the same P for all).  suffix_embeds: C lists, one [S_cg, D] tensor per question of the clip.  Returns one id tensor per clip,
        [G_c, n] (with return_first_logits (ids, fp32 [G_c, V]); with return_step_logits (ids, fp32 [G_c, n, V])): what
        generate_many(coalesce=True) returns for the sequences cat(prefix_c, suffix_cg) - the same ragged batch, EOS trim (a clip stops once
        all ITS questions have finished) and padding of finished rows - within the bf16 tolerance of the decoder (the softmax is summed in
        another order), while the prefix is prefilled, stored and, per decode step and kv head, read once per clip instead of once per question.

        Layout (shared_prefix_layout): the prefix goes through prefill() into its own cache [L, C, Hk, round_up(P, 64), d].  The B = sum G_c
        questions are the rows of one ragged decode state whose cache holds ONLY their own keys: question b is right-aligned at Smax = max S, first
        own slot Smax - S_b (the first visible key of the attention), rotary positions P + (slot - first slot) (the RoPE pass takes the offset
        first slot - P, a negative word).  Rows of a clip are consecutive; the prefix attention (crab_attn_prefix_partial) runs on tiles of up
        to 16 // (H // Hk) query rows of ONE clip: a clip's rows are cut into full tiles from its first row on and the remainder forms a partial
        tile, so clips with different numbers of questions mix freely and no tile spans two clips (ops.prefix_tile_plan).
        More rows than a decode step takes (ops.DECODE_MAX_ROWS, max_rows) or than fit the memory run as consecutive waves of whole clips
        (plan_shared_prefix).  Sample mode draws per (seed, step, row of the wave), as the coalesced form does.
        kv_cache_dtype = "fp8_e4m3" and weight_dtype = "fp8_e4m3" raise NotImplementedError: the shared prefix is a bf16 path.
        constraint = (TokenTrie, one list per clip with one set index per question, or None): closed-set generation as in generate().
        return_logprobs: every clip's result gains a LAST element, fp32 [G_c, n, 2], as in generate().
        processors = (repetition_penalty, no_repeat_ngram_size, stop_token_ids) or None, as in generate()."""
        sampling = normalize_sampling(sampling, constraint is not None)
        proc = check_processors(processors, min_new_tokens, constraint is not None, return_logprobs, eos_token_id)
        cons = self._constraints(constraint, [len(qs) for qs in suffix_embeds], eos_token_id, min_new_tokens) if constraint is not None else None
        req = _Request(max_new_tokens, one_eos(eos_token_id, ONE_EOS), pad_token_id, min_new_tokens, use_graph, sampling, proc,
                       return_step_logits=return_step_logits, return_first_logits=return_first_logits, return_logprobs=return_logprobs)
        return self._call(kv_cache_dtype, weight_dtype, None, self._generate_shared_prefix, prefix_embeds, suffix_embeds, req, cons, max_rows)

    def _generate_shared_prefix(self, prefix_embeds, suffix_embeds, req: _Request, cons, max_rows):
        if self._fp8:
            raise NotImplementedError('kv_cache_dtype="fp8_e4m3" with a shared prefix (generate_shared_prefix) is not implemented: the prefix cache and its attention kernels are bf16')
        if getattr(self, "_w_mode", "bf16") == "fp8_e4m3":
            raise NotImplementedError('weight_dtype="fp8_e4m3" with a shared prefix (generate_shared_prefix) is not implemented')
        if req.return_first_logits and req.return_step_logits:
            raise NotImplementedError("generate_shared_prefix: return_first_logits / return_step_logits one at a time")
        if prefix_embeds.dim() != 3 or prefix_embeds.dtype != BF16 or prefix_embeds.shape[1] < 1:
            raise ValueError("prefix_embeds must be a bf16 [C, P, D] tensor with P >= 1")
        C, P, D = prefix_embeds.shape
        if len(suffix_embeds) != C or any(len(qs) < 1 for qs in suffix_embeds) or \
                any(q.dim() != 2 or q.shape[0] < 1 or q.shape[1] != D or q.dtype != BF16 for qs in suffix_embeds for q in qs):
            raise ValueError("suffix_embeds must hold, per clip, a non-empty list of bf16 [S, D] tensors with S >= 1")
        Gs = [len(qs) for qs in suffix_embeds]
        Smax = max(int(q.shape[0]) for qs in suffix_embeds for q in qs)
        outs = []
        for w in self.plan_shared_prefix(Gs, P, Smax, req.max_new_tokens, max_rows):
            wc = _Constraint(cons[w[0]].dev, [r for c in w for r in cons[c].roots]) if cons is not None else None      # one root per question, in row order
            outs += self._shared_prefix_wave(prefix_embeds[w[0]:w[-1] + 1], [suffix_embeds[c] for c in w], req.replace(constraint=wc))
        return outs

    def _prefix_state(self, prefix_embeds, Gs: List[int], lens: List[int], req: _Request):
        """The set-up of a wave whose rows attend a per-clip prefix (generate_shared_prefix, generate_beam; Gs[c] consecutive rows per clip, row b
        with lens[b] own prompt rows): RoPE table and prefix buffers (before any launch bakes a pointer: positions run to P + Tmax), the prefix
        through the existing prefill, once per clip (no lm_head product), then the rows' ragged state - its key extended by the buffers'."""
        C, P, D = prefix_embeds.shape
        lay = shared_prefix_layout(P, lens, req.max_new_tokens)
        self._rope_tab(P + lay["Tmax"])
        px = self._shared_prefix_buffers(C, P, Gs, lay["Smax"])
        b0 = 0
        for n in self.plan_prefill_chunks(C, P):
            self.prefill(prefix_embeds[b0:b0 + n], px.decode.pk, px.decode.pv, b0=b0, want_logits=False)
            b0 += n
        st = self._state(len(lens), lay["Smax"], req.replace(extra_key=px.key + req.extra_key), 0, ragged=True)
        st.prefix = px.decode
        st.row_off.copy_(torch.tensor(lay["first_slot"], dtype=torch.int32))
        px.decode.rope_off.copy_(torch.tensor(lay["rope_off"], dtype=torch.int32))
        return st, px, lay

    def _shared_prefix_wave(self, prefix_embeds, suffix_embeds, req: _Request):
        D = prefix_embeds.shape[2]
        Gs = [len(qs) for qs in suffix_embeds]
        flat = [q for qs in suffix_embeds for q in qs]
        B, Smax = len(flat), max(int(q.shape[0]) for q in flat)
        assert B * Smax <= SUFFIX_PASS_ROWS, "plan_shared_prefix sizes the waves for one suffix prefill pass"
        dev = self.device
        sink = _Collect(req)
        with _ws_slot(0):
            st, px, lay = self._prefix_state(prefix_embeds, Gs, [int(q.shape[0]) for q in flat], req)
            Tmax = lay["Tmax"]
            # ---- the questions: one front-padded pass of Smax rows per question over [prefix of the clip ; own keys up to the row's]
            emb = torch.zeros((B, Smax, D), device=dev, dtype=BF16)
            for b, q in enumerate(flat):
                emb[b, Smax - q.shape[0]:] = q
            M = B * Smax
            ws = self._workspace(M)
            ops.cast_rows(emb.reshape(M, D), ws.x, M, D)
            if Smax == 1:                                      # one row per question: the decode form at slot 0
                x, hfin = self._layers(ws, B, 1, st.kc, st.vc, 0, Tmax, 0, None, None, row_off=st.row_off, prefix=px.decode)
            else:
                pos_ids = torch.tensor(lay["pos_ids"], dtype=torch.int32).to(dev)
                x, hfin = self._layers(ws, B, Smax, st.kc, st.vc, 0, Tmax, 0, None, None, pos_ids=pos_ids, kv_start=st.row_off, prefix=px.prefill)
            ops.copy_rows(hfin[Smax - 1:], st.hn, B, D, lds=Smax * D)         # the last row of every question
            ops.gemm(st.hn, self.lm_head.weight, out=st.logits, out_fp32=True)
            del emb
            self._first_token(st, sink)
        self._run_steps([st], req, False, True, sink.on_step)
        return sink.groups(st, st.out_ids, Gs, int(st.step_dev.item()))

    # ------------------------------------------------------------------ prompt-lookup speculative decoding: k draft tokens verified per step
    @torch.no_grad()
    def generate_lookup(self, embeds: torch.Tensor, max_new_tokens: int, num_draft_tokens: int, max_ngram: int = 2, prompt_ids=None,
                        eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, min_new_tokens: int = 0, use_graph: bool = True,
                        return_first_logits: bool = False, return_step_logits: bool = False, return_stats: bool = False, sampling=None,
                        processors=None, constraint=None, return_logprobs: bool = False, return_hidden: bool = False,
                        kv_cache_dtype: Optional[str] = None, weight_dtype: Optional[str] = None):
        """Greedy generation of ONE sequence (embeds [1, S, D]) with prompt-lookup speculative decoding - HF generate(prompt_lookup_num_tokens =
        num_draft_tokens, max_matching_ngram_size = max_ngram): every step drafts up to k tokens (the continuation of the earliest earlier
        occurrence of the history's last n-gram), runs [current token ; drafts] through the decoder as k + 1 rows - ONE read of the weights -
        and keeps the leading drafts the model agrees with plus its own next token.  The ids are those of generate() under the rule this
        engine uses wherever another row count selects other kernels (the logits differ within the decoder's bf16 bound).
        prompt_ids: int [S], the token id of every prompt row, -1 for a row that is no text token (a modality embedding); None: the history
        starts empty (HF's generate(inputs_embeds=...) starts from an empty input_ids too) and only the generated tokens are matched.  It is
        metadata of the drafts alone: it changes how many are accepted, never what is emitted.
        Prefill and the first token are generate()'s (_start); the step (_lookup_step) is captured as one HIP graph and driven by _run_steps.
        Returns ids [1, n] (trimmed by _trim_at_eos); then, in this order, the emitted tokens' logits fp32 [1, n, V] (return_step_logits), the
        prefill's last-row logits fp32 [1, V] (return_first_logits), and the counters (return_stats): a dict with verify_steps,
        drafts_proposed, drafts_accepted, tokens_emitted (the first token, which the prefill emits, is not counted).
        Refused by name before any device work (check_lookup): more than one row, sampling, processors, constraint, return_logprobs,
        return_hidden, kv_cache_dtype = "fp8_e4m3", weight_dtype = "fp8_e4m3"; num_draft_tokens outside 1 .. 15 and max_ngram < 1 raise
        ValueError."""
        if embeds.dim() != 3:
            raise ValueError("embeds must be a [1, S, D] tensor")
        kv = self.check_kv_cache_dtype(kv_cache_dtype) if kv_cache_dtype is not None else self._kv_mode
        wd = self.check_weight_dtype(weight_dtype) if weight_dtype is not None else getattr(self, "_w_mode", "bf16")
        k, n = check_lookup(num_draft_tokens, max_ngram, int(embeds.shape[0]), normalize_sampling(sampling), processors, constraint, return_logprobs,
                            return_hidden, kv, wd)
        S = int(embeds.shape[1])
        if prompt_ids is not None:
            prompt_ids = torch.as_tensor(prompt_ids).reshape(-1)
            if prompt_ids.numel() != S or prompt_ids.dtype.is_floating_point or prompt_ids.dtype == torch.bool:
                raise ValueError(f"prompt_ids must hold one integer id per prompt row ({S}; -1 = no text token), got {tuple(prompt_ids.shape)} {prompt_ids.dtype}")
        req = _Request(max_new_tokens, one_eos(eos_token_id, ONE_EOS), pad_token_id, min_new_tokens, use_graph, return_step_logits=return_step_logits,
                       return_first_logits=return_first_logits, lookup=(k, n, bool(return_step_logits)))
        return self._call(kv_cache_dtype, weight_dtype, None, self._generate_lookup, embeds, prompt_ids, req, return_stats)

    def _generate_lookup(self, embeds, prompt_ids, req: _Request, return_stats):
        S = int(embeds.shape[1])
        max_new_tokens, (k, max_ngram, _keep) = req.max_new_tokens, req.lookup
        firsts = []

        def sink(st):                                          # the first token's logits: row 0 of the kept rows, and the caller's copy
            if req.return_first_logits:
                firsts.append(st.logits.clone())
            if st.lookup.step_logits is not None:
                st.lookup.step_logits[:1].copy_(st.logits)

        with _ws_slot(0):
            st = self._start(embeds, req, 0, sink)
            lk = st.lookup
            if prompt_ids is not None:
                lk.hist[:S].copy_(prompt_ids.to(torch.int32))
            lk.hist[S:S + 1].copy_(st.out_ids[0, :1])           # the first token (the prefill's): the history's last entry, the current token
            if int(max_new_tokens) == 1:
                st.finished.fill_(1)
        self.last_plan = {"B": 1, "groups": [1], "mode": "lookup", "num_draft_tokens": k, "max_ngram": max_ngram, "Tmax": st.Tmax}
        # every verify step emits at least one token: max_new_tokens - 1 steps always suffice; _run_steps reads `finished` after every step of a lookup state
        self._run_steps([st], req, False, True)
        n_done = int(st.step_dev.item())
        out = _trim_at_eos(st.out_ids, n_done, st.eos_all).clone()
        res = [out]
        if req.return_step_logits:
            res.append(lk.step_logits[None, : out.shape[1]].clone())
        if req.return_first_logits:
            res.append(firsts[0])
        if return_stats:
            s = lk.stats.tolist()
            res.append({"verify_steps": s[0], "drafts_proposed": s[1], "drafts_accepted": s[2], "tokens_emitted": s[3]})
        return res[0] if len(res) == 1 else tuple(res)

    # ------------------------------------------------------------------ beam search: the beams of a clip on one prefix KV
    @torch.no_grad()
    def generate_beam(self, embeds: torch.Tensor, num_beams: int, max_new_tokens: int, eos_token_id: Optional[int] = None,
                      pad_token_id: Optional[int] = None, min_new_tokens: int = 0, length_penalty: float = 1.0, early_stopping=False,
                      num_return_sequences: int = 1, use_graph: bool = True, max_rows: Optional[int] = None, return_scores: bool = False,
                      trace: Optional[list] = None, **refused):
        """HF beam search (GenerationMixin._beam_search: num_beams, length_penalty, early_stopping in {False, True, "never"},
        num_return_sequences, min_new_tokens) from inputs_embeds [B, S, D], S >= 2.  Returns the NEW ids [B * num_return_sequences, n]: per clip
        its hypotheses best first, pad_token_id after a hypothesis's EOS, n the longest returned; with return_scores also sequences_scores, fp32
        [B * num_return_sequences] (sum of log-probs / len ** length_penalty).

        Built on the shared-prefix wave: the first S - 1 rows of a clip are prefilled and stored ONCE (HF expands to B x K full sequences and
        index_selects the whole cache every step); the K beams are K rows of the ragged decode state whose own cache starts with the last
        prompt row, and only these own keys - at most max_new_tokens slots - move when beams are reordered (crab_kv_beam_reorder).  The step is
        the ordinary decode step with the select replaced by crab_beam_row_topk -> crab_beam_merge (csrc/beam.hip), captured and replayed like
        every other; a clip that is done is frozen, the call ends when all are.  More rows than a decode step takes run as waves of whole clips.
        Deviations from HF: ONE eos id; no logits processors in beam mode; ties between equal scores go to the lower index (torch.topk leaves
        them open).  num_beams = 1 is HF's one-beam search, which is greedy.
        trace: a debugging aid - a list that receives, after the first token and after every step, a dict of clones: "step", "logits" (the
        step's raw logits), "before" / "after" (cur_ids, run_seq, finished and every ops.BeamState field around the step); the tests replay
        the steps from it.
        Refused by name before any device work: num_beams outside 1 .. ops.BEAM_MAX, num_return_sequences > num_beams, S < 2, several eos ids,
        max_new_tokens > ops.BEAM_MAX_NEW, sampling / constraint / processors / return_logprobs / return_hidden, and both FP8 modes."""
        for name, v in refused.items():
            if name not in ("sampling", "constraint", "processors", "return_logprobs", "return_hidden", "return_step_logits", "return_first_logits",
                            "kv_cache_dtype", "weight_dtype"):
                raise TypeError(f"generate_beam() got an unexpected keyword argument {name!r}")
            if name in ("kv_cache_dtype", "weight_dtype"):
                if v not in (None, "bf16"):
                    raise NotImplementedError(f'{name}="{v}" with beam search (generate_beam) is not implemented: the shared prefix is a bf16 path')
            elif v is not None and v is not False:
                raise NotImplementedError(f"generate_beam({name}=...): not implemented in beam mode")
        K, R = int(num_beams), int(num_return_sequences)
        if not 1 <= K <= ops.BEAM_MAX:
            raise NotImplementedError(f"num_beams = {num_beams}: 1 .. {ops.BEAM_MAX} beams are implemented")
        if not 1 <= R <= K:
            raise ValueError(f"`num_return_sequences` ({num_return_sequences}) has to be between 1 and `num_beams` ({K})")
        if embeds.dim() != 3 or embeds.shape[1] < 2:
            raise ValueError(f"generate_beam: embeds must be [B, S, D] with S >= 2 (the prefix needs one row), got {tuple(embeds.shape)}")
        eos = one_eos(eos_token_id, "beam search stops on ONE id")
        if int(max_new_tokens) < 1:
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new_tokens}.")
        if int(max_new_tokens) > ops.BEAM_MAX_NEW:
            raise NotImplementedError(f"max_new_tokens = {max_new_tokens} with beam search: at most {ops.BEAM_MAX_NEW}")
        if early_stopping not in (False, True, "never"):
            raise ValueError(f'early_stopping must be False, True or "never", got {early_stopping!r}')
        if 2 * K > self.lm_head.weight.shape[0]:
            raise ValueError(f"num_beams = {K}: the vocabulary holds fewer than 2 num_beams tokens")
        if self._fp8:
            raise NotImplementedError('kv_cache_dtype="fp8_e4m3" with beam search (generate_beam) is not implemented: the prefix cache and its attention kernels are bf16')
        if getattr(self, "_w_mode", "bf16") == "fp8_e4m3":
            raise NotImplementedError('weight_dtype="fp8_e4m3" with beam search (generate_beam) is not implemented')
        lp = float(length_penalty)
        req = _Request(int(max_new_tokens), eos, pad_token_id, int(min_new_tokens), use_graph, extra_key=("beam", K, lp, early_stopping))
        ids, scores = self._call(None, None, None, self._generate_beam, embeds, (K, R, lp, early_stopping), req, max_rows, trace)
        return (ids, scores) if return_scores else ids

    def _generate_beam(self, embeds, beam, req: _Request, max_rows, trace):
        """beam = (K, returned hypotheses per clip, length_penalty, early_stopping).  Returns (ids, sequences_scores)."""
        embeds = embeds.to(device=self.device, dtype=BF16)
        B, S, D = embeds.shape
        K, R = beam[:2]
        seqs, scores, lens = [], [], []
        for w in self.plan_shared_prefix([K] * B, S - 1, 1, req.max_new_tokens, max_rows):
            hs, sc, ln = self._beam_wave(embeds[w[0]:w[-1] + 1], beam, req, trace)
            seqs.append(hs[:, :R]); scores.append(sc[:, :R]); lens.append(ln[:, :R])
        seqs, scores, lens = torch.cat(seqs, 0), torch.cat(scores, 0), torch.cat(lens, 0)
        n = max(1, int(lens.max().item()))
        return seqs[:, :, :n].reshape(B * R, n).contiguous(), scores.reshape(B * R).contiguous()

    def _beam_wave(self, embeds, beam, req: _Request, trace):
        """One wave of whole clips: prefix = all but the last prompt row, once per clip; the K beams of a clip are K copies of the last row.
        Returns fresh (hyp_seq [C, K, max_new], hyp_score [C, K], hyp_len [C, K])."""
        C, S, D = embeds.shape
        K, _R, length_penalty, early_stopping = beam
        P, rows, max_new_tokens = S - 1, C * K, req.max_new_tokens
        with _ws_slot(0):
            st, px, lay = self._prefix_state(embeds[:, :P], [K] * C, [1] * rows, req)
            Tmax = lay["Tmax"]
            if st.beam is None:
                st.beam = ops.BeamState(C, K, max_new_tokens, st.pad, length_penalty, early_stopping, self.device)
            else:
                st.beam.reset()
            st.out_ids.fill_(st.pad)                           # the running histories: HF's fill value
            ws = self._workspace(rows)
            last = embeds[:, P:].expand(C, K, D).reshape(rows, D).contiguous()
            ops.cast_rows(last, ws.x, rows, D)
            x, hfin = self._layers(ws, rows, 1, st.kc, st.vc, 0, Tmax, 0, None, None, row_off=st.row_off, prefix=px.decode)
            ops.copy_rows(hfin, st.hn, rows, D)
            ops.gemm(st.hn, self.lm_head.weight, out=st.logits, out_fp32=True)
            snap = lambda: dict(st.beam.snapshot(), cur_ids=st.cur_ids.clone(), run_seq=st.out_ids.clone(), finished=st.finished.clone())
            prev = [snap()] if trace is not None else None

            def sink(s):
                if trace is not None:
                    after = snap()
                    trace.append({"step": len(trace_steps), "logits": s.logits.clone(), "before": prev[0], "after": after})
                    trace_steps.append(0)
                    prev[0] = after

            trace_steps = []
            self._first_token(st)
            sink(st)
        self._run_steps([st], req, False, True, sink if trace is not None else None)
        bs = st.beam
        return (bs.hyp_seq.view(C, K, max_new_tokens).clone(), bs.hyp_score.view(C, K).clone(), bs.hyp_len.view(C, K).clone())

    def _generate_split(self, groups, embeds, req: _Request):
        """The batch does not fit the device's memory in one piece: generate the groups one after the other (rows are independent,
        so the results are those of the one-piece run up to the kernel choice a different M implies) and join them.  A group
        that finished early (EOS) is padded to the longest group's length with pad ids, like HF pads finished rows."""
        import warnings
        p = self.last_plan
        warnings.warn(f"generate(): {p['B']} sequences x {p['bytes_per_seq'] / 2**20:.0f} MiB do not fit the {p['budget'] / 2**30:.1f} GiB "
                      f"available on {self.device}: running {len(groups)} groups of {groups} one after the other", RuntimeWarning)
        parts, b0 = [], 0
        saved = self.kv_budget_bytes
        for n in groups:
            self.kv_budget_bytes = 1 << 62                    # the group sizes are decided: no re-planning inside
            try:
                r = self._generate(embeds[b0:b0 + n], req.rows(b0, b0 + n).replace(sampling=reseed_sampling(req.sampling, 104729 * b0)))
            finally:
                self.kv_budget_bytes = saved
            parts.append(r if isinstance(r, tuple) else (r,))
            b0 += n
        self.last_plan = p
        # the first logits sit behind the per-step tensors, the scores come last (_Collect.whole)
        res = _join(parts, req.join_pad, keep=len(parts[0]) - 1 - int(req.return_logprobs) if req.return_first_logits else None)
        return res[0] if len(res) == 1 else res

    # ------------------------------------------------------------------ shed_finished: a wave drops its finished rows
    @staticmethod
    def _shed_flush(st: "_DecodeState", shed: "_Shed", step: int):
        """The ids a state holds for its real rows after decode step `step` (columns 0 .. step are written), into the call's result buffer
        under the rows' original indices.  The root state's flush also lays the pad id over the columns behind `step`: a row that stays
        behind has finished, and the unshed call writes st.pad for it at every later step."""
        if st.rows is None:
            shed.out.copy_(st.out_ids)
            shed.out[:, step + 1:] = st.pad
        else:
            shed.out[st.rows_idx] = st.out_ids[:st.n_real]

    def _shed_to(self, root: "_DecodeState", st: "_DecodeState", live: List[int], Bp: int, shed: "_Shed", step: int) -> "_DecodeState":
        """The state `st` (the wave's root state or one of its children) hands its unfinished rows `live` (ascending row indices of st) to the
        root's child state of Bp >= len(live) rows:
          * st's ids go to the result buffer (every row that stays behind has finished: its later columns are the buffer's pad fill);
          * crab_kv_compact_rows moves the live cache rows to the front of every layer, in place; the child's cache is the view [:, :Bp] of
            the root's allocation (the decode kernels take the layer stride separately);
          * the child owns cur_ids, out_ids, finished, row_off, pos_dev, step_dev, logits, workspace and graph of its own: the live rows'
            words are gathered into rows 0 .. n - 1, the counters copied.  Rows n .. Bp - 1 of the rung are dead fillers (finished = 1,
            cur_ids = pad): they step over stale but valid cache rows and nothing of theirs is read back;
          * ch.rows holds every row's index in the whole wave: sample mode keys its draws by it (_select_token), the sinks scatter by it.
        The child is cached on the root under (Bp, weight form) with its workspace and graph - the engine's decode-workspace LRU
        (_workspace) never sees it, so the root's own workspace and graph survive a ladder of any length - and refilled by every shed."""
        dev = self.device
        n = len(live)
        self._shed_flush(st, shed, step)
        # the one upload of a shed (the live list, before the compaction is launched): every index below is made from it on the device, so
        # nothing here waits for the compaction
        idx = ops.kv_compact_rows(st.kc, st.vc, live, st.pos_dev, st.row_off).to(torch.int64)
        w8, w8_key = self._w8_rows(Bp), self._w8_key(Bp)
        ch = root.children.get((Bp, w8_key))
        if ch is None:
            ch = _DecodeState()                                # a plain greedy / sampling state: check_shed refuses every option that owns more
            ch.key = _child_key(root.key, Bp, w8_key)
            ch.B, ch.Tmax, ch.kc, ch.vc, ch.slot, ch.w8 = Bp, root.Tmax, root.kc[:, :Bp], root.vc[:, :Bp], root.slot, w8
            tc, uc = self._ws_cols()
            ch.ws = _Workspace(self.cfg, Bp, dev, tc, uc)
            ch.alloc(dev, Bp, root.out_ids.shape[1], self.lm_head.weight.shape[0], root.row_off is not None)
            ch.rows = torch.empty((Bp,), device=dev, dtype=torch.int32)
            ch.eos, ch.pad, ch.min_new, ch.sampling, ch.eos_all = root.eos, root.pad, root.min_new, root.sampling, root.eos_all
            root.children[(Bp, w8_key)] = ch
        if w8:
            self._w_used = "fp8_e4m3" if self._w_used != "bf16" else "bf16"
        ch.S = st.S
        ch.cur_ids.fill_(st.pad); ch.cur_ids[:n] = st.cur_ids[idx]
        # columns 0 .. step are written; behind them the child holds the pad id, NOT the parent's fill (the root's buffer is filled with
        # pad_token_id or 0, and st.pad is the EOS id when no pad_token_id was given): a row that finishes inside the child and stays behind at
        # the next shed then carries st.pad behind its EOS into the result, as the unshed call writes it at every later step
        ch.out_ids.fill_(st.pad); ch.out_ids[:n, :step + 1] = st.out_ids[idx, :step + 1]
        ch.finished.fill_(1); ch.finished[:n] = st.finished[idx]
        if ch.row_off is not None:
            ch.row_off.zero_(); ch.row_off[:n] = st.row_off[idx]
        ch.pos_dev.copy_(st.pos_dev); ch.step_dev.copy_(st.step_dev)
        orig = st.rows_host if st.rows is not None else list(range(st.B))
        ch.rows_host, ch.n_real = [orig[i] for i in live], n
        ch.rows_idx = st.rows_idx[idx] if st.rows is not None else idx
        ch.rows.fill_(-1); ch.rows[:n] = ch.rows_idx.to(torch.int32)
        shed.log.append((int(step), int(st.B), int(Bp), sum(1 for j, s in enumerate(live) if s != j)))
        return ch

    def _capture(self, st: "_DecodeState"):
        """Capture one decode step into a HIP graph on a side stream (torch.cuda.CUDAGraph = hipGraph on ROCm); the graph is
        kept with the state and reused while the state's key holds."""
        if st.graph is not None:
            return st.graph
        # warm-up run outside capture is not possible without mutating state; instead snapshot and restore
        snap = (st.cur_ids.clone(), st.out_ids.clone(), st.finished.clone(), st.pos_dev.clone(), st.step_dev.clone(),
                st.node.clone() if st.node is not None else None,
                (st.lookup.hist.clone(), st.lookup.stats.clone()) if st.lookup is not None else None)
        if st.beam is not None:
            st.finished.fill_(1)                       # a beam step permutes its state and the cache in place: the warm-up runs with every clip done (frozen)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._decode_step(st)                      # warm-up (module load, workspace alloc)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        pos = int(snap[3].item())
        # the warm-up wrote K/V at `pos`; restoring the counters makes the first replay overwrite the same slot
        st.cur_ids.copy_(snap[0]); st.out_ids.copy_(snap[1]); st.finished.copy_(snap[2])
        st.pos_dev.copy_(snap[3]); st.step_dev.copy_(snap[4])
        if st.node is not None:
            st.node.copy_(snap[5])                     # the warm-up walked the trie one edge ahead of the ids
        if st.lookup is not None:
            st.lookup.hist.copy_(snap[6][0]); st.lookup.stats.copy_(snap[6][1])      # the warm-up verify step emitted tokens and counted them
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._decode_step(st)
        st.graph = g
        return g


class _DecodeState:
    """What one captured decode step reads and writes (built by _state, and by _shed_to for the children of a wave that sheds rows).  Born with
    every attribute "absent" - None for what an option owns - so a state built anywhere takes the plain greedy step until something is set."""

    def __init__(self):
        self.key = self.graph = self.kc = self.vc = self.ws = None
        self.B = self.S = self.Tmax = self.slot = 0
        self.ks = self.vs = None                 # the fp32 row scales of the FP8 KV cache
        self.w8 = self.want_hidden = False       # the step streams the FP8 weights / copies the hidden rows to hn
        self.cur_ids = self.out_ids = self.finished = self.pos_dev = self.step_dev = self.logits = self.row_off = self.hn = None      # alloc(), _state
        self.eos, self.pad, self.min_new, self.eos_all, self.sampling = -1, 0, 0, (-1,), None
        self.prefix = self.beam = None           # _SharedPrefix (generate_shared_prefix, generate_beam); the ops.BeamState born with the state
        self.trie = self.node = self.lp = self.lp_norm = None      # closed-set generation; return_logprobs
        self.proc = self.save_idx = self.save_val = self.stop_dev = None      # processors
        self.cfg = self.guided = self.lookup = None      # generate_guided; generate_lookup: _Lookup
        self.children = None                     # a root state's children by (rows, weight form): {} on a state that _state built
        self.rows = self.rows_idx = self.rows_host = None      # a child only: every row's index in the whole wave (device int32 / int64 / host)
        self.n_real = 0                          # a child only: its rows that are rows of the wave (the rest of the rung are fillers)

    def alloc(self, dev, B: int, n_cols: int, V: int, ragged: bool, logits=None):
        """The per-row words of B rows and n_cols tokens; logits: the rows a lookup state's verify buffer already holds."""
        self.logits = torch.empty((B, V), device=dev, dtype=torch.float32) if logits is None else logits
        self.cur_ids = torch.empty((B,), device=dev, dtype=torch.int64)
        self.out_ids = torch.empty((B, n_cols), device=dev, dtype=torch.int64)
        self.finished = torch.empty((B,), device=dev, dtype=torch.int32)
        self.pos_dev = torch.empty((1,), device=dev, dtype=torch.int32)
        self.step_dev = torch.empty((1,), device=dev, dtype=torch.int32)
        self.row_off = torch.zeros((B,), device=dev, dtype=torch.int32) if ragged else None


class _Collect:
    """What a call hands back beside the ids (the request's return_* flags), gathered while it runs and laid out at its end.  Callable as the
    sink of _first_token and as on_step of _run_steps: the first logits are cloned once per state (n_first states), the step logits / hidden
    rows at every call (st.logits / st.hn are the state's persistent, graph-baked buffers).  B: the rows of the whole wave (the scatter below)."""

    def __init__(self, req: _Request, n_first: int = 1, B: int = 0):
        self.req, self.n_first, self.B = req, n_first, B
        self.first, self.steps, self.hidden, self._sl = [], [], [], None      # _sl: rows()'s kept steps, stacked once

    @property
    def on_step(self):                           # None where nothing is kept per step: the step loop then calls nothing
        return self if (self.req.return_step_logits or self.req.return_hidden) else None

    def __call__(self, st: "_DecodeState"):
        r = self.req
        if r.return_first_logits and len(self.first) < self.n_first:
            self.first.append(st.logits.clone())
        if r.return_step_logits and st.rows is not None:
            # a child state of a wave that shed rows: its real rows under their indices in the whole wave, zeros where a row has left
            full = torch.zeros((self.B,) + tuple(st.logits.shape[1:]), device=st.logits.device, dtype=st.logits.dtype)
            full[st.rows_idx] = st.logits[:st.n_real]
            self.steps.append(full)
        elif r.return_step_logits:
            self.steps.append(st.logits.clone())
        if r.return_hidden:
            self.hidden.append(st.hn.clone())

    def whole(self, sts, out: torch.Tensor):
        """The result of generate(): ids (`out`, the trimmed view, cloned: the buffer behind it is the one the next call refills), step logits,
        hidden rows, first logits, log-probs - THIS order, not rows()'s, is the callers' contract.  sts: the call's states, in row order."""
        r, n = self.req, out.shape[1]
        res = [out.clone()]
        res += [torch.stack(kept, 1)[:, :n] for on, kept in ((r.return_step_logits, self.steps), (r.return_hidden, self.hidden)) if on]
        if r.return_first_logits:
            res.append(self.first[0] if len(self.first) == 1 else torch.cat(self.first, 0))
        if r.return_logprobs:
            res.append(torch.cat([_lp_rows(st, 0, st.B, n) for st in sts], 0))
        return res[0] if len(res) == 1 else tuple(res)

    def rows(self, st: "_DecodeState", ids: torch.Tensor, r0: int, r1: int, n_done: int):
        """What the rows r0 .. r1 of a wave return as a call of their own: their ids trimmed at THEIR EOS and cloned, then the step logits or
        the hidden rows of the kept columns (one at a time) or else the first logits, then the log-probs, last; unwrapped when alone."""
        r = self.req
        out = _trim_at_eos(ids[r0:r1], n_done, st.eos_all).clone()
        res = (out,)
        if r.return_step_logits or r.return_hidden:
            if self._sl is None:
                self._sl = torch.stack(self.hidden if r.return_hidden else self.steps, 1)
            res += (self._sl[r0:r1, : out.shape[1]].clone(),)
        elif r.return_first_logits:
            res += (self.first[0][r0:r1].clone(),)
        if r.return_logprobs:
            res += (_lp_rows(st, r0, r1, out.shape[1]),)
        return res if len(res) > 1 else out

    def groups(self, st: "_DecodeState", ids: torch.Tensor, counts, n_done: int) -> list:
        """rows() for consecutive groups of counts[g] rows."""
        ends = [sum(counts[:g + 1]) for g in range(len(counts))]
        return [self.rows(st, ids, e - n, e, n_done) for n, e in zip(counts, ends)]


def _lp_rows(st: "_DecodeState", r0: int, r1: int, n: int) -> torch.Tensor:
    """The scores of rows r0 .. r1 of a state for the n columns its ids were trimmed to, as a fresh [r1 - r0, n, 2] tensor (st.lp is the
    persistent, graph-baked buffer the next call refills)."""
    return st.lp[:, r0:r1, :n].permute(1, 2, 0).contiguous()


class _Lookup:
    """The device words of a prompt-lookup state (generate_lookup; csrc/lookup.hip): hist int32 [S + max_new] - the prompt's ids (-1: no text
    token) and then the emitted tokens; ids int64 [k + 1] - current token, drafts, pad; n_draft; stats int32 [4] - verify steps, drafts
    proposed, drafts accepted, tokens emitted; logits fp32 [k + 1, V]; step_logits fp32 [max_new, V] when the call keeps the emitted tokens'
    logits.  Born with the decode state and baked into its captured step."""

    def __init__(self, dev, S: int, max_new: int, k: int, max_ngram: int, V: int, keep_logits: bool):
        self.k, self.max_ngram, self.max_new = k, max_ngram, max_new
        self.hist = torch.empty((S + max_new,), device=dev, dtype=torch.int32)
        self.ids = torch.zeros((k + 1,), device=dev, dtype=torch.int64)
        self.n_draft = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.stats = torch.zeros((4,), device=dev, dtype=torch.int32)
        self.logits = torch.empty((k + 1, V), device=dev, dtype=torch.float32)
        self.step_logits = torch.zeros((max_new, V), device=dev, dtype=torch.float32) if keep_logits else None

    def reset(self, pad: int):
        self.hist.fill_(-1); self.ids.fill_(pad); self.n_draft.zero_(); self.stats.zero_()
        if self.step_logits is not None:
            self.step_logits.zero_()


def check_lookup(num_draft_tokens, max_ngram, B: int = 1, sampling=None, processors=None, constraint=None, return_logprobs: bool = False,
                 return_hidden: bool = False, kv_cache_dtype: str = "bf16", weight_dtype: str = "bf16",
                 names=("num_draft_tokens", "max_ngram", "sampling", "processors", "constraint", "return_logprobs", "return_hidden")):
    """What generate_lookup refuses BY NAME, before any device work (the style of check_processors; names: what the caller's surface calls the
    arguments).  Prompt-lookup decoding is greedy verification of one sequence on the bf16 path: everything that changes how a token is
    chosen, or what is recorded per chosen token, would need its own accept kernel."""
    k_name, n_name, s_name, p_name, c_name, lp_name, h_name = names
    k, n = int(num_draft_tokens), int(max_ngram)
    if not 1 <= k <= ops.LOOKUP_MAX_DRAFT:
        raise ValueError(f"`{k_name}` has to be an integer in 1 .. {ops.LOOKUP_MAX_DRAFT} (a verify step runs {k_name} + 1 <= 16 rows), but is {num_draft_tokens}")
    if n < 1:                                                  # HF: PromptLookupCandidateGenerator - "Invalid max_matching_ngram_size or num_output_tokens"
        raise ValueError(f"`{n_name}` has to be a strictly positive integer, but is {max_ngram}")
    if B != 1:
        raise NotImplementedError(f"{k_name} with a batch of {B} rows: prompt-lookup decoding verifies the drafts of ONE sequence per step (HF's assisted "
                                  "generation is batch-size 1 as well; the decode layout has one append slot for all rows)")
    if sampling is not None:
        raise NotImplementedError(f"{k_name} with {s_name}: the drafts are verified against the greedy choice (sample-mode speculative decoding needs "
                                  "rejection sampling, which crab_lookup_accept does not do)")
    if normalize_processors(processors) is not None:
        raise NotImplementedError(f"{k_name} with {p_name}: crab_lookup_accept chooses from the raw logits of k + 1 positions at once; the repetition "
                                  "penalty, n-gram ban and further stop ids edit one position per step (crab_logits_edit)")
    if constraint is not None:
        raise NotImplementedError(f"{k_name} with {c_name}: a token trie is walked one edge per step (crab_constrained_select)")
    if return_logprobs:
        raise NotImplementedError(f"{k_name} with {lp_name}: the log-probability planes are filled one token per step (crab_logprob_norm / crab_logprob_gather)")
    if return_hidden:
        raise NotImplementedError(f"{k_name} with {h_name}: the hidden rows are kept one per step")
    if kv_cache_dtype == "fp8_e4m3":
        raise NotImplementedError(f'{k_name} with kv_cache_dtype="fp8_e4m3": crab_attn_verify attends the bf16 cache (the fp8 cache takes one-row decode steps only)')
    if weight_dtype == "fp8_e4m3":
        raise NotImplementedError(f'{k_name} with weight_dtype="fp8_e4m3": the verify step runs on the bf16 weights')
    return k, n


class _Constraint:
    """Closed-set generation for some rows: dev - the device copies of a TokenTrie's CSR arrays (GenerationEngine._constraints), roots - the
    root node of every row's answer set.  rows(r0, r1) follows the rows wherever a batch is split."""

    def __init__(self, dev, roots):
        self.dev, self.roots = dev, list(roots)

    def rows(self, r0: int, r1: int) -> "_Constraint":
        return _Constraint(self.dev, self.roots[r0:r1])


class _SharedPrefix:
    """One form (decode step or suffix prefill) of a generate_shared_prefix wave as _layers(prefix=...) takes it: pk / pv - the prefix cache
    [L, C, Hk, Tp, d]; P - live prefix rows; ws - the fp32 partials of crab_attn_prefix_partial (uint8); tile_rows / row_clip - the tile plan of the
    form's query rows (ops.prefix_tile_plan, device int32); rope_off - int32 [B], first own slot - P (the decode step's rotary offset).  The two
    forms of a wave share everything but the tile plan."""

    def __init__(self, pk, pv, P, ws, rope_off, tile_rows, row_clip):
        self.pk, self.pv, self.P, self.ws, self.rope_off, self.tile_rows, self.row_clip = pk, pv, P, ws, rope_off, tile_rows, row_clip


def _round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


SUFFIX_PASS_ROWS = 32768       # rows of one suffix prefill pass of generate_shared_prefix (= the row cap of a prefill chunk)


def shared_prefix_layout(P: int, suffix_lens: List[int], max_new_tokens: int) -> dict:
    """Slots and positions of generate_shared_prefix (host arithmetic): question b of S_b rows is right-aligned at Smax = max S in an own cache of
    Tmax = round_up(Smax + max_new_tokens, 64) slots.  first_slot[b] = Smax - S_b (first visible own key); the token in slot s >= first_slot[b]
    sits at rotary position P + (s - first_slot[b]), i.e. s - rope_off[b] with rope_off[b] = first_slot[b] - P (negative whenever P exceeds the
    padding); pos_ids[b][s] for the Smax prefill slots (padding slots, never visible, get a clamped valid position).  The token decoded at step
    t lands in slot Smax + t - 1 of every row."""
    if P < 1 or not suffix_lens or min(suffix_lens) < 1:
        raise ValueError("shared_prefix_layout: P >= 1 and every question at least one row")
    Smax = max(suffix_lens)
    first = [Smax - S for S in suffix_lens]
    return {"Smax": Smax, "Tmax": _round_up(Smax + max_new_tokens, 64), "first_slot": first, "rope_off": [f - P for f in first],
            "pos_ids": [[max(P + s - f, 0) for s in range(Smax)] for f in first]}


class ScoreOutput:
    """What GenerationEngine.score / UnifiedForCausalLM.score return: `loss` (fp32 scalar: mean NLL over all labelled tokens of the batch, NaN
    when there is none), `sum_logprob` [B] fp32, `num_tokens` [B] / `num_correct` [B] int32, `token_logprobs` (a list of [n_i] fp32 tensors, or
    None).  No logits."""

    def __init__(self, loss, sum_logprob, num_tokens, num_correct, token_logprobs=None):
        self.loss, self.sum_logprob, self.num_tokens, self.num_correct, self.token_logprobs = loss, sum_logprob, num_tokens, num_correct, token_logprobs


def score_rows(labels, vocab_size: int, shape=None):
    """Host-side row selection of teacher-forced scoring.  labels [B, S] (HF convention: unshifted, -100 = ignored) ->
        row_idx int32 [n]: the flat rows b * S + t whose NEXT token is labelled (labels[b, t + 1] != -100), sequence by sequence, t ascending;
        tgt     int32 [n]: that label - the already shifted target of row row_idx[i];
        seq_off int32 [B + 1]: CSR offsets of the sequences over the n compacted rows.
    Position 0 is never a target and the last row never scores (modeling_llama.py:1265-1266).  A label that is neither -100 nor a token id
    of the vocabulary raises ValueError (CrossEntropyLoss would index out of range).  CPU tensors; pure host logic."""
    import numpy as np
    lab = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if lab.ndim != 2 or lab.dtype.kind not in "iu":
        raise ValueError(f"labels must be an integer [B, S] array, got {lab.dtype} {lab.shape}")
    if shape is not None and tuple(lab.shape) != tuple(shape):
        raise ValueError(f"labels must be {tuple(shape)} like the embeddings, got {tuple(lab.shape)}")
    lab = lab.astype(np.int64)
    B, S = lab.shape
    bad = (lab != -100) & ((lab < 0) | (lab >= int(vocab_size)))
    if bad.any():
        b, t = (int(v[0]) for v in np.nonzero(bad))
        raise ValueError(f"labels[{b}, {t}] = {int(lab[b, t])}: neither -100 nor a token id below {int(vocab_size)}")
    nxt = lab[:, 1:]
    sel = nxt != -100
    b, t = np.nonzero(sel)                                     # row-major: sequence by sequence, t ascending
    seq_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(sel.sum(1), out=seq_off[1:])
    if B * S >= 2 ** 31:
        raise ValueError("more than 2^31 rows")
    return (torch.from_numpy((b * S + t).astype(np.int32)), torch.from_numpy(nxt[sel].astype(np.int32)), torch.from_numpy(seq_off.astype(np.int32)))
