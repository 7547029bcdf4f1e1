"""Mirror of reference `models/unified_llama.py`: `UnifiedConfig`, `UnifiedModel`, `UnifiedForCausalLM` with the same
`generate(batch_input_ids, batch_labels, batch_X_modals, batch_task_names, **kw)` / `forward(...)` surface
(unified_llama.py:26-391), on the MI355X HIP path.

Differences a caller can observe, all deliberate:
  * decoding is greedy unless the caller passes `do_sample=True` (the reference inherits sampling from the checkpoint's
    generation_config, A.7: Llama-2-chat ships temperature 0.6 / top_p 0.9, HF's default top_k 50 - these are the defaults of
    `do_sample=True` here; draws come from a counter-based generator keyed by `seed`, not from torch's global stream).
  * like the reference's generate(), `attention_mask` / `position_ids` from prepare_multimodal_inputs are NOT forwarded
    to the decoder (unified_llama.py:261-267): left pads are attended and positions run 0..S-1 (A.1) -- reproduced.
    The reference's forward() DOES pass them on (unified_llama.py:129-160, the training-time batch path) and so does
    forward() here: a LEFT-padded attention_mask becomes a per-sequence first visible key in the attention kernels and
    position_ids become explicit rotary positions (golden: forward_masked_tiny_llama.npz); any other 2-D mask (holes anywhere, which
    HF's mask utilities accept) becomes one visibility bit per key (golden: forward_holes_tiny_llama.npz).  The logits of a query
    that sees no key at all (a pad row) are undefined in the reference (implementation-dependent softmax over an all-masked row)
    and finite garbage here; no valid row depends on them.
  * the model lives in bf16 on the GPU (the whole-model bf16 conversion of inference_hyper_lora.py:1470, A.8).
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from . import ops
from .decoder import DecoderConfig, DecoderModel, GenerationEngine, LMHead
from .peft_hyper import PackedLinearGroup
from .unified_arch import UnifiedMetaForCausalLM, UnifiedMetaModel

BF16 = torch.bfloat16


class UnifiedConfig(DecoderConfig):
    model_type = "unified_llm"


class UnifiedModel(UnifiedMetaModel, DecoderModel):
    config_class = UnifiedConfig

    def __init__(self, config: DecoderConfig, device="cuda"):
        DecoderModel.__init__(self, config, device)
        self.config = config
        self.pad_token_id = config.pad_token_id if config.pad_token_id is not None else 0


class CausalLMOutput:
    def __init__(self, logits, hidden_states=None, past_key_values=None, loss=None):
        self.logits, self.hidden_states, self.past_key_values, self.loss = logits, hidden_states, past_key_values, loss


class UnifiedForCausalLM(nn.Module, UnifiedMetaForCausalLM):
    config_class = UnifiedConfig

    def __init__(self, config: DecoderConfig, device="cuda", **kwargs):
        nn.Module.__init__(self)
        self.config = config
        self.model = UnifiedModel(config, device=device)
        self.vocab_size = config.vocab_size
        self.lm_head = LMHead(config.hidden_size, config.vocab_size, device)
        self.is_avs_task = False
        self._engine = GenerationEngine(self.model, self.lm_head, kv_cache_dtype=kwargs.get("kv_cache_dtype", "bf16"),   # "fp8_e4m3": the opt-in FP8 KV cache
                                        weight_dtype=kwargs.get("weight_dtype", "bf16"))                                # "fp8_e4m3": the opt-in FP8 decoder weights (decode steps of <= 16 rows)
        self._past = None

    # ------------------------------------------------------------------ plumbing
    def get_model(self) -> UnifiedModel:
        return self.model

    def packed_groups(self) -> List[PackedLinearGroup]:
        return [g for layer in self.model.layers for g in layer.groups()]

    def _invalidate_graphs(self):
        self._engine.invalidate()

    def _apply(self, fn, *args, **kwargs):
        """.to(device) / .cuda() / .cpu(): nn.Module._apply maps every Parameter separately, which would turn the view
        Parameters of the packed projection groups into independent copies and leave the packed operands the GEMMs read
        behind.  Map the packed buffers themselves, re-point the views, drop captured graphs / caches.  dtype changes raise."""
        groups = self.packed_groups()
        packed = [(g.W, g.bias, g.RA, g.B2) for g in groups]
        # refuse a dtype change BEFORE anything is converted (rebind would only notice after nn.Module._apply had already mapped every
        # other parameter, leaving a half-converted model)
        if fn(torch.empty(1, dtype=BF16, device=self.lm_head.weight.device)).dtype != BF16:
            raise TypeError("crab_amd keeps decoder weights in bfloat16: .float() / .half() / .to(dtype) are not supported")
        # detach the view Parameters of the packed groups while nn.Module._apply maps the rest: mapping each view would
        # materialise a second copy of every projection matrix on the target device before rebind() replaces it
        views = []
        for g in groups:
            for lin in g.linears:
                for mod in lin.modules():                     # the Linear and its lora_route / lora_A / lora_B{i} holders
                    for name in list(mod._parameters):
                        views.append((mod, name, mod._parameters[name]))
                        mod._parameters[name] = None
        try:
            r = super()._apply(fn, *args, **kwargs)
        finally:
            for mod, name, prm in views:
                mod._parameters[name] = prm
        for g, (W, b, RA, B2) in zip(groups, packed):
            g.W, g.bias, g.RA, g.B2 = W, b, RA, B2             # the buffers as they were: rebind maps them once
            g.rebind(fn)
        self._invalidate_graphs()
        return r

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def get_output_embeddings(self):
        return self.lm_head

    def resize_token_embeddings(self, new_num_tokens: int):
        """HF semantics: keep the old rows, new rows ~ N(0, 0.02) (initializer_range); both tables resized."""
        old = self.model.embed_tokens.weight
        if new_num_tokens == old.shape[0]:
            return self.model.embed_tokens
        dev, D = old.device, old.shape[1]
        n_keep = min(old.shape[0], new_num_tokens)
        for holder, attr in ((self.model.embed_tokens, "weight"), (self.lm_head, "weight")):
            w_old = getattr(holder, attr)
            g = torch.Generator(device="cpu").manual_seed(42)
            w_new = (0.02 * torch.randn((new_num_tokens, D), generator=g)).to(device=dev, dtype=BF16)
            w_new[:n_keep].copy_(w_old[:n_keep])
            setattr(holder, attr, nn.Parameter(w_new, requires_grad=False))
        self.model.embed_tokens.num_embeddings = new_num_tokens
        self.vocab_size = self.config.vocab_size = new_num_tokens
        self._invalidate_graphs()
        return self.model.embed_tokens

    @property
    def dtype(self):
        return BF16

    def eval(self):
        return super().eval()

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(
        self,
        batch_input_ids=None,
        batch_labels=None,
        batch_X_modals=None,
        batch_task_names=None,
        input_ids: torch.LongTensor = None,
        attention_mask: Optional[torch.Tensor] = None,
        position_ids: Optional[torch.LongTensor] = None,
        past_key_values=None,
        inputs_embeds: Optional[torch.Tensor] = None,
        labels: Optional[torch.LongTensor] = None,
        use_cache: Optional[bool] = None,
        output_attentions: Optional[bool] = None,
        output_hidden_states: Optional[bool] = None,
        return_dict: Optional[bool] = None,
        **kwargs,
    ):
        """Inference forward (unified_llama.py:47-161): the 1-token decode shortcut (:125-127), the multimodal
        branch (:129-146) and the plain inputs_embeds branch.  Returns an object with `.logits` (fp32, all rows),
        `.hidden_states` (tuple ending with the post-final-norm states when requested) and `.past_key_values`.
        With `labels` (or, in the multimodal branch, `batch_labels`: the labels prepare_multimodal_inputs splices) `.loss` is the reference's
        language-model loss (modeling_llama.py:1261-1274: shift by one, -100 ignored, mean over all labelled tokens of the batch, NaN when there
        is none) as an fp32 scalar, computed by crab_lm_head_xent from the same final hidden states; the logits are what they are without labels."""
        if self.is_avs_task:
            raise NotImplementedError("training losses / AVS forward are outside the inference hot path")      # the mask loss of the pixel tasks is training-only
        eng = self._engine
        dev = self.device
        kvd = eng.check_kv_cache_dtype(kwargs.get("kv_cache_dtype") or eng.kv_cache_dtype)
        if kvd != "bf16" and (use_cache or past_key_values is not None):
            # the FP8 KV cache is generate()'s: a caller-held cache (and the masked one-token shortcut over it, crab_attn_decode_keymask) stays bf16
            raise NotImplementedError(f'forward(use_cache=True / past_key_values) with kv_cache_dtype={kvd!r}: a caller-held KV cache is bf16 only '
                                      '(the FP8 cache serves generate() / generate_batches() / generate_avs())')
        if kvd != "bf16":
            return eng._with_kv_mode("bf16", self.forward, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, input_ids, attention_mask,
                                     position_ids, past_key_values, inputs_embeds, labels, use_cache, output_attentions, output_hidden_states,
                                     return_dict, **{**kwargs, "kv_cache_dtype": "bf16"})      # no cache is kept: the scratch cache of this pass is bf16
        if input_ids is not None and input_ids.shape[1] == 1 and past_key_values is not None:
            kc, vc, n = past_key_values
            if n >= kc.shape[3]:
                # the position travels as a device word (graph-friendly), so the kernels cannot check it: an append past
                # Tmax would write into the next head's rows / past the allocation
                raise ValueError(f"KV cache is full: position {n} >= capacity {kc.shape[3]} (the prefill call sized it as "
                                 f"round64(S + 64)); re-run the prefill with a longer cache")
            B = input_ids.shape[0]
            kv_start, key_mask = self._key_visibility(attention_mask, B, n + 1, kc.shape[3])
            pos_ids = None
            if position_ids is not None and not bool((position_ids.reshape(-1) == n).all()):
                pos_ids = self._rotary_positions(position_ids, B, 1, kc.shape[3])
                eng._rope_tab(self._rope_need)
            emb = self.model.embed_tokens(input_ids.reshape(-1))
            ws = eng._workspace(B)
            ops.cast_rows(emb, ws.x, B, emb.shape[1])
            pos = torch.full((1,), n, device=dev, dtype=torch.int32)
            x, hfin = eng._layers(ws, B, 1, kc, vc, 0, kc.shape[3], 0, pos, None, pos_ids=pos_ids, kv_start=kv_start, key_mask=key_mask)
            hn = hfin.clone()
            logits = ops.gemm(hn, self.lm_head.weight, out_fp32=True)
            loss = eng.xent_from_hidden(hn.view(B, 1, -1), labels).loss if labels is not None else None      # one row: no shifted target, NaN
            return CausalLMOutput(logits.view(B, 1, -1), (hn.view(B, 1, -1),) if output_hidden_states else None, (kc, vc, n + 1), loss)
        if inputs_embeds is None and batch_input_ids is not None:
            # the multimodal branch (unified_llama.py:129-146): mask and positions of the padded batch go to the decoder
            inputs = self.prepare_multimodal_inputs(batch_input_ids=batch_input_ids, batch_labels=batch_labels,
                                                    batch_X_modals=batch_X_modals, batch_task_names=batch_task_names)
            inputs_embeds = inputs['inputs_embeds']
            attention_mask, position_ids = inputs['attention_mask'], inputs['position_ids']
            if batch_labels is not None:
                labels = inputs['labels']                      # spliced: -100 over the modality blocks and the left pads (unified_arch.py:293-325)
        elif inputs_embeds is None and input_ids is not None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        inputs_embeds = inputs_embeds.to(device=dev, dtype=BF16)
        B, S, _ = inputs_embeds.shape
        Tmax = (S + 64 + 63) // 64 * 64 if use_cache else (S + 63) // 64 * 64
        kv_start, key_mask = self._key_visibility(attention_mask, B, S, S)
        pos_ids = None
        if position_ids is not None and not bool((position_ids.reshape(-1, S).cpu() == torch.arange(S)).all()):
            pos_ids = self._rotary_positions(position_ids, B, S, Tmax)
            eng._rope_tab(self._rope_need)
        kc, vc = eng.alloc_cache(B, Tmax)
        logits, hn = eng.prefill(inputs_embeds, kc, vc, all_logits=True, pos_ids=pos_ids, kv_start=kv_start, key_mask=key_mask)
        loss = eng.xent_from_hidden(hn, labels).loss if labels is not None else None
        return CausalLMOutput(logits, (hn,) if output_hidden_states else None, (kc, vc, S) if use_cache else None, loss)

    @torch.no_grad()
    def score(self, batch_input_ids=None, batch_labels=None, batch_X_modals=None, batch_task_names=None, inputs_embeds: Optional[torch.Tensor] = None,
              labels: Optional[torch.LongTensor] = None, attention_mask: Optional[torch.Tensor] = None,
              position_ids: Optional[torch.LongTensor] = None, return_token_logprobs: bool = False, max_rows: Optional[int] = None):
        """Teacher-forced scoring - eval loss / perplexity, the log-likelihood of a gold answer, ranking of candidate answers, token accuracy -
        with the semantics of forward(labels=...) (unified_llama.py:129-160 -> modeling_llama.py:1261-1274) and without logits: the decoder
        pass of forward() (left-pad mask and position_ids honoured), then the fused lm_head + cross entropy over the labelled rows only
        (GenerationEngine.score).  Either the four multimodal arguments (labels = the spliced batch_labels) or inputs_embeds [B, S, D] +
        labels [B, S] (HF convention: unshifted, -100 ignored) with optional attention_mask / position_ids.  Returns an object with
        .loss (fp32 scalar, mean NLL over all labelled tokens of the batch; NaN when there is none), .sum_logprob [B], .num_tokens [B],
        .num_correct [B] and, with return_token_logprobs, .token_logprobs (a list of [n_i] fp32 tensors).  max_rows caps the rows of one
        prefill chunk."""
        if self.is_avs_task:
            raise NotImplementedError("training losses / AVS forward are outside the inference hot path")
        if inputs_embeds is None:
            if batch_input_ids is None or batch_labels is None:
                raise ValueError("score() needs batch_input_ids + batch_labels (+ batch_X_modals, batch_task_names) or inputs_embeds + labels")
            if len(batch_labels) != len(batch_input_ids) or any(tuple(l.shape) != tuple(i.shape) for l, i in zip(batch_labels, batch_input_ids)):
                raise ValueError("score(): batch_labels must match batch_input_ids sample by sample")
            inputs = self.prepare_multimodal_inputs(batch_input_ids=batch_input_ids, batch_labels=batch_labels, batch_X_modals=batch_X_modals,
                                                    batch_task_names=batch_task_names)
            inputs_embeds, labels = inputs['inputs_embeds'], inputs['labels']
            attention_mask, position_ids = inputs['attention_mask'], inputs['position_ids']
        if labels is None:
            raise ValueError("score() needs labels")
        if inputs_embeds.dim() != 3 or tuple(labels.shape) != tuple(inputs_embeds.shape[:2]):
            raise ValueError(f"score(): inputs_embeds [B, S, D] and labels [B, S] expected, got {tuple(inputs_embeds.shape)} and {tuple(labels.shape)}")
        if attention_mask is not None and tuple(attention_mask.shape) != tuple(labels.shape):
            raise ValueError(f"score(): attention_mask must be {tuple(labels.shape)}, got {tuple(attention_mask.shape)}")
        if position_ids is not None and position_ids.numel() not in (labels.shape[1], labels.numel()):
            raise ValueError(f"score(): position_ids must be [B | 1, S], got {tuple(position_ids.shape)}")
        return self._engine.score(inputs_embeds, labels, attention_mask=attention_mask, position_ids=position_ids, max_rows=max_rows,
                                  return_token_logprobs=return_token_logprobs)

    def _key_visibility(self, attention_mask, B: int, T: int, width: int):
        """2-D attention_mask [B, T] over ALL keys (cached + new) -> (kv_start, key_mask) for the attention kernels: GenerationEngine.key_visibility,
        the one implementation forward() and score() share."""
        return self._engine.key_visibility(attention_mask, B, T, width)

    def _rotary_positions(self, position_ids, B: int, S: int, Tmax: int):
        """position_ids [B | 1, S] -> contiguous int32 [B, S] on the device (the caller grows the RoPE table to cover them)."""
        p, hi = self._engine.rotary_positions(position_ids, B, S)
        self._rope_need = max(hi + 1, Tmax)
        return p

    # ------------------------------------------------------------------ generate
    @torch.no_grad()
    def generate(self, batch_input_ids=None, batch_labels=None, batch_X_modals=None, batch_task_names=None, **kwargs):
        """unified_llama.py:244-267.  kwargs understood (HF names): max_new_tokens, min_new_tokens, eos_token_id,
        pad_token_id, use_cache, do_sample (+ temperature, top_k, top_p, seed), output_logits / return_dict_in_generate (parity audits),
        repetition_penalty, no_repeat_ngram_size (HF's two logits processors, over the GENERATED tokens: with inputs_embeds HF starts from an
        empty input_ids, so the prompt never enters them) and a list-valued eos_token_id (any of the ids finishes a row, min_new_tokens
        suppresses all of them, finished rows are padded with pad_token_id - by default the first id, as in HF): all three run inside the
        decode step (csrc/logits_proc.hip), in greedy and sample mode (before the warpers, HF's order); output_logits and
        output_token_logprobs keep reporting the raw logits.  Refused by name: output_token_logprobs with no_repeat_ngram_size, or with
        several stop ids under min_new_tokens; allowed_sequences with several stop ids or no_repeat_ngram_size,
        kv_cache_dtype ("bf16" | "fp8_e4m3": the KV cache of this call, default the engine's - GenerationEngine(kv_cache_dtype=...)),
        weight_dtype ("bf16" | "fp8_e4m3": the decoder weights the decode steps of this call stream, default the engine's; FP8 serves decode
        batches of at most 16 rows - prefill, larger batches, lm_head, forward() and score() stay on the bf16 weights),
        output_first_logits (ids + the fp32 logits of the first generated position, [B, V]: the record the multi-GPU eval gathers),
        inputs_embeds (skip prepare_multimodal_inputs),
        allowed_sequences / allowed_set (closed-set generation, crab_amd/constrain.py: what replaces prefix_allowed_tokens_fn, which needs a host
        callback between two tokens and stays refused).  allowed_sequences: a TokenTrie, one list of id sequences (one answer set for every row)
        or a list of such lists (several sets); allowed_set: one set index per row (default set 0; required with several sets).  Every row's
        ids, cut at EOS, are then a member of its set - greedy and do_sample alike; needs one eos_token_id, and min_new_tokens at most the
        shortest member.  A row that max_new_tokens cuts in the middle of an answer holds a proper prefix of a member, as in HF.
        output_token_logprobs (not an HF name; what replaces output_scores + compute_transition_scores): the result is a
        GenerateOutput with .sequences [B, n] and, all fp32 but the last, .token_logprobs [B, n] (log-probability of every generated token over
        the whole vocabulary, from the raw logits - the number score() gives teacher-forced), .token_logprobs_allowed [B, n] (the same within
        the set the step chose from: all but EOS under min_new_tokens, the answer trie's edges in a closed-set call = HF's transition scores
        with normalize_logits=True of a greedy call), .sum_logprob [B], .sum_logprob_allowed [B] and .num_tokens [B] (int32: generated tokens, the
        EOS included).  Entries after a row's EOS are 0.  With do_sample the warpers (temperature, top_k, top_p) enter neither number - they
        describe the model, not the draw; HF's warped `scores` are not reproduced.
        num_beams > 1: HF beam search (GenerationEngine.generate_beam; csrc/beam.hip) with length_penalty, early_stopping (False | True |
        "never"), num_return_sequences <= num_beams and min_new_tokens.  Returns the new ids [B * num_return_sequences, n], per clip best
        hypothesis first, pad_token_id after a hypothesis's EOS; with return_dict_in_generate a GenerateOutput with .sequences and, with
        output_scores, .sequences_scores [B * num_return_sequences] fp32.  The clip's prompt KV is held once, the beams keep only their own
        keys.  Refused by name with beams: do_sample, allowed_sequences, repetition_penalty / no_repeat_ngram_size (HF applies them to the
        log-probs in beam mode, a different edit from the raw-logit one here), several eos ids, output_token_logprobs / output_logits /
        output_first_logits, both fp8 modes, num_beam_groups / diversity_penalty / constraints.  num_beams = 1 with length_penalty != 1 or
        num_return_sequences > 1 stays refused.
        guidance_scale > 1: classifier-free guidance (HF's UnbatchedClassifierFreeGuidanceLogitsProcessor; GenerationEngine.generate_guided,
        csrc/cfg.hip) against the unconditional prompt negative_inputs_embeds [B, Sn, D] or negative_inputs (a dict of the four generate()
        arguments, e.g. the question without its clip: visual contrastive decoding) - one of the two is required.  Both prompts of a row
        decode as two rows of one ragged batch, every token is chosen from lu + guidance_scale * (lc - lu) over the two log-softmaxes; greedy
        and do_sample, min_new_tokens, one eos_token_id, both fp8 modes, max_rows.  output_logits + return_dict_in_generate gives the RAW
        logits of the conditional rows.  None and 1 are off.  Refused by name with guidance: num_beams > 1, allowed_sequences,
        output_token_logprobs, output_first_logits, repetition_penalty, no_repeat_ngram_size, several eos ids, decode_streams > 1, a scale
        below 1.  A token that is -inf in either row scores -inf (HF: NaN where both are).
        min_p / epsilon_cutoff / eta_cutoff (with do_sample): HF's MinPLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper, in HF's order
        after temperature, top_k and top_p - every stage on the distribution renormalised over what the stages before it kept, the largest
        token and its ties always kept (csrc/sample.hip, inside the decode step).  min_p in (0, 1] removes p_i < min_p * p_max;
        epsilon_cutoff in (0, 1) removes p_i < eps; eta_cutoff in (0, 1) removes p_i < min(eps, sqrt(eps) * exp(-H)), H the entropy of the
        current distribution.  None and 0 are off (all three off: the plain sampling call, launch for launch); without do_sample they have
        no effect, as in HF.  Also in generate_batches / generate_questions / generate_avs*, and with guidance_scale (the guided scores go
        through them).  A value out of range or NaN raises ValueError by name (HF drops a cutoff outside (0, 1) silently);
        allowed_sequences with a live one is refused by name; typical_p stays refused.
        prompt_lookup_num_tokens = k (1 .. 15), max_matching_ngram_size = n (default 2, HF's): prompt-lookup speculative decoding
        (GenerationEngine.generate_lookup; csrc/lookup.hip, csrc/attn_verify.hip) - every step drafts up to k tokens from the sequence's own
        token history and verifies them in one pass over the weights.  Greedy, one row.  The history is batch_input_ids with -1 at the rows
        a modality embedding was spliced into; with inputs_embeds alone it starts empty, as HF's does.  The ids are generate()'s own under the
        decoder's bf16 margin rule; output_logits + return_dict_in_generate gives the logits of the emitted tokens.  Refused by name next to
        it: do_sample, num_beams > 1, guidance_scale, allowed_sequences, repetition_penalty / no_repeat_ngram_size, output_token_logprobs, a
        batch of more than one row; assistant_model stays refused.
        shed_finished (not an HF name; None / False: off) / shed_every: the wave stops carrying the rows that have emitted EOS
        (GenerationEngine.generate; csrc/kv_compact.hip) - True: the default ladder of row counts, a sorted tuple: that ladder; shed_every:
        decode steps between two looks (default: the engine's EOS check).  The result is the call's without the option, within the decoder's
        bf16 tolerance; do_sample keeps every row's random stream.  Refused by name next to it: num_beams > 1, guidance_scale,
        prompt_lookup_num_tokens, allowed_sequences, repetition_penalty / no_repeat_ngram_size / several eos ids, output_token_logprobs,
        decode_streams > 1, the fp8 KV cache."""
        shed = UnifiedForCausalLM._shed_args(self, kwargs, "generate")
        if kwargs.get("prompt_lookup_num_tokens") is not None:
            return UnifiedForCausalLM._generate_lookup(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs)
        beams =int(kwargs.get("num_beams") or 1)
        # _GUIDANCE_ARGS and _WARPER_ARGS are read from the class: generate() alone routes guidance_scale, and _sampling parses the warpers, whatever
        # object stands in for self
        self._check_generate_kwargs(kwargs, (self._PROCESSOR_ARGS | self._BEAM_ARGS if beams > 1 else self._PROCESSOR_ARGS) | UnifiedForCausalLM._GUIDANCE_ARGS |
                                    UnifiedForCausalLM._WARPER_ARGS)
        scale = kwargs.get("guidance_scale")
        if scale is not None and float(scale) != 1.0:          # None and 1 are off (HF adds its processor under the same condition): the plain call below
            return UnifiedForCausalLM._generate_guided(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs)
        if beams > 1:
            return self._generate_beam(batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs)
        sampling = self._sampling(kwargs)
        eos, proc = self._processors(kwargs)
        constraint = self._constraint(kwargs, eos)
        embeds = kwargs.pop("inputs_embeds", None)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("encode_begin")
        if embeds is None:
            inputs = self.prepare_multimodal_inputs(batch_input_ids=batch_input_ids, batch_labels=batch_labels,
                                                    batch_X_modals=batch_X_modals, return_multi_scale_features=False,
                                                    return_gt_mask=False, batch_task_names=batch_task_names)
            embeds = inputs['inputs_embeds']
        embeds = embeds.to(device=self.device, dtype=BF16)
        max_new = int(kwargs.get("max_new_tokens", 20))
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        want_logits = bool(kwargs.get("output_logits")) and bool(kwargs.get("return_dict_in_generate"))
        want_first = bool(kwargs.get("output_first_logits"))      # not an HF name: ids + the first step's logits only (eval gather)
        want_lp = bool(kwargs.get("output_token_logprobs"))       # not an HF name either: the chosen tokens' log-probabilities (csrc/logprob.hip)
        res = self._engine.generate(embeds, max_new, eos_token_id=eos, pad_token_id=pad,
                                    min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0),
                                    prefill_chunk=int(kwargs.get("prefill_chunk", 0)), use_graph=kwargs.get("use_graph", True),
                                    return_step_logits=want_logits, decode_streams=int(kwargs.get("decode_streams", 1)),
                                    return_first_logits=want_first, sampling=sampling, kv_cache_dtype=kwargs.get("kv_cache_dtype"), weight_dtype=kwargs.get("weight_dtype"),
                                    constraint=constraint, return_logprobs=want_lp, processors=proc, **shed)
        if want_logits or want_first or want_lp:
            res = list(res)
            out = type("GenerateOutput", (), {})()
            if want_lp:
                _fill_logprob_fields(out, res[0], res.pop(), _stop_ids(eos, proc))
            out.sequences = res.pop(0)
            if want_logits:
                sl = res.pop(0)
                out.logits = tuple(sl[:, i] for i in range(sl.shape[1]))
            if want_first:
                out.first_logits = res.pop(0)
            return out
        return res

    def _generate_guided(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs):
        """generate(guidance_scale = g): classifier-free guidance through GenerationEngine.generate_guided.  The negative (unconditional) prompt
        comes as negative_inputs_embeds [B, Sn, D] or as negative_inputs = a dict of the four generate() arguments, which goes through
        prepare_multimodal_inputs like the prompt itself (the question without its clip: visual contrastive decoding).  HF's default - the last
        prompt token alone - has no meaning when the prompt is inputs_embeds, so a missing negative prompt is an error.  What guidance does
        not combine with is refused by name before any device work."""
        scale = float(kwargs["guidance_scale"])
        neutral = {"num_beams": 1, "allowed_sequences": None, "allowed_set": None, "output_token_logprobs": False, "output_first_logits": False,
                   "repetition_penalty": 1.0, "no_repeat_ngram_size": 0}
        for k, off in neutral.items():
            v = kwargs.get(k)
            if v is None or v == off or (isinstance(off, bool) and not v):
                continue
            raise NotImplementedError(f"generate(guidance_scale={scale}, {k}={v!r}): not implemented with guidance (greedy and do_sample with "
                                      "min_new_tokens, one eos_token_id, output_logits and both fp8 modes are)")
        eos = kwargs.get("eos_token_id", self.config.eos_token_id)
        if torch.is_tensor(eos):
            eos = eos.reshape(-1).tolist()
        if isinstance(eos, (list, tuple)):
            ids = list(dict.fromkeys(int(e) for e in eos))
            if len(ids) > 1:
                raise NotImplementedError(f"generate(guidance_scale={scale}, eos_token_id={ids}): a guided call stops on ONE eos_token_id")
            eos = ids[0] if ids else None
        neg, neg_inputs = kwargs.pop("negative_inputs_embeds", None), kwargs.pop("negative_inputs", None)
        if (neg is None) == (neg_inputs is None):
            raise ValueError(f"generate(guidance_scale={scale}) needs the unconditional prompt: negative_inputs_embeds [B, Sn, D] or negative_inputs "
                             "(a dict of batch_input_ids, batch_labels, batch_X_modals, batch_task_names), one of the two - HF's default, the "
                             "last prompt token, has no meaning with inputs_embeds")
        sampling = UnifiedForCausalLM._sampling(kwargs)
        embeds = kwargs.pop("inputs_embeds", None)
        prep = lambda d: self.prepare_multimodal_inputs(batch_input_ids=d["batch_input_ids"], batch_labels=d.get("batch_labels"),
                                                        batch_X_modals=d.get("batch_X_modals"), return_multi_scale_features=False,
                                                        return_gt_mask=False, batch_task_names=d.get("batch_task_names"))['inputs_embeds']
        if embeds is None:
            embeds = prep(dict(batch_input_ids=batch_input_ids, batch_labels=batch_labels, batch_X_modals=batch_X_modals, batch_task_names=batch_task_names))
        if neg is None:
            neg = prep(neg_inputs)
        embeds, neg = embeds.to(device=self.device, dtype=BF16), neg.to(device=self.device, dtype=BF16)
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        want_logits = bool(kwargs.get("output_logits")) and bool(kwargs.get("return_dict_in_generate"))
        res = self._engine.generate_guided(embeds, neg, scale, int(kwargs.get("max_new_tokens", 20)), eos_token_id=eos, pad_token_id=pad,
                                           min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), use_graph=kwargs.get("use_graph", True),
                                           sampling=sampling, return_step_logits=want_logits, kv_cache_dtype=kwargs.get("kv_cache_dtype"),
                                           weight_dtype=kwargs.get("weight_dtype"), max_rows=kwargs.get("max_rows"),
                                           decode_streams=int(kwargs.get("decode_streams", 1)))
        if not want_logits:
            return res
        out = type("GenerateOutput", (), {})()
        out.sequences, sl = res
        sl = sl[: out.sequences.shape[0]]                      # the raw logits of the conditional rows
        out.logits = tuple(sl[:, i] for i in range(sl.shape[1]))
        return out

    def _generate_lookup(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs):
        """generate(prompt_lookup_num_tokens = k): prompt-lookup speculative decoding through GenerationEngine.generate_lookup.  What it does not
        combine with is refused by name before any device work."""
        from .decoder import check_lookup
        k = kwargs["prompt_lookup_num_tokens"]
        neutral = {"do_sample": False, "num_beams": 1, "guidance_scale": 1.0, "allowed_sequences": None, "allowed_set": None, "repetition_penalty": 1.0,
                   "no_repeat_ngram_size": 0, "output_token_logprobs": False}
        for name, off in neutral.items():
            v = kwargs.get(name)
            if v is None or v == off or (isinstance(off, bool) and not v):
                continue
            raise NotImplementedError(f"generate(prompt_lookup_num_tokens={k}, {name}={v!r}): not implemented with prompt lookup (greedy decoding of one "
                                      "row with min_new_tokens, one eos_token_id and output_logits is)")
        # the names checked above are neutral here; the warpers have no effect on a greedy call (as in generate())
        UnifiedForCausalLM._check_generate_kwargs(kwargs, UnifiedForCausalLM._LOOKUP_ARGS | UnifiedForCausalLM._PROCESSOR_ARGS | UnifiedForCausalLM._GUIDANCE_ARGS |
                                                  UnifiedForCausalLM._WARPER_ARGS | {"num_beams"})
        eos = kwargs.get("eos_token_id", self.config.eos_token_id)
        if torch.is_tensor(eos):
            eos = eos.reshape(-1).tolist()
        if isinstance(eos, (list, tuple)):
            ids = list(dict.fromkeys(int(e) for e in eos))
            if len(ids) > 1:
                raise NotImplementedError(f"generate(prompt_lookup_num_tokens={k}, eos_token_id={ids}): a prompt-lookup call stops on ONE eos_token_id")
            eos = ids[0] if ids else None
        embeds = kwargs.pop("inputs_embeds", None)
        rows = int(embeds.shape[0]) if embeds is not None else len(batch_input_ids)
        mm = kwargs.get("max_matching_ngram_size")
        k, n = check_lookup(k, 2 if mm is None else mm, rows, kv_cache_dtype=kwargs.get("kv_cache_dtype") or self._engine.kv_cache_dtype,
                            weight_dtype=kwargs.get("weight_dtype") or self._engine.weight_dtype,
                            names=("prompt_lookup_num_tokens", "max_matching_ngram_size", "do_sample", "repetition_penalty / no_repeat_ngram_size",
                                   "allowed_sequences", "output_token_logprobs", "return_hidden"))
        prompt_ids = None
        if embeds is None:
            inputs = self.prepare_multimodal_inputs(batch_input_ids=batch_input_ids, batch_labels=batch_labels, batch_X_modals=batch_X_modals,
                                                    return_multi_scale_features=False, return_gt_mask=False, batch_task_names=batch_task_names,
                                                    return_row_token_ids=True)
            embeds = inputs['inputs_embeds']
            prompt_ids = inputs['row_token_ids'][0]            # -1 at the rows of a spliced modality block
        embeds = embeds.to(device=self.device, dtype=BF16)
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        want_logits = bool(kwargs.get("output_logits")) and bool(kwargs.get("return_dict_in_generate"))
        want_first = bool(kwargs.get("output_first_logits"))
        res = self._engine.generate_lookup(embeds, int(kwargs.get("max_new_tokens", 20)), k, n, prompt_ids=prompt_ids, eos_token_id=eos, pad_token_id=pad,
                                           min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), use_graph=kwargs.get("use_graph", True),
                                           return_step_logits=want_logits, return_first_logits=want_first, return_stats=True,
                                           kv_cache_dtype=kwargs.get("kv_cache_dtype"), weight_dtype=kwargs.get("weight_dtype"))
        res = list(res)
        self.last_lookup = {"stats": res.pop(), "prompt_ids": prompt_ids}      # the counters and the history the engine was given, for audits
        if not (want_logits or want_first):
            return res[0]
        out = type("GenerateOutput", (), {})()
        out.sequences = res.pop(0)
        if want_logits:
            sl = res.pop(0)
            out.logits = tuple(sl[:, i] for i in range(sl.shape[1]))
        if want_first:
            out.first_logits = res.pop(0)
        return out

    def _generate_beam(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, kwargs):
        """generate(num_beams > 1): HF beam search through GenerationEngine.generate_beam.  What beam mode does not take is refused by name
        before any device work."""
        neutral = {"do_sample": False, "allowed_sequences": None, "allowed_set": None, "repetition_penalty": 1.0, "no_repeat_ngram_size": 0,
                   "output_token_logprobs": False, "output_logits": False, "output_first_logits": False, "kv_cache_dtype": "bf16", "weight_dtype": "bf16"}
        for k, off in neutral.items():
            v = kwargs.get(k)
            if v is None or v == off or (isinstance(off, bool) and not v):
                continue
            raise NotImplementedError(f"generate(num_beams={kwargs['num_beams']}, {k}={v!r}): not implemented in beam mode (plain beam search with "
                                      "length_penalty, early_stopping, num_return_sequences and min_new_tokens is)")
        for k in ("kv_cache_dtype", "weight_dtype"):
            if getattr(self._engine, k, "bf16") != "bf16":
                raise NotImplementedError(f'generate(num_beams={kwargs["num_beams"]}) on an engine with {k}="{getattr(self._engine, k)}": beam mode is a bf16 path')
        eos = kwargs.get("eos_token_id", self.config.eos_token_id)
        if torch.is_tensor(eos):
            eos = eos.reshape(-1).tolist()
        if isinstance(eos, (list, tuple)):
            ids = list(dict.fromkeys(int(e) for e in eos))
            if len(ids) > 1:
                raise NotImplementedError(f"generate(num_beams={kwargs['num_beams']}, eos_token_id={ids}): beam mode stops on ONE eos_token_id")
            eos = ids[0] if ids else None
        embeds = kwargs.pop("inputs_embeds", None)
        if embeds is None:
            inputs = self.prepare_multimodal_inputs(batch_input_ids=batch_input_ids, batch_labels=batch_labels, batch_X_modals=batch_X_modals,
                                                    return_multi_scale_features=False, return_gt_mask=False, batch_task_names=batch_task_names)
            embeds = inputs['inputs_embeds']
        embeds = embeds.to(device=self.device, dtype=BF16)
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        lp = kwargs.get("length_penalty")
        want_scores = bool(kwargs.get("output_scores")) and bool(kwargs.get("return_dict_in_generate"))
        res = self._engine.generate_beam(embeds, int(kwargs["num_beams"]), int(kwargs.get("max_new_tokens", 20)), eos_token_id=eos, pad_token_id=pad,
                                         min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), length_penalty=1.0 if lp is None else float(lp),
                                         early_stopping=kwargs.get("early_stopping") or False,
                                         num_return_sequences=int(kwargs.get("num_return_sequences") or 1), use_graph=kwargs.get("use_graph", True),
                                         max_rows=kwargs.get("max_rows"), return_scores=want_scores)
        if not kwargs.get("return_dict_in_generate"):
            return res
        out = type("GenerateOutput", (), {})()
        out.sequences, out.sequences_scores = res if want_scores else (res, None)
        return out

    @torch.no_grad()
    def generate_batches(self, batches, coalesce: bool = False, max_rows: Optional[int] = None, **kwargs):
        """Throughput form of the eval loop (scripts/finetune/inference_hyper_lora.py:1466-1479 calls generate() once per collated batch of 8):
        `batches` = a list of dicts with the four generate() arguments (batch_input_ids, batch_labels, batch_X_modals, batch_task_names).  Every
        batch keeps its own prepare_multimodal_inputs result (its own left padding, like a separate call), then all of them decode together.
        coalesce = False: IN FLIGHT (GenerationEngine.generate_many: one decode group, graph and HIP stream per batch; ids equal to what
        generate() returns for each batch, bit for bit).
        coalesce = True: as ONE ragged decode batch (right-aligned in one KV cache, per-row rotary offset and first visible key): the weights
        stream once per step for all batches and the encoders run over the clips of all batches together, so batches of 8 reach the
        throughput of one large generate(); per-batch ids / logits agree with separate calls within the decoder's bf16 tolerance.
        Returns one id tensor per batch (with output_first_logits=True: (ids, fp32 logits of the first generated position)).
        allowed_sequences / allowed_set: closed-set generation as in generate(); allowed_set is one list of set indices per batch.
        repetition_penalty / no_repeat_ngram_size / a list-valued eos_token_id: as in generate(), per row.
        output_token_logprobs=True: every batch's result is a GenerateOutput with the fields generate() gives it (.sequences, .token_logprobs,
        .token_logprobs_allowed, .sum_logprob, .sum_logprob_allowed, .num_tokens; .first_logits with output_first_logits)."""
        for k in ("output_logits", "return_dict_in_generate", "inputs_embeds"):
            if kwargs.get(k) is not None and kwargs.get(k) is not False:
                raise NotImplementedError(f"generate_batches returns token ids only: {k} is a generate() argument")
        want_first = bool(kwargs.get("output_first_logits"))
        # shed_finished / shed_every: as in generate(), for every ragged wave (coalesce = True; the in-flight form is refused by name)
        shed = UnifiedForCausalLM._shed_args(self, kwargs, "generate_batches" if coalesce else "generate_batches(coalesce=False)", routed=bool(coalesce))
        self._check_generate_kwargs(kwargs, self._PROCESSOR_ARGS | UnifiedForCausalLM._WARPER_ARGS)
        sampling = self._sampling(kwargs)
        eos, proc = self._processors(kwargs)
        constraint = self._constraint(kwargs, eos)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("encode_begin")
        if coalesce:
            inputs = self.prepare_multimodal_inputs_many(batches, return_multi_scale_features=False, return_gt_mask=False)
            embeds = [d['inputs_embeds'].to(device=self.device, dtype=BF16) for d in inputs]
        else:
            embeds = []
            for b in batches:
                inputs = self.prepare_multimodal_inputs(batch_input_ids=b["batch_input_ids"], batch_labels=b.get("batch_labels"),
                                                        batch_X_modals=b["batch_X_modals"], return_multi_scale_features=False, return_gt_mask=False,
                                                        batch_task_names=b.get("batch_task_names"))
                embeds.append(inputs['inputs_embeds'].to(device=self.device, dtype=BF16))
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        want_lp = bool(kwargs.get("output_token_logprobs"))
        res = self._engine.generate_many(embeds, int(kwargs.get("max_new_tokens", 20)), eos_token_id=eos, pad_token_id=pad,
                                         min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), use_graph=kwargs.get("use_graph", True),
                                         sampling=sampling, return_first_logits=want_first, coalesce=coalesce, max_rows=max_rows,
                                         kv_cache_dtype=kwargs.get("kv_cache_dtype"), weight_dtype=kwargs.get("weight_dtype"), constraint=constraint,
                                         return_logprobs=want_lp, processors=proc, **shed)
        return [_logprob_output(r, want_first, _stop_ids(eos, proc)) for r in res] if want_lp else res

    @torch.no_grad()
    def generate_questions(self, clips, max_rows: Optional[int] = None, **kwargs):
        """Several questions per clip on one prefix KV (GenerationEngine.generate_shared_prefix).  `clips` = a list of dicts, each with the four
        generate() arguments of ONE clip (batch_input_ids = [ids of the shared part], batch_labels, batch_X_modals = [its modalities],
        batch_task_names) and `question_ids`: a list of 1-D id tensors, the text that follows the shared part - for the AVQA template
        (dataset/quick_start_dataset.py:158-159) the shared part ends with "Please answer this question: " and a question is the rest.  The
        caller splits, and tokenising the two halves separately must give the ids the whole string would give.
        prepare_multimodal_inputs runs ONCE per clip, the questions are embedded with embed_tokens; clips whose shared parts come out at the
        same length decode together (the engine takes one prefix length per call).  Returns one id tensor per clip, [questions, n]: row g is
        what generate() returns for the ids cat(shared, question g), within the decoder's bf16 tolerance (with output_first_logits=True:
        (ids, fp32 logits of the first generated position)).
        allowed_sequences / allowed_set: closed-set generation as in generate(); allowed_set is one list per clip with one set index per question.
        repetition_penalty / no_repeat_ngram_size / a list-valued eos_token_id: as in generate(), per question.
        output_token_logprobs=True: every clip's result is a GenerateOutput as generate_batches returns it (one row per question)."""
        for k in ("output_logits", "return_dict_in_generate", "inputs_embeds"):
            if kwargs.get(k) is not None and kwargs.get(k) is not False:
                raise NotImplementedError(f"generate_questions returns token ids only: {k} is a generate() argument")
        UnifiedForCausalLM._shed_args(self, kwargs, "generate_questions", routed=False)
        want_first = bool(kwargs.get("output_first_logits"))
        want_lp = bool(kwargs.get("output_token_logprobs"))
        self._check_generate_kwargs(kwargs, self._PROCESSOR_ARGS | UnifiedForCausalLM._WARPER_ARGS)
        sampling = self._sampling(kwargs)
        eos, proc = self._processors(kwargs)
        constraint = self._constraint(kwargs, eos)
        if constraint is not None and constraint[1] is not None and len(constraint[1]) != len(clips):
            raise ValueError(f"allowed_set: {len(constraint[1])} lists of set indices for {len(clips)} clips")
        if ops.PROFILER is not None:
            ops.PROFILER.mark("encode_begin")
        prefixes, questions = [], []
        for c in clips:
            if len(c["batch_input_ids"]) != 1 or not len(c["question_ids"]):
                raise ValueError("generate_questions: one shared id sequence and at least one question per clip")
            inputs = self.prepare_multimodal_inputs(batch_input_ids=c["batch_input_ids"], batch_labels=c.get("batch_labels"),
                                                    batch_X_modals=c["batch_X_modals"], return_multi_scale_features=False, return_gt_mask=False,
                                                    batch_task_names=c.get("batch_task_names"))
            prefixes.append(inputs['inputs_embeds'].to(device=self.device, dtype=BF16))
            questions.append([self.encode_ids(torch.as_tensor(q, device=self.device).reshape(-1)).to(BF16) for q in c["question_ids"]])
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        outs = [None] * len(clips)
        for P in sorted({p.shape[1] for p in prefixes}):
            idx = [i for i, p in enumerate(prefixes) if p.shape[1] == P]
            res = self._engine.generate_shared_prefix(torch.cat([prefixes[i] for i in idx], 0), [questions[i] for i in idx],
                                                      int(kwargs.get("max_new_tokens", 20)), eos_token_id=eos, pad_token_id=pad,
                                                      min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), use_graph=kwargs.get("use_graph", True),
                                                      sampling=sampling, return_first_logits=want_first, kv_cache_dtype=kwargs.get("kv_cache_dtype"),
                                                      weight_dtype=kwargs.get("weight_dtype"), max_rows=max_rows,
                                                      constraint=None if constraint is None else
                                                      (constraint[0], None if constraint[1] is None else [constraint[1][i] for i in idx]),
                                                      return_logprobs=want_lp, processors=proc)
            for i, r in zip(idx, res):
                outs[i] = _logprob_output(r, want_first, _stop_ids(eos, proc)) if want_lp else r
        return outs

    # HF generate() arguments that would CHANGE what is decoded and that this path does not implement: refused by name instead of ignored
    # (name -> the value that means "off").  Everything the reference's loops pass (use_cache, max_new_tokens; do_sample & co. from the
    # checkpoint's generation_config) is implemented; unknown names that cannot alter the ids (output_attentions = False, ...) pass through.
    _UNSUPPORTED = {"num_beams": 1, "num_beam_groups": 1, "num_return_sequences": 1, "repetition_penalty": 1.0, "no_repeat_ngram_size": 0,
                    "encoder_repetition_penalty": 1.0, "length_penalty": 1.0, "penalty_alpha": None, "bad_words_ids": None, "force_words_ids": None,
                    "logits_processor": None, "stopping_criteria": None, "prefix_allowed_tokens_fn": None, "constraints": None, "typical_p": 1.0,
                    "epsilon_cutoff": 0.0, "eta_cutoff": 0.0, "diversity_penalty": 0.0, "suppress_tokens": None, "begin_suppress_tokens": None,
                    "forced_bos_token_id": None, "forced_eos_token_id": None, "assistant_model": None, "streamer": None, "max_time": None,
                    "stop_strings": None, "min_p": None, "guidance_scale": None, "sequence_bias": None, "prompt_lookup_num_tokens": None}

    # the names of _UNSUPPORTED that the decode step implements (csrc/logits_proc.hip): an entry point that routes them to the engine says so
    _PROCESSOR_ARGS = frozenset(("repetition_penalty", "no_repeat_ngram_size"))
    # the names of _UNSUPPORTED that generate(num_beams > 1) hands to GenerationEngine.generate_beam (csrc/beam.hip); generate() alone passes them
    _BEAM_ARGS = frozenset(("num_beams", "length_penalty", "num_return_sequences"))
    # the name of _UNSUPPORTED that generate(guidance_scale > 1) hands to GenerationEngine.generate_guided (csrc/cfg.hip); generate() alone passes it
    _GUIDANCE_ARGS = frozenset(("guidance_scale",))
    # the name of _UNSUPPORTED that generate(prompt_lookup_num_tokens = k) hands to GenerationEngine.generate_lookup (csrc/lookup.hip); generate() alone passes it
    _LOOKUP_ARGS = frozenset(("prompt_lookup_num_tokens",))
    # the names of _UNSUPPORTED that _sampling parses (csrc/sample.hip): every entry point that takes do_sample through _sampling passes them
    _WARPER_ARGS = frozenset(("min_p", "epsilon_cutoff", "eta_cutoff"))

    @classmethod
    def _check_generate_kwargs(cls, kwargs, implemented=frozenset()):
        """implemented: the names of _UNSUPPORTED the calling entry point hands to the engine; a bare call refuses them like the rest."""
        for k, off in cls._UNSUPPORTED.items():
            if k in implemented:
                continue
            v = kwargs.get(k, off)
            if v is None or v == off or (isinstance(v, (list, tuple)) and len(v) == 0):
                continue
            raise NotImplementedError(f"generate({k}={v!r}): not implemented on this path (greedy and HF sample mode with temperature / top_k / top_p are); "
                                      "it would change the decoded ids, so it is refused rather than ignored")
        if "max_length" in kwargs and kwargs.get("max_length") is not None and kwargs.get("max_new_tokens") is None:
            raise NotImplementedError("generate(max_length=...): with inputs_embeds only HF counts new tokens alone - pass max_new_tokens")

    @staticmethod
    def _shed_args(self, kwargs, entry: str = "generate", routed: bool = True):
        """shed_finished / shed_every (not HF names; GenerationEngine.generate: a wave stops carrying the rows that have emitted EOS) -> the
        keyword arguments the engine call gains: {} when the option is off (None / False), so that call is the call without it.  A static
        method with an explicit self: generate() calls it on whatever object stands in for the model.  Refused by name before any device work:
        routed = False (entry points that decode through a path without the option), and next to num_beams > 1, guidance_scale,
        prompt_lookup_num_tokens, allowed_sequences, repetition_penalty / no_repeat_ngram_size / several eos ids, output_token_logprobs and
        the fp8 KV cache - each owns per-row device state that a shed would have to move as well."""
        from .decoder import shed_ladder
        sf = kwargs.get("shed_finished")
        if shed_ladder(sf) is None:
            return {}
        if not routed:
            raise NotImplementedError(f"{entry}(shed_finished={sf!r}): not implemented on this path (generate() and generate_batches(coalesce=True) shed finished rows)")
        neutral = {"num_beams": 1, "guidance_scale": 1.0, "prompt_lookup_num_tokens": None, "allowed_sequences": None, "allowed_set": None,
                   "repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "output_token_logprobs": False}
        for k, off in neutral.items():
            v = kwargs.get(k)
            if v is None or v == off or (isinstance(off, bool) and not v):
                continue
            raise NotImplementedError(f"{entry}(shed_finished={sf!r}, {k}={v!r}): not implemented with shed_finished (greedy and do_sample with "
                                      "min_new_tokens, one eos_token_id, output_logits and output_first_logits are)")
        eos = kwargs.get("eos_token_id", self.config.eos_token_id)
        if torch.is_tensor(eos):
            eos = eos.reshape(-1).tolist()
        if isinstance(eos, (list, tuple)) and len(set(int(e) for e in eos)) > 1:
            raise NotImplementedError(f"{entry}(shed_finished={sf!r}, eos_token_id={list(eos)}): a shedding call stops on ONE eos_token_id")
        kv = kwargs.get("kv_cache_dtype") or getattr(self._engine, "kv_cache_dtype", "bf16")
        if kv == "fp8_e4m3":
            raise NotImplementedError(f'{entry}(shed_finished={sf!r}) with kv_cache_dtype="fp8_e4m3": the rows of the bf16 KV cache are moved (the fp8 '
                                      "row scales would have to move too)")
        return {"shed_finished": sf, "shed_every": kwargs.get("shed_every")}

    def _processors(self, kwargs):
        """repetition_penalty / no_repeat_ngram_size / eos_token_id -> (the engine's ONE eos_token_id, its processors triple or None).  A
        list-valued eos_token_id (HF: any of the ids stops a row) gives the first id to the select kernels and the distinct rest, as
        stop_token_ids, to the processors; the refused combinations raise here, before any device work (decoder.check_processors)."""
        from .decoder import check_processors
        eos = kwargs.get("eos_token_id", self.config.eos_token_id)
        stops = ()
        if torch.is_tensor(eos):
            eos = eos.reshape(-1).tolist()
        if isinstance(eos, (list, tuple)):
            ids = list(dict.fromkeys(int(e) for e in eos))
            eos, stops = (ids[0] if ids else None), tuple(ids[1:])
        proc = check_processors((kwargs.get("repetition_penalty"), kwargs.get("no_repeat_ngram_size"), stops), int(kwargs.get("min_new_tokens", 0) or 0),
                                kwargs.get("allowed_sequences") is not None, bool(kwargs.get("output_token_logprobs")), eos,
                                names=("output_token_logprobs", "allowed_sequences", "eos_token_id beyond the first"))      # the names the caller passed
        return eos, proc

    def _constraint(self, kwargs, eos=None):
        """allowed_sequences / allowed_set -> the engine's constraint argument (TokenTrie, set indices) or None.  eos_token_id (eos: the ONE id
        _processors made of it) and min_new_tokens are checked against the trie here, before any device work (ValueError by name)."""
        seqs = kwargs.get("allowed_sequences")
        if seqs is None:
            if kwargs.get("allowed_set") is not None:
                raise ValueError("allowed_set names answer sets of allowed_sequences, which is missing")
            return None
        from .constrain import as_trie
        trie = as_trie(seqs, self.lm_head.weight.shape[0], eos, int(kwargs.get("min_new_tokens", 0) or 0))
        if kwargs.get("allowed_set") is None and trie.n_sets > 1:
            raise ValueError(f"allowed_sequences holds {trie.n_sets} sets, so every row needs a set index: pass allowed_set")
        return (trie, kwargs.get("allowed_set"))

    @staticmethod
    def _sampling(kwargs):
        """HF sample-mode arguments -> (temperature, top_k, top_p, seed) or None (greedy).  Defaults = what a Llama-2-chat checkpoint's
        generation_config + GenerationConfig's own defaults give the reference's generate() call (temperature 0.6, top_p 0.9, top_k 50).
        min_p / epsilon_cutoff / eta_cutoff (_WARPER_ARGS; HF's MinP-, Epsilon- and EtaLogitsWarper, csrc/sample.hip) are parsed and
        validated here - this is the one function every entry point that samples goes through: a live one makes the result the 7-tuple
        (temperature, top_k, top_p, seed, min_p, epsilon_cutoff, eta_cutoff)."""
        warp = []
        for name, closed in (("min_p", True), ("epsilon_cutoff", False), ("eta_cutoff", False)):
            v = kwargs.get(name)
            v = 0.0 if v is None else float(v)
            if not (0.0 <= v <= 1.0) or (v == 1.0 and not closed):      # NaN fails the first test; HF drops a cutoff outside (0, 1) silently
                raise ValueError(f"`{name}` has to be a float in " + ("[0, 1]" if closed else "[0, 1)") + f" (None and 0 are off), but is {v}")
            warp.append(v)
        if not kwargs.get("do_sample"):
            return None                                        # HF builds warpers in sample mode only: the three have no effect on a greedy call
        t, k, p_ = float(kwargs.get("temperature", 0.6)), int(kwargs.get("top_k", 50) or 0), float(kwargs.get("top_p", 0.9))
        if t <= 0 or not (0 < p_ <= 1) or k < 0:
            raise ValueError("do_sample: temperature > 0, 0 < top_p <= 1, top_k >= 0")
        if any(warp) and kwargs.get("allowed_sequences") is not None:
            live = ", ".join(f"{n}={v}" for n, v in zip(("min_p", "epsilon_cutoff", "eta_cutoff"), warp) if v)
            raise NotImplementedError(f"generate(allowed_sequences=..., {live}): the truncation warpers beyond top_p are not implemented in a closed-set "
                                      "call (crab_constrained_select is a kernel of its own; temperature, top_k and top_p are)")
        seed = kwargs.get("seed")
        if seed is None:
            # no explicit seed: like HF (whose torch.multinomial advances the global generator) every call draws a fresh stream - the seed is
            # taken from torch's default CPU generator, so torch.manual_seed(n) still reproduces a whole run while two calls on the same prompt
            # no longer return the same sample.  seed=<int> stays fully deterministic per call.  (The seed is baked into the captured decode
            # graph: an unseeded sampling call re-captures it.)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        base = (t, k, p_, int(seed) & 0x7FFFFFFFFFFFFFFF)
        return base + tuple(warp) if any(warp) else base       # all three off: the 4-tuple, i.e. the plain sampling call, key and launches

    @torch.no_grad()
    def generate_avs(self, batch_input_ids, batch_labels, batch_X_modals, batch_task_names, **kwargs):
        """unified_llama.py:270-361: greedy generation with the post-final-norm hidden state of every step kept; the states
        of the steps j with output_ids[0, j+1] in {<mask_0..5>} (bs == 1 assumed, :338) become the 6 prompt embeddings
        of the SegModule.  Returns {'output_ids', 'pred_masks'} (only 'output_ids' when != 6 mask tokens were produced).
        One deviation: step 0 contributes its LAST-row state (the reference's step-0 entry holds all S prompt rows).

        bs > 1 (r06): the reference's own bs > 1 behaviour is unusable (it reads row 0's mask positions for every row, :338, and its pixel loops
        call it with one sample, scripts/quick_start.py:270-450), so a batch here means `bs` INDEPENDENT bs-1 calls executed together
        (generate_avs_many): every sample keeps the prompt, positions and picks of its own call.  'output_ids' is then [bs, n_max] (rows that
        stopped earlier padded with pad_token_id, as HF pads finished rows) and 'pred_masks' a list with None for the rows that did not produce
        six mask tokens (the reference prints and returns ids only for such a sample, :345-352)."""
        if len(batch_input_ids) > 1:
            samples = [{"batch_input_ids": [batch_input_ids[i]], "batch_labels": [batch_labels[i]] if batch_labels is not None else None,
                        "batch_X_modals": [batch_X_modals[i]], "batch_task_names": [batch_task_names[i]]} for i in range(len(batch_input_ids))]
            res = self.generate_avs_many(samples, **kwargs)
            eos, _ = self._processors(kwargs)                  # a list-valued eos_token_id: the first id (HF pads with it)
            pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
            n_max = max(r['output_ids'].shape[1] for r in res)
            ids = torch.full((len(res), n_max), int(pad if pad is not None else 0), device=res[0]['output_ids'].device, dtype=res[0]['output_ids'].dtype)
            for i, r in enumerate(res):
                ids[i, :r['output_ids'].shape[1]] = r['output_ids'][0]
            return {'output_ids': ids, 'pred_masks': [r['pred_masks'][0] if r.get('pred_masks') is not None else None for r in res]}
        return self.generate_avs_many([{"batch_input_ids": batch_input_ids, "batch_labels": batch_labels, "batch_X_modals": batch_X_modals,
                                        "batch_task_names": batch_task_names}], **kwargs)[0]

    @torch.no_grad()
    def generate_avs_many(self, samples, max_rows: Optional[int] = None, **kwargs):
        """The pixel-task loops as a THROUGHPUT path (BASELINE configs[4]): `samples` = a list of dicts with the four generate_avs() arguments, each
        one call of the reference's loops (scripts/quick_start.py:270-450: one sample per call).  Every call keeps its own
        prepare_multimodal_inputs result, prompt length and positions; all of them decode as ONE ragged batch (GenerationEngine.generate_many
        (coalesce=True, return_hidden=True): the weights stream once per step for every sample, the encoders see all images / audio windows
        together), the <mask_i> picks are made PER ROW (:333-352), and the rows that produced six mask tokens go through the SegModule together
        (crab_amd/seg_module.py: samples of one class count batched).  Returns one dict per call, exactly what generate_avs returns for it:
        {'output_ids', 'pred_masks'} - or {'output_ids'} alone when the call's row produced != 6 mask tokens (with the reference's message)."""
        inputs, outs = self._avs_generate(samples, max_rows, kwargs)
        seg_ids = {self.SPECIAL_TOKEN_2_IDS[f'<mask_{i}>'] for i in range(6)}
        chosen = []                                           # (call, row, the six step indices)
        n_tok = [ids.shape[1] for ids, _ in outs]
        flat = torch.cat([ids.reshape(-1) for ids, _ in outs]).tolist()      # one device -> host transfer for every call's ids
        o = 0
        for g, (ids, _) in enumerate(outs):
            for r in range(ids.shape[0]):
                row = flat[o:o + n_tok[g]]
                o += n_tok[g]
                picks = [j for j in range(len(row) - 1) if row[j + 1] in seg_ids]
                if len(picks) == 0:
                    print('len(pred_embeddings) == 0')
                elif len(picks) < 6:
                    print(f'pred_embeddings.shape[1] < 6, shape: {len(picks)}')
                else:
                    if len(picks) > 6:
                        print(f'pred_embeddings.shape[1] > 6, shape: {len(picks)}')
                    chosen.append((g, r, picks[-6:]))
        return self._avs_segment(samples, inputs, outs, chosen)

    def _avs_generate(self, samples, max_rows, kwargs):
        """First half of generate_avs_many: inputs of every call (multi-scale CLIP features kept) and the ragged decode with per-step hidden states."""
        UnifiedForCausalLM._shed_args(self, kwargs, "generate_avs", routed=False)      # the hidden rows are kept per row of the wave
        self._check_generate_kwargs(kwargs, self._PROCESSOR_ARGS | UnifiedForCausalLM._WARPER_ARGS)
        sampling = self._sampling(kwargs)
        eos, proc = self._processors(kwargs)
        if ops.PROFILER is not None:
            ops.PROFILER.mark("encode_begin")
        inputs = self.prepare_multimodal_inputs_many(samples, return_multi_scale_features=True, return_gt_mask=True)
        embeds = [d['inputs_embeds'].to(device=self.device, dtype=BF16) for d in inputs]
        pad = kwargs.get("pad_token_id", self.model.pad_token_id if self.model.pad_token_id is not None else eos)
        outs = self._engine.generate_many(embeds, int(kwargs.get("max_new_tokens", 20)), eos_token_id=eos, pad_token_id=pad,
                                          min_new_tokens=int(kwargs.get("min_new_tokens", 0) or 0), use_graph=kwargs.get("use_graph", True),
                                          sampling=sampling, coalesce=True, max_rows=max_rows, return_hidden=True,
                                          kv_cache_dtype=kwargs.get("kv_cache_dtype"), weight_dtype=kwargs.get("weight_dtype"), processors=proc)
        return inputs, outs

    def _avs_segment(self, samples, inputs, outs, chosen):
        """Second half: `chosen` = [(call, row, six step indices)] -> the picked states of those rows through the SegModule (batched per class
        count), one result dict per call."""
        results = [{'output_ids': ids} for ids, _ in outs]
        if not chosen:
            return results
        pred_embeddings = torch.stack([torch.stack([outs[g][1][r, j] for j in picks]) for g, r, picks in chosen])          # [n, 6, D]
        ms = [torch.stack([inputs[g]['multi_scale_image_features'][lv][r] for g, r, _ in chosen]) for lv in range(len(inputs[0]['multi_scale_image_features']))]
        tasks = [samples[g]["batch_task_names"][r] for g, r, _ in chosen]
        seg = self.model.postprocess_seg(pred_embeddings=pred_embeddings, multi_scale_image_feature_list=ms, gt_mask=None, batch_task_names=tasks)
        for (g, r, _), m in zip(chosen, seg['pred_masks']):
            bs_g = outs[g][0].shape[0]
            results[g].setdefault('pred_masks', [None] * bs_g)[r] = m
        return results

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Checkpoints are fp32 (reference ships --bf16 False); tensors are cast to the resident bf16 storage."""
        r = super().load_state_dict(state_dict, strict=strict, assign=False)      # copy_ casts to each parameter's dtype
        self._invalidate_graphs()
        return r


def _stop_ids(eos, proc):
    """Every id that ends a row: the engine's eos_token_id and the stop_token_ids of its processors triple."""
    return ([] if eos is None else [int(eos)]) + (list(proc[2]) if proc is not None else [])


def _fill_logprob_fields(out, ids: torch.Tensor, lp: torch.Tensor, eos):
    """The output_token_logprobs fields of a GenerateOutput from the engine's scores lp [B, n, 2] (GenerationEngine.generate(return_logprobs)):
    names as in ScoreOutput.  num_tokens counts a row's ids up to and including its first EOS (all n without one); eos may be a list of stop
    ids (_stop_ids): the first of ANY of them is the row's last token."""
    out.token_logprobs, out.token_logprobs_allowed = lp[..., 0].contiguous(), lp[..., 1].contiguous()
    out.sum_logprob, out.sum_logprob_allowed = out.token_logprobs.sum(1), out.token_logprobs_allowed.sum(1)
    n = ids.shape[1]
    stops = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else (eos,)) if e is not None]
    if not stops or n == 0:
        out.num_tokens = torch.full((ids.shape[0],), n, device=ids.device, dtype=torch.int32)
    else:
        hit = ids == stops[0]
        for e in stops[1:]:
            hit = hit | (ids == e)
        first = torch.where(hit.any(1), hit.to(torch.int32).argmax(1) + 1, torch.full_like(ids[:, 0], n))
        out.num_tokens = first.to(torch.int32)


def _logprob_output(res, want_first: bool, eos):
    """One batch / clip result of the engine with return_logprobs - (ids, [first logits,] scores) - as a GenerateOutput."""
    out = type("GenerateOutput", (), {})()
    out.sequences = res[0]
    if want_first:
        out.first_logits = res[1]
    _fill_logprob_fields(out, res[0], res[-1], eos)
    return out
