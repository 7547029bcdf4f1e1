#!/usr/bin/env python3
"""Benchmark of the Crab inference hot path on MI355X:  clips/sec, prefill + decode, AVQA-shaped clip.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 launched with torch.distributed.run,
one rank per GPU over RCCL.  One "step" = one pass of the hot path over one batch of synthetic clips per GPU:
encoders (CLIP ViT-L/14 on 8 frames, BEATs on ten 1-s fbank windows, both Q-Former projectors) ->
prepare_multimodal_inputs (S = 702) -> hyper-LoRA Llama-2-7B prefill -> 256 greedy tokens (EOS suppressed) ->
RCCL gather of {clip id, token ids, fp32 first-step logits} to rank 0 (--no-gather-logits: ids only).  Per-clip sharding: every rank holds a full weight
replica and its own clips (weak scaling: clips per GPU fixed).

Workload = BASELINE.json configs[1] ("AVQA eval, Llama-2-7B + BEATs + CLIP-ViT-L/14, bf16, 1xMI355X") at the shape the
metric is quoted on (10 s clip, 8 frames, 256 output tokens, 128-token prompt).  Weights are seeded N(0,0.02)
(no checkpoints offline), inputs synthetic and already resident in HBM when the timed region starts.

A plain run does what the headline needs and no more: set-up, W warm-up steps, K timed steps, the outputs of the last timed step
when --dump-outputs DIR is given, and the JSON line.  Everything else it can measure (roofline figures, the other workloads and
operating points, the CPU baseline) runs only with --full, behind the timed steps.

The JSON line carries
  value        : clips / wall time of the K timed steps on the SHIPPED path (native sequencers, HIP-graph decode, no profiler attached);
  ms_per_step  : wall time of one timed step (the K steps between barriers / K).
With --full it also carries
  roofline     : the dominant kernel by time.  At the default batch this is the decode attention
                 kernel (HBM-bound: every live K/V row of every clip is read once per generated token): algorithmic
                 KV bytes of the sampled launches / their HIP-event time, against the 8 TB/s HBM3E peak.  Sampling: ONE extra,
                 un-timed, instrumented step after the timed region, in which every 32nd decode step runs eagerly (bit-identical
                 to the graph replay) with events around the kernel.
  roofline_mfma: the dominant MFMA kernel (prefill bf16 GEMM bucket): algorithmic FLOPs of ALL its launches in that
                 instrumented step / their HIP-event time, against the 2.5 PFLOP/s dense bf16 peak,
  prefill_roofline: the whole encoder + decoder-prefill PHASE of the LAST timed step, which carries nothing but three phase
                 marks (HIP events at encode_begin / prefill_end / decode_end): algorithmic FLOPs per clip / that time, against 2.5 PFLOP/s,
  cpu_baseline : the CPU oracle (oracle/crab_oracle.py, fp32 PyTorch eager, kind "port") timed on this host on a bounded
                 sample of the same workload and extrapolated linearly in layers / frames / tokens (rank 0, N=1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

T_PROCESS0 = time.perf_counter()   # the ONE JSON line is printed last: everything optional behind the headline is admitted against --time-budget
                                   # (seconds of this process, the torch import included), so that a launcher's time limit never costs the line itself

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes fails without it on this driver

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def time_left(args) -> float:
    return args.time_budget - (time.perf_counter() - T_PROCESS0)


QWEN_RESERVE_S, CPU_RESERVE_S = 60.0, 50.0      # what the blocks take (Qwen2 build 30 s + three steps of 256 clips: ~50 s; the CPU sample: ~30 s at 32 threads)

MFMA_PEAK_TFLOPS = 2500.0        # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
# HBM bytes per algorithmic byte of attn_decode_kernel, from a separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` pass at
# the benchmark shape (scripts/pmc_attn.sh).  profiles/r05_pmc_attn_decode_512clips.txt, 512 clips x ctx 830: FETCH_SIZE 3.40178e6 KiB x 2 (the guide's
# gfx950 correction for wide coalesced reads) + WRITE_SIZE 4096 KiB = 6.9711 GB against 6.9709 GB algorithmic (ratio 1.00002); profiles/r05_pmc_attn_decode.txt,
# 448 clips: 2.97656e6 KiB x 2 + 3584 KiB = 6.0997 GB against 6.0996 (1.0002; r04: the same; r03 at 256 clips: 3.4856 / 3.4850).  The larger of the two is used.
# r06 (profiles/r06_pmc_attn_decode.txt, 512 clips x ctx 830, the kernel unchanged): 3.40178e6 KiB x 2 + 4096 KiB again.
ATTN_DECODE_TRAFFIC_PER_ALGO_BYTE = 1.0002


def flops_per_clip(T_v=8, T_a=10, n_a=48, S=702, V=32017, cfg=None):
    """SURVEY.md 8d parametric form (minimal work).  Decoder terms default to Llama-2-7B (6.476e9 linear MAC-params,
    90.3 MFLOP/token of hyper-LoRA, 32 layers x 4096 wide attention); with `cfg` they are derived from the decoder config."""
    f_beats = 12 * 0.687e9 * (n_a / 48) + 0.453e9 + 0.050e9
    lin, lora, attn_w, D = 6.476e9, 90.3e6, 131072, 4096
    if cfg is not None:
        D, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
        H, Hk, d = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads
        lin = L * (D * (H + 2 * Hk) * d + H * d * D + 3 * D * I)
        # router + A (3+8 rows) on every projection input and three rank-8 B matrices on every projection output
        lora = 2.0 * L * (11 * (4 * D + H * d + I) + 24 * ((H + 2 * Hk) * d + D + 2 * I + D))
        attn_w = L * H * d
    return (T_v * (155.3e9 + 4.0e9) + T_a * (f_beats + 2.57e9) + S * (2 * lin + lora) + 2 * S * S * attn_w + 2 * V * D)


def dead_last_layer_flops(S, cfg):
    """What generate()'s prefill does NOT execute of the algorithmic work above (crab_llama_io.last_rows_only): attention, o_proj, gate|up, down
    of the last layer for the S - 1 rows nobody reads (lm_head takes the last row; the reference computes and drops them, modeling_llama.py:1260)."""
    D, I = cfg.hidden_size, cfg.intermediate_size
    H, d = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    lin = H * d * D + 3 * D * I
    lora = 11 * (H * d + D + I) + 24 * (D + 2 * I + D)                   # routers + A of the o / gate|up / down inputs, B of their outputs
    return (S - 1) * 2.0 * (lin + lora) + 2.0 * S * S * H * d - 4.0 * S * H * d


def decode_bytes_per_step(B, ctx, V=32017):
    return (6.476e9 + V * 4096) * 2 + 45e6 * 2 + B * 2 * 32 * 4096 * 2 * ctx


def cpu_baseline(args):
    """Bounded CPU sample (about 30 s on 32 of the GPU box's host threads): 1 CLIP frame (23 layers) and an 8-layer full-width hyper-LoRA decoder -
    prefill S = 702 and 16 decode tokens spread over the contexts the 256-token generation passes through (6 at 702, 5 at 830, 5 at 958; the
    KV cache of each point is filled directly instead of being produced by a prefill).  Every sample runs once untimed (warm-up: page-in,
    thread pool, allocator) and is then timed NREP times; the MEDIAN is used and the min-max spread reported.
    Extrapolation: x8 frames (+7.5 % for BEATs / Q-Formers by FLOPs), x(32/8) layers, 255 decode tokens at the mean of the three per-token
    times (the attention term is linear in the context, so the mean over 702 / 830 / 958 is the mean over the generation); lm_head timed separately."""
    from crab_amd import synth
    from oracle import crab_oracle as O
    torch.manual_seed(0)
    # the oracle's eager fp32 ops stop scaling well before this host's 128 hardware threads (r05, scripts/exp/cpu_baseline_threads.py on the GPU box:
    # 0.00245 clips/s with 128 threads, 0.00333 with 64, 0.00357 with 32, 0.00352 with 16): the sample runs - and `cores` reports - the best of those
    nth_all = torch.get_num_threads()
    nth = min(nth_all, int(os.environ.get("CRAB_CPU_BASELINE_THREADS", "32")))
    torch.set_num_threads(nth)
    g = torch.Generator().manual_seed(1)
    NREP, NL = 2, 8          # (two timed runs per sample after its warm-up: min / max are the spread; three cost 15-25 s more of a process whose line is printed last)
    CTX = ((702, 6), (830, 5), (958, 5))

    def rnd(*s):
        return torch.randn(*s, generator=g) * 0.02

    def timed(fn, nrep=NREP):
        fn()                                           # warm-up, untimed
        ts = []
        for _ in range(nrep):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        ts.sort()
        n = len(ts)
        return (ts[n // 2] if n & 1 else 0.5 * (ts[n // 2 - 1] + ts[n // 2])), ts[0], ts[-1]

    t, lo, hi = {}, {}, {}

    def rec(name, r):
        t[name], lo[name], hi[name] = r

    # --- CLIP 1 frame
    D, I = 1024, 4096
    W = {}
    p = "model.visual_encoder.vision_tower.vision_model"
    W[p + ".embeddings.patch_embedding.weight"] = rnd(D, 3, 14, 14)
    W[p + ".embeddings.class_embedding"] = rnd(D)
    W[p + ".embeddings.position_embedding.weight"] = rnd(257, D)
    for n in ("pre_layrnorm",):
        W[f"{p}.{n}.weight"], W[f"{p}.{n}.bias"] = torch.ones(D), torch.zeros(D)
    for i in range(23):
        q = f"{p}.encoder.layers.{i}"
        for n, (o, k) in {"self_attn.q_proj": (D, D), "self_attn.k_proj": (D, D), "self_attn.v_proj": (D, D), "self_attn.out_proj": (D, D),
                          "mlp.fc1": (I, D), "mlp.fc2": (D, I)}.items():
            W[f"{q}.{n}.weight"], W[f"{q}.{n}.bias"] = rnd(o, k), torch.zeros(o)
        for n in ("layer_norm1", "layer_norm2"):
            W[f"{q}.{n}.weight"], W[f"{q}.{n}.bias"] = torch.ones(D), torch.zeros(D)
    cc = O.ClipConfig()
    video = synth.synth_video(1)[None]
    rec("clip_frame", timed(lambda: O.visual_encoder(video, W, cc)))
    del W
    # --- decoder, NL layers full width
    dec = O.DecoderConfig(num_hidden_layers=NL)
    Wd = {"model.embed_tokens.weight": rnd(dec.vocab_size, 4096), "lm_head.weight": rnd(dec.vocab_size, 4096),
          "model.norm.weight": torch.ones(4096)}
    for i in range(NL):
        q = f"model.layers.{i}"
        Wd[q + ".input_layernorm.weight"] = torch.ones(4096)
        Wd[q + ".post_attention_layernorm.weight"] = torch.ones(4096)
        for n, (o, k) in {"self_attn.q_proj": (4096, 4096), "self_attn.k_proj": (4096, 4096), "self_attn.v_proj": (4096, 4096),
                          "self_attn.o_proj": (4096, 4096), "mlp.gate_proj": (11008, 4096), "mlp.up_proj": (11008, 4096),
                          "mlp.down_proj": (4096, 11008)}.items():
            Wd[f"{q}.{n}.weight"] = rnd(o, k)
            Wd[f"{q}.{n}.lora_route.weight"], Wd[f"{q}.{n}.lora_A.weight"] = rnd(3, k), rnd(8, k)
            for j in range(3):
                Wd[f"{q}.{n}.lora_B{j}.weight"] = rnd(o, 8)
    emb = rnd(1, 702, 4096) * 50
    rec(f"prefill_{NL}l", timed(lambda: O.decoder_forward(emb, Wd, dec, last_only=True), 2))
    e1 = rnd(1, 1, 4096) * 50
    for ctx, ntok in CTX:
        kv = [rnd(1, 32, ctx, 128) * 50 for _ in range(2 * NL)]          # a cache of `ctx` rows per layer: decode cost depends on its LENGTH only

        def decode(ctx=ctx, ntok=ntok, kv=kv):
            cache = O.KVCache(k=[x.clone() for x in kv[:NL]], v=[x.clone() for x in kv[NL:]])    # decoder_forward appends in place
            pos = torch.tensor([[ctx]])
            for j in range(ntok):
                _, _, cache = O.decoder_forward(e1, Wd, dec, cache, positions=pos + j, last_only=True)

        r = timed(decode)
        rec(f"decode_tok_ctx{ctx}_{NL}l", tuple(x / ntok for x in r))
        del kv
    h = rnd(1, 4096)
    rec("lm_head", timed(lambda: torch.nn.functional.linear(h, Wd["lm_head.weight"])))
    del Wd

    def per_clip(tt):
        # lm_head is inside the decoder_forward timings (last row): separate it out before scaling by layers
        pre = (tt[f"prefill_{NL}l"] - tt["lm_head"]) * (32 / NL) + tt["lm_head"]
        tok = sum(tt[f"decode_tok_ctx{c}_{NL}l"] for c, _ in CTX) / len(CTX)
        dec_tok = (tok - tt["lm_head"]) * (32 / NL) + tt["lm_head"]
        # encoders: BEATs + projectors are ~8 % of encoder FLOPs; scale the CLIP time by the FLOP ratio
        enc = tt["clip_frame"] * 8 * (1.242 + 0.0875 + 0.032 + 0.0257) / 1.242
        return enc + pre + 255 * dec_tok

    cpu = "unknown CPU"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), cpu)
    except OSError:
        pass
    torch.set_num_threads(nth_all)
    return {"value": 1.0 / per_clip(t), "unit": "clips/s", "cores": nth, "kind": "port", "cpu": cpu,
            "threads_note": f"{nth} intra-op threads of {nth_all} available: the eager fp32 port is slower with more (128: 0.69 x, 64: 0.93 x of this rate)",
            "value_range": [round(1.0 / per_clip(hi), 6), round(1.0 / per_clip(lo), 6)],
            "spread_rel": round((per_clip(hi) - per_clip(lo)) / per_clip(t), 3),
            "sample": (f"oracle fp32 eager, one untimed warm-up then median of {NREP} per sample (2 for the prefill): 1 CLIP frame x23 layers (x8, +7.5% for "
                       f"BEATs/Q-Formers by FLOPs), {NL}-layer full-width hyper-LoRA decoder prefill S=702 (x{32 // NL} layers) and 16 decode "
                       f"tokens at contexts 702 / 830 / 958 (6 + 5 + 5; x255 tokens at their mean, x{32 // NL} layers); median s: "
                       f"{json.dumps({k: round(v, 3) for k, v in t.items()})}; "
                       f"min s: {json.dumps({k: round(v, 3) for k, v in lo.items()})}; max s: {json.dumps({k: round(v, 3) for k, v in hi.items()})}")}


def operating_points(model, um, args, eos, t_step):
    """The reference's own operating points, reported NEXT TO the headline (never as `value`): one clip per call (scripts/quick_start.py:43),
    its eval batch of 8 clips (scripts/finetune/inference_hyper_lora.py:1477), its default 10 sampled frames (dataset/quick_start_dataset.py:83 -> S = 766)
    and the MUSIC-AVQA 2-s audio windows ([10,198,128], dataset/unified_dataset.py:1811-1828).  One warm-up + one timed
    generate() each, inputs resident in HBM, same synthetic weights."""
    from crab_amd import synth
    tab = um.SPECIAL_TOKEN_2_IDS
    out = {}
    per_clip_s = t_step / max(args.clips, 1)              # the headline's seconds per clip: the estimate of what a big point's call costs

    def admit(name, est_call_s, clips, reserve):
        """Timed calls this point gets (after its warm-up call): 1 when warm-up + 1 call and the input synthesis fit in what is left of
        --time-budget beyond `reserve` (2 when the room is ample: > 4x), 0 = skipped (recorded in the line).  est_call_s: expected seconds of one
        call.  r06: the points are sized (128-256 clips, one timed call) so that the driver's `--steps 20 --warmup 5` run admits ALL of them."""
        setup = 0.04 * clips + 1.0
        room = time_left(args) - reserve
        n = 2 if room >= 4 * (3 * est_call_s + setup) else (1 if room >= 2 * est_call_s + setup else 0)
        if n == 0:
            out[name] = {"skipped": f"--time-budget {args.time_budget:.0f} s: {max(room, 0):.0f} s left for the operating points, this one needs ~{2 * est_call_s + setup:.0f} s "
                                    "(the builder-run lines under profiles/ carry it)"}
        return n

    def run(name, B, frames, l_a, note, n_timed=2):
        ids = [synth.synth_prompt_ids(128, model.base_vocab, tab, clip=9000 + i) for i in range(B)]
        mods = [{'<video>': synth.synth_video(frames, clip=9000 + i).cuda(), '<audio>': synth.synth_audio(10, l_a, clip=9000 + i).cuda()}
                for i in range(B)]
        lab = [torch.full_like(i, -100) for i in ids]
        ids = [i.cuda() for i in ids]

        def go():
            return model.generate(batch_input_ids=ids, batch_labels=lab, batch_X_modals=mods, batch_task_names=['avqa'] * B, use_cache=True,
                                  max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, eos_token_id=eos,
                                  pad_token_id=um.model.pad_token_id, output_logits=False)
        go()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n_timed):                           # two timed calls per point when the time budget allows (the smaller is reported, both are listed)
            t0 = time.perf_counter()
            r = go()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        dt = sum(ts) / len(ts)                             # the MEAN of the timed calls (not the best one); every call is listed
        assert tuple(r.shape) == (B, args.new_tokens)
        S_ = 126 + 32 * frames + 320
        out[name] = {"clips_per_batch": B, "frames": frames, "fbank_frames_per_window": l_a, "prefill_len": S_,
                     "clips_per_s": round(B / dt, 3), "ms_per_batch": round(dt * 1e3, 1), "ms_per_batch_calls": [round(x * 1e3, 1) for x in ts],
                     "ms_per_batch_min": round(min(ts) * 1e3, 1), "note": note}
        if B <= 16:
            # small batches are weight-streaming bound: HBM floor of the whole call = every decode step reads the decoder + lm_head + adapter
            # weights once and the live KV rows of its B clips (SURVEY 8d "algorithmic bytes per clip, decode"); prefill is <2 % of it
            steps = args.new_tokens - 1
            algo = sum(decode_bytes_per_step(B, S_ + t + 1, V=um.lm_head.weight.shape[0]) for t in range(steps))
            out[name]["hbm"] = {"bound": "hbm", "algorithmic_bytes": int(algo), "achieved_GBps": round(algo / dt / 1e9, 1), "peak_GBps": HBM_PEAK_GBS,
                                "frac": round(algo / dt / 1e9 / HBM_PEAK_GBS, 4), "ms_per_token": round(dt * 1e3 / args.new_tokens, 3),
                                "note": "whole generate() call (encoders + prefill included in the time, not in the bytes)"}

    def run_in_flight(name, G, B, note, n_timed=2):
        """G of the reference's eval batches (B clips each, separate prepare_multimodal_inputs / KV caches / HIP graphs) decoding in flight
        together: UnifiedForCausalLM.generate_batches = what harness.run_inference(in_flight=G) calls; ids per batch = those of G generate() calls."""
        batches = []
        for g in range(G):
            ids = [synth.synth_prompt_ids(128, model.base_vocab, tab, clip=9100 + g * B + i) for i in range(B)]
            batches.append(dict(batch_input_ids=[i.cuda() for i in ids], batch_labels=[torch.full_like(i, -100) for i in ids],
                                batch_X_modals=[{'<video>': synth.synth_video(args.frames, clip=9100 + g * B + i).cuda(),
                                                 '<audio>': synth.synth_audio(10, 98, clip=9100 + g * B + i).cuda()} for i in range(B)],
                                batch_task_names=['avqa'] * B))

        def go():
            return model.generate_batches(batches, use_cache=True, max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, eos_token_id=eos,
                                          pad_token_id=um.model.pad_token_id)
        go()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n_timed):
            t0 = time.perf_counter()
            r = go()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        dt = sum(ts) / len(ts)
        assert len(r) == G and all(tuple(x.shape) == (B, args.new_tokens) for x in r)
        S_ = 126 + 32 * args.frames + 320
        steps = args.new_tokens - 1
        algo = G * sum(decode_bytes_per_step(B, S_ + t + 1, V=um.lm_head.weight.shape[0]) for t in range(steps))
        out[name] = {"batches_in_flight": G, "clips_per_batch": B, "frames": args.frames, "prefill_len": S_, "clips_per_s": round(G * B / dt, 3),
                     "ms_per_call": round(dt * 1e3, 1), "ms_per_call_calls": [round(x * 1e3, 1) for x in ts], "note": note,
                     "hbm": {"bound": "hbm", "algorithmic_bytes": int(algo), "achieved_GBps": round(algo / dt / 1e9, 1), "peak_GBps": HBM_PEAK_GBS,
                             "frac": round(algo / dt / 1e9 / HBM_PEAK_GBS, 4),
                             "note": "every batch streams the weights for itself (separate M = 8 launches): bytes = G x one batch's"}}

    def run_coalesced(name, G, B, spread, note, n_timed=2):
        """G of the reference's eval batches of B clips decoding as ONE ragged batch (generate_batches(coalesce=True) = what
        harness.run_inference(coalesce=True) calls): every batch keeps its own prepare_multimodal_inputs result, left padding and positions
        from 0; the weights stream once per decode step for all G x B rows and the encoders see all clips together.  spread > 0: batch g's
        prompts have 128 - spread + (7 g mod (2 spread + 1)) tokens, so the batches differ in length like a real question set does."""
        batches = []
        for g in range(G):
            nt = 128 if not spread else 128 - spread + (7 * g) % (2 * spread + 1)
            ids = [synth.synth_prompt_ids(nt, model.base_vocab, tab, clip=9500 + g * B + i) for i in range(B)]
            batches.append(dict(batch_input_ids=[i.cuda() for i in ids], batch_labels=[torch.full_like(i, -100) for i in ids],
                                batch_X_modals=[{'<video>': synth.synth_video(args.frames, clip=9500 + g * B + i).cuda(),
                                                 '<audio>': synth.synth_audio(10, 98, clip=9500 + g * B + i).cuda()} for i in range(B)],
                                batch_task_names=['avqa'] * B))

        def go():
            return model.generate_batches(batches, coalesce=True, max_rows=G * B, use_cache=True, max_new_tokens=args.new_tokens,
                                          min_new_tokens=args.new_tokens, eos_token_id=eos, pad_token_id=um.model.pad_token_id)
        go()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n_timed):
            t0 = time.perf_counter()
            r = go()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        dt = sum(ts) / len(ts)
        assert len(r) == G and all(tuple(x.shape) == (B, args.new_tokens) for x in r)
        out[name] = {"batches": G, "clips_per_batch": B, "rows_decoding_together": um._engine.last_plan.get("groups"), "frames": args.frames,
                     "prompt_tokens": "128" if not spread else f"{128 - spread}..{128 + spread} (one length per batch)",
                     "clips_per_s": round(G * B / dt, 3), "ms_per_call": [round(t * 1e3, 1) for t in ts], "note": note}

    # in order of importance; a point is skipped (and says so) rather than letting the process outlive --time-budget.  Behind these the line still
    # needs the Qwen2 variant and the CPU sample: the first group leaves room for the CPU sample only (the Qwen2 block is itself admitted against what
    # is left), the second group leaves room for both
    gco = max(2, min(args.clips, 256) // 8)      # r06: 32 eval batches = 256 rows (r05: 56 = 448 rows; the point then cost 2 x 15 s and pushed the later ones out of the budget)
    nb = min(args.clips, 96)                     # the two points that need their own input synthesis (0.04 s per clip on the host) run at 96 clips (r06 probe at 128: 15.5 s each)
    A, Bq = CPU_RESERVE_S, CPU_RESERVE_S + QWEN_RESERVE_S
    n = admit("single_clip", 1.0, 1, A)
    if n:
        run("single_clip", 1, args.frames, 98, "scripts/quick_start.py: one clip per generate() (BASELINE configs[0] shape on the GPU); latency = ms_per_batch", n)
    n = admit("eval_batch_8", 1.3, 8, A)
    if n:
        run("eval_batch_8", 8, args.frames, 98, "the reference's eval batch size; per-batch latency = ms_per_batch", n)
    n = admit("eval_batch_8_coalesced", per_clip_s * gco * 8 * 1.03, gco * 8, A)
    if n:
        run_coalesced("eval_batch_8_coalesced", gco, 8, 0, f"{gco} eval batches of 8 (inference_hyper_lora.py:1477) coalesced into one ragged decode batch "
                      "(harness.run_inference(coalesce=True)); per-batch results = those of separate generate() calls within the decoder's bf16 tolerance", n)
    if args.clips > 256:
        n = admit("batch_256", per_clip_s * 256 * 1.06, 256, A)
        if n:
            run("batch_256", 256, args.frames, 98, "the headline workload at the 256 clips per step of r01-r03 (the headline's batch is chosen from free memory: "
                "this point keeps the rounds comparable)", n)
    n = admit("eval_batch_8_coalesced_ragged", per_clip_s * gco * 8 * 1.05, gco * 8, A)
    if n:
        run_coalesced("eval_batch_8_coalesced_ragged", gco, 8, 12, "the same with a different prompt length per batch (116..140 tokens): per-batch prefill, "
                      "per-row rotary offset and first visible key in the decode kernels", n)
    n = admit("audio_2s_windows", per_clip_s * nb * 1.08, nb, A)
    if n:
        run("audio_2s_windows", nb, args.frames, 198, "MUSIC-AVQA audio shape [10,198,128] (96 BEATs tokens per window)", n)
    n = admit("frames_10", per_clip_s * nb * 1.15, nb, A)
    if n:
        run("frames_10", nb, 10, 98, "the reference's default video_frame_nums = 10 (S = 766)", n)
    n = admit("eval_batch_8_x3_in_flight", 2.7, 24, A)
    if n:
        run_in_flight("eval_batch_8_x3_in_flight", 3, 8, "three eval batches of 8 decoding concurrently on separate HIP streams (harness.run_inference in_flight=3)", n)
    n = admit("eval_batch_8_x4_in_flight", 3.5, 32, A)
    if n:
        run_in_flight("eval_batch_8_x4_in_flight", 4, 8, "four eval batches of 8 in flight", n)
    return out


def _executed_block(algo_flops_per_clip, S, cfg, ms_per_clip):
    """`frac` above prices the ALGORITHMIC FLOPs of SURVEY.md 8d (every row through every layer).  The shipped prefill skips the dead rows of the
    last layer (crab_llama_io.last_rows_only): the same phase priced on the FLOPs it actually executes, so that the skipped work is not read as
    matrix-pipe efficiency."""
    from crab_amd import decoder
    dead = dead_last_layer_flops(S, cfg) if decoder.LAST_ROWS_ONLY else 0.0
    ex = algo_flops_per_clip - dead
    return {"last_rows_only": bool(decoder.LAST_ROWS_ONLY), "tflop_per_clip": round(ex / 1e12, 3), "dead_tflop_per_clip_skipped": round(dead / 1e12, 3),
            "achieved": round(ex / (ms_per_clip * 1e-3) / 1e12, 1), "frac": round(ex / (ms_per_clip * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}


def _rccl_version():
    try:
        return ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception as e:      # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def qwen_variant(llama_model, args):
    """BASELINE configs[2]: "AVE temporal-localization eval, Qwen-7B backbone (unified_qwen.py path), bf16, 1 x MI355X" - the Qwen2-7B decoder
    (GQA 28 / 4, q|k|v bias, vocab 152k; models/unified_qwen.py) on the AVE eval's workload (r06; r05 timed it on the AVQA prompt shape):
      * prompt = the AVE instruction (dataset/quick_start_dataset.py:172: "This is a video: <video_start><video><video_end> This is an audio:
        <audio_start><audio><audio_end> Please describe the events and time range that occurred in the video.") behind the chat template:
        48 synthetic text-token ids stand in for it (no Qwen tokenizer offline) with the two placeholder triples at fixed offsets;
      * video_frame_nums = 10 frames (scripts/finetune/inference_hyper_lora.sh:58; dataset/unified_dataset.py:1839-1858) -> 320 video tokens;
      * ten 1-s audio windows of 98 fbank frames (:1861-1886) -> 320 audio tokens; prefill length 48 - 2 + 640 = 686;
      * 256 generated tokens (the metric's output length; the reference's loop allows 500, inference_hyper_lora.py:177).
    Timed by the same process right after the headline: the Llama model's KV caches and graphs are released first (its weights stay), one warm-up +
    two timed steps of 256 clips, prefill fraction from the three phase marks recorded in the second of them.  Never `value`."""
    from crab_amd import ops, synth
    from crab_amd.build_model import build_crab
    llama_model.base_model.model._engine.invalidate()
    ops._SPLITK_WS.clear()
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    model = build_crab("qwen", device=torch.device("cuda", torch.cuda.current_device()), seed=42)
    um = model.base_model.model
    FR, NT = 10, 48
    S = NT - 2 + 32 * FR + 320
    free_now, _ = torch.cuda.mem_get_info()
    per_clip = um._engine.bytes_per_sequence(S, args.new_tokens) + (16 << 20)
    B = next((b for b in (256, 128) if b * per_clip + (12 << 30) <= free_now), 64)
    tab = um.SPECIAL_TOKEN_2_IDS
    ids = [synth.synth_prompt_ids(NT, model.base_vocab, tab, clip=i) for i in range(B)]
    mods = [{'<video>': synth.synth_video(FR, clip=i).cuda(), '<audio>': synth.synth_audio(10, 98, clip=i).cuda()} for i in range(B)]
    lab = [torch.full_like(i, -100) for i in ids]
    ids = [i.cuda() for i in ids]
    build_s = time.perf_counter() - t0

    def go():
        return model.generate(batch_input_ids=ids, batch_labels=lab, batch_X_modals=mods, batch_task_names=['ave'] * B, use_cache=True,
                              max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, eos_token_id=um.config.eos_token_id,
                              pad_token_id=um.model.pad_token_id, output_logits=False)
    go()
    torch.cuda.synchronize()
    ts = []
    prof = ops.KernelProfiler(phase_only=True)
    for i in range(2):
        if i == 1:
            ops.PROFILER = prof                        # the second timed step carries the three phase marks (three HIP event records: nothing else changes)
        t1 = time.perf_counter()
        r = go()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t1)
        ops.PROFILER = None
    assert tuple(r.shape) == (B, args.new_tokens)
    pre_ms, dec_ms = prof.phase_ms()
    V = um.lm_head.weight.shape[0]
    fl = flops_per_clip(FR, 10, 48, S, V, um.config)
    dt = sum(ts) / len(ts)
    out = {"workload": "AVE temporal-localization eval, Qwen2-7B + BEATs + CLIP-ViT-L/14, bf16 (BASELINE configs[2]): AVE instruction template, 10 frames, "
                       "ten 1-s audio windows, 256 new tokens", "clips_per_step": B, "frames": FR, "prompt_tokens": NT, "prefill_len": S,
           "clips_per_s": round(B / dt, 3), "ms_per_step_calls": [round(x * 1e3, 1) for x in ts], "build_s": round(build_s, 1),
           "prefill_tflop_per_clip": round(fl / 1e12, 3),
           "prefill_roofline": {"bound": "mfma", "achieved": round(fl * B / (pre_ms * 1e-3) / 1e12, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": round(fl * B / (pre_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4), "ms_per_clip": round(pre_ms / B, 3),
                                "decode_ms_per_clip": round(dec_ms / B, 3)},
           "note": "the AVQA-shaped run of this decoder (r05: 54.5 clips/s at 512 clips) is `python bench.py --llm qwen`"}
    um._engine.invalidate()
    del model, um
    torch.cuda.empty_cache()
    return out


def avss_pixel_path(model, um, args):
    """BASELINE configs[4]: "AVSS pixel-level path (mask_decoder.py + taming_transformer VQ), bf16, 1 x MI355X" as a THROUGHPUT path (r06): the
    reference's pixel loops (scripts/quick_start.py:270-450, inference_hyper_lora.py:34-150) make one generate_avs call per sample (r05: 2.68
    samples/s, 368 ms of a 372 ms sample in bs-1 generation); UnifiedForCausalLM.generate_avs_many runs N such calls together - one ragged decode
    batch with per-step hidden states, per-row <mask_i> picks, SegModule batched per class count - and the loop's device work follows (label maps
    for the PNGs, IoU / F-measure / per-class areas).  Workload per sample: one 224 x 224 image (CLIP multi-scale features), one 1-s audio window,
    a 48-token prompt, max_new_tokens = 100 (inference_hyper_lora.py:54), 3 of 4 samples binary (s4 / ms3 / ref-avs), 1 of 4 avss (71 classes).
    A random decoder never emits the six <mask_i> tokens, so the pick rule is replaced by "the last six steps" for EVERY sample (the work of a
    sample that segments; the product's rule is exercised by tests/test_model_gpu.py::test_generate_avs_many_equals_one_sample_calls)."""
    from crab_amd import avss_utils, ops, synth
    from crab_amd.build_model import randomize_
    t0 = time.perf_counter()
    inner = model.get_model()
    if getattr(inner, "seg_module", None) is None:
        inner.init_multimodal_modules(d_model=um.config.hidden_size, segment_branch=True)
        randomize_(inner.seg_module, seed=5)
        g = torch.Generator(device="cuda").manual_seed(77)
        for name, buf in inner.seg_module.named_buffers():          # the SAM-style random Fourier matrices are buffers the reference never saves
            if name.endswith("positional_encoding_gaussian_matrix"):
                buf.normal_(generator=g)
    # samples per call (CRAB_BENCH_AVS_SAMPLES): 512 = CRAB_DECODE_MAX_ROWS, the headline's decode batch.  Measured r06: 128 samples 115.7 samples/s (8.2 ms per
    # decode step), 256 159.7 (10.4 ms), 512 181.7 (17.2 ms; it first failed with "hyperlora_route: workspace too small" - the non-monotone workspace query, fixed)
    N, NEW, NT = int(os.environ.get("CRAB_BENCH_AVS_SAMPLES", "512")), 100, 48
    sp = um.SPECIAL_TOKEN_2_IDS
    samples, gts = [], []
    gg = torch.Generator().manual_seed(9)
    for i in range(N):
        ids = synth.synth_prompt_ids(NT + (i % 5), model.base_vocab, sp, clip=7000 + i)          # prompt lengths 48 .. 52: a ragged batch, like real instructions
        for a_, b_ in (("<video_start>", "<image_start>"), ("<video>", "<image>"), ("<video_end>", "<image_end>")):
            ids[ids == sp[a_]] = sp[b_]
        task = 'avss' if i % 4 == 3 else ('s4', 'ms3', 'ref-avs')[i % 3]
        samples.append({"batch_input_ids": [ids.cuda()], "batch_labels": [torch.full_like(ids, -100)],
                        "batch_X_modals": [{'<image>': synth.synth_video(1, clip=7000 + i).cuda(), '<audio>': synth.synth_audio(1, 98, clip=7000 + i).cuda()}],
                        "batch_task_names": [task]})
        gts.append(torch.randint(0, 71, (1, 224, 224), generator=gg).cuda() if task == 'avss' else (torch.rand(1, 224, 224, generator=gg) > 0.5).float().cuda())
    kw = dict(max_new_tokens=NEW, min_new_tokens=NEW, pad_token_id=um.model.pad_token_id, eos_token_id=um.config.eos_token_id, use_cache=True)
    chosen = [(g_, 0, list(range(NEW - 7, NEW - 1))) for g_ in range(N)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def go(phase_prof=None):
        ops.PROFILER = phase_prof
        inputs, outs = um._avs_generate(samples, None, kw)
        ops.PROFILER = None
        ev[0].record()
        res = um._avs_segment(samples, inputs, outs, chosen)
        ev[1].record()
        vals = []
        for r, gt, sm in zip(res, gts, samples):          # what the loop does with every mask, on the device (harness.run_inference_avs)
            pred = r['pred_masks'][0].float()
            ops.mask_labels(pred)
            if pred.shape[0] > 1:
                vals.append(avss_utils.calc_color_miou_fscore(pred=pred.unsqueeze(0), target=gt, T=1)[0])
            else:
                vals.append(avss_utils.mask_iou(pred=pred, target=gt))
        ev[2].record()
        return res, vals

    go()
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    ts, seg_ms, met_ms = [], [], []
    prof = ops.KernelProfiler(phase_only=True)
    for i in range(2):
        t1 = time.perf_counter()
        res, vals = go(prof if i == 1 else None)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t1)
        seg_ms.append(ev[0].elapsed_time(ev[1]))
        met_ms.append(ev[1].elapsed_time(ev[2]))
    assert all(r['pred_masks'][0] is not None and r['output_ids'].shape == (1, NEW) for r in res)
    pre_ms, dec_ms = prof.phase_ms()
    dt = sum(ts) / len(ts)
    S_ = NT + 4 - 2 + 32 + 32                                   # longest prompt: text - 2 placeholders + 32 image + 32 audio tokens
    steps = NEW - 1
    algo = sum(decode_bytes_per_step(N, S_ + t + 1, V=um.lm_head.weight.shape[0]) for t in range(steps))
    um._engine.invalidate()
    torch.cuda.empty_cache()
    return {"workload": "AVSS pixel-level path, Llama-2-7B + CLIP ViT-L/14 (multi-scale) + BEATs + SegModule, bf16 (BASELINE configs[4]); one image + one "
                        "1-s audio window + 48..52-token prompt per sample, 100 new tokens, " + f"{N - N // 4} binary + {N // 4} avss (71-class) samples per call",
            "samples_per_call": N, "new_tokens": NEW, "prefill_len": f"{S_ - 4}..{S_}", "samples_per_s": round(N / dt, 2),
            "ms_per_call": [round(x * 1e3, 1) for x in ts], "ms_per_sample": round(dt * 1e3 / N, 3),
            "pixel_head_ms_per_sample": round(sum(seg_ms) / len(seg_ms) / N, 3), "labels_and_metrics_ms_per_sample": round(sum(met_ms) / len(met_ms) / N, 3),
            "encode_prefill_ms_per_sample": round(pre_ms / N, 3), "decode_ms_per_token": round(dec_ms / steps, 3),
            "decode_roofline": {"bound": "hbm", "algorithmic_bytes": int(algo), "achieved_GBps": round(algo / (dec_ms * 1e-3) / 1e9, 1), "peak_GBps": HBM_PEAK_GBS,
                                "frac": round(algo / (dec_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "note": "weights + adapters once per step + the live KV rows of the samples of the call, over the decode phase (HIP events)"},
            "reference_loop_r05": {"samples_per_s": 2.68, "source": "profiles/r05_avs_config4.json: one generate_avs call per sample, as the reference's loops run it"},
            "setup_s": round(setup_s, 1),
            "pick_rule": "the last six steps of every sample (a random decoder never emits <mask_i>): every sample goes through the SegModule",
            "api": "UnifiedForCausalLM.generate_avs_many (harness.run_inference_avs(coalesce=True)); per-sample results = those of one-sample generate_avs calls within the "
                   "mask decoder's bf16 tolerance (tests/test_model_gpu.py)"}


DUMP_BYTES = 64_000_000          # --dump-outputs writes at most this much in all


def dump_outputs(out_dir, res):
    """--dump-outputs: what the last timed step handed its caller on rank 0, as float32 .npy files: `sequences` = the generated ids of every
    clip [clips, new_tokens] in clip order (ids < 2^24 are exact in float32) and `first_logits` = the fp32 first-step logits [clips, V].  Where
    the logits of all clips would pass DUMP_BYTES, a fixed seeded sample of whole rows is written, and `first_logits_clip_ids` names its clips."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    cid, ids, logits = res
    seq = ids.cpu().numpy().astype(np.float32)
    np.save(os.path.join(out_dir, "sequences.npy"), seq)
    if logits is None:                                    # --no-gather-logits
        return
    lg = logits.float().cpu().numpy()
    n, V = lg.shape
    k = max(0, min(n, (DUMP_BYTES - seq.nbytes - 4 * n - 3 * 4096) // (4 * V)))      # room beside the ids, the clip ids and three .npy headers
    rows = np.arange(n) if k == n else np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
    np.save(os.path.join(out_dir, "first_logits.npy"), np.ascontiguousarray(lg[rows]))
    np.save(os.path.join(out_dir, "first_logits_clip_ids.npy"), cid.cpu().numpy()[rows].astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=int(os.environ.get("CRAB_BENCH_CLIPS", "0")),
                    help="clips per GPU per step (with --strong: in total); 0 = as many of 512 / 448 / 384 / 320 / 256 as the device's free memory holds "
                         "(KV cache 0.47 GiB per clip; 512 on an idle 288 GB MI355X): decode streams the weights once per step for all of them")
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--prefill-chunk", type=int, default=0, help="sequences per prefill chunk; 0 = planned per batch (whole tile rounds)")
    ap.add_argument("--decode-streams", type=int, default=int(os.environ.get("CRAB_DECODE_STREAMS", "1")),
                    help="decode groups replayed on separate HIP streams (KV-cache attention of one overlaps projections of another)")
    ap.add_argument("--llm", default="llama")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline does not need: one instrumented step for the roofline blocks and "
                         "(N = 1) the pixel path, the Qwen2 variant, the reference's operating points and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the ids and first-step logits of the last timed step to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-gather-logits", action="store_true", help="gather token ids only (default: ids + first-step fp32 logits of every clip)")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: --clips is the TOTAL over all ranks (contiguous blocks, the first total %% N ranks hold one more clip); "
                         "default is weak scaling (--clips per GPU)")
    ap.add_argument("--time-budget", type=float, default=float(os.environ.get("CRAB_BENCH_TIME_BUDGET", "540")),
                    help="with --full: seconds this process may take in all (N = 1); the pixel path, the Qwen2 variant and the reference operating points "
                         "behind the headline are admitted against it in order of importance and say so when skipped - the JSON line is printed last and "
                         "must not be lost to a launcher's limit (540 s: a --full run ends within 10 minutes unless its own steps take longer)")
    ap.add_argument("--no-operating-points", action="store_true",
                    help="with --full: skip the extra (untimed-region) runs at the reference's own operating points: eval batch 8, 10 frames, 2-s audio windows")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks here, exactly as the driver's
        # `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` would (one process per GPU, RCCL over xGMI)
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # test hooks (no effect in a normal launch): CRAB_BENCH_SINGLE_DEVICE=1 maps every rank to cuda:0 and CRAB_BENCH_BACKEND=gloo
    # swaps RCCL for gloo, so the multi-process path (rendezvous, barriers, max-over-ranks, gather, rank-0 line) can be exercised on
    # a one-GPU box
    if os.environ.get("CRAB_BENCH_SINGLE_DEVICE") == "1":
        local = 0
    backend = os.environ.get("CRAB_BENCH_BACKEND", "nccl")
    single_dev = os.environ.get("CRAB_BENCH_SINGLE_DEVICE") == "1"
    if world > 1 and not single_dev and torch.cuda.device_count() < world:
        sys.exit(f"bench.py: {world} ranks need {world} visible GPUs, found {torch.cuda.device_count()} (one process per GPU)")
    torch.cuda.set_device(local)
    if world > 1:
        # N ranks share one host: each keeps cores / N threads for its host-side work (input synthesis, the splice plan), instead of every
        # rank starting a full-width thread pool (8 x 128 threads oversubscribed the host and showed up as warm-up stragglers)
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))
    dist = None
    # CRAB_BENCH_FORCE_DIST=1 (test hook): make the process group even for ONE rank, so that the RCCL code path - communicator init with
    # device_id, barrier, all_reduce, all_gather, the result gather - really executes on a one-GPU box (tests/test_bench_launch.py)
    force_dist = os.environ.get("CRAB_BENCH_FORCE_DIST") == "1"
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)

    from crab_amd import ops, synth
    from crab_amd.build_model import build_crab
    from crab_amd.parallel import block_of, gather_results

    t_setup = time.perf_counter()
    # every rank holds a full replica (13.8 GB of weights in bf16) + its own KV cache: say so BEFORE the allocator does when a device is
    # already occupied (a stale process on one GPU of the node would otherwise surface as an OOM traceback on one rank and a hang on the others)
    free0, total0 = torch.cuda.mem_get_info(local)
    if free0 < 20 * 2 ** 30:
        sys.exit(f"bench.py: rank {rank}: cuda:{local} has {free0 / 2**30:.1f} GiB free of {total0 / 2**30:.1f}: a weight replica (13.8 GB) + the KV cache "
                 f"of even one clip do not fit; is another process holding this GPU?")
    model = build_crab(args.llm, device=torch.device("cuda", local), seed=42)
    um = model.base_model.model
    tab = um.SPECIAL_TOKEN_2_IDS
    if args.clips <= 0:
        # capacity-driven batch (r04): the decode projections amortise the weight stream over up to 512 rows (two 256-row groups per block,
        # csrc/gemm_decode.hip), so the step takes as many clips as the KV cache has room for.  Every rank evaluates the same rule on its own
        # device; the smallest answer is used by all (weak scaling keeps clips per GPU equal).
        free_now, _ = torch.cuda.mem_get_info(local)
        # per clip: its KV cache + decode rows (bytes_per_sequence) + its resident inputs and encoder outputs - measured r05: the allocator's peak grows by
        # 515 MB per clip between 448 and 512 clips (503.5 MB of it KV cache), 16.8 GiB are fixed (14.4 of them the weights, loaded before this line);
        # the rule keeps 12 GiB + 4.5 MB per clip beyond that.  512 = CRAB_DECODE_MAX_ROWS: both 256-row groups of the decode projections full
        per_clip = um._engine.bytes_per_sequence(126 + 32 * args.frames + 320, args.new_tokens) + (16 << 20)
        # (512 keeps 20 GiB beyond its estimate: an idle device has 272.9 GiB free here and ends its warm-up with 17.5 GiB to spare)
        pick = next((b for b in (512, 448, 384, 320, 256) if b * per_clip + ((20 if b == 512 else 12) << 30) <= free_now), 256)
        if dist is not None:
            tpick = torch.tensor([pick], device="cuda" if backend == "nccl" else "cpu", dtype=torch.int64)
            dist.all_reduce(tpick, op=dist.ReduceOp.MIN)
            pick = int(tpick.item())
        args.clips = pick * (world if args.strong else 1)
        args.clips_auto = True
    if args.strong:
        clip0, B = block_of(args.clips, world, rank)          # fixed TOTAL work: rank r owns a contiguous block of the args.clips clips
        if B == 0:
            sys.exit(f"bench.py --strong: {args.clips} clips over {world} ranks leave rank {rank} without work")
    else:
        B = args.clips                                        # weak scaling: args.clips per GPU
        clip0 = rank * B
    n_total = args.clips if args.strong else world * B
    ids = [synth.synth_prompt_ids(128, model.base_vocab, tab, clip=clip0 + i) for i in range(B)]
    mods = [{'<video>': synth.synth_video(args.frames, clip=clip0 + i).cuda(), '<audio>': synth.synth_audio(10, 98, clip=clip0 + i).cuda()}
            for i in range(B)]
    lab = [torch.full_like(i, -100) for i in ids]
    ids = [i.cuda() for i in ids]
    eos = um.config.eos_token_id
    V = um.lm_head.weight.shape[0]

    def step():
        out = model.generate(batch_input_ids=ids, batch_labels=lab, batch_X_modals=mods, batch_task_names=['avqa'] * B,
                             use_cache=True, max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, eos_token_id=eos,
                             pad_token_id=um.model.pad_token_id, prefill_chunk=args.prefill_chunk, output_logits=False,
                             decode_streams=args.decode_streams, output_first_logits=not args.no_gather_logits)
        if args.no_gather_logits:
            return gather_results(out, clip0, world, rank)
        # north_star: "RCCL gather of logits": rank 0 receives {clip id, ids[new_tokens]} and the fp32 first-step logits [V] of every clip
        return gather_results(out.sequences, clip0, world, rank, logits=out.first_logits)

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    t_build = time.perf_counter() - t_setup
    # early, per rank, on stderr: a straggler (slow build, occupied device) is visible long before the JSON line or a launcher timeout
    print(f"[bench rank {rank}/{world}] built in {t_build:.1f} s on cuda:{local} ({free0 / 2**30:.0f} GiB free), {B} clips per step, "
          f"{torch.get_num_threads()} host threads", file=sys.stderr, flush=True)
    t_w = time.perf_counter()
    for i in range(args.warmup):
        tw = time.perf_counter()
        step()
        if i == 0:
            torch.cuda.synchronize()
            print(f"[bench rank {rank}/{world}] first warm-up step {time.perf_counter() - tw:.1f} s", file=sys.stderr, flush=True)
        else:
            print(f"[bench rank {rank}/{world}] warm-up step {i + 1}/{args.warmup} {time.perf_counter() - tw:.1f} s", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    t_warm = time.perf_counter() - t_w
    # capacity: generate() splits a batch whose KV cache + scratch do not fit the device into groups that run one after the other (with a
    # warning); the line says so (decode_groups), and a rank that cannot hold ONE clip has already raised inside generate()
    plan = um._engine.last_plan or {}
    free1, _ = torch.cuda.mem_get_info(local)
    rank_info = {"rank": rank, "build_s": round(t_build, 1), "warmup_s": round(t_warm, 1), "clips": B, "decode_groups": len(plan.get("groups", [B])),
                 "kv_bytes_per_clip": int(plan.get("bytes_per_seq", 0)), "free_gib_before": round(free0 / 2 ** 30, 1), "free_gib_after_warmup": round(free1 / 2 ** 30, 1)}
    # ---- the timed region: the SHIPPED path (native layer sequencers, every decode step a HIP-graph replay, no profiler attached)
    assert ops.PROFILER is None
    # with --full the LAST timed step carries the three phase marks of generate() (encode_begin / prefill_end / decode_end: three HIP event records
    # on a ~16 s step, nothing else changes - the native sequencers and the graph replays run underneath): the source of prefill_roofline
    phase_prof = ops.KernelProfiler(phase_only=True) if args.full else None
    sync()
    t0 = time.perf_counter()
    step_ms = []
    for i_step in range(args.steps):
        ts = time.perf_counter()
        if i_step == args.steps - 1:
            ops.PROFILER = phase_prof
        res = step()                       # generate() ends with a device->host read of the step count: the step is complete
        ops.PROFILER = None
        step_ms.append(round((time.perf_counter() - ts) * 1e3, 1))
        # one stderr line per ~16 s step (microseconds): a long run is never silent for minutes before its JSON line
        print(f"[bench rank {rank}/{world}] timed step {i_step + 1}/{args.steps} {step_ms[-1] / 1e3:.1f} s", file=sys.stderr, flush=True)
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res)
    if args.full:
        pre_ms, dec_ms = phase_prof.phase_ms()
        # ---- ONE extra, un-timed, instrumented step for the roofline blocks: HIP events around every GEMM >= 512 rows (per-launch Python
        # sequence instead of the native sequencer) and around the decode-attention kernel on every 32nd decode step, which runs eagerly
        # (bit-identical to the graph replay it stands in for, tests/test_model_gpu.py).  Its wall time is reported next to the timed one.
        prof = ops.KernelProfiler(min_m=512, decode_every=32)
        ops.PROFILER = prof
        sync()
        ti = time.perf_counter()
        step()
        sync()
        instrumented_ms = (time.perf_counter() - ti) * 1e3
        ops.PROFILER = None
    rank_ms = [round(dt / args.steps * 1e3, 2)]
    rank_infos = [rank_info]
    if dist is not None:
        rank_infos = [None] * world
        dist.all_gather_object(rank_infos, rank_info)
        # every rank's own wall time of the K steps (a straggler shows up here); `value` uses the MAX over ranks
        tt = torch.tensor([dt], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
        allt = [torch.empty_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        rank_ms = [round(float(t.item()) / args.steps * 1e3, 2) for t in allt]
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    if rank == 0:
        # the gather really delivered every rank's clips (ordered by clip id) to rank 0
        assert res is not None and res[1].shape[0] == n_total and res[0].tolist() == list(range(n_total)), "gather incomplete"
        assert args.no_gather_logits or (res[2] is not None and tuple(res[2].shape) == (n_total, V)), "first-step logits not gathered"
        n_clips = n_total * args.steps
        S = 126 + 32 * args.frames + 320
        line = {
            "metric": "clips/sec prefill+decode (AVQA 10s clip, 8 frames, 256 out tok)",
            "value": round(n_clips / dt, 4), "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic (seeded N(0,0.02) weights, synthetic 8x224x224 frames, 10x98x128 fbank, 128-token prompt)",
            "config": {"workload": ("AVQA eval, Llama-2-7B + BEATs + CLIP-ViT-L/14, bf16 (BASELINE configs[1])" if args.llm == "llama" else
                                     "AVQA eval, Qwen2-7B + BEATs + CLIP-ViT-L/14, bf16 (BASELINE configs[2] decoder)"), "clips_per_gpu_per_step": B if not args.strong else [ri["clips"] for ri in rank_infos],
                       "total_clips_per_step": n_total,
                       "clips_chosen_by": "free device memory (KV cache per clip)" if getattr(args, "clips_auto", False) else "--clips",
                       "frames": args.frames, "audio_segments": 10, "prompt_tokens": 128, "prefill_len": S, "new_tokens": args.new_tokens,
                       "decode": "greedy, EOS suppressed, device-resident HIP-graph loop", "parallelism": f"per-clip x{world} (contiguous blocks of clips per rank), RCCL gather",
                       "collective_backend": (backend + (" (RCCL)" if backend == "nccl" else "")) if dist is not None else None,
                       "world_size_observed": dist.get_world_size() if dist is not None else 1,
                       "rccl_version": _rccl_version() if (backend == "nccl" and dist is not None) else None,
                       "host_threads_per_rank": torch.get_num_threads(),
                       "gathered_per_clip": "clip id + ids" + ("" if args.no_gather_logits else f" + first-step fp32 logits[{V}]"),
                       "gathered_clips": int(res[1].shape[0])},
            "rank_ms_per_step": rank_ms,
            "ranks": rank_infos,
            "prefill_tflop_per_clip": round(flops_per_clip(args.frames, 10, 48, S, V, um.config) / 1e12, 3),
            "step_ms": step_ms,
            "timed_region": "the shipped path: native layer sequencers + HIP-graph replay of every decode step; no profiler attached"
                            + (" except three phase-mark event records in the last step" if args.full else ""),
            "residual_stream": "fp32" if ops.RESIDUAL_FP32 else "bf16",
        }
        if args.full:
            # per-kernel roofline entries from the live HIP-event samples; the dominant kernel is the one with the largest
            # (estimated) total time in the timed region: GEMM buckets are timed on every launch, the decode-attention
            # kernel on the sampled eager decode steps (x its launch count = steps * (new_tokens-1) * layers)
            n_layers = um.config.num_hidden_layers
            entries = []
            for name, d in prof.summary().items():
                avg_ms = d["ms"] / d["launches"]
                if name.startswith("attn_decode"):
                    total_launches = args.steps * (args.new_tokens - 1) * n_layers       # launches in the TIMED region; the average comes from the instrumented step
                    ach = d["work"] / (d["ms"] * 1e-3) / 1e9
                    e = {"bound": "hbm", "kernel": name, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4),
                         "traffic": round(d["work"] / d["launches"] * ATTN_DECODE_TRAFFIC_PER_ALGO_BYTE),
                         "algorithmic_bytes_per_launch": round(d["work"] / d["launches"]),
                         "traffic_source": "PMC ratio from profiles/r06_pmc_attn_decode.txt (= r05_pmc_attn_decode_512clips.txt; separate --pmc passes at 512 clips x ctx 830) x this run's bytes"}
                else:
                    total_launches = d["launches"] * args.steps                            # the instrumented step's launches x the K timed steps
                    ach = d["work"] / (d["ms"] * 1e-3) / 1e12
                    e = {"bound": "mfma", "kernel": name, "achieved": round(ach, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(ach / MFMA_PEAK_TFLOPS, 4), "traffic": None,
                         "note": "all launches of this kernel in the instrumented step: decoder prefill projections AND the encoders' (CLIP K = 1024) shapes",
                         "by_class": {c: {"launches": v["launches"], "achieved": round(v["work"] / (v["ms"] * 1e-3) / 1e12, 1),
                                          "frac": round(v["work"] / (v["ms"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}
                                      for c, v in d.get("classes", {}).items() if v["ms"] > 0}}
                e.update({"sampled_launches": d["launches"], "avg_launch_us": round(avg_ms * 1e3, 1),
                          "est_total_ms_in_timed_region": round(avg_ms * total_launches, 1)})
                entries.append(e)
            entries.sort(key=lambda e: -e["est_total_ms_in_timed_region"])
            # the north-star target quantity: fused encoder + decoder prefill (prepare_multimodal_inputs + chunked prefill +
            # first-token selection) of all clips, algorithmic FLOPs / HIP-event time of that phase
            pre_ms_instr, _ = prof.phase_ms()
            pre_flops = flops_per_clip(args.frames, 10, 48, S, V, um.config) * B                    # the ONE instrumented step
            line.update({
                "instrumented_step": {"ms": round(instrumented_ms, 1), "timed": False,
                                      "note": "one extra step after the timed region with HIP events on every GEMM >= 512 rows and on the decode attention of "
                                              "every 32nd (eager) decode step: the source of roofline / roofline_mfma / prefill_roofline"},
                "prefill_roofline": {"bound": "mfma", "phase": "encoders + decoder prefill (whole phase, all kernels)",
                                     "achieved": round(pre_flops / (pre_ms * 1e-3) / 1e12, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                     "frac": round(pre_flops / (pre_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                                     "ms_per_clip": round(pre_ms / B, 3), "decode_ms_per_clip": round(dec_ms / B, 3),
                                     "executed": _executed_block(pre_flops / B, S, um.config, pre_ms / B),
                                     "source": "the last timed step of the shipped path, which carries three phase marks (HIP event records); the per-launch "
                                               f"instrumented step measures {round(pre_ms_instr / B, 3)} ms per clip for the same phase"},
                "roofline": entries[0] if entries else None,
                "roofline_mfma": next((e for e in entries if e["bound"] == "mfma"), None),
            })
            # ---- behind the headline, in order of importance (every block admitted against --time-budget; the line is printed last):
            #      BASELINE configs[4] (pixel path), configs[2] (Qwen2 on the AVE workload), the reference's own operating points, the CPU sample
            if world == 1 and not args.no_operating_points and args.llm == "llama":
                if time_left(args) < 25 + QWEN_RESERVE_S + CPU_RESERVE_S:
                    line["avss_pixel_path"] = {"skipped": f"--time-budget {args.time_budget:.0f} s: {max(time_left(args), 0):.0f} s left; `python scripts/bench_avs.py` gives it on its own"}
                else:
                    try:
                        um._engine.invalidate()                # the headline's 2 x 100 GiB of KV cache: the pixel batch allocates its own (small) one
                        torch.cuda.empty_cache()
                        line["avss_pixel_path"] = avss_pixel_path(model, um, args)
                    except Exception as e:      # the headline must still be reported
                        line["avss_pixel_path"] = {"error": f"{type(e).__name__}: {e}"}
                if time_left(args) < QWEN_RESERVE_S + CPU_RESERVE_S:
                    line["qwen2_7b_variant"] = {"skipped": f"--time-budget {args.time_budget:.0f} s: {max(time_left(args), 0):.0f} s left; `python bench.py --llm qwen` gives the "
                                                           "decoder as a line of its own"}
                else:
                    try:
                        line["qwen2_7b_variant"] = qwen_variant(model, args)
                    except Exception as e:      # the headline must still be reported
                        line["qwen2_7b_variant"] = {"error": f"{type(e).__name__}: {e}"}
                line["reference_operating_points"] = operating_points(model, um, args, eos, dt / args.steps)
            line["process_s"] = {"time_budget": args.time_budget, "before_cpu_baseline": round(time.perf_counter() - T_PROCESS0, 1)}
            if world == 1 and not args.no_cpu_baseline:
                try:
                    line["cpu_baseline"] = cpu_baseline(args)
                except Exception as e:      # the GPU number must still be reported
                    line["cpu_baseline"] = {"value": None, "unit": "clips/s", "cores": torch.get_num_threads(), "kind": "port",
                                            "sample": f"failed: {type(e).__name__}: {e}"}
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
