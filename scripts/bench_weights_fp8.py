"""The opt-in FP8 decoder weights (weight_dtype = "fp8_e4m3") against the bf16 weights: what the M <= 16 weight-streaming kernel does with half
the bytes, and what the mode costs in accuracy.  Writes / updates profiles/weights_fp8.json.

usage: bench_weights_fp8.py [--timing] [--accuracy] [--out FILE] [--rounds 5] [--layers 32] [--new-tokens 33]   (default: both parts)

TIMING (GPU box).  gemm_skinny_dma_kernel (bf16) and gemm_skinny_dma_w8_kernel (FP8) run ALTERNATELY in one process on the four projection
groups of Llama-2-7B and of Qwen2-7B at M = 1, 8, 16.  Each timed round walks a ring of weight copies larger than the 256 MB last-level cache,
so every launch streams its weights from HBM as a decode step's launches do (the 32 layers of a step never meet their weights in a cache); three
warm-up walks, then `rounds` rounds per kernel, medians, and the run-to-run spread (max - min over the rounds) of each.  A shape whose FP8 median
is not below the bf16 median by more than the larger of the two spreads is listed under "no_gain".  Then a whole decode step (HIP-graph replay,
context ~700) of 1 clip and of 8 clips on the synthetic full-size Llama decoder in both modes, alternating, per-token milliseconds from the
phase marks of ops.KernelProfiler(phase_only=True).
ACCURACY (CPU, the oracle; no GPU needed).  The mode against bf16 weights - prefill with W, decode steps with dequant(quant(W)) (tests/w8_ref.py)
- on full_tiny_llama (max logit deviation over the logit scale), on the full-width single layer llama_layer_wide (decode-step outputs) and the
teacher-forced greedy-id agreement on id_stats_tiny_llama.  Reported, not gated: no trained checkpoint exists here."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF = torch.bfloat16
FP8 = "fp8_e4m3"
LLC_BYTES = 256 << 20
# (name, N, K): q|k|v, o, gate|up (interleaved), down of one decoder layer
SHAPES = {
    "llama2_7b": [("qkv", 3 * 4096, 4096), ("o", 4096, 4096), ("gate_up", 2 * 11008, 4096), ("down", 4096, 11008)],
    "qwen2_7b": [("qkv", (28 + 2 * 4) * 128, 3584), ("o", 3584, 3584), ("gate_up", 2 * 18944, 3584), ("down", 3584, 18944)],
}


def _timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3            # us per launch


def time_projections(rounds):
    from crab_amd import ops
    out, no_gain = [], []
    g = torch.Generator(device="cuda").manual_seed(1)
    for model, shapes in SHAPES.items():
        for name, N, K in shapes:
            copies = max(3, math.ceil(3 * LLC_BYTES / (N * K * 2)))       # the FP8 ring (half the bytes) still exceeds the cache
            ws = [(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF) for _ in range(copies)]
            w8 = [ops.weight_quant_fp8(w) for w in ws]
            for M in (1, 8, 16):
                x = torch.randn(M, K, device="cuda", generator=g).to(BF)
                y = torch.empty(M, N, device="cuda", dtype=BF)
                f16 = lambda i: ops.gemm(x, ws[i % copies], out=y)
                f8 = lambda i: ops.gemm(x, ws[i % copies], out=y, w8=w8[i % copies])
                with ops.launch_trace(0) as tr:
                    f16(0); f8(0)
                assert tr.launched("gemm_skinny_dma_kernel") == 1 and tr.launched("gemm_skinny_dma_w8_kernel") == 1, tr.counts
                n = 4 * copies
                for _ in range(3):
                    _timed(f16, n); _timed(f8, n)
                t16, t8 = [], []
                for _ in range(rounds):
                    t16.append(_timed(f16, n)); t8.append(_timed(f8, n))
                m16, m8 = statistics.median(t16), statistics.median(t8)
                s16, s8 = max(t16) - min(t16), max(t8) - min(t8)
                row = {"model": model, "group": name, "N": N, "K": K, "M": M, "weight_copies": copies,
                       "bf16_us": round(m16, 2), "fp8_us": round(m8, 2), "bf16_spread_us": round(s16, 2), "fp8_spread_us": round(s8, 2),
                       "bf16_TBps": round(N * K * 2 / m16 / 1e6, 3), "fp8_TBps": round((N * K + 4 * N) / m8 / 1e6, 3),
                       "fp8_over_bf16_time": round(m8 / m16, 3), "gain": bool(m16 - m8 > max(s16, s8))}
                out.append(row)
                if not row["gain"]:
                    no_gain.append(f"{model} {name} M={M}")
                print(json.dumps(row), flush=True)
            del ws, w8
            torch.cuda.empty_cache()
    return out, no_gain


def time_decode_step(layers, new_tokens, rounds):
    """ms per decoded token (graph replay) of 1 clip and of 8 clips at context ~700, both modes alternating in one process."""
    from crab_amd import ops
    from crab_amd.build_model import build_crab
    model = build_crab("llama", num_hidden_layers=layers, visual=False, audio=False)
    um = model.base_model.model
    out = []
    for B in (1, 8):
        emb = (torch.randn(B, 700, um.config.hidden_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)) * 0.5).to(BF)

        def per_token(mode):
            ops.PROFILER = prof = ops.KernelProfiler(phase_only=True)
            try:
                prof.mark("encode_begin")
                model.generate(inputs_embeds=emb, use_cache=True, max_new_tokens=new_tokens, min_new_tokens=new_tokens, eos_token_id=None, pad_token_id=2,
                               weight_dtype=mode)
                _, dec = prof.phase_ms()
            finally:
                ops.PROFILER = None
            assert um._engine.last_plan["weight_dtype_used"] == mode
            return dec / (new_tokens - 1)
        for mode in ("bf16", FP8):                     # warm-up: quantise, capture the graph of each mode
            per_token(mode)
        t = {"bf16": [], FP8: []}
        for _ in range(rounds):
            for mode in ("bf16", FP8):
                t[mode].append(per_token(mode))
        m16, m8 = statistics.median(t["bf16"]), statistics.median(t[FP8])
        s16, s8 = max(t["bf16"]) - min(t["bf16"]), max(t[FP8]) - min(t[FP8])
        row = {"clips": B, "context": 700, "layers": layers, "new_tokens": new_tokens, "bf16_ms_per_token": round(m16, 4), "fp8_ms_per_token": round(m8, 4),
               "bf16_spread_ms": round(s16, 4), "fp8_spread_ms": round(s8, 4), "fp8_over_bf16_time": round(m8 / m16, 3), "gain": bool(m16 - m8 > max(s16, s8)),
               "note": "whole step: the four FP8 groups of every layer + attention + tails + the bf16 lm_head"}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def accuracy():
    from oracle import crab_oracle as O
    from tests import w8_ref as WR
    from tests.test_oracle_golden import _full_cfg
    from tests.util import load_fixture, stored_params, weights_from_table, wide_layer_inputs
    res = {}
    # ---- full_tiny_llama: per-step logits, FP8-weight decode steps vs bf16-weight steps on the same contexts (the stored bf16 parameters, fp32 arithmetic)
    meta, A = load_fixture("full_tiny_llama")
    Ws = stored_params(O.strip_peft_prefix(weights_from_table(meta)))
    cfg = _full_cfg(meta)
    Wq = WR.dequantised_weights(Ws)
    for key in ("bs1", "bs2"):
        emb, ids = A[f"embeds_{key}"], A[f"ids_{key}"]
        plain, mixed = WR.mixed_steps(emb, Ws, Ws, cfg.decoder, ids), WR.mixed_steps(emb, Ws, Wq, cfg.decoder, ids)
        sc = plain.abs().max().item()
        res[f"full_tiny_llama/{key}"] = {"max_logit_deviation_over_logit_scale": (mixed - plain).abs().max().item() / sc, "logit_scale": sc,
                                         "first_token_deviation": (mixed[:, 0] - plain[:, 0]).abs().max().item(),
                                         "greedy_ids_equal_share": (mixed.argmax(-1) == plain.argmax(-1)).float().mean().item()}
    # ---- id_stats_tiny_llama: teacher-forced greedy ids of 24 unsearched clips against the reference's, both weight forms
    meta, A = load_fixture("id_stats_tiny_llama")
    Ws = stored_params(O.strip_peft_prefix(weights_from_table(meta)))
    cfg = _full_cfg(meta)
    Wq = WR.dequantised_weights(Ws)
    from tests.test_kv_fp8_gpu import _clip_inputs
    eq16 = eq8 = eq_modes = tot = 0
    worst = 0.0
    for i in range(len(meta["clips"])):
        ids, mods = _clip_inputs(meta, i)
        emb = O.prepare_multimodal_inputs([ids], mods, Ws, cfg)["inputs_embeds"]
        ref_ids = A["ids"][i:i + 1]
        plain, mixed = WR.mixed_steps(emb, Ws, Ws, cfg.decoder, ref_ids), WR.mixed_steps(emb, Ws, Wq, cfg.decoder, ref_ids)
        eq16 += int((plain.argmax(-1) == ref_ids).sum()); eq8 += int((mixed.argmax(-1) == ref_ids).sum())
        eq_modes += int((plain.argmax(-1) == mixed.argmax(-1)).sum()); tot += ref_ids.numel()
        worst = max(worst, (mixed - plain).abs().max().item() / plain.abs().max().item())
    res["id_stats_tiny_llama"] = {"steps": tot, "share_equal_reference_bf16_weights": eq16 / tot, "share_equal_reference_fp8_weights": eq8 / tot,
                                  "share_equal_between_modes": eq_modes / tot, "max_logit_deviation_over_logit_scale": worst,
                                  "smallest_recorded_margin": float(A["margin"].min())}
    # ---- llama_layer_wide: one Llama-2-7B-wide hyper-LoRA layer, prefill with W, the recorded decode steps with the dequantised weights
    meta, A = load_fixture("llama_layer_wide")
    Wt = weights_from_table(meta)
    ocfg = O.DecoderConfig(**{**meta["cfg"], "num_hidden_layers": 1, "vocab_size": 320})
    x, xs = wide_layer_inputs(meta)
    B, S, _ = x.shape
    Wl = {k: v for k, v in Wt.items()}
    Wlq = {k: (WR.roundtrip(v) if WR.PROJ.search("model." + k if not k.startswith("model.") else k) else v) for k, v in Wl.items()}
    n_q = sum(1 for k in Wl if not torch.equal(Wl[k].float(), Wlq[k].float()))
    rows = []
    with torch.no_grad():
        caches = [O.KVCache(), O.KVCache()]
        pos = torch.arange(S)[None].expand(B, S)
        for c in caches:
            O.decoder_layer(x, Wl, 0, ocfg, c, pos)
        scale = A["y_rows"].abs().max().item()
        seqs = A["step_seqs"]
        for t, x1 in enumerate(xs):
            p1 = torch.full((B, 1), S + t)
            y16 = O.decoder_layer(x1, Wl, 0, ocfg, caches[0], p1)[seqs, 0]
            y8 = O.decoder_layer(x1, Wlq, 0, ocfg, caches[1], p1)[seqs, 0]
            rows.append({"step": t, "fp8_vs_bf16_weights_over_output_scale": (y8 - y16).abs().max().item() / scale,
                         "bf16_weights_vs_reference": (y16 - A["y_steps"][t]).abs().max().item() / scale,
                         "fp8_weights_vs_reference": (y8 - A["y_steps"][t]).abs().max().item() / scale})
    res["llama_layer_wide"] = {"quantised_matrices": n_q, "decode_steps": rows, "rows": int(B), "output_scale": scale}
    for k, v in res.items():
        print(k, json.dumps(v), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_fp8.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=33)
    ap.add_argument("--no-step", action="store_true", help="projection shapes only")
    a = ap.parse_args()
    both = not (a.timing or a.accuracy)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.timing or both:
        if not torch.cuda.is_available():
            raise SystemExit("the timing part needs the GPU (no fallback): run --accuracy alone on a CPU box")
        t0 = time.time()
        proj, no_gain = time_projections(a.rounds)
        doc["projections"] = proj
        doc["no_gain"] = no_gain
        if not a.no_step:
            doc["decode_step"] = time_decode_step(a.layers, a.new_tokens, max(3, a.rounds - 2))
            doc["no_gain"] = no_gain + [f"decode step, {r['clips']} clip(s)" for r in doc["decode_step"] if not r["gain"]]
        doc["method"] = ("bf16 and FP8 kernels alternating in one process; every launch streams weights from HBM (ring of copies > 256 MB); medians of "
                         f"{a.rounds} rounds; spread = max - min over the rounds; gain = bf16 median - fp8 median > max(spread)")
        doc["device"] = torch.cuda.get_device_name(0)
        doc["timing_seconds"] = round(time.time() - t0, 1)
    if a.accuracy or both:
        doc["accuracy"] = accuracy()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
