"""Teacher-forced scoring benchmark (GPU box; a run without a GPU fails - there is nothing to fall back to).

Head alone: the fused lm_head + cross entropy (crab_lm_head_xent: lm_head_xent_kernel + xent_finish_kernel, no logits stored) against the
parent path's ops.gemm(out_fp32=True) on the SAME operands - the lower bound of any unfused scorer, which would still have to read the fp32
logits back.  The two alternate in one process, warmed, timed with device events; the plain GEMM's own run-to-run spread (p90 - p10 of its
repetitions) is the unit the difference is held against.  Share of peak = algorithmic FLOPs (2 M N K) over the time, over the dense bf16 MFMA
peak; the bounding resource is the larger of FLOPs / peak and bytes / HBM peak.

Whole call: UnifiedForCausalLM.score() at the benchmark's clip shape (S = 702 rows per clip, 16 labelled tail tokens), in clips/s, next to
the prefill phase time of generate(max_new_tokens=1) on the same batch (the engine's phase marks; the whole call is recorded too).  Recorded,
not asserted.

    python scripts/bench_score.py [--out profiles/score_lm_head.json] [--clips 128] [--reps 20] [--no-model]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

BF = torch.bfloat16
PEAK_BF16 = 2.5e15        # dense bf16 MFMA, FLOP/s (MI355X spec)
PEAK_HBM = 8.0e12         # bytes/s (spec)


def _pct(v, p):
    s = sorted(v)
    return s[min(len(s) - 1, max(0, round(p * (len(s) - 1))))]


def head_alone(M, N, K, reps, inner=3):
    from crab_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn((M, K), device="cuda", generator=g).to(BF)
    w = (0.02 * torch.randn((N, K), device="cuda", generator=g)).to(BF)
    lab = torch.randint(0, N, (M,), device="cuda", generator=g).to(torch.int32)
    logits = torch.empty((M, N), device="cuda", dtype=torch.float32)
    lp, ls = torch.empty((M,), device="cuda"), torch.empty((M,), device="cuda")
    am = torch.empty((M,), device="cuda", dtype=torch.int32)
    ws = torch.empty((ops.lm_head_xent_bytes(M, N),), device="cuda", dtype=torch.uint8)
    fused = lambda: ops.lm_head_xent(x, w, lab, logprob=lp, lse=ls, argmax=am, workspace=ws)
    plain = lambda: ops.gemm(x, w, out=logits, out_fp32=True)
    with ops.launch_trace() as tr:
        for _ in range(3):
            fused(); plain()
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3          # us per call

    tf, tp = [], []
    for _ in range(reps):                                  # alternating: drift and neighbours on the host hit both alike
        tf.append(timed(fused))
        tp.append(timed(plain))
    # same numbers? (the parent path's logits reduced by torch, on a sample of rows)
    rows = torch.arange(0, M, max(1, M // 64), device="cuda")
    ref = torch.logsumexp(logits[rows].double(), -1)
    d_lse = float((ls[rows].double() - ref).abs().max())
    flops = 2.0 * M * N * K
    by_f = (M * K + N * K) * 2 + ws.numel()
    by_p = (M * K + N * K) * 2 + M * N * 4
    mf, mp = statistics.median(tf), statistics.median(tp)
    t_mfma, t_hbm_f, t_hbm_p = flops / PEAK_BF16 * 1e6, by_f / PEAK_HBM * 1e6, by_p / PEAK_HBM * 1e6      # us: the larger one names the bounding resource
    spread = _pct(tp, 0.9) - _pct(tp, 0.1)
    row = {"M": M, "N": N, "K": K, "reps": reps, "calls_per_rep": inner,
           "fused_us": {"median": round(mf, 1), "min": round(min(tf), 1), "p10": round(_pct(tf, 0.1), 1), "p90": round(_pct(tf, 0.9), 1)},
           "plain_gemm_fp32_logits_us": {"median": round(mp, 1), "min": round(min(tp), 1), "p10": round(_pct(tp, 0.1), 1), "p90": round(_pct(tp, 0.9), 1)},
           "plain_spread_us_p90_minus_p10": round(spread, 1),
           "fused_minus_plain_us": round(mf - mp, 1),
           "expectation_fused_le_plain_within_spread": bool(mf <= mp + spread),
           "fused_tflops": round(flops / mf / 1e6, 1), "plain_tflops": round(flops / mp / 1e6, 1),
           "fused_share_of_bf16_mfma_peak": round(flops / (mf * 1e-6) / PEAK_BF16, 3),
           "plain_share_of_bf16_mfma_peak": round(flops / (mp * 1e-6) / PEAK_BF16, 3),
           "fused_bytes": by_f, "plain_bytes": by_p,
           "floor_us": {"mfma": round(t_mfma, 1), "hbm_fused": round(t_hbm_f, 1), "hbm_plain": round(t_hbm_p, 1)},
           "bound": {"fused": "MFMA" if t_mfma >= t_hbm_f else "HBM", "plain": "MFMA" if t_mfma >= t_hbm_p else "HBM"},
           "max_abs_lse_diff_vs_torch_on_plain_logits": d_lse, "launches": tr.counts}
    print(json.dumps(row), flush=True)
    return row


def whole_call(clips, S=702, tail=16, reps=3):
    from crab_amd.build_model import build_crab
    t0 = time.perf_counter()
    model = build_crab("llama", device="cuda", visual=False, audio=False, seed=42)
    um = model.base_model.model
    V, D = um.lm_head.weight.shape
    g = torch.Generator(device="cuda").manual_seed(1)
    emb = torch.randn((clips, S, D), device="cuda", generator=g).to(BF)
    labels = torch.full((clips, S), -100, dtype=torch.long)
    labels[:, -tail:] = torch.randint(3, 32000, (clips, tail), generator=torch.Generator().manual_seed(2))
    build_s = time.perf_counter() - t0

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    score = lambda: model.score(inputs_embeds=emb, labels=labels)
    gen1 = lambda: model.generate(inputs_embeds=emb, max_new_tokens=1, min_new_tokens=1, eos_token_id=None, pad_token_id=2)
    from crab_amd import ops
    wall(score); wall(gen1)                                # warm-up: workspaces, code objects
    ts, tg, tpre = [], [], []
    for _ in range(reps):
        dt, sc = wall(score)
        ts.append(dt)
        prof = ops.KernelProfiler(phase_only=True)         # three event records: the prefill phase of that generate() call (encode_begin -> prefill_end)
        ops.PROFILER = prof
        try:
            tg.append(wall(gen1)[0])
        finally:
            ops.PROFILER = None
        tpre.append(prof.phase_ms()[0] * 1e-3)
    row = {"clips": clips, "S": S, "labelled_tail_tokens": tail, "vocab": V, "build_s": round(build_s, 1),
           "score_s": [round(t, 4) for t in ts], "score_clips_per_s": round(clips / statistics.median(ts), 2),
           "prefill_phase_s": [round(t, 4) for t in tpre], "prefill_phase_clips_per_s": round(clips / statistics.median(tpre), 2) if min(tpre) > 0 else None,
           "generate_1_token_s": [round(t, 4) for t in tg], "generate_1_token_clips_per_s": round(clips / statistics.median(tg), 2),
           "loss": float(sc.loss), "num_tokens_total": int(sc.num_tokens.sum()),
           "note": "prefill_phase_s: the phase marks (encode_begin -> prefill_end) of generate(max_new_tokens=1) on the same embeddings; generate_1_token_s "
                   "is that whole call. score() runs every row through every layer (the last layer too) and the fused head over the labelled rows; "
                   "generate()'s prefill runs the last layer for the last rows only. Random weights: the loss is ~log V."}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_lm_head.json"))
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="head alone (skips the 7B build)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_score.py needs an MI355X: no GPU is visible and there is no fallback")
    res = {"device": torch.cuda.get_device_name(0), "head_alone": [head_alone(16384, 32000, 4096, args.reps), head_alone(8192, 152064, 3584, args.reps)]}
    if not args.no_model:
        res["whole_call"] = whole_call(args.clips)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
