"""Differential fuzz of the pixel-task kernels through the C-ABI at random shapes (r06): the SegModule helpers of csrc/seg_ops.hip (3x3 im2col plain
and strided, the ConvTranspose pixel shuffle, bilinear resize in both input formats with accumulation, the random-Fourier positional encoding, the
row-broadcast add, the previous-mask gate, the group mean, the PNG label map, the in-place activation), the VQGAN helpers of csrc/vq_ops.hip that
fuzz_ops.py does not reach (nearest upsampling, the two row softmaxes, codebook norms, the bf16-path arg-min) and the eval loops' metrics of
csrc/seg_metrics.hip (mask_iou / metric_s_for_null / Eval_Fmeasure / calc_color_miou_fscore / color_mask_to_label) against torch and against
oracle/metrics_oracle.py (test infrastructure, pinned to the reference's own functions by tests/golden/seg_metrics.npz).  Copies, index work and
pixel counts must be EQUAL (the batched row copy included); floating-point values: fp64 references on the GPU, every element against the derived
bound of tests/fuzz_bounds.py (no tolerance constant here); outputs a caller owns sit inside sentinel guards.   python scripts/fuzz_seg.py [cases] [seed]"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from crab_amd import ops, _lib, avss_utils as AU, harness
from oracle import metrics_oracle as MO
from tests import fuzz_bounds as FB

BF = torch.bfloat16
NCASE = int(sys.argv[1]) if len(sys.argv) > 1 else 300
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad, rejected, done, why, worst, ratios = [], 0, 0, {}, {}, {}
run = FB.Run()                                        # the floating-point kinds: every element against its derived bound
S = 777.0
KINDS = ["im2col", "im2col_strided", "pixel_shuffle", "bilinear", "dense_pe", "add_rows", "mask_gate", "group_mean", "mask_labels", "act",
         "upsample", "softmax", "sqnorm", "vq_argmin", "mask_iou", "fmeasure", "miou_fscore", "color_to_label", "copy_batched"]


def guarded(M, N, dtype, gap):
    buf = torch.full((M + 2, N + gap), S, device="cuda", dtype=dtype)
    return buf, buf[1:M + 1, :N]


def intact(buf, N):
    return bool((buf[0] == S).all()) and bool((buf[-1] == S).all()) and bool((buf[:, N:] == S).all())


def judge(what, got, ref, bound):
    ratios[kind] = max(ratios.get(kind, 0.0), run.judge(bad, desc, what, got, ref, bound))


def tokens(x):                                        # [B, C, h, w] -> token-major [B*h*w, C]
    B, C, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * h * w, C).contiguous()


def close64(a, b, rel=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return bool(np.all(np.abs(a[m] - b[m]) <= rel * np.maximum(1.0, np.abs(b[m]))))


for case in range(NCASE):
    g = torch.Generator(device="cuda").manual_seed(case)
    kind = rng.choice(KINDS)
    desc, err, tol, ok_guard = f"case {case}: {kind}", 0.0, 0.0, True
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    try:
        if kind in ("im2col", "im2col_strided"):
            B, h, w, C = rng.choice([1, 2, 3]), rng.choice([1, 2, 5, 14, 16, 33]), rng.choice([1, 3, 8, 14, 31]), rng.choice([8, 16, 64, 136])
            x = rn(B, C, h, w).to(BF)
            if kind == "im2col":
                got = ops.im2col3x3(tokens(x), B, h, w)
                cols = F.unfold(x.float(), 3, padding=1)                                      # [B, C*9, h*w], row index c*9 + tap
                oh, ow = h, w
            else:
                stride, pt, pl = rng.choice([1, 2]), rng.choice([0, 1]), rng.choice([0, 1])
                pb, pr = rng.choice([0, 1, 2]), rng.choice([0, 1, 2])
                oh, ow = (h + pt + pb - 3) // stride + 1, (w + pl + pr - 3) // stride + 1
                if oh < 1 or ow < 1:
                    continue
                got = ops.im2col3x3_strided(tokens(x), B, h, w, stride, pt, pl, oh, ow)
                cols = F.unfold(F.pad(x.float(), (pl, pr, pt, pb)), 3, stride=stride)
                desc += f" stride={stride} pad=({pt},{pl},{pb},{pr})"
            want = cols.view(B, C, 9, oh * ow).permute(0, 3, 2, 1).reshape(B * oh * ow, 9 * C)    # column (tap, c)
            err = float((got.float() != want).sum())
            desc += f" B={B} h={h} w={w} C={C}"
        elif kind == "pixel_shuffle":
            h, w, Co = rng.choice([1, 3, 14, 28]), rng.choice([1, 5, 14, 28]), rng.choice([1, 8, 20, 64])
            gm, bias = rn(h * w, 4 * Co).to(BF), (rn(Co).to(BF) if rng.random() < 0.7 else None)
            got = ops.pixel_shuffle2x(gm, bias, h, w, Co)
            v = gm.float().view(h, w, 2, 2, Co).permute(0, 2, 1, 3, 4).reshape(4 * h * w, Co)
            want = (v + (bias.float() if bias is not None else 0.0)).to(BF)
            err = float((got.view(torch.int16) != want.view(torch.int16)).sum())
            desc += f" h={h} w={w} Co={Co} bias={bias is not None}"
        elif kind == "bilinear":
            C, h, w = rng.choice([1, 3, 71]), rng.choice([1, 2, 7, 28, 56]), rng.choice([1, 3, 28, 56])
            H, W = rng.choice([1, h, 2 * h, 37, 224]), rng.choice([1, w, 4 * w, 50, 224])
            f32 = rng.random() < 0.5
            x = rn(C, h, w) if f32 else rn(C, h, w).to(BF)
            tm = rng.random() < 0.5                                                             # token-major storage [h*w, C]
            store = x.permute(1, 2, 0).contiguous() if tm else x.contiguous()
            strides = (1, w * C, C) if tm else (h * w, w, 1)
            alpha, beta = rng.choice([1.0, 0.5]), rng.choice([0.0, 0.0, 1.0, 0.25])
            out0 = rn(C, H, W)
            if beta == 0.0: out0.fill_(float("nan"))                                            # beta = 0 must not read the output (the SegModule passes torch.empty)
            buf, rows = guarded(C, H * W, torch.float32, 0)
            out = rows.view(C, H, W)
            out.copy_(out0)
            desc += f" C={C} {h}x{w}->{H}x{W} fp32={f32} token_major={tm} alpha={alpha} beta={beta}"
            ops.bilinear(store, strides, C, h, w, out, alpha, beta)
            judge("bilinear", out, *FB.bilinear_bound(store, strides, h, w, H, W, alpha, beta, out0))
            ok_guard = intact(buf, H * W)
        elif kind == "dense_pe":
            h, w, Fq = rng.choice([1, 7, 28, 64]), rng.choice([1, 9, 28, 64]), rng.choice([1, 16, 128])
            G = rn(2, Fq) * rng.choice([1.0, 1.0, 10.0])
            desc += f" h={h} w={w} F={Fq}"
            judge("dense_pe", ops.dense_pe(G, h, w), *FB.dense_pe_bound(G, h, w))
        elif kind == "add_rows":
            M, D, br = rng.choice([1, 5, 64, 300, 1024]), rng.choice([8, 64, 256, 1000]), rng.choice([1, 3, 64])
            a, b = rn(M, D + 8).to(BF)[:, :D], rn(br, D).to(BF)
            buf, got = guarded(M, D, BF, rng.choice([0, 8]))
            ops.add_rows(a, b, out=got)
            want = (a.float() + b.float()[torch.arange(M, device="cuda") % br]).to(BF)
            err = float((got.view(torch.int16) != want.view(torch.int16)).sum())
            ok_guard = intact(buf, D)
            desc += f" M={M} D={D} brows={br}"
        elif kind == "mask_gate":
            M, D, nc = rng.choice([1, 3, 4, 5, 784]), rng.choice([1, 32, 100, 256]), rng.choice([1, 2, 71, 130])
            prev, src = (rn(M, nc) * 3).to(BF), rn(M, D).to(BF)
            desc += f" M={M} D={D} classes={nc}"
            buf, got = guarded(M, D, BF, rng.choice([0, 3]))
            got.copy_(src)
            ops.mask_gate(prev, got)
            judge("mask_gate", got, *FB.mask_gate_bound(prev, src))
            ok_guard = intact(buf, D)
        elif kind == "group_mean":
            G_, T, D = rng.choice([1, 6, 71]), rng.choice([1, 2, 6, 10]), rng.choice([1, 8, 256, 4096])
            x = rn(G_ * T, D).to(BF)
            sc = rng.choice([1.0, 1.0 / T])
            desc += f" G={G_} T={T} D={D}"
            judge("group_mean", ops.group_mean(x, G_, T, sc), *FB.group_mean_bound(x, T, sc))
        elif kind == "mask_labels":
            C, H, W = rng.choice([1, 2, 71, 255]), rng.choice([1, 7, 224]), rng.choice([1, 13, 224])
            pred = rn(C, H, W)
            mode = rng.choice(["plain", "ties", "nan", "zeros"])
            if mode == "ties": pred = pred.round()
            if mode == "zeros": pred = torch.zeros_like(pred)
            if mode == "nan": pred[rng.randrange(C), :, ::3] = float("nan")
            got = ops.mask_labels(pred)
            want = ((pred[0] > 0).to(torch.uint8) * 255) if C == 1 else pred.argmax(0).to(torch.uint8)      # sigmoid(x) > 0.5 <=> x > 0; NaN = the maximum, first wins
            err = float((got != want).sum())
            desc += f" C={C} {H}x{W} {mode}"
        elif kind == "act":
            n, act = rng.choice([1, 7, 256, 100003]), rng.choice(["gelu", "quick_gelu", "relu", "silu"])
            x = (rn(n) * 3).to(BF)
            desc += f" n={n} {act}"
            judge("act", ops.act_inplace(x.clone(), act), *FB.act_bound(x, act))
        elif kind == "upsample":
            B, h, w, C = rng.choice([1, 2]), rng.choice([1, 3, 16]), rng.choice([1, 5, 16]), rng.choice([8, 64, 136])
            x = rn(B, C, h, w).to(BF)
            got = ops.upsample_nearest2x(tokens(x), B, h, w)
            want = tokens(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"))
            err = float((got.float() != want).sum())
            desc += f" B={B} h={h} w={w} C={C}"
        elif kind == "softmax":
            M, N = rng.choice([1, 3, 256, 1000]), rng.choice([1, 2, 63, 256, 257, 4096])
            x = (rn(M, N + 3) * rng.choice([1.0, 30.0]))[:, :N]
            sc = rng.choice([1.0, 0.125])
            if rng.random() < 0.3: x[0, 0] = 3.0e4                                               # one dominant entry: exp of the rest underflows
            f32 = rng.random() < 0.5
            desc += f" M={M} N={N} scale={sc} fp32={f32}"
            if f32:
                got = ops.softmax_rows_f32(x, sc)
            else:
                buf, got = guarded(M, N, BF, rng.choice([0, 5]))                                  # an [M, N] view of a wider buffer
                ops.softmax_rows(x, sc, out=got)
                ok_guard = intact(buf, N)
            judge("softmax", got, *FB.softmax_rows_bound(x, sc, out_bf16=not f32))
        elif kind == "sqnorm":
            N, D = rng.choice([1, 3, 4, 5, 1000, 16384]), rng.choice([1, 4, 8, 256, 300])
            if rng.random() < 0.5:
                e = rn(N, D + 2)[:, :D]
                got = ops.row_sqnorm_f32(e)
            else:
                e = rn(N, D + 8).to(BF)[:, :D]
                got = ops.row_sqnorm(e)
            desc += f" N={N} D={D} {e.dtype}"
            judge("sqnorm", got, *FB.sqnorm_bound(e))
        elif kind == "vq_argmin":
            M, N = rng.choice([1, 5, 256, 1000]), rng.choice([1, 2, 255, 256, 257, 16384])
            dots, e2 = rn(M, N + 1)[:, :N], rn(N).abs()
            if N > 4:
                dots[:, N - 1] = dots[:, 1]                                                      # a duplicated candidate: the first index wins
                e2[N - 1] = e2[1]
            got = ops.vq_argmin(dots, e2, offset=3)
            want = torch.argmin(e2[None, :] - 2 * dots, 1) + 3                                   # 2 * dots is exact: the same fp32 expression
            err = float((got != want).sum())
            desc += f" M={M} N={N}"
        elif kind in ("mask_iou", "fmeasure"):
            N, H, W = rng.choice([1, 2, 5]), rng.choice([1, 7, 32, 224]), rng.choice([1, 9, 32, 223, 224])
            pred = rn(N, H, W) * rng.choice([0.5, 4.0])
            gt = (rn(N, H, W) > rng.choice([-0.5, 0.0, 1.5])).float()
            mode = rng.choice(["plain", "empty gt", "full gt", "all negative", "all positive"])
            if mode == "empty gt": gt[rng.randrange(N)] = 0
            if mode == "full gt": gt[rng.randrange(N)] = 1
            if mode == "all negative": pred[rng.randrange(N)] = -pred[0].abs() - 1
            if mode == "all positive": pred[rng.randrange(N)] = pred[0].abs() + 1
            pn, gn = pred.cpu().numpy(), gt.cpu().numpy()
            desc += f" N={N} {H}x{W} {mode}"
            if kind == "mask_iou":
                iou, counts = AU.mask_iou(pred, gt, details=True)
                ok = np.array_equal(counts[:, :5].numpy(), MO.mask_counts(pn, gn)) and close64(iou.item(), MO.mask_iou(pn, gn))
                s = AU.metric_s_for_null(pred[:1])
                ok = ok and float(s.item()) == float(MO.metric_s_for_null(pn[:1]))
                if N == 1: ok = ok and float(iou.item()) == float(MO.mask_iou(pn, gn))          # one image: no sum involved, every operation rounded once
                err = 0.0 if ok else 1.0
            else:
                T = rng.choice([1, 2, 255, 1024])
                val, d = AU.Eval_Fmeasure(pred, gt, T, details=True)
                want, dw = MO.eval_fmeasure(pn, gn, T, th=AU.fmeasure_thresholds(T), details=True)
                ok = np.array_equal(d["ge"].numpy(), dw["ge"])
                ok = ok and d["images"] == dw["images"] and close64(val, want)
                err = 0.0 if ok else 1.0
                desc += f" T={T}"
        elif kind == "miou_fscore":
            BFr, C, H, W = rng.choice([1, 2, 10]), rng.choice([1, 2, 5, 71, 200]), rng.choice([1, 8, 31, 224]), rng.choice([1, 8, 30, 224])
            pred = rn(BFr, C, H, W)
            tgt = torch.randint(0, C, (BFr, H, W), device="cuda", generator=g)
            mode = rng.choice(["plain", "ignore 255", "negative", "ties", "one class"])
            if mode == "ignore 255": tgt[:, ::2, ::3] = 255
            if mode == "negative": tgt[0, :, ::2] = -1
            if mode == "ties": pred = pred.round()
            if mode == "one class": tgt[:] = C - 1
            ious, fs, cc, vid, d = AU.calc_color_miou_fscore(pred, tgt, details=True)
            pn, tn = pred.cpu().numpy(), tgt.cpu().numpy()
            mi, fw, cw, vw, iou_fc = MO.batch_miou_fscore(pn, tn)
            ok = np.array_equal(d["areas"].numpy(), MO.class_areas(pn, tn)) and np.array_equal(d["iou_fc"].numpy(), iou_fc)
            ok = ok and close64(ious.cpu().numpy(), mi) and close64(fs.cpu().numpy(), fw) and np.array_equal(cc.cpu().numpy(), cw)
            ok = ok and close64(torch.stack(vid).cpu().numpy(), vw)
            err = 0.0 if ok else 1.0
            desc += f" BF={BFr} C={C} {H}x{W} {mode}"
        elif kind == "copy_batched":
            batch, rows, cols = rng.choice([1, 3]), rng.choice([1, 5, 32, 257]), rng.choice([8, 24, 256, 1024])
            form = rng.choice(["broadcast", "drop first row", "strided rows"])
            gap = rng.choice([0, 8])                                                             # ldd > cols
            buf, dst = guarded(batch * rows, cols, BF, gap)
            ldd = buf.stride(0)
            if form == "broadcast":                                                              # sbs = 0: the query tokens of every sample
                src = rn(rows, cols).to(BF)
                ops.copy_rows_batched(src, cols, 0, dst, ldd, rows * ldd, batch, rows, cols)
                want = src.repeat(batch, 1)
            elif form == "drop first row":                                                       # an offset source view, sbs = (rows + 1) cols
                full = rn(batch, rows + 1, cols).to(BF)
                ops.copy_rows_batched(full[:, 1:], cols, (rows + 1) * cols, dst, ldd, rows * ldd, batch, rows, cols)
                want = full[:, 1:].reshape(batch * rows, cols)
            else:                                                                                # lds > cols on the source as well
                full = rn(batch, rows, cols + 16).to(BF)
                ops.copy_rows_batched(full[:, :, 8:], cols + 16, rows * (cols + 16), dst, ldd, rows * ldd, batch, rows, cols)
                want = full[:, :, 8:8 + cols].reshape(batch * rows, cols)
            err = float((dst.view(torch.int16) != want.view(torch.int16)).sum())
            ok_guard = intact(buf, cols)
            desc += f" batch={batch} rows={rows} cols={cols} {form} gap={gap}"
        else:
            n, H, W = rng.choice([1, 2, 71, 256]), rng.choice([1, 7, 224]), rng.choice([1, 5, 224])
            pal = harness.default_palette(max(n, 71))[:n] if n <= 71 else np.random.RandomState(case).randint(0, 256, (n, 3)).astype(np.uint8)
            idx = np.random.RandomState(case + 1).randint(0, n, (H, W))
            img = pal[idx].astype(np.uint8)
            if rng.random() < 0.5: img[::2, ::2] = (1, 2, 3)                                     # a colour outside the table
            got = harness.color_mask_to_label(img, pal).cpu().numpy()
            err = float((got != MO.color_mask_to_label(img, pal)).sum())
            desc += f" colours={n} {H}x{W}"
        torch.cuda.synchronize()
    except _lib.CrabHipError as e:
        msg = str(e)
        if "error -1:" in msg or "error -3:" in msg:
            rejected += 1
            k = kind + ": " + msg.split(":", 2)[-1].strip()[:80]
            why[k] = why.get(k, 0) + 1
            continue
        bad.append(desc + " -> " + msg[:200]); continue
    done += 1
    n_, w_ = worst.get(kind, (0, 0.0))
    worst[kind] = (n_ + 1, max(w_, err))
    if not (err <= tol): bad.append(desc + f" -> err {err:.3e} (tol {tol})")
    if not ok_guard: bad.append(desc + " -> a store landed outside the output block")
print("  per kind (cases, mismatches of the equality kinds): " + ", ".join(f"{k} {n} {w:.0f}" for k, (n, w) in sorted(worst.items())))
print("  per kind, worst err / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(ratios.items())))
print(f"{done} cases computed, {rejected} rejected by the library, {len(bad)} failures; floating-point kinds: {run}")
for k_, v_ in sorted(why.items(), key=lambda kv: -kv[1]): print(f"  rejected x{v_}: {k_}")
for b_ in bad[:40]: print("FAIL", b_)
sys.exit(1 if bad else 0)
