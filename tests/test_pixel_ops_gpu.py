"""Directed edge cases of the pixel-path kernels (csrc/seg_ops.hip, csrc/vq_ops.hip, copy_rows_batched of csrc/ops.hip) at the smallest shapes at
which each can still go wrong: sizes around the 64-lane wave, the 256-thread block, the 16-row / 64-entry tiles of the fp32 quantiser and the
64-chunk cap of the GroupNorm statistics; strided operands; outputs the caller owns inside sentinel guards.  Floating-point outputs are held,
element by element, to the fp64 references and derived bounds of tests/fuzz_bounds.py; copies and index work bit for bit."""
import pytest
import torch

from tests import fuzz_bounds as FB

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
S = 777.0


def _ops():
    from crab_amd import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def _guarded(M, N, dtype, gap=8):
    """(buffer [M + 2, N + gap] of sentinels, its [M, N] interior view)."""
    buf = torch.full((M + 2, N + gap), S, device="cuda", dtype=dtype)
    return buf, buf[1:M + 1, :N]


def _intact(buf, N):
    return bool((buf[0] == S).all()) and bool((buf[-1] == S).all()) and bool((buf[:, N:] == S).all())


def _judge(what, got, ref, bound):
    ratio, idx = FB.worst(got, ref, bound)
    print(f"{what}: err / bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3f} at {idx}"


# ------------------------------------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("h,w,H,W", [(1, 1, 5, 7), (7, 5, 1, 1), (7, 5, 3, 2), (3, 5, 7, 11), (4, 6, 4, 6)])
def test_bilinear(h, w, H, W):
    """Both layouts and input formats; two accumulating calls (alpha 1/2, beta 0 then 1, as the SegModule sums its two mask levels) into an output
    that starts as NaN inside sentinels: beta = 0 must not read it."""
    ops, C, pad = _ops(), 3, 64
    g = _gen(h * 100 + W)
    for f32 in (False, True):
        for tm in (True, False):
            xs = [_rn(g, C, h, w) if f32 else _rn(g, C, h, w).to(BF) for _ in range(2)]
            stores = [x.permute(1, 2, 0).contiguous() if tm else x.contiguous() for x in xs]
            strides = (1, w * C, C) if tm else (h * w, w, 1)
            buf = torch.full((C * H * W + 2 * pad,), S, device="cuda")
            out = buf[pad:pad + C * H * W].view(C, H, W)
            out.fill_(float("nan"))
            what = f"bilinear {h}x{w}->{H}x{W} fp32={f32} token_major={tm}"
            ref, bound = FB.bilinear_bound(stores[0], strides, h, w, H, W, 0.5, 0.0, out)
            ops.bilinear(stores[0], strides, C, h, w, out, 0.5, 0.0)
            assert bool(torch.isfinite(out).all()), what + ": beta = 0 read the NaN output"
            _judge(what + " beta=0", out, ref, bound)
            first = out.clone()
            ref, bound = FB.bilinear_bound(stores[1], strides, h, w, H, W, 0.5, 1.0, first)
            ops.bilinear(stores[1], strides, C, h, w, out, 0.5, 1.0)
            _judge(what + " beta=1", out, ref, bound)
            assert bool((buf[:pad] == S).all()) and bool((buf[pad + C * H * W:] == S).all()), what + ": a store outside the output"
            if (h, w) == (H, W):
                assert torch.equal(out, 0.5 * xs[0].float() + 0.5 * xs[1].float())         # the identity: weights 1 and 0, every product exact


# ----------------------------------------------------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("HW", [1, 65, 4097])
@pytest.mark.parametrize("C,G", [(8, 8), (24, 8), (1024, 32)])
def test_groupnorm_four_forms(C, G, HW):
    """C/G = 1, 3, 32; HW = 1, two chunks, the 64-chunk cap (65 rows a chunk); B = 3; an ordinary image, a constant one (var = 0: the output is the
    bias), mean 100 against spread 0.01; fp32, bf16 with fp32 / bf16 parameters, bf16 in place; with and without swish; out= inside guards."""
    ops, B = _ops(), 3
    g = _gen(C + HW)
    wt, bs = 1 + 0.2 * _rn(g, C), 0.1 * _rn(g, C)
    images = {"ordinary": _rn(g, B * HW, C) * 2 + 0.5, "constant": torch.full((B * HW, C), 3.25, device="cuda"), "mean 100": 100 + 0.01 * _rn(g, B * HW, C)}
    for name, xf in images.items():
        for form in ("f32", "bf16, fp32 params", "bf16, bf16 params", "bf16, in place"):
            for sw in ((False, True) if name == "ordinary" else (False,)):
                what = f"groupnorm C={C} G={G} HW={HW} {name} {form} swish={sw}"
                if form == "f32":
                    x, w_, b_ = xf, wt, bs
                    y = ops.groupnorm_f32(x, B, HW, G, w_, b_, 1e-6, sw)
                else:
                    x = xf.to(BF)
                    w_, b_ = (wt, bs) if form == "bf16, fp32 params" else (wt.to(BF), bs.to(BF))
                    buf, out = _guarded(B * HW, C, BF, gap=0)
                    if form == "bf16, in place":
                        out.copy_(x)
                        y = ops.groupnorm(out, B, HW, G, w_, b_, 1e-6, sw, out=out)
                    else:
                        y = ops.groupnorm(x, B, HW, G, w_, b_, 1e-6, sw, out=out)
                    assert _intact(buf, C), what + ": a store outside the output"
                ref, bound = FB.groupnorm_bound(x, B, HW, G, w_, b_, 1e-6, sw, out_fp32=form == "f32")
                if name == "constant": assert float((ref - b_.double()).abs().max()) == 0.0
                _judge(what, y, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_softmax_rows_both_forms(N):
    """A row with one dominant entry (the rest underflows) next to ordinary rows; the bf16 form writes an [M, N] view of a wider guarded buffer."""
    ops, M = _ops(), 4
    g = _gen(N)
    for scale in (1.0, 0.125, 0.37):
        x = (_rn(g, M, N + 3) * 5)[:, :N]
        x[1, N // 2] = 3.0e4
        ref, bound = FB.softmax_rows_bound(x, scale, out_bf16=False)
        _judge(f"softmax_rows_f32 N={N} scale={scale}", ops.softmax_rows_f32(x, scale), ref, bound)
        ref, bound = FB.softmax_rows_bound(x, scale, out_bf16=True)
        buf, out = _guarded(M, N, BF, gap=5)
        ops.softmax_rows(x, scale, out=out)
        _judge(f"softmax_rows N={N} scale={scale}", out, ref, bound)
        assert _intact(buf, N)
        _judge(f"softmax_rows N={N} scale={scale} (own output)", ops.softmax_rows(x, scale), ref, bound)


# ------------------------------------------------------------------------------------------------------------------------ the quantisers
def _codebook(g, N, D):
    """A row-strided codebook with copies of an entry 64 and 128 places on (another tile of the fp32 quantiser, another split)."""
    e = _rn(g, N, D + 4)[:, :D]
    first = 0
    for step in (64, 128):
        if first + step < N: e[first + step] = e[first]
    return e, first


@pytest.mark.parametrize("D", [4, 256])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_vq_nearest_f32_edges(N, D):
    ops = _ops()
    g = _gen(N * 7 + D)
    e, first = _codebook(g, N, D)
    e2 = ops.row_sqnorm_f32(e)
    for M in (1, 15, 16, 17):
        z = _rn(g, M, D + 1)[:, :D]
        z[0] = e[first]                                                     # the duplicated entry itself: the first copy wins
        idx = ops.vq_nearest_f32(z, e, e2, offset=100)
        bad, share = FB.vq_verdict(idx, z, e, offset=100)
        print(f"vq_nearest_f32 M={M} N={N} D={D}: {bad} rows outside their margin, EITHER share {share:.4f}")
        assert bad == 0 and int(idx[0]) == 100 + first                     # (the cap on the EITHER share is for cases of hundreds of rows: fuzz_ops.py, test_vqgan.py)


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_vq_argmin_edges(N):
    """Equal minima at n, n + 64 (another wave's lane) and n + 256 (the same thread's next step): the first wins; equal to torch.argmin of the
    same fp32 expression."""
    ops = _ops()
    g = _gen(N)
    for M in (1, 5):
        dots, e2 = _rn(g, M, N + 1)[:, :N], _rn(g, N).abs()
        for n in (0, 64, 256):
            if n < N:
                dots[:, n], e2[n] = 50.0, 1.0
        want = torch.argmin(e2[None, :] - 2 * dots, 1) + 3
        assert torch.equal(ops.vq_argmin(dots, e2, offset=3), want) and want.tolist() == [3] * M
        dots[:, 0] = -50.0                                                  # now the first of the equal minima is not the first entry
        want = torch.argmin(e2[None, :] - 2 * dots, 1) + 3
        assert torch.equal(ops.vq_argmin(dots, e2, offset=3), want)
        if N > 64: assert want.tolist() == [67] * M


@pytest.mark.parametrize("N", [1, 63, 130, 257])
def test_quantisers_on_non_finite_rows(N):
    """torch.argmin's rule, which mask_labels_kernel follows for arg-max: a NaN counts as the minimum and the first one wins; a row that is all
    +inf gives entry 0.  Every id lies in [offset, offset + N)."""
    ops, inf, nan = _ops(), float("inf"), float("nan")
    g = _gen(N)
    # vq_argmin: v = e2 - 2 dots
    dots, e2 = _rn(g, 6, N), _rn(g, N).abs()
    dots[0] = -inf                                                          # all +inf
    dots[1, N // 2] = nan                                                   # one NaN
    dots[2, N - 1], dots[2, N // 3] = nan, nan                              # two: the first
    dots[3] = nan                                                           # all NaN
    dots[4] = -inf; dots[4, N - 1] = nan                                    # +inf, then a NaN in the last place
    dots[5, 0] = -inf                                                       # an ordinary row behind one +inf entry
    want = torch.argmin((e2[None, :] - 2 * dots).cpu(), 1) + 9
    got = ops.vq_argmin(dots, e2, offset=9).cpu()
    assert bool(((got >= 9) & (got < 9 + N)).all()), got.tolist()
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    # vq_nearest_f32: d = (|z|^2 + |e|^2) - 2 z . e
    D = 8
    e, z = _rn(g, N, D), _rn(g, 5, D)
    z[0] = nan                                                              # every distance NaN
    z[1] = 1.0e20                                                           # |z|^2 overflows, the dot products do not: every distance +inf
    z[2, 3] = inf                                                           # NaN where e[n, 3] > 0 (inf - inf), +inf elsewhere
    z[3, 0] = -inf
    zc, ec = z.cpu(), e.cpu()
    d = ((zc ** 2).sum(1, keepdim=True) + (ec ** 2).sum(1)) - 2 * zc @ ec.t()
    assert bool(torch.isnan(d[0]).all()) and bool((d[1] == inf).all()) and not bool(torch.isfinite(d[2:4]).any()) and bool(torch.isfinite(d[4]).all())
    want = torch.argmin(d[:4], 1) + 9
    got = ops.vq_nearest_f32(z, e, ops.row_sqnorm_f32(e), offset=9).cpu()
    assert bool(((got >= 9) & (got < 9 + N)).all()), got.tolist()
    assert torch.equal(got[:4], want), (got.tolist(), want.tolist())
    assert FB.vq_verdict(got[4:], z[4:], e, offset=9)[0] == 0               # the ordinary row next to them


@pytest.mark.parametrize("D", [1, 63, 64, 65])
def test_row_sqnorm_both_forms(D):
    ops = _ops()
    g = _gen(D)
    for N in (1, 3, 4, 5):
        for e in (_rn(g, N, D + 2)[:, :D], _rn(g, N, D + 8).to(BF)[:, :D]):
            got = ops.row_sqnorm_f32(e) if e.dtype == torch.float32 else ops.row_sqnorm(e)
            _judge(f"row_sqnorm N={N} D={D} {e.dtype}", got, *FB.sqnorm_bound(e))


# -------------------------------------------------------------------------------------------------------------------- SegModule helpers
@pytest.mark.parametrize("ncls", [1, 64, 65])
def test_mask_gate(ncls):
    """prev and src as column views of wider buffers; src is gated in place inside sentinels."""
    ops = _ops()
    g = _gen(ncls)
    for M in (1, 3, 4, 5):
        for D in (1, 63, 65):
            prev = (_rn(g, M, ncls + 3) * 3).to(BF)[:, 1:1 + ncls]
            src0 = _rn(g, M, D).to(BF)
            buf, src = _guarded(M, D, BF, gap=3)
            src.copy_(src0)
            ref, bound = FB.mask_gate_bound(prev, src0)
            ops.mask_gate(prev, src)
            _judge(f"mask_gate M={M} ncls={ncls} D={D}", src, ref, bound)
            assert _intact(buf, D)


@pytest.mark.parametrize("G_,T,D", [(1, 1, 1), (3, 1, 5), (4, 6, 1), (5, 3, 257), (300, 2, 1)])
def test_group_mean(G_, T, D):
    ops = _ops()
    g = _gen(G_ + T + D)
    x = _rn(g, G_ * T, D + 5).to(BF)[:, 2:2 + D]                            # strided rows, an offset first column
    for sc in (1.0, 1.0 / T):
        _judge(f"group_mean G={G_} T={T} D={D} scale={sc:.3f}", ops.group_mean(x, G_, T, sc), *FB.group_mean_bound(x, T, sc))


@pytest.mark.parametrize("h,w,Fq,gs", [(1, 1, 1, 1.0), (3, 7, 1, 1.0), (3, 7, 16, 1.0), (7, 3, 16, 10.0), (1, 1, 128, 10.0)])
def test_dense_pe(h, w, Fq, gs):
    ops = _ops()
    G = _rn(_gen(h + Fq), 2, Fq) * gs
    _judge(f"dense_pe {h}x{w} F={Fq} G x{gs}", ops.dense_pe(G, h, w), *FB.dense_pe_bound(G, h, w))


@pytest.mark.parametrize("act", ["gelu", "quick_gelu", "relu", "silu"])
def test_act_inplace(act):
    ops = _ops()
    g = _gen(5)
    for n in (1, 255, 257):
        x = (_rn(g, n) * 3).to(BF)
        x[0] = -2.5
        _judge(f"act_inplace n={n} {act}", ops.act_inplace(x.clone(), act), *FB.act_bound(x, act))


def test_pixel_shuffle_stacked_samples():
    """The SegModule hands the shuffle B stacked samples as ONE image of B h rows (with and without a bias): equal to shuffling each sample."""
    ops = _ops()
    g = _gen(8)
    for B, h, w, Co in ((1, 1, 1, 1), (3, 2, 5, 20), (2, 3, 1, 8)):
        gm = _rn(g, B * h * w, 4 * Co).to(BF)
        for bias in (None, _rn(g, Co).to(BF)):
            got = ops.pixel_shuffle2x(gm, bias, B * h, w, Co)
            v = gm.float().view(B, h, w, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * h * w, Co)
            want = (v + (bias.float() if bias is not None else 0.0)).to(BF)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B, h, w, Co, bias is not None)


def test_copy_rows_batched_call_shapes():
    """The three call shapes of the library, bit for bit inside sentinels: the query broadcast of the SegModule and of the Q-former (source batch
    stride 0), the drop-CLS copy of the CLIP features (an offset source view, source batch stride T D); also a destination row stride > cols."""
    ops = _ops()
    g = _gen(9)
    for batch in (1, 3):
        for rows, cols in ((1, 8), (5, 24), (33, 264)):
            q = _rn(g, rows, cols).to(BF)
            buf, rep = _guarded(batch * rows, cols, BF)                                      # ldd = cols + 8 > cols
            ldd = buf.stride(0)
            ops.copy_rows_batched(q, cols, 0, rep, ldd, rows * ldd, batch, rows, cols)       # sbs = 0: broadcast
            assert torch.equal(rep, q.repeat(batch, 1)) and _intact(buf, cols), (batch, rows, cols)
            rep = torch.full((batch * rows * cols + 16,), S, device="cuda", dtype=BF)
            ops.copy_rows_batched(q, cols, 0, rep[8:], cols, rows * cols, batch, rows, cols)  # as seg_module / multimodal_encoder: contiguous
            assert torch.equal(rep[8:-8].view(batch * rows, cols), q.repeat(batch, 1)) and bool((rep[:8] == S).all()) and bool((rep[-8:] == S).all())
            T = rows + 1
            x = _rn(g, batch, T, cols).to(BF)
            buf, f = _guarded(batch * rows, cols, BF)
            ops.copy_rows_batched(x[:, 1:], cols, T * cols, f, ldd, rows * ldd, batch, rows, cols)      # drop CLS: sbs > 0, offset source view
            assert torch.equal(f, x[:, 1:].reshape(batch * rows, cols)) and _intact(buf, cols), (batch, rows, cols)
