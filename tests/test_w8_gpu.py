"""The opt-in FP8 decoder weights on the GPU (include/crab_hip.h "FP8 decoder weights"): the quantiser bit for bit against its torch statement
(tests/w8_ref.py), gemm_skinny_dma_w8_kernel against float64 on the dequantised operands for every epilogue form the decode step uses, the
fused RoPE + KV append against the unfused pair, the refusals, and generate() end to end in the mode."""
import os
import subprocess
import sys

import pytest
import torch

from tests import w8_ref as WR
from tests.test_kv_fp8_gpu import _rows_with_spread

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = "fp8_e4m3"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "gemm_skinny_dma_w8_kernel"


# ------------------------------------------------------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("K", [64, 200, 4096])
def test_quantiser_equals_the_torch_statement_bit_for_bit(K):
    """crab_weight_quant_fp8 == w8_ref.quant_rows: torch.equal on codes and scales.  N = 40 rows (ten blocks of four, rows with an amax spread
    over ten decades, an all-zero row, a row of bf16 subnormals, bf16 max next to subnormals, one repeated value) into a code matrix whose
    row stride exceeds K: the bytes between the rows, and rows beside the written ones, keep their poison."""
    from crab_amd import ops
    N = 40
    W = _rows_with_spread(N, K, seed=K)
    ld = (K + 15) // 16 * 16 + 32
    codes = torch.full((N + 2, ld), 0xA5, dtype=torch.uint8, device="cuda")
    scale = torch.full((N + 2,), -7.0, dtype=torch.float32, device="cuda")
    src = torch.full((N, K + 8), float("nan"), dtype=BF, device="cuda")               # ldw > K as well
    src[:, :K] = W.cuda()
    with ops.launch_trace(0) as tr:
        ops.weight_quant_fp8(src[:, :K], codes=codes[1:N + 1, :K], scale=scale[1:N + 1])
    assert tr.launched("weight_quant_fp8_kernel") == 1, tr.counts
    want_c, want_s = WR.quant_rows(W)
    want = torch.full((N + 2, ld), 0xA5, dtype=torch.uint8)
    want[1:N + 1, :K] = want_c
    ws = torch.full((N + 2,), -7.0)
    ws[1:N + 1] = want_s
    assert torch.equal(scale.cpu(), ws), f"{(scale.cpu() != ws).sum().item()} scales differ"
    bad = codes.cpu() != want
    assert not bad.any(), f"{bad.sum().item()} bytes differ, first at {bad.nonzero()[0].tolist()}"
    assert torch.isfinite(WR.dequant_rows(want_c, want_s)).all()
    # the allocating form: fresh codes with a 16-byte row stride
    c2, s2 = ops.weight_quant_fp8(W.cuda())
    assert c2.stride(0) % 16 == 0 and torch.equal(c2.cpu(), want_c) and torch.equal(s2.cpu(), want_s)


# ------------------------------------------------------------------------------------------------------------------ 2. the kernel
def _operands(M, N, K, K2, seed):
    """bf16 activations, weights whose row scales spread over 10^4 (so a scale taken from the wrong row shows), adapters, bias, residual."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(BF)
    mag = 10 ** (torch.rand(N, 1, generator=g) * 4 - 2)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * mag).to(BF)
    o = {"x": x, "w": w, "bias": (torch.randn(N, generator=g) * 0.3).to(BF), "res": torch.randn(M, N, generator=g).to(BF),
         "x2": (torch.randn(M, max(K2, 8), generator=g) * 0.5).to(BF), "w2": (torch.randn(N, max(K2, 8), generator=g) * 0.3).to(BF)}
    o["codes"], o["scale"] = WR.quant_rows(w)
    return o


def _dev_codes(codes):
    """Codes on the device as the library wants them: a row stride that is a multiple of 16 bytes.  The padding bytes hold 0xFF (an e4m3fn NaN):
    at K % 16 == 8 the kernel's last 16-byte piece of a row reads eight of them and must mask them."""
    N, K = codes.shape
    buf = torch.full((N, (K + 15) // 16 * 16 + 16), 0xFF, dtype=torch.uint8, device="cuda")
    buf[:, :K] = codes.cuda()
    return buf[:, :K]


def _held(got, ref, bound, bf16_out, what):
    """|got - ref| <= bound (+ one bf16 rounding of the result: 2^-8 |ref| with the bound's own slack) element by element."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    lim = bound + ((ref.abs() + bound) * 2.0 ** -8 if bf16_out else 0.0) + 1e-300
    worst = ((got - ref).abs() / lim).max().item()
    assert worst <= 1.0, f"{what}: |err| / bound = {worst:.3f}"
    return worst


SHAPES = [(48, 64), (176, 200), (176, 2816), (256, 4096), (64, 11008)]


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("N,K", SHAPES)
def test_w8_kernel_against_float64_on_the_dequantised_operands(M, N, K):
    """Every epilogue form of the decode step, one launch of gemm_skinny_dma_w8_kernel each (waves without a K slot at K = 64, a K tail through
    the zero page and K % 16 == 8 at K = 200, more slots per wave than the ring holds at K = 11008, an N tail at N = 48 / 176), against
    w8_ref.gemm_ref with its derived bound.  Then the scale-mapping probe: all scales 1.0 and the weights pre-scaled by powers of two must
    give the same numbers to the same bound."""
    from crab_amd import ops
    o = _operands(M, N, K, 96, seed=M * 131 + N + K)
    dv = {k: (_dev_codes(v) if k == "codes" else v.cuda()) for k, v in o.items()}
    w8 = (dv["codes"], dv["scale"])
    seen = 0

    def run(what, bf16_out=True, **kw):
        nonlocal seen
        with ops.launch_trace(0) as tr:
            y = ops.gemm(dv["x"], dv["w"], w8=kw.pop("w8", w8), out_fp32=not bf16_out, **{k: (dv[v] if k in ("bias", "residual") and isinstance(v, str) else v) for k, v in kw.items()})
        assert tr.launched(KERNEL) == 1 and sum(tr.counts.values()) == 1, (what, tr.counts)
        seen += 1
        return y

    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"])
    _held(run("bf16 out"), ref, bnd, True, "bf16 out")
    y32 = run("fp32 out", bf16_out=False)
    _held(y32, ref, bnd, False, "fp32 out")
    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], bias=o["bias"])
    _held(run("bias", bias="bias"), ref, bnd, True, "bias")
    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], bias=o["bias"], residual=o["res"], res_scale=0.5)
    _held(run("bf16 residual", bias="bias", residual="res", res_scale=0.5), ref, bnd + 2.0 ** -23 * o["res"].double().abs(), True, "bf16 residual")
    r32 = o["res"].float() * 1.0009765625
    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], residual=r32)
    _held(run("fp32 residual", bf16_out=False, residual=r32.cuda()), ref, bnd + 2.0 ** -23 * r32.double().abs(), False, "fp32 residual")
    for K2 in (32, 96):
        x2, w2 = o["x2"][:, :K2].contiguous(), o["w2"][:, :K2].contiguous()
        ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], a2=x2, b2=w2, bias=o["bias"])
        _held(run(f"K-extension {K2}", bf16_out=False, x2=x2.cuda(), w2=w2.cuda(), bias="bias"), ref, bnd, False, f"K-extension K2={K2}")
    # the SwiGLU pair over interleaved (gate, up) rows
    pre, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], bias=o["bias"])
    ref = WR._silu(pre[:, 0::2]) * pre[:, 1::2]
    sb = WR.swiglu_bound(pre, bnd)
    _held(run("swiglu", act="swiglu_pair", bias="bias"), ref, sb, True, "swiglu pair, bf16 out")
    _held(run("swiglu fp32", bf16_out=False, act="swiglu_pair", bias="bias"), ref, sb, False, "swiglu pair, fp32 out")
    # scale-mapping probe: the SAME matrix stated two ways - codes q with per-row scales 2^e[n], and the pre-scaled codes q * 2^e[n] with all
    # scales 1.0 (q of magnitude 2^-3 .. 2^2 * 1.875 and |e| <= 3: every pre-scaled value is a normal e4m3 value).  Both must meet the same
    # float64 reference to the same bound: a scale taken from the wrong row moves the first form by a power of two.
    g = torch.Generator().manual_seed(N + K)
    q = ((torch.randint(0, 2, (N, K), generator=g) * 2 - 1) * 2.0 ** torch.randint(-3, 3, (N, K), generator=g) * (1 + torch.randint(0, 8, (N, K), generator=g) / 8))
    e = torch.randint(-3, 4, (N, 1), generator=g)
    code = lambda v: v.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(code(q).view(torch.float8_e4m3fn).float(), q) and torch.equal(code(q * 2.0 ** e).view(torch.float8_e4m3fn).float(), q * 2.0 ** e)
    pscale = (2.0 ** e[:, 0]).float()
    refp, bndp = WR.gemm_ref(o["x"], code(q), pscale, bias=o["bias"])
    got_a = run("probe: scales", bf16_out=False, w8=(_dev_codes(code(q)), pscale.cuda()), bias="bias")
    _held(got_a, refp, bndp, False, "probe: per-row power-of-two scales")
    got_b = run("probe: ones", bf16_out=False, w8=(_dev_codes(code(q * 2.0 ** e)), torch.ones(N).cuda()), bias="bias")
    _held(got_b, refp, bndp, False, "probe: all scales 1.0, weights pre-scaled")
    assert seen == 11                                                                  # bf16, fp32, bias, two residuals, two K-extensions, two SwiGLU, two probes


def _norm_case(M, N, K, res_fp32, with_lora):
    """The post-norm route of o_proj / down_proj at M <= 16 in FP8 mode: raw fp32 sums from the w8 kernel (tune 9 inside the library), then the
    row-owning tail.  Returns nothing; asserts.  The residual row against float64 (derived bound + the hyper-LoRA update's own bf16 rounding of
    u), the normalised row against the oracle's rmsnorm of the stored row with the bound of tests/test_ops_gpu.py's bf16 tests of this epilogue."""
    from crab_amd import ops
    from oracle import crab_oracle as O
    o = _operands(M, N, K, 8, seed=M + N + K + 7)
    nl, r, sc = 3, 8, 2.0
    g = torch.Generator().manual_seed(5)
    RA = torch.zeros(16, K, dtype=BF)
    RA[:nl + r] = (torch.randn(nl + r, K, generator=g) * K ** -0.5).to(BF)
    B2 = torch.zeros(N, 32, dtype=BF)
    B2[:, :nl * r] = (torch.randn(N, nl * r, generator=g) * 0.2).to(BF)
    nw = (1 + 0.1 * torch.randn(N, generator=g)).to(BF)
    rdt = torch.float32 if res_fp32 else BF
    c = o["res"].cuda().to(rdt)
    h = torch.empty(M, N, dtype=BF, device="cuda")
    kw = {"lora_self": (RA.cuda(), nl, r, sc, B2.cuda())} if with_lora else {}
    with ops.launch_trace(0) as tr:
        ops.gemm(o["x"].cuda(), o["w"].cuda(), w8=(_dev_codes(o["codes"]), o["scale"].cuda()), bias=o["bias"].cuda(), residual=c, out=c,
                 post_norm=(nw.cuda(), 1e-5, h), **kw)
    assert tr.launched(KERNEL) == 1 and tr.launched("gemm_skinny_dma_kernel") == 0, tr.counts
    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], bias=o["bias"], residual=o["res"])
    bnd = bnd + 2.0 ** -23 * o["res"].double().abs()
    if with_lora:
        t = o["x"].double() @ RA[:nl + r].double().t()
        p = torch.softmax(t[:, :nl], -1)
        u = (sc * p[:, :, None] * t[:, None, nl:]).reshape(M, nl * r)
        ref = ref + u @ B2[:, :nl * r].double().t()
        bnd = bnd + 2.0 ** -7 * (u.abs() @ B2[:, :nl * r].double().abs().t())         # u is rounded to bf16 (2^-9) behind an fp32 softmax; lora_B products summed in fp32
    _held(c, ref, bnd, not res_fp32, f"post-norm route: residual row M={M} N={N} K={K} fp32={res_fp32} lora={with_lora}")
    with O.residual_storage(res_fp32):
        want = O.rmsnorm(c.cpu().float(), nw.float(), 1e-5, emulate=BF)
    err = (h.cpu().float() - want).abs().max().item() / want.abs().max().item()
    assert err <= (4.5e-3 if res_fp32 else 2e-3), ("post-norm row", err)
    return tr.counts


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("N,K", [(176, 200), (256, 4096), (64, 11008)])
def test_w8_post_norm_route_rowfin_tail(M, N, K):
    for res_fp32 in (True, False):
        for with_lora in (True, False):
            counts = _norm_case(M, N, K, res_fp32, with_lora)
            assert any(k.startswith("rowfin") for k in counts), counts


def test_w8_post_norm_route_workspace_reduction():
    """The same route with the wide tail switched off (CRAB_ROWFIN=0, read once per process: a child process): the raw sums go through the
    row-owning workspace reduction of gemm.hip."""
    code = ("from tests.test_w8_gpu import _norm_case\n"
            "for M, N, K in ((1, 176, 200), (5, 256, 4096), (16, 64, 11008)):\n"
            "    for f32 in (True, False):\n"
            "        c = _norm_case(M, N, K, f32, False)\n"
            "        assert not any(k.startswith('rowfin') for k in c) and any('norm' in k for k in c), c\n"
            "print('reduction route ok')\n")
    env = dict(os.environ, CRAB_ROWFIN="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reduction route ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------------ 3. fused RoPE + KV append
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("M", [1, 7])
@pytest.mark.parametrize("d", [64, 128])
def test_w8_fused_rope_append_equals_the_unfused_pair(d, M, ragged):
    """The q|k|v projection with RoPE + KV append in the w8 kernel's epilogue (weight rows read in permuted order: a column's scale is the
    scale of the row it came from) == the FP8 GEMM to bf16 rows followed by crab_qkv_rope_split: torch.equal on the rows and on the caches,
    poison elsewhere in the cache intact.  With a bias (the Qwen2 form) and the hyper-LoRA K-extension."""
    from crab_amd import ops
    H, Hk, K, Tmax, pos = 4, 2, 256, 64, 9
    N = (H + 2 * Hk) * d
    o = _operands(M, N, K, 32, seed=d + M)
    dv = {k: (_dev_codes(v) if k == "codes" else v.cuda()) for k, v in o.items()}
    tab = ops.rope_table(Tmax, d, 10000.0, "cuda")
    pd = torch.tensor([pos - 2], dtype=torch.int32, device="cuda")
    off = torch.tensor([(3 * m) % (pos + 1) for m in range(M)], dtype=torch.int32, device="cuda") if ragged else None
    poison = lambda: torch.full((M, Hk, Tmax, d), 777.0, dtype=BF, device="cuda")
    k1, v1, k2, v2 = poison(), poison(), poison(), poison()
    kw = dict(w8=(dv["codes"], dv["scale"]), bias=dv["bias"], x2=dv["x2"][:, :32].contiguous(), w2=dv["w2"][:, :32].contiguous())
    q1 = ops.gemm(dv["x"], dv["w"], **kw)
    ops.qkv_rope_split(q1, tab, k1, v1, None, M, 1, H, Hk, d, Tmax, pos0=2, pos_dev=pd, row_off=off)
    with ops.launch_trace(0) as tr:
        q2 = ops.gemm(dv["x"], dv["w"], rope=(tab, k2, v2, H, Hk, d, Tmax, 2, pd), rope_row_off=off, **kw)
    assert tr.launched(KERNEL) == 1 and sum(tr.counts.values()) == 1, tr.counts
    assert torch.equal(q1[:, :H * d], q2[:, :H * d]), "rotated q rows differ from the unfused pair"
    assert torch.equal(k1, k2) and torch.equal(v1, v2), "cache rows differ from the unfused pair"
    assert (k2[:, :, :pos] == 777.0).all() and (k2[:, :, pos + 1:] == 777.0).all() and (v2[:, :, :pos] == 777.0).all() and (v2[:, :, pos + 1:] == 777.0).all()
    assert not (k2[:, :, pos] == 777.0).any()
    # and the rows are right, not merely equal: the unrotated v columns against float64
    ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], a2=o["x2"][:, :32], b2=o["w2"][:, :32], bias=o["bias"])
    _held(q2[:, (H + Hk) * d:], ref[:, (H + Hk) * d:], bnd[:, (H + Hk) * d:], True, "v columns")


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_w8_is_refused_outside_its_kernel():
    from crab_amd import _lib, ops
    from crab_amd._lib import CrabHipError
    N, K = 64, 128
    o = _operands(17, N, K, 8, seed=3)
    x, w, codes, scale = o["x"].cuda(), o["w"].cuda(), _dev_codes(o["codes"]), o["scale"].cuda()
    out = torch.full((17, N), 5.0, dtype=BF, device="cuda")
    with ops.launch_trace(0) as tr:
        with pytest.raises(CrabHipError, match=r"error -3.*M <= 16"):
            ops.gemm(x, w, w8=(codes, scale), out=out)                                   # M = 17
        with pytest.raises(CrabHipError, match=r"error -3"):
            ops.gemm(x[:4], w, w8=(codes, scale), out=out[:4], tune=1)                   # a forced register-direct kernel
        pad = torch.zeros(N, K + 8, dtype=torch.uint8, device="cuda")
        with pytest.raises(CrabHipError, match=r"error -1.*ldb8"):
            ops.gemm(x[:4], w, w8=(pad[:, :K], scale), out=out[:4])                      # ldb8 % 16 != 0

        def desc(M=4):
            g = _lib.GemmDesc()
            g.A, g.B, g.C, g.lda, g.ldb, g.ldc = x.data_ptr(), w.data_ptr(), out.data_ptr(), K, K, N
            g.M, g.N, g.K, g.res_scale, g.batch, g.nb0 = M, N, K, 1.0, 1, 1
            g.B8, g.ldb8, g.b_scale = codes.data_ptr(), codes.stride(0), scale.data_ptr()
            return g
        g = desc()
        g.batch, g.nb0 = 2, 2
        with pytest.raises(CrabHipError, match=r"error -3"):
            ops.gemm_desc(g)                                                             # batched
        g = desc()
        g.b_scale = None
        with pytest.raises(CrabHipError, match=r"error -1.*b_scale"):
            ops.gemm_desc(g)
    assert not tr.counts, tr.counts                                                      # nothing was launched ...
    assert (out == 5.0).all()                                                            # ... and nothing computed
    ops.gemm_desc(desc())                                                                # the same descriptor, unbatched, M = 4: served
    assert not (out[:4] == 5.0).all()


# ------------------------------------------------------------------------------------------------------------------ 5. the engine end to end
def _random_model(qwen):
    """hidden 256, intermediate 704, 2 layers, 4 heads / 2 KV heads (head_dim 64), vocabulary 96, hyper-LoRA on every projection."""
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from oracle import crab_oracle as O
    if qwen:
        from crab_amd.unified_qwen import UnifiedConfig, UnifiedForCausalLM
    else:
        from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    dims = dict(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=96)
    torch.manual_seed(23 + int(qwen))
    cfg = UnifiedConfig(**dims, pad_token_id=2, **({"attention_bias": True} if qwen else {}))
    model = get_peft_model(UnifiedForCausalLM(cfg, device="cuda"), LoraConfig())
    for n_, p in model.named_parameters():
        small = 0.2 if ("o_proj" in n_ or "down_proj" in n_ or "lora_B" in n_) else 1.0
        if p.dim() > 1:
            p.data.copy_((torch.randn(p.shape) * 0.06 * small).to(p.dtype))
        elif n_.endswith(".bias"):
            p.data.copy_((0.1 * torch.randn(p.shape)).to(p.dtype))
        else:
            p.data.copy_((1 + 0.1 * torch.randn(p.shape)).to(BF).to(p.dtype))
    W = {k: v.detach().float().cpu() for k, v in O.strip_peft_prefix(model.state_dict()).items() if v.dtype.is_floating_point}
    return model, W, O.DecoderConfig(**dims, rms_norm_eps=cfg.rms_norm_eps, rope_theta=cfg.rope_theta)    # (Qwen2's defaults differ from Llama's)


def _gen(model, emb, n, **kw):
    r = model.generate(inputs_embeds=emb, use_cache=True, max_new_tokens=n, pad_token_id=2, eos_token_id=None, output_logits=True,
                       return_dict_in_generate=True, **kw)
    return r.sequences.cpu(), torch.stack(r.logits, 1).float().cpu()


@pytest.mark.parametrize("qwen", [False, True])
def test_generate_in_fp8_weight_mode(qwen):
    """(a) first-token logits torch.equal to bf16 mode (prefill never sees the codes); (b) native == Python sequencer, graph == eager, bit for
    bit; (c) the trace shows the w8 kernel for every projection of every decode step at B <= 16 and none at B = 20, where last_plan reports
    bf16; (d) per-step logits, teacher-forced along the ids the run produced, within w8_ref.mixed_bound of the fp32 oracle that prefills on W
    and decodes on the dequantised weights; (e) interleaved calls in both modes reproduce each mode's own results."""
    from crab_amd import decoder, ops
    model, W, ocfg = _random_model(qwen)
    eng = model.base_model.model._engine
    n, L = 5, 2
    for B in (1, 8):
        emb = (torch.randn(B, 7, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(BF).cuda()
        for kv in ("bf16", FP8):
            ids16, lg16 = _gen(model, emb, n, kv_cache_dtype=kv)
            assert eng.last_plan["weight_dtype_used"] == "bf16"
            ids8, lg8 = _gen(model, emb, n, kv_cache_dtype=kv, weight_dtype=FP8)
            assert eng.last_plan["weight_dtype_used"] == FP8 and eng.weight_dtype == "bf16"
            assert torch.equal(lg8[:, 0], lg16[:, 0]), "(a) first-token logits differ between the weight modes"
            assert torch.isfinite(lg8).all() and not torch.equal(lg8[:, 1:], lg16[:, 1:]), "decode steps must see the quantised weights"
            # (c) every projection of every decode step: 4 groups x L layers x (n - 1) steps
            with ops.launch_trace(0) as tr:
                ids8e, lg8e = _gen(model, emb, n, kv_cache_dtype=kv, weight_dtype=FP8, use_graph=False)
            assert tr.launched(KERNEL) == 4 * L * (n - 1), tr.counts
            assert torch.equal(ids8, ids8e) and torch.equal(lg8, lg8e), "(b) HIP-graph replay differs from plain launches"
            decoder.NATIVE_LAYERS = False
            try:
                with ops.launch_trace(0) as trp:
                    ids8p, lg8p = _gen(model, emb, n, kv_cache_dtype=kv, weight_dtype=FP8, use_graph=False)
            finally:
                decoder.NATIVE_LAYERS = True
            assert trp.counts == tr.counts, (trp.counts, tr.counts)
            assert torch.equal(ids8, ids8p) and torch.equal(lg8, lg8p), "(b) the Python per-launch sequence differs from the native one"
            # (e) back and forth: no graph crosses the modes
            a16 = _gen(model, emb, n, kv_cache_dtype=kv)
            a8 = _gen(model, emb, n, kv_cache_dtype=kv, weight_dtype=FP8)
            assert torch.equal(a16[0], ids16) and torch.equal(a16[1], lg16) and torch.equal(a8[0], ids8) and torch.equal(a8[1], lg8)
            if kv == "bf16":
                # (d)
                ref, bound = WR.mixed_bound(emb.cpu(), W, ocfg, ids8)
                err = (lg8 - ref).abs().max().item() / ref.abs().max().item()
                print(f"qwen={qwen} B={B}: FP8-weight generate vs the mixed fp32 oracle {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (B, err, bound)
        # seeded sampling in the mode: reproducible, first token shared with bf16 mode's distribution
        s1 = model.generate(inputs_embeds=emb, max_new_tokens=n, pad_token_id=2, eos_token_id=None, do_sample=True, seed=5, weight_dtype=FP8)
        s2 = model.generate(inputs_embeds=emb, max_new_tokens=n, pad_token_id=2, eos_token_id=None, do_sample=True, seed=5, weight_dtype=FP8)
        s3 = model.generate(inputs_embeds=emb, max_new_tokens=n, pad_token_id=2, eos_token_id=None, do_sample=True, seed=5)
        assert torch.equal(s1, s2) and torch.equal(s1[:, 0], s3[:, 0])
    # B = 20: above the kernel's regime - the mode is accepted, the decode steps run on the bf16 weights
    emb = (torch.randn(20, 7, 256, generator=torch.Generator().manual_seed(20)) * 0.5).to(BF).cuda()
    with ops.launch_trace(0) as tr:
        ids20, lg20 = _gen(model, emb, n, weight_dtype=FP8, use_graph=False)
    assert tr.launched(KERNEL) == 0 and eng.last_plan["weight_dtype_used"] == "bf16", (tr.counts, eng.last_plan)
    ids20b, lg20b = _gen(model, emb, n)
    assert torch.equal(ids20, ids20b) and torch.equal(lg20, lg20b)
    # the engine-level switch is the same switch, and generate_many in flight / coalesced at <= 16 rows runs in the mode
    embs = [(torch.randn(b, s, 256, generator=torch.Generator().manual_seed(40 + b)) * 0.5).to(BF).cuda() for b, s in ((2, 7), (3, 5))]
    solo = [_gen(model, e, n, weight_dtype=FP8)[0] for e in embs]
    eng.weight_dtype = FP8
    try:
        many = eng.generate_many(embs, n, eos_token_id=None, pad_token_id=2)
        assert all(torch.equal(m.cpu(), s) for m, s in zip(many, solo)), "generate_many in flight differs from separate calls (fp8 weights)"
        assert eng.last_plan["weight_dtype_used"] == FP8
        with ops.launch_trace(0) as tr:
            co = eng.generate_many(embs, n, eos_token_id=None, pad_token_id=2, coalesce=True, use_graph=False)
        assert tr.launched(KERNEL) > 0 and tr.launched(KERNEL) % (4 * L) == 0, tr.counts   # whole decode steps (lm_head and the prefill tail stay on the bf16 kernel)
        assert eng.last_plan["weight_dtype_used"] == FP8, eng.last_plan
        assert all(c.shape == s.shape for c, s in zip(co, solo))
        again = _gen(model, embs[0], n)[0]
        assert torch.equal(again, solo[0])
    finally:
        eng.weight_dtype = "bf16"
    # a weight update is seen: the codes are rebuilt, the result changes, and bf16 mode agrees that the weights moved
    g = model.base_model.model.model.layers[0].mlp._down
    with torch.no_grad():
        g.linears[0].weight.mul_(1.5)
    moved = _gen(model, embs[0], n, weight_dtype=FP8)
    assert not torch.equal(moved[1][:, 1:], _gen(model, embs[0], n)[1][:, 1:]) and torch.equal(g.quantize_fp8()[1].cpu(), WR.quant_rows(g.W)[1])


# ------------------------------------------------------------------------------------------------------------------ 6. full width
def test_full_width_layer_groups_spot_check():
    """The four projection groups of a Llama-2-7B layer at M = 8 with the full K (4096 / 11008) and N cut to 256 rows per group: the forms the
    decode step runs them in - q|k|v with the K-extension, o and down as raw sums + tail, gate|up with the SwiGLU pair - to the bound of
    test 2."""
    from crab_amd import ops
    M = 8
    for name, K, form in (("qkv", 4096, "ext"), ("o", 4096, "plain"), ("gate|up", 4096, "swiglu"), ("down", 11008, "plain")):
        o = _operands(M, 256, K, 32, seed=K + len(name))
        dv = {k: (_dev_codes(v) if k == "codes" else v.cuda()) for k, v in o.items()}
        w8 = (dv["codes"], dv["scale"])
        with ops.launch_trace(0) as tr:
            if form == "ext":
                y = ops.gemm(dv["x"], dv["w"], w8=w8, x2=dv["x2"][:, :32].contiguous(), w2=dv["w2"][:, :32].contiguous())
                ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], a2=o["x2"][:, :32], b2=o["w2"][:, :32])
            elif form == "swiglu":
                y = ops.gemm(dv["x"], dv["w"], w8=w8, act="swiglu_pair")
                pre, b0 = WR.gemm_ref(o["x"], o["codes"], o["scale"])
                ref, bnd = WR._silu(pre[:, 0::2]) * pre[:, 1::2], WR.swiglu_bound(pre, b0)
            else:
                y = ops.gemm(dv["x"], dv["w"], w8=w8, residual=dv["res"])
                ref, bnd = WR.gemm_ref(o["x"], o["codes"], o["scale"], residual=o["res"])
                bnd = bnd + 2.0 ** -23 * o["res"].double().abs()
        assert tr.launched(KERNEL) == 1, tr.counts
        _held(y, ref, bnd, True, f"full-width {name}")
