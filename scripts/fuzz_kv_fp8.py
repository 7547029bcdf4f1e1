"""Differential fuzz of the opt-in FP8 (e4m3fn) KV cache (crab_amd/csrc/kv_fp8.hip, the fp8 mode of crab_amd/decoder.py), four parts:
  A  the two kernels through the C ABI: crab_kv_quant_fp8 against tests/kv_fp8_ref.py bit for bit; crab_attn_decode_fp8 - appended codes / scales
     bit for bit, every other slot unchanged, the output against fp64 softmax attention over the dequantised rows PER (sequence, head) under the
     bound of the bf16 decode attention (TOL_BF16) - at cached-key counts on every residue modulo 64 and around 32 / 64 / 96 / 128, with K and V
     row scales spread over decades, all three forms of the slot argument, padded row strides; every documented refusal of both entry points;
  B  ONE decode step of the whole layer stack on a cache constructed on the CPU, native and Python sequencer bit-identical, the post-final-norm
     rows against the fp32 oracle within FACTOR_VS_EMULATION x the oracle's own |bf16 emulation - fp32| on that same case;
  C  generate() / generate_many() in fp8 mode: first-token logits and the CACHE CONTENTS after the call equal to kv_fp8_ref.quant of the bf16
     mode's cache rows under every prefill chunking, graph == eager == Python sequencer, the EOS / min_new_tokens state machine, ragged waves;
  D  sequences of calls on one engine that mix the two modes per call and at engine level: carried state against fresh state bit for bit, the
     engine's mode restored after every call, kv_cache_dtype=None equal to the engine's mode passed explicitly.
make_cases(n, seed) needs no GPU and no library (tests/test_kv_fp8_host.py asserts its coverage).   python scripts/fuzz_kv_fp8.py [cases] [seed]"""
import importlib.util, os, random, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)
import torch

BF = torch.bfloat16
FP8 = "fp8_e4m3"
TOL_BF16 = 6e-3                     # tests/test_ops_gpu.py / tests/test_kv_fp8_gpu.py: the bound of the bf16 decode attention against exact arithmetic on the same operands
BOUNDARY_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
ATTN_B, ATTN_HK, ATTN_G, ATTN_TMAX = [1, 2, 3, 8, 40, 130], [1, 2, 4, 8], [1, 2, 4, 7, 8], [64, 128, 200, 960]
POS_FORMS = ["pos0", "pos_dev", "both"]
STEP_B = [1, 3, 16, 17, 40, 128, 130, 256, 260]
GEN_B = [2, 5, 17, 40, 130, 260]


def split_counts(n):
    """cases -> (attention, quantiser, layer-step, generate configurations, calls per mode-mixing sequence): part A gets the bulk"""
    return max(1, n * 50 // 100), max(1, n * 25 // 100), max(1, n * 10 // 100), max(1, n * 25 // 1000), max(3, n * 125 // 1000)


def _model_cfg(rng, i):
    """a tiny Llama / Qwen2 configuration drawn like scripts/fuzz_decoder.py draws them (from this file's own generator)"""
    while True:
        qwen = rng.random() < 0.4
        d, Hk = rng.choice([64, 128]), rng.choice([1, 2, 4])
        G = rng.choice([1, 1, 2, 4]) if not qwen else rng.choice([1, 2, 7])
        if Hk * G * d <= 1024: break
    hid = Hk * G * d
    r, nl = rng.choice([(8, 3), (8, 3), (4, 2), (16, 3), (4, 8)])
    c = dict(qwen=qwen, d=d, Hk=Hk, G=G, hid=hid, inter=rng.choice([64, 136, 352, 1000, 2 * hid + 8]), L=rng.choice([1, 2, 3]), V=rng.choice([320, 515, 1000]),
             r=r, nl=nl, eps=rng.choice([1e-5, 1e-6]), theta=rng.choice([1e4, 1e6]), wseed=300 + i)
    if os.environ.get("CRAB_FUZZ_WIDE") == "1":      # full-width rows, as fuzz_decoder's
        c.update(d=128, L=2, r=8, nl=3)
        c.update(dict(Hk=4, G=7, hid=3584, inter=18944, V=4000) if qwen else dict(Hk=32, G=1, hid=4096, inter=11008, V=32017))
    return c


def make_cases(n, seed):
    """Plain descriptions of every case of the four parts (shapes, flags, data seeds); the same for the same (n, seed)."""
    rng = random.Random(seed)
    n_attn, n_quant, n_step, n_gen, n_calls = split_counts(n)
    wide = os.environ.get("CRAB_FUZZ_WIDE") == "1"
    # ---- A: decode attention.  The cached-key count of sequence 0 walks the boundary list, then every residue modulo 64
    sched = BOUNDARY_COUNTS + list(range(64))
    attn = []
    for i in range(n_attn):
        want = sched[i % len(sched)]
        nc = want if i % len(sched) < len(BOUNDARY_COUNTS) else want + 64 * rng.choice([0, 0, 1, 2, 5, 13])
        B = ATTN_B[i % len(ATTN_B)] if i < 2 * len(ATTN_B) else rng.choice(ATTN_B)
        G, d = ATTN_G[(i // 2) % len(ATTN_G)] if i < 4 * len(ATTN_G) else rng.choice(ATTN_G), rng.choice([64, 128])
        Hk = rng.choice(ATTN_HK if B < 40 else [1, 2])
        tm = [t for t in ATTN_TMAX if t > nc + 1 and B * Hk * G * t * d <= 24_000_000]
        if not tm:
            B = rng.choice([1, 2, 3]); tm = [t for t in ATTN_TMAX if t > nc + 1]
        Tmax = rng.choice(tm)
        ragged = rng.choice(["none", "random", "random", "empty"]) if B > 1 else rng.choice(["none", "none", "random"])
        ks = [0] * B
        if ragged != "none":
            room = Tmax - 1 - nc                                   # the slot is nc + ks[0] and must stay below Tmax
            ks[0] = rng.randrange(0, room + 1)
            slot = nc + ks[0]
            for b in range(1, B): ks[b] = rng.randrange(0, slot + 1)
            if ragged == "empty": ks[rng.randrange(1, B)] = slot   # a sequence with zero cached keys
        slot = nc + ks[0]
        form = POS_FORMS[i % 3]
        pos0 = slot if form == "pos0" else 0 if form == "pos_dev" else (rng.randrange(1, slot) if slot >= 2 else None)
        if pos0 is None: form, pos0 = "pos_dev", 0
        attn.append(dict(B=B, Hk=Hk, G=G, d=d, Tmax=Tmax, slot=slot, kv_start=None if ragged == "none" else ks, counts=[slot - k for k in ks],
                         pos_form=form, pos0=pos0, pad_q=rng.choice([0, 0, 2, 8, 64]), pad_o=rng.choice([0, 0, 1, 8, 64]),
                         new_k=rng.choice(["plain", "plain", "dominant", "zero", "subnormal"]), new_v=rng.choice(["plain", "plain", "dominant", "zero", "subnormal"]),
                         seed=5000 + i))
    # ---- A: quantiser
    quant = []
    for i in range(n_quant):
        L, Bc, Hk, d = rng.choice([1, 2, 3]), rng.choice([1, 2, 3, 5]), rng.choice([1, 2, 4]), rng.choice([64, 128])
        S, t0 = rng.choice([1, 2, 7, 19, 33, 40]), rng.choice([0, 0, 3, 5])
        Tsrc = max(t0 + S + rng.choice([0, 0, 2, 11]), 8)
        b0, t_dst = rng.choice([0, 0, 1, 4]), rng.choice([0, 0, 7, 30])
        B, Tmax = b0 + Bc + rng.choice([0, 1, 3]), t_dst + S + rng.choice([0, 5, 64])
        mode = rng.choice(["none", "random", "edges"])
        off = None if mode == "none" else [rng.randrange(0, S) for _ in range(Bc)]
        if mode == "edges":
            off[0] = 0
            off[-1] = S - 1 if Bc > 1 or rng.random() < 0.5 else 0
        quant.append(dict(L=L, Bc=Bc, Hk=Hk, d=d, Tsrc=Tsrc, t0=t0, S=S, B=B, Tmax=Tmax, b0=b0, t_dst=t_dst, row_off=off, seed=7000 + i))
    # ---- B: one decode step of the stack on a given cache
    step = []
    sizes = STEP_B + ([300, 383, 448, 511, 512] if wide else [])
    for i in range(n_step):
        cfg = _model_cfg(rng, i)
        B = sizes[i % len(sizes)]
        nc = rng.choice([8, 63, 64, 65, 300])
        ro = None
        if B > 1 and rng.random() < 0.5:
            offs = [0, rng.randrange(1, nc), rng.randrange(1, nc)]           # a few distinct front paddings: the oracle runs once per value
            ro = [offs[rng.randrange(3)] for _ in range(B)]
            ro[0] = 0
        step.append(dict(cfg=cfg, B=B, slot=nc, row_off=ro, seed=9000 + i))
    # ---- C: generate() / generate_many() plumbing
    gen = []
    for i in range(n_gen):
        cfg = _model_cfg(rng, 100 + i)
        big = GEN_B[2 + i % 4]
        shapes = []
        for B in (rng.choice([2, 5]), big):
            S = rng.choice([1, 6, 33]) if B < 100 else rng.choice([1, 6])
            pcs = sorted({0, 1, 7, B // 2})
            shapes.append(dict(B=B, S=S, n=3, chunks=pcs, variant_chunk=rng.choice(pcs), streams2=(i + (B > 5)) % 2 == 0, budget=B >= 8 and rng.random() < 0.5,
                               min_new=rng.choice([0, 0, 1, 3]), seed=11000 + 10 * i + (B > 5)))
        sizes_ = [rng.choice([1, 2, 3, 8]) for _ in range(3)]
        lens = rng.choice([[9, 7, 9], [12, 10, 11], [20, 17, 20]])          # front padding of a merged wave below half of the rows
        gen.append(dict(cfg=cfg, shapes=shapes, ragged=dict(sizes=sizes_, S=lens, n=3, seed=12000 + i)))
    # ---- D: mode-mixing call sequences (dictionaries scripts/fuzz_engine_state.py's run() takes, plus "kv" and "engine")
    calls = []
    def gcall(j, B, S, n, kv, **kw):
        c = dict(kind="generate", seed=13000 + j, B=B, S=S, n=n, graph=True, streams=1, eos=None, min_new=0, extra=None, budget=None, sampling=None, kv=kv, engine=None)
        c.update(kw)
        if kv is not None: c["budget"] = None                                 # run() sizes a tight budget under the ENGINE's mode: only calls that decode in it take one
        return c
    j = 0
    while len(calls) < n_calls:
        B, S, n_ = rng.choice([1, 2, 8, 17, 40, 130]), rng.choice([1, 6, 33]), rng.choice([3, 5])
        other = dict(B=rng.choice([2, 16, 65]), S=rng.choice([6, 40]), n=rng.choice([2, 3]))
        flags = dict(graph=rng.random() < 0.8, streams=rng.choice([1, 1, 2]), eos=rng.choice([None, "pick"]), min_new=rng.choice([0, 2]),
                     extra=rng.choice([None, "hidden", "logits", "first"]), budget=rng.choice([None, None, "tight"]),
                     sampling=rng.choice([None, None, (0.7, 20, 0.9)]))
        engine = rng.choice([None, None, FP8])                                # some triples run under the engine-level switch with kv=None calls
        trip = [gcall(j, B, S, n_, "bf16" if engine is None else None, engine=engine, **flags)]
        trip.append(gcall(j + 1, other["B"], other["S"], other["n"], rng.choice([None, "bf16", FP8])))             # a changed shape in between
        trip.append(gcall(j + 2, B, S, n_, FP8 if engine is None else "bf16", **flags))
        kind = rng.choice(["batches", "forward", "generate"])
        if kind == "batches":
            trip.append(dict(kind="batches", seed=13000 + j + 3, sizes=[rng.choice([1, 2, 3, 8]) for _ in range(rng.choice([2, 3]))], S=[rng.choice([2, 5, 9, 20]) for _ in range(5)],
                             n=rng.choice([3, 4]), coalesce=rng.random() < 0.7, max_rows=rng.choice([None, None, 9]), kv=rng.choice([None, "bf16", FP8]), engine=None))
        elif kind == "forward":
            trip.append(dict(kind="forward", seed=13000 + j + 3, B=rng.choice([1, 2, 4]), S=rng.choice([5, 17]), kv=None, engine=None))
        else:
            trip.append(gcall(j + 3, other["B"], S, n_, FP8))
        trip.append(gcall(j + 4, B, S, n_, "bf16" if engine is None else None, engine="bf16" if engine is not None and rng.random() < 0.7 else None, **flags))
        calls += trip
        j += 5
    return dict(attn=attn, quant=quant, step=step, gen=gen, calls=calls)


def attention_fp64(q, K, V, visible, scale):
    """The reference of part A: softmax attention in fp64.  q [B, H, d], K / V [B, Hk, T, d] (head h reads KV head h // (H / Hk)), visible [B, T]
    bool (at least one key per sequence) -> [B, H, d] fp64."""
    B, H, d = q.shape
    Hk = K.shape[1]
    qq = q.double().view(B, Hk, H // Hk, d)
    s = torch.einsum("bkgd,bktd->bkgt", qq, K.double()) * scale
    s = s.masked_fill(~visible[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bkgt,bktd->bkgd", p, V.double()).reshape(B, H, d)


def head_rel_err(got, ref):
    """tests.util.rel_err's measure, max |got - ref| / (max |ref| + 1e-9), per (sequence, head): got / ref [B, H, d] -> [B, H]"""
    return (got.double() - ref.double()).abs().amax(-1) / (ref.double().abs().amax(-1) + 1e-9)


def spread_rows(shape, lo, hi, gen, zero_share=0.03):
    """bf16 rows [..., d] whose amax spreads over 10^lo .. 10^hi row by row (neighbouring rows carry very different scales), some all zero"""
    x = torch.randn(*shape, generator=gen) * 10 ** (torch.rand(*shape[:-1], 1, generator=gen) * (hi - lo) + lo)
    x = x * (torch.rand(*shape[:-1], 1, generator=gen) >= zero_share)
    return x.to(BF)


# ====================================================================================================================== execution (GPU)
bad, why = [], {}
stats = dict(A_attn=0, A_quant=0, A_reject=0, B=0, B_skipped=0, C=0, D=0, rejected=0, worst_attn=0.0, worst_ratio=0.0, c_err=0.0, c_yard=0.0, c_same=0, c_steps=0,
             worst_attn_oracle_q=0.0, heads=0, heads_q_differs=0, heads_over_oracle_q=0)


def note_reject(e):
    """a refusal, counted and listed by message; True when the message is one of the library's (error -1 / -3) or a wrapper's"""
    msg = str(e)
    k = msg.split(":", 2)[-1].strip()[:90] if ("error -1:" in msg or "error -3:" in msg) else msg.strip()[:90]
    why[k] = why.get(k, 0) + 1
    stats["rejected"] += 1
    return "error -1:" in msg or "error -3:" in msg


def guarded(n, dtype, fill, guard=64):
    """n elements between two guards of `guard` elements holding `fill` (16-byte aligned inside): (whole buffer, the middle)"""
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n]


def guards_ok(buf, n, fill, guard=64):
    return bool((buf[:guard] == fill).all()) and bool((buf[guard + n:] == fill).all())


def run_quant(c):
    from crab_amd import ops, _lib
    from tests import kv_fp8_ref as R
    from tests.test_kv_fp8_gpu import _rows_with_spread
    L, Bc, Hk, d, Tsrc, t0, S, B, Tmax, b0, t_dst = (c[k] for k in ("L", "Bc", "Hk", "d", "Tsrc", "t0", "S", "B", "Tmax", "b0", "t_dst"))
    desc = f"quant {c}"
    rows = L * Bc * Hk * Tsrc
    ks = _rows_with_spread(rows, d, c["seed"], at=c["seed"] % (rows - 4)).view(L, Bc, Hk, Tsrc, d)
    vs = _rows_with_spread(rows, d, c["seed"] + 1, at=(3 * c["seed"]) % (rows - 4)).flip(0).view(L, Bc, Hk, Tsrc, d).contiguous()
    off = torch.tensor(c["row_off"], dtype=torch.int32) if c["row_off"] is not None else None
    nC, nS = L * B * Hk * Tmax * d, L * B * Hk * Tmax
    bufs = {"kc": guarded(nC, torch.uint8, 0xAA), "vc": guarded(nC, torch.uint8, 0x55), "ksc": guarded(nS, torch.float32, -7.0), "vsc": guarded(nS, torch.float32, -9.0)}
    kc, vc = bufs["kc"][1].view(L, B, Hk, Tmax, d), bufs["vc"][1].view(L, B, Hk, Tmax, d)
    ksc, vsc = bufs["ksc"][1].view(L, B, Hk, Tmax), bufs["vsc"][1].view(L, B, Hk, Tmax)
    try:
        ops.kv_quant_fp8(ks.cuda(), vs.cuda(), kc, vc, ksc, vsc, b0=b0, t0=t0, t_dst=t_dst, S=S, row_off=off.cuda() if off is not None else None)
        torch.cuda.synchronize()
    except _lib.CrabHipError as e:
        if not note_reject(e): bad.append(desc + " -> " + str(e)[:200])
        return
    stats["A_quant"] += 1
    for src, got_c, got_s, cn, sn, cfill, sfill in ((ks, kc, ksc, "kc", "ksc", 0xAA, -7.0), (vs, vc, vsc, "vc", "vsc", 0x55, -9.0)):
        codes, scale = R.quant(src[:, :, :, t0:t0 + S])
        want_c = torch.full((L, B, Hk, Tmax, d), cfill, dtype=torch.uint8)
        want_s = torch.full((L, B, Hk, Tmax), sfill, dtype=torch.float32)
        for b in range(Bc):
            lo = int(off[b]) if off is not None else 0
            want_c[:, b0 + b, :, t_dst + lo:t_dst + S] = codes[:, b, :, lo:]
            want_s[:, b0 + b, :, t_dst + lo:t_dst + S] = scale[:, b, :, lo:]
        if not torch.equal(got_s.cpu(), want_s): bad.append(desc + f" -> {sn}: {int((got_s.cpu() != want_s).sum())} scales differ from kv_fp8_ref.quant (or poison lost)")
        if not torch.equal(got_c.cpu(), want_c): bad.append(desc + f" -> {cn}: {int((got_c.cpu() != want_c).sum())} codes differ from kv_fp8_ref.quant (or poison lost)")
        if not (guards_ok(bufs[cn][0], nC, cfill) and guards_ok(bufs[sn][0], nS, sfill)): bad.append(desc + f" -> a guard of {cn} / {sn} was overwritten")


def attn_inputs(c):
    """CPU side of one attention case: (qkv [B, (H + 2 Hk) d] bf16, clean codes / scales of the whole cache)"""
    from tests import kv_fp8_ref as R
    B, Hk, G, d, Tmax = c["B"], c["Hk"], c["G"], c["d"], c["Tmax"]
    H = Hk * G
    g = torch.Generator().manual_seed(c["seed"])
    k = spread_rows((B, Hk, Tmax, d), -2, 2, g)                   # K row amax over 1e-2 .. 1e2: a pair's two rows carry very different scales
    v = spread_rows((B, Hk, Tmax, d), -3, 3, g)
    kc, ksc = R.quant(k)
    vc, vsc = R.quant(v)
    qkv = torch.randn(B, H + 2 * Hk, d, generator=g)
    for nm, at in (("new_k", slice(H, H + Hk)), ("new_v", slice(H + Hk, H + 2 * Hk))):
        m = c[nm]
        if m == "dominant": qkv[:, at] *= 100.0
        elif m == "zero": qkv[::2, at] = 0
        elif m == "subnormal": qkv[:, at] *= 3e-40
    return qkv.reshape(B, -1).to(BF), kc, ksc, vc, vsc


def run_attn(c):
    from crab_amd import ops, _lib
    from oracle import crab_oracle as O
    from tests import kv_fp8_ref as R
    B, Hk, G, d, Tmax, slot = c["B"], c["Hk"], c["G"], c["d"], c["Tmax"], c["slot"]
    H, theta = Hk * G, 10000.0
    desc = f"attn {({k: v for k, v in c.items() if k not in ('kv_start', 'counts')})} counts[:4]={c['counts'][:4]}"
    qkv, kc, ksc, vc, vsc = attn_inputs(c)
    off = torch.tensor(c["kv_start"] if c["kv_start"] is not None else [0] * B, dtype=torch.int32)
    t = torch.arange(Tmax)[None]
    visible = (t >= off[:, None]) & (t < slot)                    # the cached keys; everything else is poisoned: NaN codes, huge scales
    kcp, vcp = (torch.where(visible[:, None, :, None], x, torch.full_like(x, 0x7F)) for x in (kc, vc))
    kscp, vscp = (torch.where(visible[:, None], x, torch.full_like(x, 3e30)) for x in (ksc, vsc))
    nC, nS = B * Hk * Tmax * d, B * Hk * Tmax
    bk, bv, bks, bvs = guarded(nC, torch.uint8, 0x7F), guarded(nC, torch.uint8, 0x7F), guarded(nS, torch.float32, 3e30), guarded(nS, torch.float32, 3e30)
    dk, dv, dks, dvs = bk[1].view(B, Hk, Tmax, d), bv[1].view(B, Hk, Tmax, d), bks[1].view(B, Hk, Tmax), bvs[1].view(B, Hk, Tmax)
    dk.copy_(kcp); dv.copy_(vcp); dks.copy_(kscp); dvs.copy_(vscp)
    ldq, ldo = (H + 2 * Hk) * d + c["pad_q"], H * d + c["pad_o"]
    qbuf = torch.full((B, ldq), 555.0, dtype=BF, device="cuda")
    qbuf[:, :(H + 2 * Hk) * d] = qkv.cuda()
    obuf = torch.full((B + 2, ldo), 777.0, dtype=BF, device="cuda")         # guard rows above and below, guard columns beside every row
    q_in, o = qbuf[:, :(H + 2 * Hk) * d], obuf[1:B + 1, :H * d]
    tab = ops.rope_table(Tmax, d, theta, "cuda")
    pd = None if c["pos_form"] == "pos0" else torch.tensor([slot - c["pos0"]], dtype=torch.int32, device="cuda")
    offd = off.cuda() if c["kv_start"] is not None else None
    try:
        ops.attn_decode_fp8(q_in, tab, dk, dv, dks, dvs, o, B, H, Hk, d, Tmax, c["pos0"], d ** -0.5, pos_dev=pd, kv_start=offd)
        torch.cuda.synchronize()
    except _lib.CrabHipError as e:
        if not note_reject(e): bad.append(desc + " -> " + str(e)[:200])
        return
    stats["A_attn"] += 1
    # ---- the appended slot: the bf16 rows the bf16 path stores (crab_qkv_rope_split), quantised on the CPU
    kb = torch.zeros(B, Hk, Tmax, d, dtype=BF, device="cuda")
    vb = torch.zeros_like(kb)
    qrot = qkv.cuda().clone()                                     # crab_qkv_rope_split rotates q in place: the bf16 q the bf16 path attends with
    ops.qkv_rope_split(qrot, tab, kb, vb, None, B, 1, H, Hk, d, Tmax, pos0=0, pos_dev=torch.tensor([slot], dtype=torch.int32, device="cuda"), row_off=offd)
    wk, wks = R.quant(kb[:, :, slot].cpu())
    wv, wvs = R.quant(vb[:, :, slot].cpu())
    gk, gv, gks, gvs = dk.cpu(), dv.cpu(), dks.cpu(), dvs.cpu()
    if not (torch.equal(gk[:, :, slot], wk) and torch.equal(gks[:, :, slot], wks)): bad.append(desc + " -> appended K codes / scale differ from kv_fp8_ref.quant of the rows crab_qkv_rope_split stores")
    if not (torch.equal(gv[:, :, slot], wv) and torch.equal(gvs[:, :, slot], wvs)): bad.append(desc + " -> appended V codes / scale differ from kv_fp8_ref.quant")
    keep = torch.ones(Tmax, dtype=torch.bool); keep[slot] = False
    if not all(torch.equal(got[:, :, keep], before[:, :, keep]) for got, before in ((gk, kcp), (gv, vcp), (gks, kscp), (gvs, vscp))): bad.append(desc + " -> a slot other than the appended one changed")
    if not (guards_ok(bk[0], nC, 0x7F) and guards_ok(bv[0], nC, 0x7F) and guards_ok(bks[0], nS, 3e30) and guards_ok(bvs[0], nS, 3e30)): bad.append(desc + " -> a guard around the cache was overwritten")
    ob = obuf.cpu()
    if not (bool((ob[0] == 777).all()) and bool((ob[-1] == 777).all()) and bool((ob[:, H * d:] == 777).all())): bad.append(desc + " -> a guard around the output rows was overwritten")
    if not bool((qbuf.cpu()[:, :(H + 2 * Hk) * d] == qkv).all()): bad.append(desc + " -> the q|k|v row was modified")
    got = ob[1:B + 1, :H * d].float().view(B, H, d)
    if not torch.isfinite(got).all():
        bad.append(desc + " -> non-finite output"); return
    # ---- the attention in fp64 over the dequantised rows (the appended row included, as stored).  q: rotated by the oracle and rounded to bf16,
    # and - the asserted reference - the bf16 q crab_qkv_rope_split leaves, itself held to the oracle's rotation.  The two differ in the last
    # bf16 bit of a few elements (fp32 cos / sin of a large angle from the table vs torch's); against K rows of magnitude 1e2 one such bit moves a
    # score by K_amax x 2^-9 x |q| x d^-0.5 ~ 2e-2 and with it the weight of a dominant key: the oracle-rotated reference is recorded per head
    # and may exceed the bound ONLY on heads whose rotated q differs from the oracle's bit pattern (profiles/kv_fp8_fuzz.md).
    cos, sin = O.rope_cos_sin((slot - off)[:, None].long(), d, theta)
    q3 = qkv.view(B, H + 2 * Hk, d)
    qr, _ = O.apply_rope(q3[:, :H].float()[:, :, None], q3[:, :1].float()[:, :, None], cos, sin)
    q_or, q_hip = qr[:, :, 0], qrot.cpu()[:, :H * d].view(B, H, d)
    qe = float(head_rel_err(q_hip.float(), q_or).max())
    if qe > TOL_BF16: bad.append(desc + f" -> the rotated q of crab_qkv_rope_split is {qe:.3e} from the oracle's rotation")
    K = torch.where(visible[:, None, :, None], R.dequant(kc, ksc), torch.zeros(()))
    V = torch.where(visible[:, None, :, None], R.dequant(vc, vsc), torch.zeros(()))
    K[:, :, slot], V[:, :, slot] = R.dequant(wk, wks), R.dequant(wv, wvs)
    vis = visible.clone(); vis[:, slot] = True
    err = head_rel_err(got, attention_fp64(q_hip, K, V, vis, d ** -0.5))
    err_or = head_rel_err(got, attention_fp64(q_or.to(BF), K, V, vis, d ** -0.5))
    same_q = (q_hip == q_or.to(BF)).all(-1)
    w = float(err.max())
    stats["worst_attn"] = max(stats["worst_attn"], w)
    stats["worst_attn_oracle_q"] = max(stats["worst_attn_oracle_q"], float(err_or.max()))
    stats["heads"] += err.numel(); stats["heads_q_differs"] += int((~same_q).sum()); stats["heads_over_oracle_q"] += int((err_or > TOL_BF16).sum())
    if bool(((err_or > TOL_BF16) & same_q).any()): bad.append(desc + " -> a head whose rotated q equals the oracle's bit for bit exceeds the bound against the oracle-rotated reference")
    if w > TOL_BF16:
        b, h = divmod(int(err.argmax()), H)
        bad.append(desc + f" -> sequence {b} head {h} ({c['counts'][b]} cached keys): rel err {w:.3e} > {TOL_BF16:.1e} against fp64 ({int((err > TOL_BF16).sum())} heads over)")


def run_rejections():
    """Every documented refusal of the two entry points (host-side argument checks only: nothing here reaches a kernel): the call raises with the
    library's / the wrapper's message and leaves codes, scales and output untouched."""
    from crab_amd import ops, _lib
    B, H, Hk, d, Tmax, L = 2, 4, 2, 64, 64, 1
    dev = "cuda"
    def fresh():
        s = dict(kc=torch.full((B * Hk * Tmax * d + 64,), 0xAA, dtype=torch.uint8, device=dev), vc=torch.full((B * Hk * Tmax * d + 64,), 0x55, dtype=torch.uint8, device=dev),
                 ks=torch.full((B, Hk, Tmax), -7.0, device=dev), vs=torch.full((B, Hk, Tmax), -9.0, device=dev), o=torch.full((B, H * d), 777.0, dtype=BF, device=dev),
                 qkv=torch.full((B, (H + 2 * Hk) * d + 1), 0.5, dtype=BF, device=dev))
        return s
    tab = ops.rope_table(Tmax, d, 1e4, dev)
    codes = lambda s, nm, o=0, dd=d, hk=Hk: s[nm][o:o + B * hk * Tmax * dd].view(B, hk, Tmax, dd)
    row = lambda s, dd=d, o=0: s["qkv"].view(-1)[o:o + B * (H + 2 * Hk) * dd].view(B, (H + 2 * Hk) * dd)
    attn = lambda s, **k: ops.attn_decode_fp8(k.get("qkv", row(s)), k.get("tab", tab), k.get("kc", codes(s, "kc")), k.get("vc", codes(s, "vc")), k.get("ks", s["ks"]), k.get("vs", s["vs"]),
                                              s["o"], B, k.get("H", H), Hk, k.get("d", d), Tmax, k.get("pos0", 5), d ** -0.5, pos_dev=None)
    src = torch.full((L * B * Hk * 16 * d + 8,), 0.25, dtype=BF, device=dev)
    blk = lambda o=0, dd=d: src[o:o + L * B * Hk * 16 * dd].view(L, B, Hk, 16, dd)
    quant = lambda s, **k: ops.kv_quant_fp8(k.get("src", blk()), k.get("src", blk()), k.get("kc", codes(s, "kc"))[None], k.get("vc", codes(s, "vc"))[None], k.get("ks", s["ks"])[None],
                                            k.get("vs", s["vs"])[None], b0=k.get("b0", 0), t0=k.get("t0", 0), t_dst=k.get("t_dst", 0), S=k.get("S", 8), row_off=k.get("row_off"))
    cases = [
        ("attn: head_dim 32", lambda s: attn(s, d=32, qkv=row(s, 32), kc=codes(s, "kc", 0, 32), vc=codes(s, "vc", 0, 32)), "head_dim must be 64 or 128"),
        ("attn: H % Hk != 0", lambda s: attn(s, H=3), "attn_decode_fp8: bad argument"),
        ("attn: pos0 >= Tmax", lambda s: attn(s, pos0=Tmax), "position outside the KV cache"),
        ("attn: pos0 < 0", lambda s: attn(s, pos0=-1), "position outside the KV cache"),
        ("attn: K codes off 16 bytes", lambda s: attn(s, kc=codes(s, "kc", 8)), "attn_decode_fp8: alignment"),
        ("attn: V codes off 16 bytes", lambda s: attn(s, vc=codes(s, "vc", 4)), "attn_decode_fp8: alignment"),
        ("attn: q|k|v row off 4 bytes", lambda s: attn(s, qkv=row(s, d, 1)), "attn_decode_fp8: alignment"),
        ("attn: odd row stride", lambda s: attn(s, qkv=s["qkv"][:, :(H + 2 * Hk) * d]), "attn_decode_fp8: alignment"),
        ("attn: codes of another shape", lambda s: attn(s, kc=codes(s, "kc", 0, d, 1)), "codes [B, Hk, Tmax, d] / scales [B, Hk, Tmax] expected"),
        ("attn: scales not float32", lambda s: attn(s, ks=s["ks"].double()), "codes are uint8, scales float32"),
        ("quant: head_dim 32", lambda s: quant(s, src=blk(0, 32), kc=codes(s, "kc", 0, 32), vc=codes(s, "vc", 0, 32)), "head_dim must be 64 or 128"),
        ("quant: t0 + S > T_src", lambda s: quant(s, t0=9, S=8), "must lie in the source block"),
        ("quant: t0 < 0", lambda s: quant(s, t0=-1), "must lie in the source block"),
        ("quant: t_dst + S > Tmax", lambda s: quant(s, t_dst=Tmax - 7, S=8), "must lie in the source block"),
        ("quant: S = 0", lambda s: quant(s, S=0), "kv_quant_fp8: bad argument"),
        ("quant: b0 < 0", lambda s: quant(s, b0=-1), "do not match"),
        ("quant: b0 + Bc > B", lambda s: quant(s, b0=1), "do not match"),
        ("quant: codes off 8 bytes", lambda s: quant(s, kc=codes(s, "kc", 4)), "kv_quant_fp8: alignment"),
        ("quant: source off 16 bytes", lambda s: quant(s, src=blk(1)), "kv_quant_fp8: alignment"),
        ("quant: codes not uint8", lambda s: quant(s, kc=codes(s, "kc").view(torch.int8)), "codes are uint8, scales float32"),
        ("quant: row_off not int32", lambda s: quant(s, row_off=torch.zeros(B, dtype=torch.int64, device=dev)), "row_off must be a contiguous int32"),
    ]
    for name, call, expect in cases:
        s = fresh()
        try:
            call(s)
            torch.cuda.synchronize()
            bad.append(f"rejection {name} -> the call was accepted")
        except (_lib.CrabHipError, ValueError) as e:
            note_reject(e)
            stats["A_reject"] += 1
            if expect not in str(e): bad.append(f"rejection {name} -> raised {str(e)[:160]!r}, expected the message to hold {expect!r}")
        t = fresh()
        if not all(torch.equal(s[k], t[k]) for k in s): bad.append(f"rejection {name} -> a refused call wrote to {[k for k in s if not torch.equal(s[k], t[k])]}")


def build_model(cfg, device="cuda"):
    """The tiny model of a configuration under fuzz_decoder's weight law, its oracle weights and oracle configuration."""
    from crab_amd.peft_hyper import LoraConfig, get_peft_model
    from oracle import crab_oracle as O
    if cfg["qwen"]:
        from crab_amd.unified_qwen import UnifiedConfig, UnifiedForCausalLM
    else:
        from crab_amd.unified_llama import UnifiedConfig, UnifiedForCausalLM
    H = cfg["Hk"] * cfg["G"]
    kw = dict(hidden_size=cfg["hid"], intermediate_size=cfg["inter"], num_hidden_layers=cfg["L"], num_attention_heads=H, num_key_value_heads=cfg["Hk"],
              vocab_size=cfg["V"], rms_norm_eps=cfg["eps"], rope_theta=cfg["theta"])
    torch.manual_seed(cfg["wseed"])
    um = UnifiedForCausalLM(UnifiedConfig(**kw, pad_token_id=2, **({"attention_bias": True} if cfg["qwen"] else {})), device=device)
    model = get_peft_model(um, LoraConfig(r=cfg["r"], lora_alpha=2 * cfg["r"], lora_nums=cfg["nl"]))
    for n_, p in model.named_parameters():
        small = 0.2 if ("o_proj" in n_ or "down_proj" in n_ or "lora_B" in n_) else 1.0
        p.data.copy_((torch.randn(p.shape) * (1.4 / cfg["hid"] ** 0.5) * small).to(BF) if p.dim() > 1 else
                     ((1 + 0.1 * torch.randn(p.shape)) if "norm" in n_ else 0.1 * torch.randn(p.shape)).to(BF))
    W = {k: v.detach().float().cpu() for k, v in O.strip_peft_prefix(model.state_dict()).items() if v.dtype.is_floating_point}
    ocfg = O.DecoderConfig(**kw, lora_r=cfg["r"], lora_alpha=2 * cfg["r"], lora_nums=cfg["nl"])
    return model, W, ocfg


def step_cache(c):
    """CPU side of a part-B case: per layer bf16 K / V rows [L, B, Hk, slot, d] (random, row magnitudes within a decade), the hidden rows [B, hid]"""
    cfg = c["cfg"]
    g = torch.Generator().manual_seed(c["seed"])
    k = spread_rows((cfg["L"], c["B"], cfg["Hk"], c["slot"], cfg["d"]), -0.5, 0.5, g, zero_share=0.0)
    v = spread_rows((cfg["L"], c["B"], cfg["Hk"], c["slot"], cfg["d"]), -0.5, 0.5, g, zero_share=0.0)
    x = (torch.randn(c["B"], cfg["hid"], generator=g) * 0.5).to(BF)
    return k, v, x


def oracle_step(c, W, ocfg, emulate, kq, vq, x):
    """The step on the dequantised cache rows by the oracle (appended row through the fp8 format: tests.kv_fp8_emu.Fp8Rows), once per distinct
    front padding: post-final-norm rows [B, hid]"""
    from oracle import crab_oracle as O
    from tests.kv_fp8_emu import Fp8Rows
    B, L = c["B"], c["cfg"]["L"]
    ro = c["row_off"] or [0] * B
    out = torch.empty(B, x.shape[1])
    for o in sorted(set(ro)):
        rows = [b for b in range(B) if ro[b] == o]
        cache = O.KVCache(k=Fp8Rows(kq[l][rows][:, :, o:] for l in range(L)), v=Fp8Rows(vq[l][rows][:, :, o:] for l in range(L)))
        _, hn, _ = O.decoder_forward(O._r(x[rows].float()[:, None], emulate), W, ocfg, cache, last_only=True, emulate=emulate)
        out[rows] = hn[:, -1]
    return out


def step_yardstick(c, W, ocfg):
    """(fp32 rows, |bf16 emulation - fp32| / scale, |operand floor - fp32| / scale) of a part-B case: the oracle alone"""
    from oracle import crab_oracle as O
    from tests import kv_fp8_ref as R
    k, v, x = step_cache(c)
    kq, vq = R.roundtrip(k), R.roundtrip(v)
    ref = oracle_step(c, W, ocfg, None, kq, vq, x)
    scale = float(ref.abs().max())
    emu = oracle_step(c, W, ocfg, BF, kq, vq, x)
    opd = oracle_step(c, W, ocfg, O.OPERANDS, kq, vq, x)
    return ref, float((emu - ref).abs().max()) / scale, float((opd - ref).abs().max()) / scale


def run_step(c):
    from crab_amd import decoder, ops
    from tests import bounds as PB
    from tests import kv_fp8_ref as R
    cfg, B, slot = c["cfg"], c["B"], c["slot"]
    desc = f"step {c['cfg']} B={B} slot={slot} row_off={'yes' if c['row_off'] else 'no'}"
    model, W, ocfg = build_model(cfg)
    eng = model.base_model.model._engine
    ref, yard, opd = step_yardstick(c, W, ocfg)
    k, v, x = step_cache(c)
    (kc, ksc), (vc, vsc) = R.quant(k), R.quant(v)
    Tmax = (slot + 1 + 63) // 64 * 64
    ro = torch.tensor(c["row_off"], dtype=torch.int32) if c["row_off"] else None
    live = torch.arange(slot)[None] >= (ro[:, None] if ro is not None else 0)                    # [B, slot] or [1, slot]
    live = live.expand(B, slot)[None, :, None]
    eng.kv_cache_dtype = FP8
    outs = []
    try:
        for native in (True, False):
            decoder.NATIVE_LAYERS = native
            k8, v8, ks, vs = eng.alloc_cache(B, Tmax)
            k8.fill_(0x7F); v8.fill_(0x7F); ks.fill_(3e30); vs.fill_(3e30)                       # what the step must not read
            k8[:, :, :, :slot] = torch.where(live[..., None], kc, torch.full_like(kc, 0x7F)).cuda()
            v8[:, :, :, :slot] = torch.where(live[..., None], vc, torch.full_like(vc, 0x7F)).cuda()
            ks[:, :, :, :slot] = torch.where(live, ksc, torch.full_like(ksc, 3e30)).cuda()
            vs[:, :, :, :slot] = torch.where(live, vsc, torch.full_like(vsc, 3e30)).cuda()
            ws = eng._workspace(B, 0, decode=True)
            ops.cast_rows(x.cuda(), ws.x, B, cfg["hid"])
            posd = torch.full((1,), slot, device="cuda", dtype=torch.int32)
            with ops.launch_trace(0) as tr:
                _, h = eng._layers(ws, B, 1, k8, v8, 0, Tmax, 0, posd, None, row_off=ro.cuda() if ro is not None else None, kv_scales=(ks, vs))
            if tr.launched(f"attn_decode_fp8_kernel<{cfg['d']}>") != cfg["L"]: bad.append(desc + f" -> the fp8 attention kernel ran {tr.launched('attn_decode_fp8_kernel<%d>' % cfg['d'])} times for {cfg['L']} layers")
            outs.append((h[:B].float().cpu(), k8[:, :, :, slot].cpu(), v8[:, :, :, slot].cpu(), ks[:, :, :, slot].cpu(), vs[:, :, :, slot].cpu()))
    except Exception as e:      # noqa: BLE001
        bad.append(desc + f" -> {type(e).__name__}: {str(e)[:200]}"); return
    finally:
        decoder.NATIVE_LAYERS = True
        eng.kv_cache_dtype = "bf16"
    if not all(torch.equal(a, b) for a, b in zip(*outs)): bad.append(desc + " -> the native and the Python sequencer differ (rows or appended codes / scales)")
    got = outs[0][0]
    if not torch.isfinite(got).all():
        bad.append(desc + " -> non-finite hidden rows"); return
    if opd > PB.FACTOR_VS_EMULATION * yard:          # the operand floor itself is beyond the bound: the case says nothing
        stats["B_skipped"] += 1
        return
    stats["B"] += 1
    hip = float((got - ref).abs().max()) / float(ref.abs().max())
    stats["worst_ratio"] = max(stats["worst_ratio"], hip / yard)
    if hip > PB.FACTOR_VS_EMULATION * yard:
        bad.append(desc + f" -> hidden rows {hip:.3e} of scale from the fp32 oracle, bf16 emulation {yard:.3e}, operand floor {opd:.3e}: ratio {hip / yard:.2f} > {PB.FACTOR_VS_EMULATION}")
    del model
    torch.cuda.empty_cache()


def snapshot(eng):
    """the prompt slots of every decode state the last call left: {slot: (S, row_off or None, cache tensors [..., :S] on the CPU)}"""
    out = {}
    for slot, st in eng._dec.items():
        ts = [st.kc, st.vc] + ([st.ks, st.vs] if st.ks is not None else [])
        out[slot] = (st.S, st.row_off.cpu() if st.row_off is not None else None, [t[:, :, :, :st.S].cpu().clone() for t in ts])
    return out


def cache_mismatch(s16, s8):
    """None when every fp8 state holds kv_fp8_ref.quant of the bf16 state's prompt rows (slots row_off[b] .. S - 1), else what differs"""
    from tests import kv_fp8_ref as R
    if sorted(s16) != sorted(s8): return f"decode slots {sorted(s16)} (bf16) vs {sorted(s8)} (fp8)"
    for slot in s16:
        (S, ro, (k16, v16)), (S8, ro8, t8) = s16[slot], s8[slot]
        if len(t8) != 4: return f"slot {slot}: the fp8 call left a {len(t8)}-tensor state"
        if S != S8 or k16.shape[:4] != t8[0].shape[:4] or (ro is None) != (ro8 is None) or (ro is not None and not torch.equal(ro, ro8)): return f"slot {slot}: shapes / row_off differ between the modes"
        ro = ro if ro is not None else torch.zeros(k16.shape[1], dtype=torch.int32)
        for o in sorted(set(ro.tolist())):
            rows = (ro == o).nonzero().flatten()
            for nm, src, codes, scales in (("K", k16, t8[0], t8[2]), ("V", v16, t8[1], t8[3])):
                wc, wsc = R.quant(src[:, rows][:, :, :, o:])
                gc, gs = codes[:, rows][:, :, :, o:], scales[:, rows][:, :, :, o:]
                if not torch.equal(gs, wsc) or not torch.equal(gc, wc):
                    l, b = (gs != wsc).nonzero()[0].tolist()[:2] if not torch.equal(gs, wsc) else (gc != wc).nonzero()[0].tolist()[:2]
                    return f"slot {slot}: {nm} rows of layer {l} sequence {int(rows[b])} differ from kv_fp8_ref.quant of the bf16 mode's cache rows"
    return None


def run_gen(c):
    from crab_amd import decoder
    from oracle import crab_oracle as O
    from tests import kv_fp8_emu as E
    cfg = c["cfg"]
    model, W, ocfg = build_model(cfg)
    eng = model.base_model.model._engine
    hid = cfg["hid"]
    rngl = random.Random(c["shapes"][0]["seed"])
    kw0 = dict(eos_token_id=None, pad_token_id=2)

    def gen(emb, n, mode, **kw):
        eng._dec.clear()
        r = eng.generate(emb, n, **{**kw0, **kw}, kv_cache_dtype=mode)
        r = r if isinstance(r, tuple) else (r,)
        return tuple(t.clone().cpu() for t in r), snapshot(eng)

    for sh in c["shapes"]:
        B, S, n = sh["B"], sh["S"], sh["n"]
        desc = f"gen {cfg} B={B} S={S}"
        g = torch.Generator().manual_seed(sh["seed"])
        emb = (torch.randn(B, S, hid, generator=g) * 0.5).to(BF).cuda()
        try:
            first = {}
            for pc in sh["chunks"]:
                (i16, l16), s16 = gen(emb, n, "bf16", prefill_chunk=pc, return_step_logits=True)
                (i8, l8), s8 = gen(emb, n, FP8, prefill_chunk=pc, return_step_logits=True)
                stats["C"] += 1
                first[pc] = (l16[:, 0], l8[:, 0])
                if not torch.equal(l16[:, 0], l8[:, 0]): bad.append(desc + f" prefill_chunk={pc} -> first-token logits differ between the modes")
                m = cache_mismatch(s16, s8)
                if m: bad.append(desc + f" prefill_chunk={pc} -> cache contents: {m}")
                if not torch.isfinite(l8).all(): bad.append(desc + f" prefill_chunk={pc} -> non-finite logits in fp8 mode")
                if pc == sh["variant_chunk"]: base = (i8, l8)
            for pc in sh["chunks"]:
                if torch.equal(first[pc][0], first[0][0]) and not torch.equal(first[pc][1], first[0][1]):
                    bad.append(desc + f" -> first-token logits depend on prefill_chunk={pc} in fp8 mode only")
            pc = sh["variant_chunk"]
            (ie, le), _ = gen(emb, n, FP8, prefill_chunk=pc, return_step_logits=True, use_graph=False)
            if not (torch.equal(ie, base[0]) and torch.equal(le, base[1])): bad.append(desc + f" prefill_chunk={pc} -> graph replay differs from plain launches (fp8)")
            decoder.NATIVE_LAYERS = False
            try:
                (ip, lp), _ = gen(emb, n, FP8, prefill_chunk=pc, return_step_logits=True, use_graph=False)
            finally:
                decoder.NATIVE_LAYERS = True
            if not (torch.equal(ip, base[0]) and torch.equal(lp, base[1])): bad.append(desc + f" prefill_chunk={pc} -> the Python sequencer differs from the native one (fp8)")
            extra = [dict(decode_streams=2)] if sh["streams2"] and B >= 2 else []
            if sh["budget"]: extra.append("budget")
            for kw in extra:
                res = []
                for mode in ("bf16", FP8):
                    if kw == "budget":
                        eng.kv_budget_bytes = int(eng.fixed_bytes(B, S) / 0.94 + 0.6 * B * eng.bytes_per_sequence(S, n) / 0.94)
                    try:
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore", RuntimeWarning)
                            res.append(gen(emb, n, mode, prefill_chunk=pc, return_first_logits=True, **({} if kw == "budget" else kw)) + (list(eng.last_plan["groups"]),))
                    finally:
                        eng.kv_budget_bytes = None
                ((_, f16), s16, g16), ((_, f8), s8, g8) = res
                stats["C"] += 1
                if g16 != g8: continue                             # the budget split the two modes differently: other kernels per group, nothing to compare
                if not torch.equal(f16, f8): bad.append(desc + f" {kw} -> first-token logits differ between the modes")
                m = cache_mismatch(s16, s8)
                if m: bad.append(desc + f" {kw} -> cache contents: {m}")
            # ---- the EOS / min_new_tokens / pad state machine from the run's own step logits (fuzz_decoder.py's check, fp8 mode)
            n2 = 6
            (free, _), _ = gen(emb, n2, FP8, return_step_logits=True)
            eos, mn = int(free[rngl.randrange(B), rngl.randrange(1, n2)]), sh["min_new"]
            (ids2, lg2), _ = gen(emb, n2, FP8, return_step_logits=True, eos_token_id=eos, min_new_tokens=mn)
            fin, exp, steps = torch.zeros(B, dtype=torch.bool), [], 0
            for s in range(ids2.shape[1]):
                l = lg2[:, s].float().clone()
                if s < mn: l[:, eos] = float("-inf")
                tok = torch.where(fin, torch.full((B,), 2), l.argmax(-1))
                exp.append(tok)
                fin = fin | (tok == eos)
                steps = s + 1
                if bool(fin.all()): break
            exp = torch.stack(exp, 1)
            if ids2.shape[1] != (steps if bool(fin.all()) else n2) or not torch.equal(ids2[:, :exp.shape[1]], exp):
                bad.append(desc + f" eos={eos} min_new={mn} -> ids {tuple(ids2.shape)} do not follow the EOS / pad rules from their own logits (fp8)")
            # ---- recorded, not asserted: ids against the fp32 oracle's, step logits against the fp8-KV emulation (steps on the oracle's context)
            if B <= 5 and S > 1:
                ref_ids, _ = O.greedy_generate(emb.float().cpu(), W, ocfg, n)
                ref, emu, dist = E.fp8_yardstick(emb.float().cpu(), W, W, ocfg, ref_ids)
                scale = float(ref.abs().max())
                for b in range(B):
                    for s in range(n):
                        if s and not torch.equal(base[0][b, :s], ref_ids[b, :s]): break
                        stats["c_err"] = max(stats["c_err"], float((base[1][b, s].float() - emu[b, s]).abs().max()) / scale)
                        stats["c_same"] += int(base[0][b, s] == ref_ids[b, s])
                    stats["c_steps"] += n
                stats["c_yard"] = max(stats["c_yard"], dist)
        except Exception as e:      # noqa: BLE001
            bad.append(desc + f" -> {type(e).__name__}: {str(e)[:200]}")
        finally:
            decoder.NATIVE_LAYERS = True
    # ---- coalesced ragged waves, both prefill forms
    rg = c["ragged"]
    g = torch.Generator().manual_seed(rg["seed"])
    embeds = [(torch.randn(b, s, hid, generator=g) * 0.5).to(BF).cuda() for b, s in zip(rg["sizes"], rg["S"])]
    saved = decoder.RAGGED_PAD_MAX
    try:
        for pad_max, form in ((0.0, "per_group"), (0.5, "merged")):
            decoder.RAGGED_PAD_MAX = pad_max
            desc = f"gen {cfg} ragged {rg['sizes']} x {rg['S']} {form}"
            res = {}
            for key, mode, kw in (("16", "bf16", {}), ("8", FP8, {}), ("8e", FP8, dict(use_graph=False)), ("8p", FP8, dict(use_graph=False))):
                decoder.NATIVE_LAYERS = key != "8p"
                eng._dec.clear()
                r = eng.generate_many(embeds, rg["n"], **kw0, coalesce=True, return_step_logits=True, kv_cache_dtype=mode, **kw)
                res[key] = ([(a.clone().cpu(), b.clone().cpu()) for a, b in r], snapshot(eng))
                if eng.last_ragged_prefill != form: bad.append(desc + f" -> the wave was prefilled in the {eng.last_ragged_prefill} form")
            decoder.NATIVE_LAYERS = True
            stats["C"] += 1
            if not all(torch.equal(a[1][:, 0], b[1][:, 0]) for a, b in zip(res["16"][0], res["8"][0])): bad.append(desc + " -> first-token logits differ between the modes")
            m = cache_mismatch(res["16"][1], res["8"][1])
            if m: bad.append(desc + f" -> cache contents: {m}")
            for key, what in (("8e", "graph replay differs from plain launches"), ("8p", "the Python sequencer differs from the native one")):
                if not all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(res["8"][0], res[key][0])): bad.append(desc + f" -> {what} (fp8)")
    except Exception as e:      # noqa: BLE001
        bad.append(f"gen {cfg} ragged -> {type(e).__name__}: {str(e)[:200]}")
    finally:
        decoder.RAGGED_PAD_MAX = saved
        decoder.NATIVE_LAYERS = True
    if eng.kv_cache_dtype != "bf16": bad.append(f"gen {cfg} -> the engine's mode is {eng.kv_cache_dtype!r} after per-call fp8 calls")
    del model
    torch.cuda.empty_cache()


def run_calls(calls):
    """Part D on scripts/fuzz_engine_state.py's two models with its run(): every call once on an invalidated engine, once straight through."""
    spec = importlib.util.spec_from_file_location("fuzz_engine_state", os.path.join(ROOT, "scripts", "fuzz_engine_state.py"))
    ES = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ES)
    same = lambda a, b: len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))
    for qwen in (False, True):
        model = ES.build(qwen)
        um = model.base_model.model
        eng = um._engine
        hid, V = um.config.hidden_size, um.lm_head.weight.shape[0]
        name = "qwen" if qwen else "llama"

        def one(c, mode):
            """(results | exception, results of the same call with the engine's mode passed explicitly | None, note on the mode after the call)"""
            note = None
            try:
                r = ES.run(model, c, hid, V)
            except Exception as e:      # noqa: BLE001
                r = e
            if eng.kv_cache_dtype != mode: note = f"the engine's mode is {eng.kv_cache_dtype!r} after the call, {mode!r} was set"
            r2 = None
            if c["kind"] != "forward" and c.get("kv") is None and not isinstance(r, Exception):
                try:
                    r2 = ES.run(model, dict(c, kv=mode), hid, V)
                except Exception as e:      # noqa: BLE001
                    r2 = e
            eng.kv_cache_dtype = mode                       # (a lost restore is reported once, not on every later call)
            return r, r2, note

        passes = []
        for carried in (False, True):
            eng.invalidate()
            eng.kv_cache_dtype = mode = "bf16"
            outs = []
            for c in calls:
                if not carried: eng.invalidate()
                if c.get("engine"): eng.kv_cache_dtype = mode = c["engine"]
                outs.append(one(c, mode))
            passes.append(outs)
        eng.kv_cache_dtype = "bf16"
        for i, (c, (f, f2, fn), (g, g2, gn)) in enumerate(zip(calls, *passes)):
            desc = f"calls {name} {i}: {c}"
            for note in {fn, gn} - {None}: bad.append(desc + " -> " + note)
            if isinstance(f, Exception) or isinstance(g, Exception):
                refusal = isinstance(f, NotImplementedError) and isinstance(g, NotImplementedError) and "kv_cache_dtype" in str(f) and str(f) == str(g)
                if refusal: note_reject(f)
                else: bad.append(desc + f" -> fresh state: {type(f).__name__ if isinstance(f, Exception) else 'ok'}, carried state: {type(g).__name__ if isinstance(g, Exception) else 'ok'}: {str(f if isinstance(f, Exception) else g)[:160]}")
                continue
            stats["D"] += 1
            if not same(f, g): bad.append(desc + " -> results differ between carried and fresh engine state")
            for a, a2, what in ((f, f2, "fresh"), (g, g2, "carried")):
                if a2 is not None and (isinstance(a2, Exception) or not same(a, a2)): bad.append(desc + f" -> kv_cache_dtype=None differs from the engine's mode passed explicitly ({what} state)")
        torch.cuda.synchronize()
        del model, um, eng
        torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 160
    seed = int(argv[1]) if len(argv) > 1 else 0
    warnings.filterwarnings("ignore", category=RuntimeWarning)
    cases = make_cases(n, seed)
    only = os.environ.get("CRAB_FUZZ_KV_FP8_PARTS", "ABCD")        # a subset of the parts (while working on one of them)
    t0 = [time.time()]
    def lap():
        t0.append(time.time())
        return f"{t0[-1] - t0[-2]:.1f} s"
    if "A" in only:
        for c in cases["quant"]: run_quant(c)
        for c in cases["attn"]: run_attn(c)
        run_rejections()
        print(f"A: {stats['A_quant']} quantiser and {stats['A_attn']} attention cases computed, {stats['A_reject']} refusals checked; worst attention error per head "
              f"{stats['worst_attn']:.3e} (bound {TOL_BF16:.1e}); against the oracle-rotated q {stats['worst_attn_oracle_q']:.3e}, {stats['heads_over_oracle_q']} heads over the bound, all among the "
              f"{stats['heads_q_differs']} of {stats['heads']} heads whose rotated q differs from the oracle's in a bf16 bit; {lap()}; failures so far {len(bad)}", flush=True)
    if "B" in only:
        for c in cases["step"]: run_step(c)
        nb = stats["B"] + stats["B_skipped"]
        print(f"B: {stats['B']} layer-stack steps computed, {stats['B_skipped']} of {nb} skipped (operand floor beyond the bound); worst HIP / yardstick ratio "
              f"{stats['worst_ratio']:.2f} (factor 2.5); {lap()}; failures so far {len(bad)}", flush=True)
        if stats["B_skipped"] * 20 > max(nb, 20): bad.append(f"part B skipped {stats['B_skipped']} of {nb} cases: more than 5 %")
    if "C" in only:
        for c in cases["gen"]: run_gen(c)
        print(f"C: {stats['C']} bf16 / fp8 call pairs computed; recorded: step logits vs the fp8-KV emulation {stats['c_err']:.3e} of scale (emulation vs fp32 {stats['c_yard']:.3e}), "
              f"{stats['c_same']} of {stats['c_steps']} (row, step) ids on the fp32 oracle's; {lap()}; failures so far {len(bad)}", flush=True)
    if "D" in only:
        run_calls(cases["calls"])
        print(f"D: {stats['D']} calls bit-identical between carried and fresh engine state across the modes; {lap()}; failures so far {len(bad)}", flush=True)
    print(f"{stats['rejected']} rejected:")
    for k, v in sorted(why.items(), key=lambda kv: -kv[1]): print(f"    {v:5d}  {k}")
    total = stats["A_quant"] + stats["A_attn"] + stats["B"] + stats["C"] + stats["D"]
    print(f"{total} cases computed (A {stats['A_quant'] + stats['A_attn']}, B {stats['B']} + {stats['B_skipped']} skipped, C {stats['C']}, D {stats['D']}), worst attention error {stats['worst_attn']:.3e}, "
          f"worst B ratio {stats['worst_ratio']:.2f}; {len(bad)} failures")
    for b_ in bad[:40]: print("FAIL", b_)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
