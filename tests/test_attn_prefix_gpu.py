"""crab_attn_prefix_partial + crab_attn_own_merge (csrc/attn_prefix.hip): attention over the keys [prefix of the row's clip ; the row's own keys] with the
prefix stored once per clip.

Reference: fp64 softmax attention over the concatenated keys, computed with torch on the CPU from the same bf16 inputs.  The bound holds no constant
(tests/bounds.py' policy): the concatenated cache is materialised per row, the EXISTING ops.attn_decode runs on it on the GPU, its max error against
the fp64 reference is measured, and the new pair is allowed FACTOR = 1.5 x that (the summation order differs), never less than one bf16 ulp of the
output scale.  Both measured errors are printed (pytest -s) before the assertion.

Inputs: one prefix key per clip is 2 x the query of the clip's first row and one own key of every other row is 2 x that row's query, so the merge
is exercised in both directions (a prefix-dominated and an own-dominated softmax); every cache slot outside the visible ranges holds NaN - a read of
one of them poisons the output.  Workspace and output sit inside sentinel guards."""
import ctypes as C
import math

import pytest
import torch

from crab_amd import _lib, ops

pytestmark = pytest.mark.gpu
FACTOR = 1.5
DEV = "cuda:0"
BF16 = torch.bfloat16
GUARD = 64                                                       # guard rows of o / 520-byte units of the workspace on either side
LLAMA, QWEN = (2, 2, 128), (14, 2, 128)                          # (H, Hk, d): H / Hk = 1, and 7 = two siblings x 7 heads per tile


def _cases():
    out = []
    # prefix length: 16-key tile edge, chunk edge (PX_CH = 512) +- 1, more than two chunks
    for n, P in enumerate((1, 15, 16, 17, 511, 512, 513, 1030)):
        for m in (LLAMA, QWEN):
            out.append(dict(P=P, Gs=(5,), m=m, kv0=3, own=2, word=bool(n & 1), Sq=1))
    # siblings per clip: a full tile (16 rows at H == Hk, 2 at H / Hk = 7), a tile + 1
    for n, G in enumerate((1, 2, 5, 16, 17)):
        for m in (LLAMA, QWEN):
            out.append(dict(P=17, Gs=(G,), m=m, kv0=0, own=65, word=not (n & 1), Sq=1))
    # three clips of 1, 17 and 5 questions in one call: partial tiles, tiles that do not span clips
    for m in (LLAMA, QWEN):
        for word in (False, True):
            out.append(dict(P=513, Gs=(1, 17, 5), m=m, kv0=3, own=64, word=word, Sq=1))
    # the own range
    for kv0 in (0, 3):
        for n, own in enumerate((1, 2, 63, 64, 65)):
            for m in (LLAMA, QWEN):
                out.append(dict(P=16, Gs=(2,), m=m, kv0=kv0, own=own, word=bool((n + kv0) & 1), Sq=1))
    # the prefill form: query i sees the own keys up to its own; own = 3 < Sq leaves the first two queries of every row without an own key
    for m in (LLAMA, QWEN):
        out.append(dict(P=17, Gs=(1, 17, 5), m=m, kv0=0, own=7, word=False, Sq=5))
        out.append(dict(P=513, Gs=(3, 1), m=m, kv0=3, own=5, word=True, Sq=5))
        out.append(dict(P=15, Gs=(2,), m=m, kv0=3, own=3, word=False, Sq=5))
    # the other instantiated combinations: head_dim 64 (the tiny test models), H / Hk = 2, 4, 8
    for m in ((4, 2, 64), (2, 2, 64), (8, 2, 128), (16, 2, 128)):
        out.append(dict(P=513, Gs=(1, 9, 3), m=m, kv0=3, own=65, word=True, Sq=1))
        out.append(dict(P=17, Gs=(3, 1), m=m, kv0=0, own=6, word=False, Sq=5))
    return out


def _id(c):
    H, Hk, d = c["m"]
    return f"P{c['P']}-G{'_'.join(map(str, c['Gs']))}-H{H}k{Hk}d{d}-s{c['kv0']}-own{c['own']}-{'word' if c['word'] else 'host'}-Sq{c['Sq']}"


def _build(c, seed=0):
    """All inputs on the CPU (bf16) + the fp64 reference [rows, H, d]."""
    g = torch.Generator().manual_seed(seed)
    H, Hk, d = c["m"]
    P, Gs, kv0, own, Sq = c["P"], c["Gs"], c["kv0"], c["own"], c["Sq"]
    GH, Cn, B = H // Hk, len(Gs), sum(Gs)
    rows = B * Sq
    clip_of = [ci for ci, G in enumerate(Gs) for _ in range(G)]
    ctx0 = kv0 + own - (Sq - 1)                                      # query i sees the own slots kv0 .. ctx0 - 1 + i
    Tp, Tmax = (P + 7) // 8 * 8 + 8, (kv0 + own + 8) // 8 * 8
    ldq = (H + 2 * Hk) * d                                           # the packed q|k|v row of the projection
    qkv = torch.randn((rows, ldq), generator=g).to(BF16)
    pk = torch.full((Cn, Hk, Tp, d), float("nan"), dtype=BF16); pv = pk.clone()
    kc = torch.full((B, Hk, Tmax, d), float("nan"), dtype=BF16); vc = kc.clone()
    pk[:, :, :P] = (0.5 * torch.randn((Cn, Hk, P, d), generator=g)).to(BF16)
    pv[:, :, :P] = torch.randn((Cn, Hk, P, d), generator=g).to(BF16)
    kc[:, :, kv0:kv0 + own] = (0.5 * torch.randn((B, Hk, own, d), generator=g)).to(BF16)
    vc[:, :, kv0:kv0 + own] = torch.randn((B, Hk, own, d), generator=g).to(BF16)
    q3 = qkv[:, :H * d].view(rows, H, d)
    first = 0
    for ci, G in enumerate(Gs):
        pk[ci, :, (7 * ci + P // 2) % P] = (2 * q3[first * Sq + Sq - 1, ::GH].float()).to(BF16)       # dominates the clip's first row
        for b in range(first + 1, first + G):
            kc[b, :, kv0 + (b % own)] = (2 * q3[b * Sq + Sq - 1, ::GH].float()).to(BF16)              # dominates row b (its last query)
        first += G
    ref = torch.empty((rows, H, d), dtype=torch.float64)
    scale = 1.0 / math.sqrt(d)
    n_own = []
    for r in range(rows):
        b, i = divmod(r, Sq)
        n = max(0, ctx0 + i - kv0)
        n_own.append(n)
        K = torch.cat([pk[clip_of[b], :, :P], kc[b, :, kv0:kv0 + n]], 1).double()                     # [Hk, P + n, d]
        V = torch.cat([pv[clip_of[b], :, :P], vc[b, :, kv0:kv0 + n]], 1).double()
        K, V = K.repeat_interleave(GH, 0), V.repeat_interleave(GH, 0)
        s = torch.einsum("hd,htd->ht", q3[r].double(), K) * scale
        ref[r] = torch.einsum("ht,htd->hd", torch.softmax(s, -1), V)
    assert torch.isfinite(ref).all()
    return dict(qkv=qkv, pk=pk, pv=pv, kc=kc, vc=vc, ref=ref, n_own=n_own, clip_of=clip_of, ctx0=ctx0, Tp=Tp, Tmax=Tmax, rows=rows, B=B, scale=scale)


def _existing(c, t):
    """ops.attn_decode on the concatenated cache of every query row, right-aligned (kv_start = first live slot)."""
    H, Hk, d = c["m"]
    P, kv0, Sq, rows = c["P"], c["kv0"], c["Sq"], t["rows"]
    T = (P + c["own"] + 7) // 8 * 8
    ck = torch.zeros((rows, Hk, T, d), dtype=BF16); cv = torch.zeros_like(ck)
    start = []
    for r in range(rows):
        b, n = r // Sq, t["n_own"][r]
        s0 = T - (P + n)
        ck[r, :, s0:s0 + P], cv[r, :, s0:s0 + P] = t["pk"][t["clip_of"][b], :, :P], t["pv"][t["clip_of"][b], :, :P]
        ck[r, :, s0 + P:], cv[r, :, s0 + P:] = t["kc"][b, :, kv0:kv0 + n], t["vc"][b, :, kv0:kv0 + n]
        start.append(s0)
    o = torch.zeros((rows, H * d), device=DEV, dtype=BF16)
    ops.attn_decode(t["qkv"].to(DEV), ck.to(DEV), cv.to(DEV), o, rows, H, Hk, d, T, T, t["scale"],
                    kv_start=torch.tensor(start, dtype=torch.int32, device=DEV))
    return o.float().cpu().view(rows, H, d)


SENT = 12345.0


def _new(c, t):
    """K1 + K2 with o and the workspace inside sentinel guards; returns o [rows, H, d] (fp32, CPU) after checking the guards."""
    H, Hk, d = c["m"]
    rows, B, Sq = t["rows"], t["B"], c["Sq"]
    tiles, row_clip = ops.prefix_tile_plan([G * Sq for G in c["Gs"]], H, Hk)
    tile_rows = torch.tensor(tiles, dtype=torch.int32, device=DEV).reshape(-1)
    row_clip = torch.tensor(row_clip, dtype=torch.int32, device=DEV)
    nb = ops.attn_prefix_bytes(rows, H, d)
    assert nb == rows * H * (d + 2) * 4
    unit = (d + 2) * 4 * 4                                           # keeps the workspace 16-byte aligned behind the guard
    wbuf = torch.full((GUARD * unit + nb + GUARD * unit,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wbuf[GUARD * unit:GUARD * unit + nb]
    obuf = torch.full((rows + 2 * GUARD, H * d), SENT, dtype=BF16, device=DEV)
    o = obuf[GUARD:GUARD + rows]
    qkv = t["qkv"].to(DEV)
    ops.attn_prefix_partial(qkv, t["pk"].to(DEV), t["pv"].to(DEV), ws, tile_rows, row_clip, rows, H, Hk, d, c["P"], t["scale"])
    if c["word"]:
        ctx_host, ctx_dev = 1, torch.tensor([t["ctx0"] - 1], dtype=torch.int32, device=DEV)
    else:
        ctx_host, ctx_dev = t["ctx0"], None
    kv_start = torch.full((B,), c["kv0"], dtype=torch.int32, device=DEV) if c["kv0"] else None
    ops.attn_own_merge(qkv, ws, t["kc"].to(DEV), t["vc"].to(DEV), o, B, Sq, H, Hk, d, t["Tmax"], ctx_host, t["scale"], ctx_dev=ctx_dev, kv_start=kv_start)
    torch.cuda.synchronize()
    assert bool((obuf[:GUARD] == SENT).all()) and bool((obuf[GUARD + rows:] == SENT).all()), "write outside o"
    assert bool((wbuf[:GUARD * unit] == 0xA5).all()) and bool((wbuf[GUARD * unit + nb:] == 0xA5).all()), "write outside the workspace"
    return o.float().cpu().view(rows, H, d), ws.clone()


@pytest.mark.parametrize("c", _cases(), ids=_id)
def test_prefix_pair_against_fp64(c):
    t = _build(c)
    ref = t["ref"]
    out_scale = ref.abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(out_scale)) - 7)             # one bf16 ulp at the output scale
    e_old = (_existing(c, t).double() - ref).abs().max().item()
    got, ws1 = _new(c, t)
    e_new = (got.double() - ref).abs().max().item()
    print(f"\n{_id(c)}: max|err| existing attn_decode on the concatenated cache {e_old:.3e}, prefix pair {e_new:.3e}, bf16 ulp {ulp:.3e} (scale {out_scale:.3f})")
    assert torch.isfinite(got).all()
    assert e_new <= max(FACTOR * e_old, ulp), (e_new, e_old, ulp)
    # determinism: a second run gives bit-equal partials and outputs
    got2, ws2 = _new(c, t)
    assert torch.equal(got, got2) and torch.equal(ws1, ws2)


def test_unsupported_combinations_are_refused_without_a_launch():
    """Another head size, H % Hk != 0, a ratio that is not instantiated -> CRAB_E_UNSUPPORTED; a null or short workspace -> CRAB_E_WORKSPACE; a bad
    prefix length -> CRAB_E_INVALID - all decided before any launch (the launch trace stays empty)."""
    lib, h = _lib.load(), _lib.ctx(0)
    E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -3, -4
    buf = torch.zeros((1 << 16,), dtype=torch.uint8, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    f = C.c_float(0.1)

    def partial(H, Hk, d, ws=p, nbytes=1 << 16, P=4):
        return lib.crab_attn_prefix_partial(h, None, p, 1024, p, p, ws, nbytes, p, 1, p, 1, 1, H, Hk, d, 8, P, f)

    def merge(H, Hk, d, ws=p, nbytes=1 << 16):
        return lib.crab_attn_own_merge(h, None, p, 1024, ws, nbytes, p, p, p, 1024, 1, 1, H, Hk, d, 8, 1, None, f, None)

    with ops.launch_trace(0) as tr:
        for fn in (partial, merge):
            assert fn(2, 2, 32) == E_UNSUPPORTED and fn(2, 2, 96) == E_UNSUPPORTED and fn(2, 2, 256) == E_UNSUPPORTED
            assert fn(3, 2, 128) == E_UNSUPPORTED and fn(6, 2, 128) == E_UNSUPPORTED and fn(32, 2, 128) == E_UNSUPPORTED
            assert fn(2, 2, 128, ws=None) == E_WORKSPACE and fn(2, 2, 128, nbytes=2 * 130 * 4 - 1) == E_WORKSPACE
        assert partial(2, 2, 128, P=0) == E_INVALID and partial(2, 2, 128, P=9) == E_INVALID
        assert lib.crab_attn_prefix_workspace(3, 14, 128) == 3 * 14 * 130 * 4
    assert not tr.counts, tr.counts
    with pytest.raises(ValueError):
        ops.attn_prefix_partial(buf.view(BF16)[:256].view(1, 256), buf.view(BF16)[:2 * 8 * 128].view(1, 2, 8, 128), buf.view(BF16)[:2 * 8 * 128].view(1, 2, 8, 128),
                                buf, torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 1, 2, 2, 128, 4, 0.1)


def test_launch_trace_names():
    """The pair reports its instantiations: the row kernel for H == Hk at one query per row, the grouped one otherwise."""
    for m, sq, name in ((LLAMA, 1, "attn_own_merge_row_kernel<128>"), (LLAMA, 5, "attn_own_merge_kernel<128>"), (QWEN, 1, "attn_own_merge_kernel<128>"),
                        ((4, 2, 64), 1, "attn_own_merge_kernel<64>")):
        c = dict(P=16, Gs=(2,), m=m, kv0=0, own=6, word=False, Sq=sq)
        t = _build(c)
        with ops.launch_trace(0) as tr:
            _new(c, t)
        assert tr.counts == {f"attn_prefix_partial_kernel<{m[2]}>": 1, name: 1}, tr.counts


@pytest.mark.parametrize("d", (64, 128))
def test_row_kernel_with_an_empty_prefix_is_attn_decode(d):
    """attn_own_merge_row_kernel and attn_decode_kernel are one function (dec_stream + dec_group_merge, csrc/attn_decode_core.h): with the partial
    px_attend documents for no keys (o = 0, m = -1e30, l = 0) in the workspace the merge is O / L, and the outputs must be bit-equal - at every key
    count around the 16-key group and the 32-key prefetch edges, one row each through kv_start."""
    keys = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65, 97)
    H, B, Tmax, ctx = 2, len(keys), 104, 97
    g = torch.Generator().manual_seed(d)
    q = torch.randn((B, H * d), generator=g).to(BF16).to(DEV)
    kc = torch.full((B, H, Tmax, d), float("nan"), dtype=BF16); vc = kc.clone()
    for b, n in enumerate(keys):
        kc[b, :, ctx - n:ctx] = (0.5 * torch.randn((H, n, d), generator=g)).to(BF16)
        vc[b, :, ctx - n:ctx] = torch.randn((H, n, d), generator=g).to(BF16)
    kc, vc = kc.to(DEV), vc.to(DEV)
    kv_start = torch.tensor([ctx - n for n in keys], dtype=torch.int32, device=DEV)
    part = torch.zeros((B * H, d + 2), dtype=torch.float32, device=DEV)
    part[:, d] = -1e30
    ws = part.view(torch.uint8).reshape(-1)
    assert ws.numel() == ops.attn_prefix_bytes(B, H, d)
    with ops.launch_trace(0) as tr:
        got = ops.attn_own_merge(q, ws, kc, vc, torch.zeros_like(q), B, 1, H, H, d, Tmax, ctx, d ** -0.5, kv_start=kv_start)
        ref = ops.attn_decode(q, kc, vc, torch.zeros_like(q), B, H, H, d, Tmax, ctx, d ** -0.5, kv_start=kv_start)
    assert tr.counts == {f"attn_own_merge_row_kernel<{d}>": 1, f"attn_decode_kernel<{d}>": 1}, tr.counts
    assert torch.isfinite(ref.float()).all()
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()
