"""crab_logprob_norm / crab_logprob_gather (csrc/logprob.hip) on bare logits against the fp64 reference (tests/logprob_ref.py).

Shapes: B = 3 rows; V in {1, 63, 1000, 1025, 4099, 152064} - one element, less than a wave, less than / just above the 1024 threads of the block,
several 16-byte chunks per thread plus a scalar tail, Qwen2's vocabulary; ldl = V from an aligned base, and ldl = V + 1 from a base one float off
(rows off 16-byte alignment: the scalar head and tail).  Rows: normal(0, 4); all-equal; one token 60 above the rest with the chosen token among
the rest.  `live` and the zero entries are exact; values are held to logprob_ref's bound eps * (2 * (|z_y - max| + |log S|) + 8).  The largest
observed ratio to that bound is printed (profiles/README.md quotes it)."""
import types

import numpy as np
import pytest
import torch

from tests import logprob_ref as L

pytestmark = pytest.mark.gpu
SENT = 777.0
VS = [1, 63, 1000, 1025, 4099, 152064]
WORST = {"ratio": 0.0}


def _rows(V, off, seed):
    """[3, V] fp32 logits on the device as a view with row stride V + off that starts `off` floats into its buffer; the dominant token's index."""
    g = torch.Generator().manual_seed(seed)
    z = torch.empty(3, V)
    z[0] = torch.randn(V, generator=g) * 4
    z[1] = 1.5
    z[2] = torch.randn(V, generator=g)
    dom = (2 * V) // 3
    z[2, dom] = z[2].max() + 60
    buf = torch.full((3 * (V + off) + off + 8,), SENT, dtype=torch.float32, device="cuda")
    view = buf[off:off + 3 * (V + off)].view(3, V + off)[:, :V]
    view.copy_(z)
    assert view.stride(0) == V + off and (view.data_ptr() % 16 == 0) == (off == 0)
    return view, dom


def _run(view, chosen, step, finished, eos, min_new, trie=None, nodes=None, n_steps=4):
    from crab_amd import ops
    B, V = view.shape
    dev = view.device
    norm = torch.full((B, 4), SENT, device=dev)
    lp = torch.full((2, B, n_steps), SENT, device=dev)
    step_dev = torch.tensor([step], dtype=torch.int32, device=dev)
    fin = torch.tensor(finished, dtype=torch.int32, device=dev)
    cur = torch.tensor(chosen, dtype=torch.int64, device=dev)
    kw = {}
    if trie is not None:
        kw = dict(edge_off=torch.from_numpy(trie.edge_off).to(dev), edge_tok=torch.from_numpy(trie.edge_tok).to(dev),
                  node=torch.tensor(nodes, dtype=torch.int32, device=dev))
    ops.logprob_norm(view, step_dev, fin, eos, min_new, norm, **kw)
    ops.logprob_gather(view, cur, step_dev, norm, lp)
    torch.cuda.synchronize()
    return norm.cpu(), lp.cpu()


def _check(view, chosen, step, finished, eos, min_new, what, trie=None, nodes=None):
    n_steps = 4
    norm, lp = _run(view, chosen, step, finished, eos, min_new, trie, nodes, n_steps)
    ref, live, bound = L.step_ref(view, chosen, step, finished, eos, min_new, trie, nodes)
    assert norm[:, 2].tolist() == [1.0 if l else 0.0 for l in live.tolist()], f"{what}: live {norm[:, 2].tolist()} vs {live.tolist()}"
    assert bool((norm[:, 3] == 0).all())
    col = lp[:, :, step].double()
    others = [c for c in range(n_steps) if c != step]
    assert bool((lp[:, :, others] == SENT).all()), f"{what}: a column other than `step` was written"
    zero = bound == 0                                            # not live, or no token: exactly 0.0f
    assert bool((col[zero] == 0).all()), f"{what}: {col[zero]} where the reference has no token"
    err = (col - ref).abs()
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: max |got - ref| {float(err.max()):.3e}, largest ratio to the bound {ratio:.3f} (so far {WORST['ratio']:.3f})")
    assert bool((err <= bound).all()), f"{what}: {err} > {bound}"
    norm2, lp2 = _run(view, chosen, step, finished, eos, min_new, trie, nodes, n_steps)
    assert torch.equal(norm, norm2) and torch.equal(lp, lp2), f"{what}: two launches differ"
    return norm, lp


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", VS)
def test_rows_against_fp64(V, off):
    view, dom = _rows(V, off, 100 + V)
    rest = [(V // 5) % V, (V // 2) % V, (V // 7) % V]                         # never the dominant token (dom = 2V / 3) unless V == 1
    if V > 1:
        assert dom not in rest
    # step >= min_new: one normaliser; the row that emits EOS (= the dominant token of row 2) is live
    norm, _ = _check(view, [rest[0], rest[1], dom], 2, [0, 0, 0], dom, 2, f"V={V} off={off} step>=min_new")
    assert torch.equal(norm[:, 0], norm[:, 1])
    # EOS = the dominant token, suppressed (step < min_new): the allowed sum must not come from a subtraction
    if V > 1:
        norm, lp = _check(view, rest, 1, [0, 0, 0], dom, 2, f"V={V} off={off} EOS dominant and suppressed")
        assert float(norm[2, 0] - norm[2, 1]) > 45 and float(lp[1, 2, 1]) > float(lp[0, 2, 1]) + 45
    else:
        _check(view, [0, 0, 0], 0, [0, 0, 0], 0, 1, "V=1, its only token suppressed: nothing allowed")
    # finished-before rows with pad == eos: the same token id, no value
    _check(view, [dom, rest[1], dom], 3, [1, 0, 1], dom, 0, f"V={V} off={off} finished rows, pad == eos")
    # no EOS at all; a token outside the vocabulary
    _check(view, [V, rest[1], -1], 0, [0, 0, 0], -1, 5, f"V={V} off={off} tokens outside [0, V)")


def _hand_trie(V):
    """node 0: one edge; node 1: 1500 edges (more than the block has threads); node 2: none; node 3: EOS, a token >= V, a negative one and two
    good ones; node 4: only bad entries."""
    rng = np.random.default_rng(9)
    many = np.sort(rng.permutation(V)[:1500]).astype(np.int32)
    edges = [np.array([17], np.int32), many, np.zeros((0,), np.int32), np.array([-4, 5, 40, 2000, V, V + 7], np.int32), np.array([-1, V], np.int32)]
    off = np.zeros(len(edges) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in edges])
    tok = np.concatenate(edges).astype(np.int32)
    return types.SimpleNamespace(edge_off=off, edge_tok=tok, edge_dst=np.zeros_like(tok)), many


@pytest.mark.parametrize("off", [0, 1])
def test_trie_rows_against_fp64(off):
    V = 4099
    view, dom = _rows(V, off, 7)
    trie, many = _hand_trie(V)
    eos = 5
    _check(view, [17, int(many[700]), 3], 0, [0, 0, 0], eos, 0, f"trie off={off}: 1 edge, 1500 edges, no edges", trie, [0, 1, 2])
    norm, lp = _check(view, [17, int(many[3]), 40], 1, [0, 1, 0], eos, 0, f"trie off={off}: a finished row", trie, [0, 1, 3])
    assert float(lp[1, 0, 1]) == 0.0 and float(lp[0, 0, 1]) < 0, "one edge: probability 1 within the set, not over the vocabulary"
    _check(view, [40, 3, 3], 1, [0, 0, 0], eos, 2, f"trie off={off}: EOS edge suppressed, bad tokens, bad nodes", trie, [3, 9, -1])
    _check(view, [3, 2000, 5], 2, [0, 0, 0], eos, 2, f"trie off={off}: only bad entries; EOS edge allowed", trie, [4, 3, 3])


def test_gather_past_the_last_step_writes_nothing():
    from crab_amd import ops
    view, _ = _rows(1000, 0, 3)
    norm = torch.zeros((3, 4), device="cuda")
    fin = torch.zeros((3,), dtype=torch.int32, device="cuda")
    cur = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    lp = torch.full((2, 3, 4), SENT, device="cuda")
    for step in (4, 5, 1 << 20, -1):
        step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
        ops.logprob_norm(view, step_dev, fin, -1, 0, norm)
        ops.logprob_gather(view, cur, step_dev, norm, lp)
    torch.cuda.synchronize()
    assert bool((lp == SENT).all())
    # a strided destination (the planes of a wider buffer) is honoured
    wide = torch.full((2, 3, 9), SENT, device="cuda")
    step_dev = torch.tensor([3], dtype=torch.int32, device="cuda")
    ops.logprob_gather(view, cur, step_dev, norm, wide[:, :, :4])
    torch.cuda.synchronize()
    assert bool((wide[:, :, 4:] == SENT).all()) and bool((wide[:, :, :3] == SENT).all()) and bool((wide[:, :, 3] != SENT).all())


def test_wrappers_refuse_what_the_kernels_would_misread():
    from crab_amd import ops
    view, _ = _rows(63, 0, 3)
    norm = torch.zeros((3, 4), device="cuda")
    fin = torch.zeros((3,), dtype=torch.int32, device="cuda")
    step_dev = torch.zeros((1,), dtype=torch.int32, device="cuda")
    cur = torch.zeros((3,), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.logprob_norm(view, step_dev, fin.long(), -1, 0, norm)
    with pytest.raises(ValueError):
        ops.logprob_norm(view, step_dev, fin, -1, 0, norm[:2])
    with pytest.raises(ValueError):
        ops.logprob_norm(view, step_dev, fin, -1, 0, norm, edge_off=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.logprob_gather(view, cur, step_dev, norm, torch.zeros((2, 4, 4), device="cuda"))
    with pytest.raises(ValueError):
        ops.logprob_gather(view, cur.int(), step_dev, norm, torch.zeros((2, 3, 4), device="cuda"))
