"""Wildcard CTC loss and gradient from block checkpoints on the GPU (ctc_amd_wildcard_loss_grad_ckpt, csrc/ctc_wild_loss_ckpt.hip)
against the float64 oracle, with the helpers and the bars of tests/test_gpu_wildcard_loss.py as they stand: loss 1e-4 + 1e-6 |loss|,
gradient 1e-4 per element (+ 2^-8 |oracle| for a 16-bit one).  In every case the loss has the bits of the forward-only call and the
rows t >= T_b are exactly zero.  F = 32 / 16 / 8 frames per block at U <= 64 / 128 / 256."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_wildcard_loss as G

pytestmark = pytest.mark.gpu
W, KINDS, dev = G.W, G.KINDS, G.dev


def run_ck(*a, **kw):
    """G.run with checkpoint=True."""
    from tf_seq2seq_losses_amd import ops
    with mock.patch.object(ops, "wildcard_loss_grad", functools.partial(ops.wildcard_loss_grad, checkpoint=True)):
        return G.run(*a, **kw)


def raw_ck(*a):
    """G.raw_call on ctc_amd_wildcard_loss_grad_ckpt."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    with mock.patch.object(lib, "ctc_amd_wildcard_loss_grad", lib.ctc_amd_wildcard_loss_grad_ckpt):
        G.raw_call(*a)


def check(what, kind, wrt, x, labels, ll, tl, ref=None, sixteen=False, **kw):
    """The checkpointed call against the oracle (of the float32 values of x), the forward-only call's loss bits, zeros from T_b on."""
    xr = x.float().cpu().numpy() if isinstance(x, torch.Tensor) else x
    ref = ref or G.oracle(kind, wrt, xr, labels, ll, tl, **{k: v for k, v in kw.items() if k in ("blank", "weight", "d_loss")})
    loss, grad = run_ck(kind, wrt, x, labels, ll, tl, **kw)
    G.compare(what, loss, grad, *ref, d_loss=kw.get("d_loss"), wrt=wrt, sixteen=sixteen)
    loss0, _ = G.run(kind, wrt, x, labels, ll, tl, want_grad=False, **{k: v for k, v in kw.items() if k != "d_loss"})
    assert OW.same_bits(loss0, loss), what
    for b in range(len(tl)):
        assert torch.all(grad[b, int(tl[b]):] == 0), (what, "zeros beyond T_b")
    return loss, grad


PATTERNS = [[W, 1, 2], [1, 2, W], [1, W, 2, 3], [1, W, W, 2, 2, 3], [1, 1, 2, 3, 3, 1]]  # first, last, middle, a pair, none
EDGES = [(U, F, T, i) for U, F in ((3, 32), (65, 16), (129, 8)) for i, T in enumerate((1, F - 1, F, F + 1, 2 * F + 1, 3 * F + 2))]


@pytest.mark.parametrize("U,F,T,i", EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_block_edges_and_pipeline_fill_and_drain(kind, wrt, U, F, T, i):
    """1 to 4 blocks, T_b = (T, 0, max(T - 2, 1)); short transcripts (cut to the frames there are) in the widths of all three tiers."""
    rng = np.random.default_rng(100 * U + T)
    x = rng.standard_normal((3, T, 6)).astype(np.float32)
    if wrt:
        x = G.logprobs32(x) - np.float32(0.25)
    tl = np.asarray([T, 0, max(T - 2, 1)], np.int32)
    labels = rng.integers(1, 6, (3, max(U, 6))).astype(np.int32)
    ll = np.zeros(3, np.int32)
    for b in range(3):
        pat = PATTERNS[(i + 2 * b) % 5][:min(U, max(int(tl[b]), 1))]
        labels[b, :len(pat)] = pat
        ll[b] = len(pat)
    check(f"ckpt {kind} wrt={wrt} U={U} T={T}", kind, wrt, x, labels, ll, tl, U=U)


@pytest.mark.parametrize("U", [64, 65, 129, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_full_tiers(kind, U):
    x, labels, ll, tl = G.make_inputs(kind, 3, 2 * U + 4, 8, U, seed=U)
    ll[:] = U
    need = [G.needed_frames(kind, labels[b]) for b in range(3)]
    tl[:] = [need[0] + 3, need[1] - 1, need[2] + 2]  # the second a frame short
    d = np.asarray([1.5, np.nan, -0.7], np.float32)
    loss, grad = check(f"ckpt {kind} full U={U}", kind, 0, x, labels, ll, tl, d_loss=d)
    assert float(loss[1]) == np.inf and torch.all(grad[1] == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_above_256_labels_it_is_the_per_frame_call(kind):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = 2, 329, 8, 257
    x, labels, ll, tl = G.make_inputs(kind, B, T, V, U, seed=U)
    got, base = run_ck(kind, 0, x, labels, ll, tl), G.run(kind, 0, x, labels, ll, tl)
    assert OW.same_bits(got[0], base[0]) and OW.same_bits(got[1], base[1])
    k = G.kind_id(kind)
    assert _lib.wildcard_loss_ckpt_workspace_bytes(k, B, T, V, U) == _lib.wildcard_loss_workspace_bytes(k, B, T, V, U)
    assert 3 * _lib.wildcard_loss_ckpt_workspace_bytes(k, B, T, V, 256) < _lib.wildcard_loss_workspace_bytes(k, B, T, V, 256)


@pytest.mark.parametrize("V,blank", [(5, 0), (5, 2), (5, 4), (1030, 0), (1030, 515), (1030, 1029)])
@pytest.mark.parametrize("kind", KINDS)
def test_vocabulary_and_blank(kind, V, blank):
    x, labels, ll, tl = G.make_inputs(kind, 2, 40, V, 6, seed=30 + blank, blank=blank)
    if V > 1024:
        labels[0, 1], labels[1, 1] = 1025, 1025  # a token of the second column pass
        tl[:] = 40
    check(f"ckpt {kind} V={V} blank={blank}", kind, 0, x, labels, ll, tl, blank=blank)


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    B, T, V, U = G.FMT
    x, labels, ll, tl = G.make_inputs(kind, B, T, V, U, seed=20)
    xt = dev(x)
    loss_c, grad_c = check(f"ckpt {kind} float32", kind, 0, x, labels, ll, tl, ref=G.oracle(kind, 0, x, labels, ll, tl, key=("fmt", kind)))
    for dt in (torch.bfloat16, torch.float16):
        xh = xt.to(dt)
        ref = G.oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl, key=("fmt", kind, str(dt)))
        _, grad = check(f"ckpt {kind} {dt}", kind, 0, xh, labels, ll, tl, ref=ref, sixteen=True)
        assert grad.dtype == dt
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)  # time-major, read in place
    flat = torch.zeros(B * T * V + 1, dtype=torch.float32, device=G.DEV)
    xo = flat[1:].view(B, T, V)  # an unaligned base pointer: the element-wise accesses
    xo.copy_(xt)
    assert xtm.stride() == (V, B * V, 1) and xo.data_ptr() % 16 == 4
    for xv in (xtm, xo):
        loss, grad = run_ck(kind, 0, xv, labels, ll, tl)
        assert OW.same_bits(loss, loss_c) and OW.same_bits(grad.contiguous(), grad_c)


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_wildcard_weight_and_d_loss(kind, wrt):
    x, labels, ll, tl = G.make_inputs(kind, 4, 70, 7, 20, seed=7)
    x = G.logprobs32(x) if wrt else x
    d = np.random.default_rng(1).standard_normal(4).astype(np.float32) * 3
    d[2] = 0.0
    _, grad = check(f"ckpt {kind} w=-0.5 wrt={wrt}", kind, wrt, x, labels, ll, tl, weight=-0.5, d_loss=d)
    assert torch.all(grad[2].view(torch.int32) == 0), "+0 throughout"


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_whatever_the_buffers_held_and_under_graph_capture(kind):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = G.SINGLE
    x, labels, ll, tl = G.make_inputs(kind, B, T, V, U, seed=60)
    tl[1] = int(ll[1]) - 1  # one infeasible utterance: its zeros are written, not left over
    args = (kind, 0, dev(x), dev(labels), dev(ll), dev(tl), 0, -0.25, U, dev(np.asarray([1.5, np.nan], np.float32)))
    n = _lib.wildcard_loss_ckpt_workspace_bytes(G.kind_id(kind), B, T, V, U)

    def buffers(pattern):
        return OW.filled((B,), torch.float32, pattern, G.DEV), OW.filled((B, T, V), torch.float32, pattern, G.DEV), OW.byte_fill(n, pattern, G.DEV)
    outs = []
    for pattern in (0x00, 0xFF):
        loss, grad, ws = buffers(pattern)
        raw_ck(*args, loss, grad, ws)
        torch.cuda.synchronize()
        outs.append((loss, grad))
    assert OW.same_bits(outs[0][0], outs[1][0]) and OW.same_bits(outs[0][1], outs[1][1])
    assert float(outs[0][0][1]) == np.inf and torch.all(outs[0][1][1] == 0) and torch.isfinite(outs[0][1]).all()
    loss, grad, ws = buffers(0x5A)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        raw_ck(*args, loss, grad, ws)
    for _ in range(2):
        loss.fill_(7.0)
        grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert OW.same_bits(loss, outs[0][0]) and OW.same_bits(grad, outs[0][1])


@pytest.mark.parametrize("kind", KINDS)
def test_public_route(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 3, 40, 6, 10
    x, labels, ll, tl = G.make_inputs(kind, B, T, V, U, seed=70)
    fn = ctc.classic_ctc_wildcard_loss if kind == "classic" else ctc.simplified_ctc_wildcard_loss

    def public(**kw):
        xt = dev(x).requires_grad_(True)
        loss = fn(dev(labels), xt, dev(ll), dev(tl), 0, **kw)
        loss.sum().backward()
        return loss.detach(), xt.grad
    loss, grad = public(checkpoint=True)
    want = run_ck(kind, 0, x, labels, ll, tl, d_loss=np.ones(B, np.float32))
    assert OW.same_bits(loss, want[0]) and OW.same_bits(grad, want[1])
    window = torch.tensor([0, T - 1], dtype=torch.int32, device=G.DEV).expand(B, U, 2).contiguous()
    for other in (dict(frame_window=window), dict(optional_wildcards=True), dict(exclude_next_label=True)):  # owed: today's path
        got, base = public(checkpoint=True, **other), public(**other)
        assert OW.same_bits(got[0], base[0]) and OW.same_bits(got[1], base[1]), other
    xt = dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(fn(dev(labels), xt, dev(ll), dev(tl), 0, checkpoint=True).sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
