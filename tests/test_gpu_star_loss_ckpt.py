"""Star CTC loss and gradient from block checkpoints on the GPU (ctc_amd_star_loss_grad_ckpt) against the float64 oracle
tests/tools/star_exclusion_oracle.py, at the project's bars: loss 1e-4 + 1e-6 |loss|, gradient 1e-4 per element (+ 2^-8 |oracle| for
a 16-bit one).  F = 32 / 16 / 8 frames per block at U <= 64 / 128 / 256."""
import numpy as np
import pytest
import torch

import tf_seq2seq_losses_amd as ctc
from tf_seq2seq_losses_amd import _lib, ops
from tests import test_gpu_star_exclusion as S
from tests.tools import star_exclusion_oracle as SO

pytestmark = pytest.mark.gpu
DEV, W, Q, WEIGHT, LATTICES, dev, logits = S.DEV, S.W, S.Q, S.WEIGHT, S.LATTICES, S.dev, S.logits
FLAGS = [(True, False), (False, True), (True, True)]  # (optional_wildcards, exclude_next_label)


def stars(labels, optional):  # without optional_wildcards an optional star is a mandatory one
    labels = np.asarray(labels, np.int32)
    return labels if optional else np.where(labels == Q, W, labels).astype(np.int32)


def run(kind, wrt, x, labels, ll, tl, flags, blank=0, d_loss=None, U=None, fn=None):
    a = (ops.KINDS[kind], wrt, dev(labels), dev(x), dev(ll), dev(tl), blank, None if d_loss is None else dev(d_loss), U, None, WEIGHT)
    loss, grad = (fn or ops.star_loss_grad)(*a, optional_wildcards=flags[0], exclude_next_label=flags[1])
    torch.cuda.synchronize()
    return loss, grad


def check(kind, wrt, x, labels, ll, tl, flags, blank=0, d_loss=None, U=None, xdev=None, sixteen=False):
    """Against the oracle on the values in x (xdev: as the device holds them); the forward-only per-frame loss bits; +0 from T_b on."""
    loss, grad = run(kind, wrt, x if xdev is None else xdev, labels, ll, tl, flags, blank, d_loss, U)
    rl, rg = SO.loss_and_grad(kind, wrt, labels, x, ll, tl, blank, WEIGHT, d_loss, optional=flags[0], exclude=flags[1])
    fin = np.isfinite(rl)
    got, gg = loss.cpu().numpy(), grad.float().cpu().numpy()
    assert np.array_equal(np.isfinite(got), fin)
    assert np.all(np.abs(got[fin] - rl[fin]) <= 1e-4 + 1e-6 * np.abs(rl[fin]))
    assert np.all(np.abs(gg - rg) <= 1e-4 + (2.0 ** -8 * np.abs(rg) if sixteen else 0.0))
    loss0 = ops.wildcard_loss_grad(ops.KINDS[kind], wrt, dev(labels), dev(x if xdev is None else xdev), dev(ll), dev(tl), blank, None, U,
                                   None, WEIGHT, False, optional_wildcards=flags[0], exclude_next_label=flags[1])[0]
    assert same([loss0], [loss])
    bits = grad.view(torch.int32 if grad.dtype == torch.float32 else torch.int16)
    assert all(torch.all(bits[b, int(tl[b]):] == 0) and (fin[b] or torch.all(bits[b] == 0)) for b in range(len(tl)))
    return loss, grad, fin


# an optional star first, last (end states before it), between every pair of labels; a mandatory one before a repeated label; none
PATTERNS = [[Q, 1, 2], [1, 2, Q], [1, Q, 2, Q, 3], [1, W, 2, 2, 3], [1, 1, 2, 3, 3, 1]]
EDGES = [(U, F, T, i) for U, F in ((3, 32), (65, 16), (129, 8)) for i, T in enumerate((1, F - 1, F, F + 1, 2 * F + 1, 3 * F + 2))]


@pytest.mark.parametrize("U,F,T,i", EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_block_edges_and_pipeline_fill_and_drain(kind, wrt, flags, U, F, T, i):
    """1 to 4 blocks, T_b = (T, 0, max(T - 2, 1)), V = 6; short transcripts (cut to the frames there are) in all three tiers."""
    rng = np.random.default_rng(100 * U + T)
    x = logits(rng, 3, T, 6, wrt)
    tl = np.asarray([T, 0, max(T - 2, 1)], np.int32)
    labels = rng.integers(1, 6, (3, max(U, 6))).astype(np.int32)
    ll = np.zeros(3, np.int32)
    for b in range(3):
        pat = PATTERNS[(i + 2 * b) % 5][:min(U, max(int(tl[b]), 1))]
        labels[b, :len(pat)] = pat
        ll[b] = len(pat)
    check(kind, wrt, x, stars(labels, flags[0]), ll, tl, flags, U=U)


def cyclic(B, U, V, w=None, q=None, optional=True):
    """Ordinary labels no two of which are equal at a distance of one or two (a skipped star joins its neighbours), stars at w and q."""
    labels = (1 + (np.arange(U)[None, :] + 2 * np.arange(B)[:, None]) % (V - 1)).astype(np.int32)
    labels[:, w if w is not None else []] = W
    labels[:, q if q is not None else []] = Q
    return stars(labels, optional)


def same(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


@pytest.mark.parametrize("NL,U", [(1, 43), (2, 85), (4, 169)])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_lane_and_register_boundaries(kind, wrt, flags, NL, U):
    """An excluding star on a lane's last position (its label is the next lane's first), an optional star on a lane's last and
    first position (the skip reaches two positions back across lanes; NL = 1: two lanes); the second utterance ends on an optional star."""
    B, V, T = 2, 8, U + 5
    labels = cyclic(B, U, V, [5 * NL - 1, 13 * NL + NL // 2], [9 * NL - 1, 17 * NL, U - 2], flags[0])
    assert check(kind, wrt, logits(np.random.default_rng(U), B, T, V, wrt), labels, np.asarray([U, U - 1], np.int32),
                 np.asarray([T, T - 3], np.int32), flags)[2].all()


@pytest.mark.parametrize("U", [64, 65, 129, 256])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_full_tiers(kind, wrt, flags, U):
    """T a few frames above the fewest that fit; the second utterance a frame short: +inf, zeros, the NaN in its d_loss ignored."""
    B, V = 3, 8
    labels = cyclic(B, U, V, slice(3, None, 8), slice(7, None, 16), flags[0])
    need = int((labels[0] != Q).sum())  # (every mandatory position takes a frame; no blank is forced between unequal labels)
    tl = np.asarray([need + 3, need - 1, need + 2], np.int32)
    x = logits(np.random.default_rng(U), B, need + 3, V, wrt)
    loss, grad, fin = check(kind, wrt, x, labels, np.full(B, U, np.int32), tl, flags, d_loss=np.asarray([1.5, np.nan, -0.7], np.float32))
    assert list(fin) == [True, False, True] and float(loss[1]) == np.inf


@pytest.mark.parametrize("V,blank", [(5, 0), (5, 2), (5, 4), (516, 0), (516, 258), (516, 515), (1030, 0), (1030, 515), (1030, 1029)])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_column_passes_and_the_blank(kind, wrt, flags, V, blank):
    """The excluded token and an ordinary label in the row stage's last column pass (512 columns with the exclusion, 1024 without)."""
    hi = [k for k in range(V - 1, 0, -1) if k != blank][:3]
    lo = [k for k in range(1, V) if k != blank][:2]
    labels = stars([[W, hi[0], lo[0], Q, hi[1], hi[2]], [hi[1], Q, hi[0], W, hi[0], lo[1]]], flags[0])
    x = logits(np.random.default_rng(V + blank), 2, 40, V, wrt, scale=3.0)
    assert check(kind, wrt, x, labels, np.asarray([6, 6], np.int32), np.asarray([40, 31], np.int32), flags, blank=blank)[2].all()


@pytest.mark.parametrize("flags", FLAGS[1:])
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_confident_frame(kind, wrt, flags):
    """1 - p of 1e-4 .. 1e-5 on frames the star must own: tests/test_gpu_star_exclusion.py::test_confident_frame on this route."""
    labels = np.asarray([[W, 2, 1], [3, W, 2], [3, W, 2]], np.int32)
    ll, tl = np.asarray([3, 3, 3], np.int32), np.asarray([3, 3, 5], np.int32)
    x = logits(np.random.default_rng(2), 3, 12, 5, 0, scale=1.0)
    x[0, 0, 2] += 9.0
    x[1, 1, 2] += 12.0
    x[2, 1:4, 2] += np.asarray([10.0, 11.0, 9.5], np.float32)
    if wrt:
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(axis=-1, keepdims=True))).astype(np.float32)
    assert np.isfinite(SO.loss_and_grad(kind, wrt, labels, x, ll, tl, 0, WEIGHT, optional=flags[0])[0]).all()  # (on the CPU first)
    assert check(kind, wrt, x, labels, ll, tl, flags)[2].all()


@pytest.mark.parametrize("fmt", [torch.bfloat16, torch.float16, "time-major"], ids=str)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_formats(kind, wrt, flags, fmt):
    B, T, V, U = 3, 45, 12, 20
    labels = cyclic(B, U, V, slice(2, None, 6), slice(5, None, 6), flags[0])
    ll, tl = np.asarray([U, U - 3, 7], np.int32), np.asarray([T, T - 4, 20], np.int32)
    xdev = dev(logits(np.random.default_rng(5), B, T, V, wrt))
    xdev = xdev.transpose(0, 1).contiguous().transpose(0, 1) if fmt == "time-major" else xdev.to(fmt)
    _, grad, fin = check(kind, wrt, xdev.float().cpu().numpy(), labels, ll, tl, flags, xdev=xdev, sixteen=fmt != "time-major")
    assert fin.all() and grad.dtype == xdev.dtype


def raw(kind, wrt, x, labels, ll, tl, flags, d_loss, fill):  # the C entry point into outputs and a workspace prefilled with `fill`
    (B, T, V), U = x.shape, labels.shape[1]
    n = _lib.star_loss_ckpt_workspace_bytes(ops.KINDS[kind], B, T, V, U)
    loss, grad, ws = (torch.full(s, fill, device=DEV) for s in ((B,), (B, T, V), (n // 4 + 1,)))
    rc = _lib.load().ctc_amd_star_loss_grad_ckpt(
        ops.KINDS[kind], wrt, x.data_ptr(), 0, T * V, V, labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0, int(flags[0]), int(flags[1]),
        WEIGHT, B, T, V, U, d_loss.data_ptr(), loss.data_ptr(), grad.data_ptr(), 0, T * V, V, ws.data_ptr(), n,
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_star_loss_grad_ckpt")
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_same_bits_whatever_the_buffers_held(kind, wrt, flags):
    """Prefilled with 7.0 and -7.0; d_loss = 0 gives +0 throughout; two adjacent -3 give +inf and zeros (two mandatory stars are feasible)."""
    B, T, V, U = 4, 45, 7, 70
    labels = cyclic(B, U, V, slice(4, None, 9), slice(8, None, 9))
    labels[3, 9] = Q  # beside the optional star at 8
    labels = stars(labels, flags[0])
    x = dev(logits(np.random.default_rng(9), B, T, V, wrt))
    ll, tl = np.asarray([30, 12, 25, 20], np.int32), np.asarray([T, 30, 40, T], np.int32)
    a = (kind, wrt, x, dev(labels), dev(ll), dev(tl), flags, dev(np.asarray([1.5, 0.0, -2.0, np.nan if flags[0] else 1.0], np.float32)))
    (l1, g1), (l2, g2) = raw(*a, 7.0), raw(*a, -7.0)
    assert same((l1, g1), (l2, g2))
    assert torch.isfinite(l1[:3]).all() and torch.all(g1[1].view(torch.int32) == 0) and g1[0].abs().max() > 0
    assert (float(l1[3]) == np.inf and torch.all(g1[3].view(torch.int32) == 0)) == flags[0]


@pytest.mark.parametrize("flags", FLAGS + [(False, False)])
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_without_such_a_star_it_is_the_mandatory_wildcard_call(kind, wrt, flags):
    """No -3 and no star in front of an ordinary label: the loss and gradient bits of wildcard_loss_grad(checkpoint=True)."""
    B, T, V, U = 3, 150, 8, 129
    labels = cyclic(B, U, V)
    labels[0, 100:] = W  # (followed by stars alone)
    labels[1, 59] = W    # (the last position)
    x, ll, tl = logits(np.random.default_rng(3), B, T, V, wrt), np.asarray([U, 60, 40], np.int32), np.asarray([T, T - 9, 70], np.int32)
    got = run(kind, wrt, x, labels, ll, tl, flags)
    want = run(kind, wrt, x, labels, ll, tl, (False, False), fn=lambda *a, **kw: ops.wildcard_loss_grad(*a, checkpoint=True))
    assert torch.isfinite(got[0]).all() and same(got, want)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_above_256_labels_it_is_the_per_frame_call(kind, wrt, flags):
    B, T, V, U = 2, 300, 8, 257
    labels = cyclic(B, U, V, slice(3, None, 8), slice(7, None, 16), flags[0])
    x, ll, tl = logits(np.random.default_rng(4), B, T, V, wrt), np.asarray([U, 200], np.int32), np.asarray([T, T - 5], np.int32)
    assert same(run(kind, wrt, x, labels, ll, tl, flags), run(kind, wrt, x, labels, ll, tl, flags, fn=ops.wildcard_loss_grad))
    size, per_frame, k = _lib.star_loss_ckpt_workspace_bytes, _lib.wildcard_loss_workspace_bytes, ops.KINDS[kind]
    assert size(k, B, T, V, U) == per_frame(k, B, T, V, U) and 3 * size(k, B, T, V, 256) < per_frame(k, B, T, V, 256)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_public_route(kind, wrt, flags):
    """The three public functions return ops.star_loss_grad's bits through autograd; a second derivative raises."""
    B, T, V, U = 3, 40, 6, 10
    labels = cyclic(B, U, V, slice(2, None, 5), slice(4, None, 5), flags[0])
    ll, tl = np.asarray([U, 6, 9], np.int32), np.asarray([T, 30, 5], np.int32)  # (the last infeasible)
    x = logits(np.random.default_rng(70), B, T, V, wrt)
    kw = dict(wildcard_log_weight=WEIGHT, optional_wildcards=flags[0], exclude_next_label=flags[1])
    cls = [ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData] if wrt else []
    star = ctc.ctc_star_loss_from_logproba if wrt else ctc.classic_ctc_star_loss if kind == "classic" else ctc.simplified_ctc_star_loss
    fn = lambda xt: star(dev(labels), xt, dev(ll), dev(tl), 0, *cls, **kw)  # noqa: E731
    xt, d = dev(x).requires_grad_(True), torch.tensor([1.0, -2.0, 0.5], device=DEV)
    loss = fn(xt)
    (loss * d).sum().backward()
    want = run(kind, wrt, x, labels, ll, tl, flags, d_loss=d)
    assert same((loss.detach(), xt.grad), want)
    xt = dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(fn(xt)[:2].sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
