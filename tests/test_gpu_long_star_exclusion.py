"""exclude_next_label=True above 1024 labels: the long-form loss, gradient and label posteriors against
tests/tools/star_exclusion_oracle.py (float64).  Bars (section 5.27's): loss 1e-4 + 1e-6 |loss|; gradient and posterior element
1e-4 (16-bit gradient: + 2^-8 |oracle element|); duration within 1e-4 max(1, oracle)."""
import numpy as np
import pytest
import torch

import tf_seq2seq_losses_amd as ctc
from tf_seq2seq_losses_amd import _lib, ops
from tests.tools import star_exclusion_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, Q = SO.WILDCARD, SO.OPTIONAL
KINDS = SO.KINDS


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(kind, wrt, x, labels, ll, tl, blank=0, optional=False, exclude=True, d_loss=None, weight=0.0, tf=0, checkpoint=False,
        dense=True, grad_dtype=None):
    """(loss, grad, the seven posterior outputs) on the device."""
    k = ops.KINDS[kind]
    a = (k, wrt, dev(labels), dev(x), dev(ll), dev(tl), blank)
    d = None if d_loss is None else dev(d_loss)
    if exclude:
        loss, grad = ops.long_star_loss_grad(*a, d, None, grad_dtype, weight, True, tf, checkpoint, optional)
        post = ops.long_star_label_posterior(*a, None, weight, tf, dense, optional_wildcards=optional)
    else:
        fn = ops.long_optional_wildcard_loss_grad if optional else ops.long_wildcard_loss_grad
        loss, grad = fn(*a, d, None, grad_dtype, weight, True, tf, checkpoint)
        pf = ops.long_optional_wildcard_label_posterior if optional else ops.long_label_posterior
        post = pf(*a, None, weight, tf, dense)
    return loss, grad, post


def bits(out):
    loss, grad, post = out
    return [t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16) for t in (loss, grad) + tuple(post) if t is not None]


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(bits(a), bits(b)))


def check(kind, wrt, x, labels, ll, tl, blank=0, optional=False, d_loss=None, weight=0.0, xdev=None, sixteen=False, **kw):
    """Loss, gradient and posteriors against the oracle on the values in x (xdev: the same values as the device holds them)."""
    loss, grad, post = run(kind, wrt, x if xdev is None else xdev, labels, ll, tl, blank, optional, d_loss=d_loss, weight=weight, **kw)
    rl, rg = SO.loss_and_grad(kind, wrt, labels, x, ll, tl, blank, weight, d_loss, optional=optional)
    rp = SO.label_posterior(kind, wrt, labels, x, ll, tl, blank, weight, U=post[1].shape[2], optional=optional)
    loss, grad = loss.cpu().numpy(), grad.float().cpu().numpy()
    fin = np.isfinite(rl)
    assert np.array_equal(np.isfinite(loss), fin)
    err = [np.abs(loss[fin] - rl[fin]).max(initial=0.0), np.abs(grad - rg).max()]
    assert np.all(np.abs(loss[fin] - rl[fin]) <= 1e-4 + 1e-6 * np.abs(rl[fin]))
    assert np.all(np.abs(grad - rg) <= 1e-4 + (2.0 ** -8 * np.abs(rg) if sixteen else 0.0))
    assert torch.equal(post[0].cpu(), torch.from_numpy(loss))  # the posterior call's loss has the bits of the loss call's
    p = [t.cpu().numpy() for t in post]
    err += [np.abs(p[1] - rp[1]).max(), np.abs(p[2] - rp[2]).max(), (np.abs(p[3] - rp[3]) / np.maximum(1.0, rp[3])).max()]
    assert err[2] <= 1e-4 and err[3] <= 1e-4 and err[4] <= 1e-4
    assert np.array_equal(p[4] < 0, rp[4] < 0)
    print(kind, wrt, "optional" if optional else "mandatory", "worst loss / grad / label / blank / duration error:", *("%.2e" % e for e in err))
    return fin


def transcript(B, U, V, blank=0):
    """No equal neighbours, no blank."""
    tok = [t for t in range(V) if t != blank][:7]
    return np.asarray(tok, np.int32)[(np.arange(U)[None, :] + 3 * np.arange(B)[:, None]) % len(tok)]


def logits(rng, B, T, V, wrt=0, scale=2.0):
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if wrt:
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(axis=-1, keepdims=True))).astype(np.float32)
    return x


def boundary_case(B, optional):
    """Stars at 1023 (its label is the next block's first), at 1024, on a lane's last position (31, 47), last in the transcript and in
    front of a star; the last utterance is shorter than T and than U."""
    U = 1030
    labels = transcript(B, U, 8)
    star = Q if optional else W
    labels[0, [31, 1023, 1029]] = star
    labels[0, [500, 501]] = [W, star]
    labels[B - 1, [47, 1026] + ([1024] if B > 1 else [])] = star  # (B = 1: 1023 holds one already)
    if B > 2:
        labels[1, [1023, 1025]] = star
    ll, tl = np.full(B, U, np.int32), np.full(B, 1400, np.int32)
    ll[B - 1], tl[B - 1] = 1027, 1300
    return labels, ll, tl


@pytest.mark.parametrize("optional", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_at_the_block_boundary(kind, optional):
    rng = np.random.default_rng(1030)
    labels, ll, tl = boundary_case(3, optional)
    d_loss = rng.uniform(0.5, 2.0, 3).astype(np.float32)
    assert check(kind, 0, logits(rng, 3, 1400, 8), labels, ll, tl, optional=optional, d_loss=d_loss).all()


@pytest.mark.parametrize("optional", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_on_log_probabilities(kind, optional):
    rng = np.random.default_rng(7)
    labels, ll, tl = boundary_case(1, optional)
    assert check(kind, 1, logits(rng, 1, 1400, 8, 1), labels, ll, tl, optional=optional, weight=-0.7).all()


@pytest.mark.parametrize("kind", KINDS)
def test_two_boundaries_and_another_tile_height(kind):
    B, T, V, U = 2, 2600, 8, 2100
    rng = np.random.default_rng(2100)
    labels = transcript(B, U, V)
    labels[0, [1023, 2047, 2049]] = W
    labels[1, [1022, 1024, 2046, 2048]] = W
    ll, tl = np.asarray([U, 2060], np.int32), np.asarray([T, 2500], np.int32)
    assert check(kind, 0, logits(rng, B, T, V), labels, ll, tl, tf=64, checkpoint=True).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_star_between_every_pair_of_labels(kind):
    """515 labels and 514 optional stars: feasible in 600 frames, not in 500."""
    B, T, V, U = 2, 600, 8, 1029
    labels = transcript(B, U, V)
    labels[:, 1::2] = Q
    ll, tl = np.full(B, U, np.int32), np.asarray([600, 500], np.int32)
    x = logits(np.random.default_rng(515), B, T, V)
    fin = check(kind, 0, x, labels, ll, tl, optional=True)
    assert fin.tolist() == [True, False]
    loss, grad, post = run(kind, 0, x, labels, ll, tl, optional=True)
    assert torch.isposinf(loss[1]) and not grad[1].any() and (post[4][1] == -1).all()


@pytest.mark.parametrize("kind", KINDS)
def test_confident_frames(kind):
    """On the frames a star of label block 1 must own (L = T: every position one frame), 1 - p_t(y) of 1e-4 .. 1e-5; one frame on
    which y holds all the mass makes the loss +inf."""
    T = U = 1030
    labels = transcript(1, U, 8)
    labels[0, [1025, 1027]] = W
    y = [int(labels[0, 1026]), int(labels[0, 1028])]
    x = logits(np.random.default_rng(3), 1, T, 8)
    for t, tok, r in ((1025, y[0], 1e-4), (1027, y[1], 1e-5)):  # seven tokens at 0 and y at ln(7 (1 - r) / r): 1 - p = r
        x[0, t, :] = 0.0
        x[0, t, tok] = np.log(7.0 * (1.0 - r) / r)
    ll, tl = np.asarray([U], np.int32), np.asarray([T], np.int32)
    rest = 1.0 - np.exp(SO.log_probs(x[0], 0))[[1025, 1027], y]
    assert np.all(rest < 2e-4) and np.all(rest > 5e-6)
    assert check(kind, 0, x, labels, ll, tl).all()
    x[0, 1027, :] = -np.inf
    x[0, 1027, y[1]] = 0.0
    assert torch.isposinf(run(kind, 0, x, labels, ll, tl)[0]).all()


@pytest.mark.parametrize("optional", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_identities(kind, optional):
    rng = np.random.default_rng(11)
    labels, ll, tl = boundary_case(3, optional)
    x, d_loss = logits(rng, 3, 1400, 8), rng.uniform(0.5, 2.0, 3).astype(np.float32)
    a = (kind, 0, x, labels, ll, tl, 0, optional)
    ref = run(*a, d_loss=d_loss)
    assert torch.isfinite(ref[0]).all() and torch.equal(ref[0], ref[2][0])
    for kw in (dict(checkpoint=True), dict(tf=4), dict(tf=64, checkpoint=True)):
        assert same(ref, run(*a, d_loss=d_loss, **kw)), kw
    sparse = run(*a, d_loss=d_loss, dense=False)
    assert sparse[2][1] is None and same((ref[0], ref[1], ref[2][:1] + ref[2][2:]), (sparse[0], sparse[1], sparse[2][:1] + sparse[2][2:]))
    one = run(kind, 0, x[1:2], labels[1:2], ll[1:2], tl[1:2], 0, optional, d_loss=d_loss[1:2])  # alone / in a batch
    assert torch.equal(one[0], ref[0][1:2]) and torch.equal(one[1], ref[1][1:2]) and torch.equal(one[2][3], ref[2][3][1:2])
    big = torch.zeros((3, 1400, 14), device=DEV)  # strided
    big[:, :, 2:10] = dev(x)
    assert same(ref, run(kind, 0, big[:, :, 2:10], labels, ll, tl, 0, optional, d_loss=d_loss))
    # one graph capture and replay equals eager
    t = [dev(v) for v in (labels, x, ll, tl, d_loss)]
    k = ops.KINDS[kind]
    call = lambda: ops.long_star_loss_grad(k, 0, t[0], t[1], t[2], t[3], 0, t[4], None, None, 0.0, True, 0, True, optional)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1].view(torch.int32), ref[1].view(torch.int32))


def raw(kind, wrt, x, labels, ll, tl, optional, d_loss, fill):
    """ctc_amd_long_star_loss_grad_ckpt and _label_posterior on outputs and exact-size workspaces prefilled with `fill`."""
    lib, k = _lib.load(), ops.KINDS[kind]
    B, T, V = x.shape
    U = labels.shape[1]
    buf = lambda n: torch.full((int(n),), fill, dtype=torch.uint8, device=DEV)
    f32 = lambda *sh: buf(4 * int(np.prod(sh))).view(torch.float32).reshape(sh)
    t = [dev(v) for v in (x, labels, ll, tl, d_loss)]
    head = (k, wrt, t[0].data_ptr(), 0, T * V, V, t[1].data_ptr(), U, t[2].data_ptr(), t[3].data_ptr(), 0, int(optional), 0.0, B, T, V, U, 0)
    n = _lib.long_star_loss_workspace_bytes(k, B, T, V, U, 0, True, optional, True)
    m = _lib.long_star_label_posterior_workspace_bytes(k, B, T, V, U, 0, optional)
    st = torch.cuda.current_stream().cuda_stream
    loss, grad, ploss = f32(B), f32(B, T, V), f32(B)
    post = (f32(B, T, U), f32(B, T), f32(B, U), f32(B, U), f32(B, U), f32(B, U))
    ws, wp = buf(n), buf(m)
    rc = lib.ctc_amd_long_star_loss_grad_ckpt(*head, t[4].data_ptr(), loss.data_ptr(), grad.data_ptr(), 0, T * V, V, ws.data_ptr(), n, st)
    assert rc == 0, lib.ctc_amd_last_error()
    rc = lib.ctc_amd_long_star_label_posterior(*head, ploss.data_ptr(), *(p.data_ptr() for p in post), wp.data_ptr(), m, st)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    return [v.view(torch.int32) for v in (loss, grad, ploss) + post]


@pytest.mark.parametrize("kind", KINDS)
def test_prefilled_outputs_and_workspaces(kind):
    rng = np.random.default_rng(5)
    labels, ll, tl = boundary_case(3, True)
    tl[1] = 400  # an infeasible utterance as well
    x, d_loss = logits(rng, 3, 1400, 8), np.asarray([1.5, 1.0, 0.5], np.float32)
    a, b = (raw(kind, 0, x, labels, ll, tl, True, d_loss, fill) for fill in (0x00, 0xFF))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("optional", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_no_excluding_star_has_the_bits_of_the_call_without_the_keyword(kind, optional):
    B, T, U = 3, 1400, 1030
    labels = transcript(B, U, 8)
    star = Q if optional else W
    labels[0, [500, 1029]] = [3, star]   # a star last in the transcript (500: so that 499 .. 501 have no equal neighbours)
    labels[0, 500] = labels[0, 500 + 7]
    labels[1, [1023, 1024]] = [star, W]  # a star in front of a star across the boundary, the second one last (label_length 1025)
    labels[2, 1023] = star               # an infeasible utterance (too few frames) with a star that would exclude
    ll, tl = np.asarray([U, 1025, U], np.int32), np.asarray([T, T, 300], np.int32)
    x = logits(np.random.default_rng(9), B, T, 8)
    on, off = run(kind, 0, x, labels, ll, tl, 0, optional), run(kind, 0, x, labels, ll, tl, 0, optional, exclude=False)
    assert torch.isfinite(on[0][:2]).all() and torch.isposinf(on[0][2]) and same(on, off)


@pytest.mark.parametrize("shape", ((169, 129), (1300, 1024)))
@pytest.mark.parametrize("kind", KINDS)
def test_one_label_block_has_the_short_form_bits(kind, shape):
    T, U = shape
    labels = transcript(2, U, 8)
    labels[0, [3, U - 2]] = W
    labels[1, [15, 40]] = [Q, W]
    ll, tl = np.asarray([U, U - 5], np.int32), np.asarray([T, T - 7], np.int32)
    rng = np.random.default_rng(U)
    x, d_loss = logits(rng, 2, T, 8), rng.uniform(0.5, 2.0, 2).astype(np.float32)
    loss, grad, post = run(kind, 0, x, labels, ll, tl, 0, True, d_loss=d_loss)
    a = (ops.KINDS[kind], 0, dev(labels), dev(x), dev(ll), dev(tl), 0)
    sl, sg = ops.wildcard_loss_grad(*a, dev(d_loss), None, None, 0.0, True, optional_wildcards=True, exclude_next_label=True)
    sp = ops.label_posterior(*a, None, 0.0, optional_wildcards=True, exclude_next_label=True)
    assert torch.equal(loss, sl) and torch.equal(grad.view(torch.int32), sg.view(torch.int32))
    assert torch.equal(post[1], sp[1]) and torch.equal(post[3], sp[3])


@pytest.mark.parametrize("fmt,blank", (("strided", 5), ("bfloat16", 1029), ("float16", 5)))
@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind, fmt, blank):
    """V = 1030: three column passes of the star row stage, excluded tokens and the blank in the last."""
    B, T, V, U = 2, 1200, 1030, 1030
    rng = np.random.default_rng(V)
    labels = transcript(B, U, V, blank)
    labels[0, 1::9] = 1024 + np.arange(len(labels[0, 1::9])) % 5  # tokens of the third pass
    labels[0, [9, 1023]] = W                                       # (position 10 holds such a token)
    labels[1, [1024, 700]] = W
    ll, tl = np.asarray([U, 1026], np.int32), np.asarray([T, 1100], np.int32)
    x = logits(rng, B, T, V, scale=3.0)
    if fmt == "strided":
        big = torch.zeros((B, T, V + 6), device=DEV)
        xdev = big[:, :, 2:V + 2]
        xdev.copy_(dev(x))
    else:
        xdev = dev(x).to(torch.bfloat16 if fmt == "bfloat16" else torch.float16)
        x = xdev.float().cpu().numpy()
    d_loss = np.asarray([1.25, 0.75], np.float32)
    assert check(kind, 0, x, labels, ll, tl, blank, d_loss=d_loss, xdev=xdev, sixteen=fmt != "strided").all()
    g = run(kind, 0, xdev, labels, ll, tl, blank, d_loss=np.zeros(B, np.float32))[1]
    assert not g.view(torch.int32 if fmt == "strided" else torch.int16).any()  # a weight of zero: +0 throughout


def test_python_layer():
    labels, ll, tl = boundary_case(1, False)
    x = dev(logits(np.random.default_rng(2), 1, 1400, 8)).requires_grad_(True)
    a = (dev(labels), x, dev(ll), dev(tl), 0)
    with pytest.raises(ValueError):
        ctc.classic_ctc_long_loss(*a, exclude_next_label=True, frame_window=torch.zeros((1, 1030, 2), dtype=torch.int32, device=DEV))
    loss = ctc.simplified_ctc_long_loss(*a, exclude_next_label=True, checkpoint=True)
    (g,) = torch.autograd.grad(loss.sum(), x, create_graph=True)
    rl, rg = ops.long_star_loss_grad(1, 0, a[0], x.detach(), a[2], a[3], 0, torch.ones(1, device=DEV))
    assert torch.equal(loss.detach(), rl) and torch.equal(g.detach(), rg)
    with pytest.raises(RuntimeError):  # a second derivative keeps raising
        torch.autograd.grad(g.sum(), x)
    post = ctc.simplified_ctc_long_star_label_posterior(*a, dense=False)
    assert post.label_posterior is None and torch.equal(post.loss, rl)
