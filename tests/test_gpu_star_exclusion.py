"""exclude_next_label=True on the GPU (star temporal classification: the star excludes the label behind it): loss, gradient,
label posteriors and alignment against tests/tools/star_exclusion_oracle.py (float64, pinned in
tests/test_star_exclusion_oracle.py).  Bars: loss 1e-4 + 1e-6 |loss|; gradient element 1e-4 (+ 2^-8 |oracle| for a 16-bit
gradient); posterior element and row sum 1e-4; alignment paths and per-label frames exact, score and label_score
1e-4 + 1e-6 |score| (the wildcard alignment tests' bar).  Two stars with a successor each need four positions, so the smallest
shape runs at U = 3 and U = 4."""
import numpy as np
import pytest
import torch

import tf_seq2seq_losses_amd as ctc
from tf_seq2seq_losses_amd import ops
from tests.tools import star_exclusion_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, Q = SO.WILDCARD, SO.OPTIONAL
WEIGHT = -0.25
LATTICES = [(k, w) for k in SO.KINDS for w in (0, 1)]


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def run(kind, wrt, x, labels, ll, tl, blank=0, optional=True, exclude=True, d_loss=None):
    """(loss, grad, posteriors tuple) as CPU tensors; x: numpy or a device tensor in any format."""
    k = ops.KINDS[kind]
    kw = dict(optional_wildcards=optional, exclude_next_label=exclude)
    a = (dev(labels), dev(x), dev(ll), dev(tl), blank)
    loss, grad = ops.wildcard_loss_grad(k, wrt, *a, None if d_loss is None else dev(d_loss), None, None, WEIGHT, True, **kw)
    post = ops.label_posterior(k, wrt, *a, None, WEIGHT, **kw)
    torch.cuda.synchronize()
    return loss.cpu(), grad.float().cpu(), tuple(p.cpu() for p in post)


def check(kind, wrt, x, labels, ll, tl, blank=0, optional=True, xdev=None, sixteen=False):
    """The three summed-lattice calls against the oracle on the values in x (numpy; xdev: the same values as the device holds them)."""
    loss, grad, post = run(kind, wrt, x if xdev is None else xdev, labels, ll, tl, blank, optional)
    rl, rg = SO.loss_and_grad(kind, wrt, labels, x, ll, tl, blank, WEIGHT, optional=optional)
    rp = SO.label_posterior(kind, wrt, labels, x, ll, tl, blank, WEIGHT, optional=optional)
    fin = np.isfinite(rl)
    assert np.array_equal(np.isfinite(loss.numpy()), fin)
    assert np.all(np.abs(loss.numpy()[fin] - rl[fin]) <= tol(rl[fin]))
    assert np.all(np.abs(grad.numpy() - rg) <= 1e-4 + (2.0 ** -8 * np.abs(rg) if sixteen else 0.0))
    assert torch.equal(post[0], loss)  # the posterior call's loss has the bits of the loss call
    assert np.abs(post[1].numpy() - rp[1]).max() <= 1e-4 and np.abs(post[2].numpy() - rp[2]).max() <= 1e-4
    rows = post[1].numpy().sum(axis=2) + post[2].numpy()
    for b in np.nonzero(fin)[0]:
        assert np.abs(rows[b, :int(tl[b])] - 1.0).max() <= 1e-4
    return fin


def align(kind, wrt, x, labels, ll, tl, blank=0, optional=True, **kw):
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    a = (dev(labels), dev(x), dev(ll), dev(tl), blank)
    if wrt:
        return ctc.ctc_wildcard_alignment_from_logproba(*a, cls, optional_wildcards=optional, **kw)
    fn = ctc.classic_ctc_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_wildcard_alignment
    return fn(*a, optional_wildcards=optional, **kw)


def check_align(kind, wrt, x, labels, ll, tl, blank=0, optional=True):
    got = align(kind, wrt, x, labels, ll, tl, blank, optional, exclude_next_label=True)
    score, rest = SO.best_path(kind, labels, x, ll, tl, blank, wrt, optional=optional)
    g = {k: v.cpu().numpy() for k, v in got._asdict().items()}
    for b, r in enumerate(rest):
        if r is None:
            assert g["score"][b] == -np.inf and np.all(g["tokens"][b] == -1)
            continue
        path, index, first, last, lscore = r
        Tb, Lb = len(path), len(first)
        assert np.array_equal(g["tokens"][b, :Tb], path) and np.array_equal(g["label_index"][b, :Tb], index)
        assert np.array_equal(g["first_frame"][b, :Lb], first) and np.array_equal(g["last_frame"][b, :Lb], last)
        assert abs(g["score"][b] - score[b]) <= tol(score[b])
        assert np.all(np.abs(g["label_score"][b, :Lb] - lscore) <= tol(score[b]))
    return score


def logits(rng, B, T, V, wrt, scale=2.0):
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    if wrt:
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(axis=-1, keepdims=True))).astype(np.float32)
    return x


# stars first, last and in the middle, a star followed by a star, an optional star that must be skipped (its utterance has two frames
# for two ordinary labels); two stars with the same next token, with different ones, and two optional ones
SMALL = {3: ([[W, 2, W], [1, W, 3], [W, W, 3], [Q, 2, 1]], [12, 9, 12, 2]),
         4: ([[W, 2, W, 2], [W, 2, W, 3], [Q, 1, Q, 1], [2, W, W, 1]], [12, 10, 7, 12])}


@pytest.mark.parametrize("optional", (True, False))
@pytest.mark.parametrize("U", (3, 4))
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_smallest_shape(kind, wrt, U, optional):
    labels, tl = (np.asarray(a, dtype=np.int32) for a in SMALL[U])
    if not optional:  # the same transcripts with mandatory stars (the two-frame utterance is then infeasible)
        labels = np.where(labels == Q, W, labels).astype(np.int32)
    ll = np.full(4, U, np.int32)
    x = logits(np.random.default_rng(U), 4, 12, 5, wrt)
    fin = check(kind, wrt, x, labels, ll, tl, optional=optional)
    assert fin.sum() >= 3
    check_align(kind, wrt, x, labels, ll, tl, optional=optional)


@pytest.mark.parametrize("shape,stars", [((2, 88, 8, 64), (5, 40, 63)), ((2, 169, 8, 129), (3, 63, 127))], ids=("nl1", "nl4"))
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_next_label_in_the_next_lane(kind, wrt, shape, stars):
    """Stars on a lane's last position (its next label is the next lane's first), at 63 / 127 among them; the second utterance is
    shorter, so that its star at 63 / 127 is followed by nothing or by a label, and has an optional star."""
    B, T, V, U = shape
    rng = np.random.default_rng(U)
    labels = (1 + (np.arange(U)[None, :] + np.asarray([[0], [3]])) % (V - 1)).astype(np.int32)  # (no equal neighbours)
    labels[:, list(stars)] = W
    labels[1, 7] = Q
    ll, tl = np.asarray([U, U - 1], np.int32), np.asarray([T, T - 3], np.int32)
    x = logits(rng, B, T, V, wrt)
    assert check(kind, wrt, x, labels, ll, tl).all()
    check_align(kind, wrt, x, labels, ll, tl)


@pytest.mark.parametrize("fmt", ("strided", "bfloat16"))
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_second_column_pass(kind, wrt, fmt):
    """V = 1030: the excluded tokens and the blank lie in the row stage's second pass of 1024 columns."""
    B, T, V, U = 2, 40, 1030, 6
    rng = np.random.default_rng(11)
    labels = np.asarray([[W, 1029, 5, W, 1025, 1026], [1028, Q, 1029, W, 1029, 7]], np.int32)
    ll, tl = np.asarray([6, 6], np.int32), np.asarray([40, 31], np.int32)
    x = logits(rng, B, T, V, wrt, scale=3.0)
    if fmt == "strided":
        big = torch.zeros((B, T, V + 6), device=DEV)
        xdev = big[:, :, 2:V + 2]
        xdev.copy_(dev(x))
    else:
        xdev = dev(x).to(torch.bfloat16)
        x = xdev.float().cpu().numpy()
    assert check(kind, wrt, x, labels, ll, tl, blank=1027, xdev=xdev, sixteen=fmt == "bfloat16").all()
    check_align(kind, wrt, x, labels, ll, tl, blank=1027)


@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_confident_frame(kind, wrt):
    """1 - p of 1e-4 .. 1e-5 on frames the star must own (three frames for three positions; five for the third utterance, whose
    star may own any of three), at the same bars: what the (max, sum of the rest) statistics are for."""
    labels = np.asarray([[W, 2, 1], [3, W, 2], [3, W, 2]], np.int32)
    ll, tl = np.asarray([3, 3, 3], np.int32), np.asarray([3, 3, 5], np.int32)
    x = np.random.default_rng(2).standard_normal((3, 12, 5)).astype(np.float32)
    x[0, 0, 2] += 9.0
    x[1, 1, 2] += 12.0
    x[2, 1:4, 2] += np.asarray([10.0, 11.0, 9.5], np.float32)
    if wrt:
        x = (x - np.log(np.exp(x.astype(np.float64)).sum(axis=-1, keepdims=True))).astype(np.float32)
    assert np.isfinite(SO.loss_and_grad(kind, wrt, labels, x, ll, tl, 0, WEIGHT)[0]).all()
    assert check(kind, wrt, x, labels, ll, tl).all()


@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_alignment_rows(kind, wrt):
    """A row whose arg max is the excluded token; two equal maxima of which the lower token is the excluded one; V = 2 with the other
    token at -inf: the emission is -inf and the utterance, whose star is forced there, infeasible."""
    x = np.random.default_rng(4).standard_normal((2, 6, 4)).astype(np.float32)
    x[0, :, 2] = 5.0                 # the arg max of every row is token 2 ...
    x[1, :, 1] = x[1, :, 3] = 4.0    # ... tokens 1 and 3 tie
    labels = np.asarray([[W, 2, 3], [W, 1, 2]], np.int32)
    ll, tl = np.asarray([3, 3], np.int32), np.asarray([6, 6], np.int32)
    check_align(kind, wrt, x, labels, ll, tl)
    got = align(kind, wrt, x, labels, ll, tl, exclude_next_label=True)
    assert 2 not in got.tokens[0, :int(got.last_frame[0, 0]) + 1].tolist() and got.tokens[1, 0].item() == 3
    x2 = np.zeros((1, 2, 2), np.float32)
    x2[:, :, 0] = -np.inf
    lab2, one, two = np.asarray([[W, 1]], np.int32), np.asarray([2], np.int32), np.asarray([2], np.int32)
    assert check_align(kind, 1, x2, lab2, one, two)[0] == -np.inf
    assert run(kind, 1, x2, lab2, one, two)[0].item() == np.inf


@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_contracts(kind, wrt):
    rng = np.random.default_rng(9)
    x = logits(rng, 4, 12, 5, wrt)
    ll, tl = np.full(4, 3, np.int32), np.asarray([12, 9, 12, 5], np.int32)
    plain = np.asarray([[2, W, W], [1, 3, W], [2, W, Q], [Q, W, W]], np.int32)  # no star has an ordinary successor
    star = np.asarray(SMALL[3][0], np.int32)

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))

    def same_path(a, b):
        return all(torch.equal(p, q) for p, q in zip(a, b))

    # False is the call without the keyword; True without an excluding star has the bits of False; a second run has the same bits
    k = ops.KINDS[kind]
    a = (dev(star), dev(x), dev(ll), dev(tl), 0)
    off = ops.wildcard_loss_grad(k, wrt, *a, None, None, None, WEIGHT, True, optional_wildcards=True)
    off_kw = run(kind, wrt, x, star, ll, tl, exclude=False)
    assert torch.equal(off[0].cpu(), off_kw[0]) and torch.equal(off[1].cpu(), off_kw[1])
    assert same(run(kind, wrt, x, plain, ll, tl, exclude=True), run(kind, wrt, x, plain, ll, tl, exclude=False))
    assert same(run(kind, wrt, x, star, ll, tl), run(kind, wrt, x, star, ll, tl))
    assert not torch.equal(run(kind, wrt, x, star, ll, tl)[0], off_kw[0])
    assert same_path(align(kind, wrt, x, star, ll, tl), align(kind, wrt, x, star, ll, tl, exclude_next_label=False))
    assert same_path(align(kind, wrt, x, plain, ll, tl, exclude_next_label=True), align(kind, wrt, x, plain, ll, tl))
    assert same_path(align(kind, wrt, x, star, ll, tl, exclude_next_label=True), align(kind, wrt, x, star, ll, tl, exclude_next_label=True))
    # a weight of zero: +0 in every element
    g = run(kind, wrt, x, star, ll, tl, d_loss=np.zeros(4, np.float32))[1]
    assert torch.equal(g.view(torch.int32), torch.zeros_like(g, dtype=torch.int32))
    # not with a frame window
    fw = torch.zeros((4, 3, 2), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        align(kind, wrt, x, star, ll, tl, optional=False, exclude_next_label=True, frame_window=fw)
    with pytest.raises(ValueError):
        ops.wildcard_loss_grad(k, wrt, *a, frame_window=fw, exclude_next_label=True)
    with pytest.raises(ValueError):
        ops.label_posterior(k, wrt, *a, frame_window=fw, exclude_next_label=True)


def raw_calls(kind, wrt, x, labels, ll, tl, fill, d_loss):
    """The three C entry points on outputs and workspaces prefilled with `fill`: every output as a CPU tensor, in one tuple."""
    from tf_seq2seq_losses_amd import _lib
    lib, k = _lib.load(), ops.KINDS[kind]
    B, T, V = x.shape
    U = labels.shape[1]
    buf = lambda n: torch.full((int(n),), fill, dtype=torch.uint8, device=DEV)
    f32 = lambda *sh: buf(4 * int(np.prod(sh))).view(torch.float32).reshape(sh)
    i32 = lambda *sh: buf(4 * int(np.prod(sh))).view(torch.int32).reshape(sh)
    t = [dev(v) for v in (x, labels, ll, tl, d_loss)]
    head = (k, wrt, t[0].data_ptr(), 0, T * V, V, t[1].data_ptr(), U, t[2].data_ptr(), t[3].data_ptr(), 0, 1)
    n = _lib.wildcard_loss_workspace_bytes(k, B, T, V, U)
    na = _lib.star_best_path_workspace_bytes(k, B, T, V, U, True)
    st = torch.cuda.current_stream().cuda_stream
    loss, grad, ploss = f32(B), f32(B, T, V), f32(B)
    post = (f32(B, T, U), f32(B, T), f32(B, U), f32(B, U))
    path = (f32(B), i32(B, T), i32(B, T), i32(B, U), i32(B, U), f32(B, U))
    ws, wp, wa = buf(n), buf(n), buf(na)
    rc = lib.ctc_amd_star_loss_grad(*head, WEIGHT, B, T, V, U, t[4].data_ptr(), loss.data_ptr(), grad.data_ptr(), 0, T * V, V,
                                    ws.data_ptr(), n, st)
    assert rc == 0, lib.ctc_amd_last_error()
    rc = lib.ctc_amd_star_label_posterior(*head, WEIGHT, B, T, V, U, ploss.data_ptr(), *(p.data_ptr() for p in post), wp.data_ptr(), n, st)
    assert rc == 0, lib.ctc_amd_last_error()
    rc = lib.ctc_amd_star_best_path(*head, B, T, V, U, *(p.data_ptr() for p in path), wa.data_ptr(), na, st)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in (loss, grad, ploss) + post + path)


@pytest.mark.parametrize("shape", [(4, 12, 5, 4), (4, 169, 8, 129)], ids=("nl1", "nl4"))
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_prefilled_outputs_and_a_second_run(kind, wrt, shape):
    """Every element of every output has a writer and nothing is read that was not written: 0x00 and 0xFF in the outputs and the
    workspaces, and a second run, give the same bits -- with utterances shorter than T, an infeasible one, one without an excluding
    star and weights of zero (on an excluding and on a plain utterance)."""
    B, T, V, U = shape
    rng = np.random.default_rng(T)
    labels = (1 + (np.arange(U)[None, :] + np.arange(B)[:, None]) % (V - 1)).astype(np.int32)
    labels[:, 0::3] = W
    labels[0, 1] = Q                                        # an optional star as well
    labels[3] = 1 + (np.arange(U) + 3) % (V - 1)            # no star at all
    ll, tl = np.full(B, U, np.int32), np.asarray([T - 2, T, 2, T - 3], np.int32)  # (two frames: infeasible)
    x = logits(rng, B, T, V, wrt)
    d_loss = np.asarray([1.5, 0.0, 1.0, 0.0], np.float32)
    a = raw_calls(kind, wrt, x, labels, ll, tl, 0x00, d_loss)
    for fill in (0xFF, 0xFF):
        b = raw_calls(kind, wrt, x, labels, ll, tl, fill, d_loss)
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    loss, grad = a[0].numpy(), a[1]
    assert np.isfinite(loss[[0, 1, 3]]).all() and np.isposinf(loss[2]) and torch.equal(a[2], a[0])
    assert not grad[[1, 2, 3]].view(torch.int32).any() and not grad[0, tl[0]:].view(torch.int32).any() and grad[0].abs().max() > 0
    rl, rg = SO.loss_and_grad(kind, wrt, labels, x, ll, tl, 0, WEIGHT, d_loss)
    assert np.abs(grad.numpy() - rg).max() <= 1e-4


@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_no_excluding_star_has_the_bits_of_false_at_four_positions_per_lane(kind, wrt):
    """The same contract as in test_contracts where a lane holds four positions, on bfloat16 logits: stars only in front of stars or
    at the end."""
    B, T, V, U = 2, 169, 8, 129
    rng = np.random.default_rng(6)
    labels = (1 + (np.arange(U)[None, :] + np.asarray([[0], [2]])) % (V - 1)).astype(np.int32)
    labels[0, [127, 128]] = W
    labels[1, [63, 64]] = [Q, W]
    ll, tl = np.asarray([U, 65], np.int32), np.asarray([T, T - 5], np.int32)
    x = dev(logits(rng, B, T, V, wrt)).to(torch.bfloat16)
    on, off = run(kind, wrt, x, labels, ll, tl, exclude=True), run(kind, wrt, x, labels, ll, tl, exclude=False)
    assert torch.isfinite(on[0]).all() and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert all(torch.equal(p, q) for p, q in zip(on[2], off[2]))
    assert all(torch.equal(p, q) for p, q in zip(align(kind, wrt, x, labels, ll, tl, exclude_next_label=True), align(kind, wrt, x, labels, ll, tl)))


def test_autograd_carries_the_keyword():
    rng = np.random.default_rng(1)
    labels, tl = (np.asarray(a, dtype=np.int32) for a in SMALL[4])
    ll = np.full(4, 4, np.int32)
    x = dev(logits(rng, 4, 12, 5, 0)).requires_grad_(True)
    loss = ctc.classic_ctc_wildcard_loss(dev(labels), x, dev(ll), dev(tl), 0, wildcard_log_weight=WEIGHT, optional_wildcards=True,
                                         exclude_next_label=True)
    (g,) = torch.autograd.grad(loss.sum(), x, create_graph=True)
    rl, rg = SO.loss_and_grad("classic", 0, labels, x.detach().cpu().numpy(), ll, tl, 0, WEIGHT)
    assert np.abs(g.detach().cpu().numpy() - rg).max() <= 1e-4
    with pytest.raises(RuntimeError):  # a second derivative keeps raising
        torch.autograd.grad(g.sum(), x)
