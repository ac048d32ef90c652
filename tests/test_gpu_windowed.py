"""Frame windows per label on the GPU: the windowed loss, gradient, label posteriors and (long-form) alignment against
tests/tools/window_oracle.py (float64, checked in tests/test_window_oracle.py), and the properties include/ctc_amd.h promises.

Inputs are feasible by construction: a random valid state path is drawn per utterance on the host (every label at least one
frame, a blank between equal neighbours on the classic lattice) and each position's segment -/+ a slack of 0..3 frames is its
window.  Infeasibility is tested separately and deliberately.  Bars: those of tests/test_gpu_wildcard_loss.py, 1e-4 + 1e-6 |loss|
on the loss (and on a path's score), 1e-4 per gradient or posterior element."""
import ctypes

import numpy as np
import pytest
import torch

from tests.tools import window_oracle as WO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = WO.WILDCARD
KINDS = WO.KINDS
SHAPES = [(4, 12, 5, 3), (2, 88, 8, 64), (2, 169, 8, 129), (2, 649, 8, 513)]  # (B, T, V, U): NL = 1, 1, 4 and 16 ... and 2 below
LONG = (1400, 8, 1030)  # T, V, U: two label blocks


def tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def draw(kind, B, T, V, U, seed, scale=1.0, wild=True, full_first=True):
    """(x, labels, ll, tl, window, segments): a random path per utterance and the windows around its segments."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    if wild:
        labels[rng.random((B, U)) < 0.15] = W
    ll = rng.integers((U + 1) // 2, U + 1, B).astype(np.int32)
    tl = np.zeros(B, np.int32)
    window = np.zeros((B, U, 2), np.int32)
    window[..., 1] = -1  # (beyond label_length: empty, and ignored)
    segs = []
    for b in range(B):
        if b == 0 and full_first:
            ll[b] = U
        L = int(ll[b])
        lab = labels[b, :L]
        gap_min = np.zeros(L + 1, np.int64)
        if kind == "classic":
            for i in range(1, L):
                gap_min[i] = int(lab[i] == lab[i - 1] and lab[i] != W)
        need = L + int(gap_min.sum())
        assert need <= T, (need, T)
        Tb = T if (b == 0 and full_first) else int(rng.integers(need, T + 1))
        tl[b] = Tb
        # slots: gap_0, pos_0, gap_1, ..., pos_{L-1}, gap_L; the frames beyond the minimum go to the slots that can take them
        can = np.ones(2 * L + 1, bool)
        if kind == "simplified":
            for i in range(L):
                can[2 * i + 1] = lab[i] == W            # an ordinary label is one frame
                can[2 * i + 2] = lab[i] != W            # a stay behind a wildcard is the wildcard's, not a blank
        size = np.zeros(2 * L + 1, np.int64)
        size[0::2] = gap_min
        size[1::2] = 1
        where = np.nonzero(can)[0]
        if Tb > need:
            size[where] += rng.multinomial(Tb - need, np.full(len(where), 1.0 / len(where)))
        ends = np.cumsum(size)
        seg = np.stack([ends[1::2] - size[1::2], ends[1::2] - 1], axis=1)  # [L, 2]: first and last frame of every position
        segs.append(seg)
        window[b, :L, 0] = seg[:, 0] - rng.integers(0, 4, L)
        window[b, :L, 1] = seg[:, 1] + rng.integers(0, 4, L)
    return x, labels, ll, tl, window, segs


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lattice_fns(kind, wrt):
    import tf_seq2seq_losses_amd as ctc
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    if wrt:
        return tuple((lambda *a, _f=f, **k: _f(*a[:4], a[4], cls, **k)) for f in (
            ctc.ctc_wildcard_loss_from_logproba, ctc.ctc_label_posterior_from_logproba, ctc.ctc_wildcard_alignment_from_logproba,
            ctc.ctc_long_wildcard_alignment_from_logproba))
    c = kind == "classic"
    return (ctc.classic_ctc_wildcard_loss if c else ctc.simplified_ctc_wildcard_loss,
            ctc.classic_ctc_label_posterior if c else ctc.simplified_ctc_label_posterior,
            ctc.classic_ctc_wildcard_alignment if c else ctc.simplified_ctc_wildcard_alignment,
            ctc.classic_ctc_long_wildcard_alignment if c else ctc.simplified_ctc_long_wildcard_alignment)


def run_all(kind, wrt, x, labels, ll, tl, window, weight=-0.25, long_form=False, d_loss=None, blank=0, **kw):
    """Every windowed call of the short form (or the long-form alignment alone) as numpy: dict of outputs.  d_loss: the
    grad_outputs of the loss (default: ones); kw (max_label_length, and frames_per_tile for the long form) goes to every call."""
    loss_fn, post_fn, align_fn, long_fn = lattice_fns(kind, wrt)
    wk = {} if window is None else {"frame_window": window if isinstance(window, torch.Tensor) else dev(window)}
    lab, l1, l2 = dev(labels), dev(ll), dev(tl)
    out = {}
    if long_form:
        a = long_fn(lab, dev(x), l1, l2, blank, **wk, **kw)
        out.update({"a_" + k: v for k, v in a._asdict().items()})
    else:
        xt = dev(x).clone().requires_grad_(True)
        loss = loss_fn(lab, xt, l1, l2, blank, wildcard_log_weight=weight, **wk, **kw)
        dl = torch.ones_like(loss) if d_loss is None else dev(d_loss)
        (grad,) = torch.autograd.grad(loss, xt, dl)
        out.update(loss=loss.detach(), grad=grad)
        p = post_fn(lab, dev(x), l1, l2, blank, wildcard_log_weight=weight, **wk, **kw)
        out.update({"p_" + k: v for k, v in p._asdict().items()})
        a = align_fn(lab, dev(x), l1, l2, blank, **wk, **kw)
        out.update({"a_" + k: v for k, v in a._asdict().items()})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        u, v = a[k].contiguous().reshape(-1), b[k].contiguous().reshape(-1)
        assert u.dtype == v.dtype and u.shape == v.shape, k
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), k


def check_owners(index, window, ll, tl):
    """label_index[t] == i only inside the window of i."""
    for b in range(index.shape[0]):
        for t in range(int(tl[b])):
            i = int(index[b, t])
            if i >= 0:
                assert i < ll[b] and window[b, i, 0] <= t <= window[b, i, 1], (b, t, i, window[b, i])


def check_path(kind, wrt, x64, labels, ll, tl, window, got, what, blank=0):
    """The alignment against the oracle: an admissible path inside the windows whose float64 value is the oracle's optimum, and the
    score.  (The path itself is not compared: a wildcard frame whose best token is the blank ties with a blank frame.)"""
    o_score, o_paths, _ = WO.best_path(kind, labels, x64, ll, tl, window, blank, wrt)
    score, tokens, index = got["a_score"].numpy(), got["a_tokens"].numpy(), got["a_label_index"].numpy()
    check_owners(index, window, ll, tl)
    for b in range(len(ll)):
        assert o_paths[b] is not None, (what, b)  # feasible by construction
        Tb, L = int(tl[b]), int(ll[b])
        lp = WO._rows(x64[b, :Tb], wrt)[0]
        idx = index[b, :Tb]
        owned = idx[idx >= 0]
        assert np.array_equal(np.unique(owned), np.arange(L)) and np.all(np.diff(owned) >= 0), (what, b)
        arg = np.asarray(x64[b, :Tb], np.float32).argmax(axis=-1)
        want_tok = np.where(idx < 0, blank, np.where(labels[b][np.maximum(idx, 0)] == W, arg, labels[b][np.maximum(idx, 0)]))
        assert np.array_equal(tokens[b, :Tb], want_tok), (what, b)
        value = float(lp[np.arange(Tb), tokens[b, :Tb]].sum())
        print(f"{what} b={b}: score {score[b]:.6f} oracle {o_score[b]:.6f} path value {value:.6f}")
        assert abs(value - o_score[b]) <= tol(o_score[b]), (what, b, value, o_score[b])
        assert abs(float(score[b]) - o_score[b]) <= tol(o_score[b]), (what, b, score[b], o_score[b])
        first, last = got["a_first_frame"].numpy()[b], got["a_last_frame"].numpy()[b]
        for i in range(L):
            fr = np.nonzero(idx == i)[0]
            assert first[i] == fr[0] and last[i] == fr[-1] and np.all(np.diff(fr) == 1), (what, b, i)


def check_sums(kind, wrt, x64, labels, ll, tl, window, got, free, weight, what, grad_tol=1e-4, blank=0):
    """Loss, gradient and posteriors against the oracle; zero outside the windows; rows sum to 1; at least the unwindowed loss.
    Returns the oracle's results."""
    o_loss, o_grad = WO.loss_and_grad(kind, wrt, labels, x64, ll, tl, window, blank, weight)
    _, o_post, o_blk, o_dur, o_exf = WO.label_posterior(kind, wrt, labels, x64, ll, tl, window, blank, weight)
    loss = got["loss"].numpy().astype(np.float64)
    assert np.isfinite(o_loss).all() and np.isfinite(loss).all(), what
    e_loss = np.abs(loss - o_loss)
    e_grad = np.abs(got["grad"].float().numpy() - o_grad)
    e_post = np.abs(got["p_label_posterior"].numpy() - o_post)
    e_blk = np.abs(got["p_blank_posterior"].numpy() - o_blk)
    print(f"{what}: loss err {e_loss.max():.3g} grad err {e_grad.max():.3g} posterior err {e_post.max():.3g} blank err {e_blk.max():.3g}")
    assert np.all(e_loss <= tol(o_loss)), (what, loss, o_loss)
    assert e_grad.max() <= grad_tol and e_post.max() <= 1e-4 and e_blk.max() <= 1e-4, what
    assert np.all(np.abs(got["p_duration"].numpy() - o_dur) <= 1e-4 * np.maximum(1.0, o_dur)), what
    same_bits(got, got | {"p_loss": got["loss"]}, ["p_loss"])  # the posterior call's loss is the loss call's
    post = got["p_label_posterior"].numpy()
    B, T, U = post.shape
    t = np.arange(T)[None, :, None]
    outside = (t < window[:, None, :, 0]) | (t > window[:, None, :, 1])
    assert np.all(post[outside] == 0.0), what  # exactly
    total = post.sum(axis=2) + got["p_blank_posterior"].numpy()
    for b in range(B):
        assert np.all(np.abs(total[b, :tl[b]] - 1.0) <= 1e-4), (what, b)
    assert np.all(loss >= free["loss"].numpy() - tol(loss)), what  # fewer paths: no less loss
    return dict(loss=o_loss, grad=o_grad, post=o_post, blk=o_blk, dur=o_dur, exf=o_exf)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(kind, shape):
    """Logits and log-probabilities on every shape; N(0, 4^2) logits on the second."""
    B, T, V, U = shape
    for wrt, scale in ((0, 1.0), (1, 1.0)) + (((0, 4.0),) if U == 64 else ()):
        x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=1000 * U + 10 * wrt + int(scale), scale=scale)
        if wrt:
            x = torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()
        what = f"{kind} {shape} wrt={wrt} scale={scale}"
        got = run_all(kind, wrt, x, labels, ll, tl, window)
        free = run_all(kind, wrt, x, labels, ll, tl, None)
        x64 = x.astype(np.float64)
        check_sums(kind, wrt, x64, labels, ll, tl, window, got, free, -0.25, what)
        check_path(kind, wrt, x64, labels, ll, tl, window, got, what)
        assert np.all(got["a_score"].numpy() <= free["a_score"].numpy())


def test_two_labels_per_lane():
    """U = 100: NL = 2, the one lane width the issue's shapes leave out."""
    for kind in KINDS:
        x, labels, ll, tl, window, _ = draw(kind, 2, 140, 8, 100, seed=77)
        got = run_all(kind, 0, x, labels, ll, tl, window)
        free = run_all(kind, 0, x, labels, ll, tl, None)
        check_sums(kind, 0, x.astype(np.float64), labels, ll, tl, window, got, free, -0.25, f"{kind} U=100")
        check_path(kind, 0, x.astype(np.float64), labels, ll, tl, window, got, f"{kind} U=100")


@pytest.mark.parametrize("kind", KINDS)
def test_covering_windows_and_none_are_the_unwindowed_bits(kind):
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops
    for B, T, V, U in (SHAPES[0], SHAPES[2]):
        x, labels, ll, tl, _, _ = draw(kind, B, T, V, U, seed=5 + U)
        tl[-1] = max(1, int(ll[-1]) // 2)  # one utterance with too few frames: the degenerate outputs too
        cover = WO.full_window(B, U, T).astype(np.int32)
        free = run_all(kind, 0, x, labels, ll, tl, None)
        same_bits(free, run_all(kind, 0, x, labels, ll, tl, cover))
        wide = cover.copy()
        wide[..., 0], wide[..., 1] = -5, T + 5  # beyond the frames: clipped
        same_bits(free, run_all(kind, 0, x, labels, ll, tl, wide))
        # frame_window=None is the existing C entry: the ops layer called without the argument
        prep = ops.Prepared(dev(labels), dev(x), dev(ll), dev(tl), 0, keep_format=True, host_max_label_length=U)
        raw = ops.wildcard_best_path(ops.KINDS[kind], 0, prep)
        torch.cuda.synchronize()
        for k, v in zip(ctc.CtcWildcardAlignment._fields, raw):
            same_bits({k: v.cpu()}, {k: free["a_" + k]})
    T, V, U = LONG
    x, labels, ll, tl, _, _ = draw(kind, 1, T, V, U, seed=9)
    free = run_all(kind, 0, x, labels, ll, tl, None, long_form=True)
    same_bits(free, run_all(kind, 0, x, labels, ll, tl, WO.full_window(1, U, T).astype(np.int32), long_form=True))


@pytest.mark.parametrize("kind", KINDS)
def test_windows_from_the_free_alignment_return_it(kind):
    """ctc_frame_window of the unconstrained alignment, slack 0, returns that alignment bit for bit, short and long form.  The
    logits are random float32, so two paths through ordinary labels do not tie; where a wildcard frame's best token is the blank it
    does tie with a blank frame, but the windowed lattice is a sub-lattice that still holds the chosen path, every state on it keeps
    its value and the tie rule its order, so the choice is the same."""
    import tf_seq2seq_losses_amd as ctc
    for long_form, (B, T, V, U) in ((False, SHAPES[1]), (False, SHAPES[2]), (True, (1,) + LONG)):
        x, labels, ll, tl, _, _ = draw(kind, B, T, V, U, seed=31 + U)
        free = run_all(kind, 0, x, labels, ll, tl, None, long_form=long_form)
        win = ctc.ctc_frame_window(free["a_first_frame"].to(DEV), free["a_last_frame"].to(DEV), dev(tl))
        assert win.dtype == torch.int32 and tuple(win.shape) == (B, U, 2) and win.is_cuda
        again = run_all(kind, 0, x, labels, ll, tl, win, long_form=long_form)
        same_bits(free, again, [k for k in free if k.startswith("a_")])
        slack = ctc.ctc_frame_window(free["a_first_frame"].to(DEV), free["a_last_frame"].to(DEV), dev(tl), before=2, after=3).cpu().numpy()
        f, l = free["a_first_frame"].numpy(), free["a_last_frame"].numpy()
        top = np.maximum(tl[:, None] - 1, 0)
        assert np.array_equal(slack[..., 0], np.minimum(np.maximum(f - 2, 0), top))
        assert np.array_equal(slack[..., 1], np.minimum(np.maximum(l + 3, 0), top))


@pytest.mark.parametrize("kind", KINDS)
def test_a_window_that_excludes_the_free_path_changes_it(kind):
    B, T, V, U = 2, 60, 8, 6
    x, labels, ll, tl, _, _ = draw(kind, B, T, V, U, seed=3, wild=False)
    ll[:], tl[:] = U, T
    free = run_all(kind, 0, x, labels, ll, tl, None)
    window = WO.full_window(B, U, T).astype(np.int32)
    last0 = free["a_last_frame"].numpy()[:, 0]
    assert np.all(last0 + 1 + 2 * U <= T)  # room for every label behind the free path's first one
    window[:, 0, 0] = last0 + 1
    got = run_all(kind, 0, x, labels, ll, tl, window)
    assert np.all(got["a_first_frame"].numpy()[:, 0] > last0)
    assert not np.array_equal(got["a_label_index"].numpy(), free["a_label_index"].numpy())
    assert np.all(np.isfinite(got["a_score"].numpy())) and np.all(got["a_score"].numpy() <= free["a_score"].numpy())
    check_path(kind, 0, x.astype(np.float64), labels, ll, tl, window, got, f"{kind} excluded")


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_window_is_infeasible_and_alone(kind):
    B, T, V, U = 3, 40, 8, 70
    x, labels, ll, tl, window, _ = draw(kind, B, T + 60, V, U, seed=11)
    good = run_all(kind, 0, x, labels, ll, tl, window)
    bad = window.copy()
    i = int(ll[1]) // 2
    bad[1, i] = (window[1, i, 1] + 1, window[1, i, 1])  # first > last
    got = run_all(kind, 0, x, labels, ll, tl, bad)
    assert got["loss"][1] == float("inf") and got["a_score"][1] == float("-inf")
    assert not got["grad"][1].any() and not got["p_label_posterior"][1].any() and not got["p_blank_posterior"][1].any()
    assert torch.all(got["a_tokens"][1] == -1) and torch.all(got["a_label_index"][1] == -1)
    assert torch.all(got["a_first_frame"][1] == -1) and torch.all(got["a_label_score"][1] == float("-inf"))
    assert torch.all(got["p_expected_frame"][1] == -1) and not got["p_duration"][1].any()
    for b in (0, 2):
        same_bits({k: v[b] for k, v in good.items()}, {k: v[b] for k, v in got.items()})
    T2, V2, U2 = LONG
    x, labels, ll, tl, window, _ = draw(kind, 2, T2, V2, U2, seed=12)
    good = run_all(kind, 0, x, labels, ll, tl, window, long_form=True)
    window[0, 1024] = (5, 4)
    got = run_all(kind, 0, x, labels, ll, tl, window, long_form=True)
    assert got["a_score"][0] == float("-inf") and torch.all(got["a_label_index"][0] == -1)
    same_bits({k: v[1] for k, v in good.items()}, {k: v[1] for k, v in got.items()})


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    """int64 windows and time-major strided logits: the bits of int32 windows on contiguous logits.  bfloat16 logits: the oracle on
    the values the kernel reads; the gradient comes back in bfloat16, half a unit in its 8th bit on top of the bar."""
    B, T, V, U = SHAPES[2]
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=21)
    base = run_all(kind, 0, x, labels, ll, tl, window)
    same_bits(base, run_all(kind, 0, x, labels, ll, tl, dev(window.astype(np.int64))))
    big = torch.zeros((T, B, V + 8), device=DEV)
    big[:, :, :V] = dev(x).transpose(0, 1)
    strided = run_all(kind, 0, big[:, :, :V].transpose(0, 1), labels, ll, tl, window)
    same_bits(base, strided)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    got = run_all(kind, 0, xb.to(DEV), labels, ll, tl, window)
    assert got["grad"].dtype == torch.bfloat16
    free = run_all(kind, 0, xb.to(DEV), labels, ll, tl, None)
    x64 = xb.double().numpy()
    check_sums(kind, 0, x64, labels, ll, tl, window, got, free, -0.25, f"{kind} bfloat16", grad_tol=1e-4 + 2.0 ** -9)
    check_path(kind, 0, x64, labels, ll, tl, window, got, f"{kind} bfloat16")


def _raw_calls(kind, x, labels, ll, tl, window, fill, long_form, blank=0, U=None, window_stride=None, d_loss=None):
    """The C entry points themselves on outputs and a workspace prefilled with the byte `fill`.  U: the bound the calls, their
    outputs and their workspaces get (default: the width of `labels`, which is always the label stride); window_stride: that of
    `window`, any int32 array that holds what it implies (default: 2 * the width of a [B, width, 2] one); d_loss: float32 [B] for
    the gradient (default: NULL)."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = x.shape
    label_stride = labels.shape[1]
    U = label_stride if U is None else U
    window_stride = 2 * window.shape[1] if window_stride is None else window_stride
    k = KINDS.index(kind)
    t = {n: dev(a) for n, a in dict(x=x, labels=labels, ll=ll, tl=tl, win=window).items()}
    dl = None if d_loss is None else dev(np.asarray(d_loss, np.float32))
    lead = (k, 0, t["x"].data_ptr(), 0, T * V, V, t["labels"].data_ptr(), label_stride, t["ll"].data_ptr(), t["tl"].data_ptr(), blank,
            t["win"].data_ptr(), window_stride)

    def buf(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=DEV)[:n].view(dtype).reshape(shape)

    def ws(n):
        return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=DEV)

    out = {}
    al = dict(score=buf((B,), torch.float32), tokens=buf((B, T), torch.int32), label_index=buf((B, T), torch.int32),
              first_frame=buf((B, U), torch.int32), last_frame=buf((B, U), torch.int32), label_score=buf((B, U), torch.float32))
    if long_form:
        w = ws(_lib.long_wildcard_best_path_workspace_bytes(k, B, T, V, U, 64))
        rc = lib.ctc_amd_long_windowed_best_path(*lead, B, T, V, U, 64, *(v.data_ptr() for v in al.values()), w.data_ptr(), w.numel(), None)
        assert rc == 0, lib.ctc_amd_last_error()
    else:
        w = ws(_lib.wildcard_best_path_workspace_bytes(k, B, T, V, U))
        rc = lib.ctc_amd_windowed_best_path(*lead, B, T, V, U, *(v.data_ptr() for v in al.values()), w.data_ptr(), w.numel(), None)
        assert rc == 0, lib.ctc_amd_last_error()
        lg = dict(loss=buf((B,), torch.float32), grad=buf((B, T, V), torch.float32))
        w = ws(_lib.wildcard_loss_workspace_bytes(k, B, T, V, U, True))
        rc = lib.ctc_amd_windowed_loss_grad(*lead, ctypes.c_float(-0.25), B, T, V, U, None if dl is None else dl.data_ptr(),
                                            lg["loss"].data_ptr(), lg["grad"].data_ptr(),
                                            0, T * V, V, w.data_ptr(), w.numel(), None)
        assert rc == 0, lib.ctc_amd_last_error()
        po = dict(ploss=buf((B,), torch.float32), post=buf((B, T, U), torch.float32), blk=buf((B, T), torch.float32),
                  dur=buf((B, U), torch.float32), exf=buf((B, U), torch.float32))
        w = ws(_lib.label_posterior_workspace_bytes(k, B, T, V, U))
        rc = lib.ctc_amd_windowed_label_posterior(*lead, ctypes.c_float(-0.25), B, T, V, U, *(v.data_ptr() for v in po.values()),
                                                  w.data_ptr(), w.numel(), None)
        assert rc == 0, lib.ctc_amd_last_error()
        out.update(lg)
        out.update(po)
    out.update(al)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_prefilled_outputs_do_not_show(kind):
    """Every element of every output has a writer: 0x00 and 0xFF in the outputs and the workspace give the same bits."""
    for long_form, (B, T, V, U) in ((False, SHAPES[2]), (True, (2,) + LONG)):
        x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=41, full_first=False)
        tl[-1] = max(1, int(ll[-1]) // 2)  # an infeasible utterance: its outputs are written too
        a = _raw_calls(kind, x, labels, ll, tl, window, 0x00, long_form)
        b = _raw_calls(kind, x, labels, ll, tl, window, 0xFF, long_form)
        same_bits(a, b)
        assert np.isinf(a["score"].numpy()).any() and np.isfinite(a["score"].numpy()).any()


def long_windows(kind, B, seed, TF=(64, 128)):
    """The long-form case: windows from a drawn path, with edges put on the last frame of a time block and the first of the next for
    both tile heights, and no slack at all on the two positions either side of the label-block boundary."""
    T, V, U = LONG
    x, labels, ll, tl, window, segs = draw(kind, B, T, V, U, seed=seed)
    for b in range(B):
        seg, L = segs[b], int(ll[b])
        for tf in TF:
            for edge in (tf, 2 * tf, 5 * tf):
                if edge >= tl[b]:
                    continue
                i = int(np.searchsorted(seg[:, 1], edge))  # the first position that ends at or behind `edge`
                if 0 < i < L:
                    if seg[i, 0] >= edge:
                        window[b, i, 0] = edge              # opens on the block's first frame
                    if seg[i - 1, 1] <= edge - 1:
                        window[b, i - 1, 1] = edge - 1      # closes on the last frame of the block before
        for i in (1023, 1024):
            if i < L:
                window[b, i] = seg[i]
    return x, labels, ll, tl, window


@pytest.mark.parametrize("kind", KINDS)
def test_long_form(kind):
    """U = 1030, T = 1400: against the oracle; the same bits for frames_per_tile 64 and 128 and for B = 1 against the same utterance
    inside B = 3 (score's last bits apart, as for the unwindowed call: its log-sum-exps are added per time block)."""
    x, labels, ll, tl, window = long_windows(kind, 3, seed=51)
    assert ll[0] == 1030 and tl[0] == 1400
    runs = {tf: run_all(kind, 0, x, labels, ll, tl, window, long_form=True, frames_per_tile=tf) for tf in (64, 128)}
    exact = [k for k in runs[64] if k != "a_score"]
    same_bits(runs[64], runs[128], exact)
    assert np.all(np.abs(runs[64]["a_score"].numpy() - runs[128]["a_score"].numpy()) <= tol(runs[64]["a_score"].numpy()))
    check_path(kind, 0, x.astype(np.float64), labels, ll, tl, window, runs[64], f"{kind} long")
    for b in (0, 2):
        alone = run_all(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], window[b:b + 1], long_form=True, frames_per_tile=128,
                        max_label_length=labels.shape[1])  # (the bound of the batch: the same U, the same outputs' width)
        same_bits({k: v[0] for k, v in alone.items()}, {k: v[b] for k, v in runs[128].items()})
    free = run_all(kind, 0, x, labels, ll, tl, None, long_form=True)
    assert np.all(runs[64]["a_score"].numpy() <= free["a_score"].numpy())


def test_graph_capture_replays():
    """The windowed calls neither synchronise nor allocate outside the graph's pool: one capture, one replay, the eager bits."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = SHAPES[2]
    x, labels, ll, tl, window, _ = draw("classic", B, T, V, U, seed=61)
    eager = run_all("classic", 0, x, labels, ll, tl, window)
    xs, lab, l1, l2, win = dev(x), dev(labels), dev(ll), dev(tl), dev(window)
    al = ctc.classic_ctc_wildcard_alignment(lab, xs, l1, l2, 0, max_label_length=U)
    first, last = al.first_frame.clone(), al.last_frame.clone()

    def work():
        xg = xs.clone().requires_grad_(True)
        loss = ctc.classic_ctc_wildcard_loss(lab, xg, l1, l2, 0, wildcard_log_weight=-0.25, max_label_length=U, frame_window=win)
        (g,) = torch.autograd.grad(loss.sum(), xg)
        p = ctc.classic_ctc_label_posterior(lab, xs, l1, l2, 0, wildcard_log_weight=-0.25, max_label_length=U, frame_window=win)
        a = ctc.classic_ctc_wildcard_alignment(lab, xs, l1, l2, 0, max_label_length=U, frame_window=win)
        w2 = ctc.ctc_frame_window(first, last, l2, before=1, after=1)
        return dict(loss=loss.detach(), grad=g, p_label_posterior=p.label_posterior, a_label_index=a.label_index, a_score=a.score, w2=w2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = work()
    graph.replay()
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    same_bits(eager, out, ["loss", "grad", "p_label_posterior", "a_label_index", "a_score"])
    assert tuple(out["w2"].shape) == (B, U, 2)
