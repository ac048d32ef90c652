"""Frame windows per label above 1024 labels on the GPU: the windowed long-form loss and gradient (both workspaces) and the
long-form label posteriors against tests/tools/window_oracle.py (float64, no limit on U), and the properties include/ctc_amd.h
promises for them.  Inputs, windows and bit comparison are those of tests/test_gpu_windowed.py (imported, not copied): a random
valid path per utterance and each position's segment -/+ 0..3 frames; long_windows puts edges on the last frame of a time block
and the first of the next for both tile heights and leaves positions 1023 and 1024 no slack.

Bars: those of tests/test_gpu_windowed.py, 1e-4 + 1e-6 |loss| on the loss, 1e-4 per gradient or posterior element, duration
within 1e-4 max(1, oracle).  Every oracle result is computed once per input and shared."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_gpu_windowed as TW
from tests.tools import window_oracle as WO

pytestmark = pytest.mark.gpu
DEV = TW.DEV
KINDS = WO.KINDS
LONG = TW.LONG
draw, dev, same_bits, tol, long_windows = TW.draw, TW.dev, TW.same_bits, TW.tol, TW.long_windows
WEIGHT = -0.25
POST_KEYS = ("p_loss", "p_blank_posterior", "p_duration", "p_expected_frame", "p_peak_posterior", "p_peak_frame")


def fns(kind, wrt):
    """(loss, label posterior, wildcard alignment, label posterior without the keyword) of the long form for a lattice and an input
    kind.  The posterior that takes `frame_window` is *_long_windowed_label_posterior: the unwindowed functions keep their
    signatures."""
    import tf_seq2seq_losses_amd as ctc
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    if wrt:
        return tuple((lambda *a, _f=f, **k: _f(*a[:4], a[4], cls, **k)) for f in (
            ctc.ctc_long_loss_from_logproba, ctc.ctc_long_windowed_label_posterior_from_logproba,
            ctc.ctc_long_wildcard_alignment_from_logproba, ctc.ctc_long_label_posterior_from_logproba))
    c = kind == "classic"
    return (ctc.classic_ctc_long_loss if c else ctc.simplified_ctc_long_loss,
            ctc.classic_ctc_long_windowed_label_posterior if c else ctc.simplified_ctc_long_windowed_label_posterior,
            ctc.classic_ctc_long_wildcard_alignment if c else ctc.simplified_ctc_long_wildcard_alignment,
            ctc.classic_ctc_long_label_posterior if c else ctc.simplified_ctc_long_label_posterior)


def short_fns(kind):
    import tf_seq2seq_losses_amd as ctc
    c = kind == "classic"
    return (ctc.classic_ctc_wildcard_loss if c else ctc.simplified_ctc_wildcard_loss,
            ctc.classic_ctc_label_posterior if c else ctc.simplified_ctc_label_posterior)


def run_long(kind, wrt, x, labels, ll, tl, window, weight=WEIGHT, checkpoint=False, dense=True, post=True, short=False, blank=0,
             d_loss=None, **kw):
    """The windowed long-form loss + gradient (one `checkpoint` setting) and, with `post`, the label posteriors, as a dict of CPU
    tensors.  window=None passes no frame_window at all.  short: the short-form calls on the same arguments instead.  d_loss: the
    grad_outputs of the loss (default: its sum, that is ones)."""
    loss_fn, post_fn = short_fns(kind) if short else fns(kind, wrt)[:2]
    if window is None and not short:
        post_fn = fns(kind, wrt)[3]  # no window: the function that has no such keyword
    wk = {} if window is None else {"frame_window": window if isinstance(window, torch.Tensor) else dev(window)}
    lab, l1, l2 = dev(labels), dev(ll), dev(tl)
    xt = dev(x).clone().requires_grad_(True)
    ck = {} if short else {"checkpoint": checkpoint}
    loss = loss_fn(lab, xt, l1, l2, blank, wildcard_log_weight=weight, **ck, **wk, **kw)
    (grad,) = torch.autograd.grad(loss.sum(), xt) if d_loss is None else torch.autograd.grad(loss, xt, dev(d_loss))
    out = dict(loss=loss.detach(), grad=grad)
    if post:
        dk = {} if short else {"dense": dense}
        p = post_fn(lab, dev(x), l1, l2, blank, wildcard_log_weight=weight, **dk, **wk, **kw)
        out.update({"p_" + k: v for k, v in p._asdict().items() if v is not None})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


_ORACLE = {}


def oracle(key, kind, wrt, x64, labels, ll, tl, window, weight=WEIGHT, blank=0, d_loss=None, post=True):
    """The float64 results for an input, computed once per `key` and not changed by anybody.  d_loss: the weights of the gradient
    (part of the key); post=False: the loss and the gradient alone."""
    k = (key, kind, wrt, weight) if (blank == 0 and d_loss is None and post) else \
        (key, kind, wrt, weight, blank, None if d_loss is None else tuple(np.asarray(d_loss, np.float64).tolist()), post)
    if k not in _ORACLE:
        loss, grad = WO.loss_and_grad(kind, wrt, labels, x64, ll, tl, window, blank, weight, d_loss)
        res = dict(loss=loss, grad=grad)
        if post:
            loss2, res["post"], res["blk"], res["dur"], res["exf"] = WO.label_posterior(kind, wrt, labels, x64, ll, tl, window, blank, weight)
            assert np.array_equal(loss, loss2)
        for a in res.values():
            a.setflags(write=False)
        _ORACLE[k] = res
    return _ORACLE[k]


def check(ref, got, window, tl, what, free_loss=None, grad_tol=1e-4):
    """What `got` holds of loss, gradient and posteriors against the oracle at the bars; posteriors exactly zero outside every
    window; every frame sums to 1; at least the unwindowed loss."""
    o_loss = ref["loss"]
    loss = got["loss"].numpy().astype(np.float64)
    assert np.isfinite(o_loss).all() and np.isfinite(loss).all(), (what, o_loss, loss)
    e_loss = np.abs(loss - o_loss)
    e_grad = np.abs(got["grad"].float().numpy() - ref["grad"]).max()
    print(f"{what}: oracle loss {o_loss}, loss err {e_loss.max():.3g} grad err {e_grad:.3g}")
    assert np.all(e_loss <= tol(o_loss)), (what, loss, o_loss)
    assert e_grad <= grad_tol, (what, e_grad)
    if free_loss is not None:
        assert np.all(loss >= free_loss.numpy() - tol(loss)), what  # fewer paths: no less loss
    if "p_loss" not in got:
        return
    same_bits(got, got | {"p_loss": got["loss"]}, ["p_loss"])  # the posterior call's loss is the loss call's
    e_blk = np.abs(got["p_blank_posterior"].numpy() - ref["blk"]).max()
    dur = got["p_duration"].numpy()
    e_dur = np.abs(dur - ref["dur"])
    print(f"{what}: blank err {e_blk:.3g} duration err {e_dur.max():.3g}")
    assert e_blk <= 1e-4, (what, e_blk)
    assert np.all(e_dur <= 1e-4 * np.maximum(1.0, ref["dur"])), what
    if "p_label_posterior" not in got:
        return
    post = got["p_label_posterior"].numpy()
    e_post = np.abs(post - ref["post"]).max()
    print(f"{what}: posterior err {e_post:.3g}")
    assert e_post <= 1e-4, (what, e_post)
    B, T, U = post.shape
    t = np.arange(T)[None, :, None]
    outside = (t < window[:, None, :, 0]) | (t > window[:, None, :, 1])
    assert np.all(post[outside] == 0.0), what  # exactly
    total = post.sum(axis=2, dtype=np.float64) + got["p_blank_posterior"].numpy()
    for b in range(B):
        assert np.all(np.abs(total[b, :tl[b]] - 1.0) <= 1e-4), (what, b)


def row(out, b):
    return {k: v[b] for k, v in out.items()}


_MAIN = {}


def main_input(kind):
    """The main input (T = 1400, V = 8, U = 1030, three utterances of which only the first reaches the second label block)."""
    if kind not in _MAIN:
        x, labels, ll, tl, window = long_windows(kind, 3, seed=51)
        assert ll[0] == 1030 and tl[0] == 1400 and np.all(ll[1:] <= 1024)
        _MAIN[kind] = (x, labels, ll, tl, window)
    return _MAIN[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_oracle(kind):
    x, labels, ll, tl, window = main_input(kind)
    ref = oracle("main", kind, 0, x.astype(np.float64), labels, ll, tl, window)
    free = run_long(kind, 0, x, labels, ll, tl, None, post=False)
    got = run_long(kind, 0, x, labels, ll, tl, window)
    check(ref, got, window, tl, f"{kind} main", free["loss"])
    ckpt = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=True, post=False)
    check(ref, ckpt, window, tl, f"{kind} main checkpoint=True", free["loss"])


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_oracle_on_log_probabilities(kind):
    """Utterance 0 of the main input (both label blocks) as log-probabilities used as they stand."""
    x, labels, ll, tl, window = (a[:1] for a in main_input(kind))
    x = torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()
    ref = oracle("main[0] logproba", kind, 1, x.astype(np.float64), labels, ll, tl, window)
    free = run_long(kind, 1, x, labels, ll, tl, None, post=False)
    for ck in (False, True):
        got = run_long(kind, 1, x, labels, ll, tl, window, checkpoint=ck, post=not ck)
        check(ref, got, window, tl, f"{kind} logproba checkpoint={ck}", free["loss"])


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_for_both_workspaces_every_tile_height_and_batch(kind):
    x, labels, ll, tl, window = main_input(kind)
    U = labels.shape[1]
    base = run_long(kind, 0, x, labels, ll, tl, window)
    assert np.isfinite(base["loss"].numpy()).all()
    same_bits(base, base | {"p_loss": base["loss"]}, ["p_loss"])
    for tf in (64, 128, 4):
        for ck in (False, True):
            got = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck, post=ck, frames_per_tile=tf)
            same_bits(base, got, got.keys())
    for b in (0, 2):
        for ck in (False, True):
            alone = run_long(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], window[b:b + 1], checkpoint=ck, post=ck,
                             max_label_length=U)  # (the bound of the batch: the same U, the same outputs' width)
            same_bits(row(alone, 0), row(base, b), alone.keys())


@pytest.mark.parametrize("kind", KINDS)
def test_covering_windows_and_none_are_the_unwindowed_bits(kind):
    from tf_seq2seq_losses_amd import ops
    T, V, U = LONG
    x, labels, ll, tl, _, _ = draw(kind, 3, T, V, U, seed=5)
    tl[-1] = max(1, int(ll[-1]) // 2)  # one utterance with too few frames: the degenerate outputs too
    cover = WO.full_window(3, U, T).astype(np.int32)
    wide = cover.copy()
    wide[..., 0], wide[..., 1] = -5, T + 5  # beyond the frames: clipped
    k = KINDS.index(kind)
    lab, xs, l1, l2 = dev(labels), dev(x), dev(ll), dev(tl)
    for ck in (False, True):
        free = run_long(kind, 0, x, labels, ll, tl, None, checkpoint=ck)
        assert np.isinf(free["loss"].numpy()[-1]) and np.isfinite(free["loss"].numpy()[:-1]).all()
        same_bits(free, run_long(kind, 0, x, labels, ll, tl, cover, checkpoint=ck))
        same_bits(free, run_long(kind, 0, x, labels, ll, tl, wide, checkpoint=ck))
        # frame_window=None is the existing C entry: the ops layer called without the argument
        loss, grad = ops.long_wildcard_loss_grad(k, 0, lab, xs, l1, l2, 0, None, U, None, WEIGHT, True, 0, ck)
        post = ops.long_label_posterior(k, 0, lab, xs, l1, l2, 0, U, WEIGHT)
        torch.cuda.synchronize()
        raw = dict(loss=loss, grad=grad, **{"p_" + n: v for n, v in zip(free_fields(), post)})
        same_bits(free, {n: v.cpu() for n, v in raw.items()})
        # ... and so is the windowed posterior function called with frame_window=None, spelled out or left to its default
        for kw in ({}, {"frame_window": None}):
            p = fns(kind, 0)[1](lab, xs, l1, l2, 0, wildcard_log_weight=WEIGHT, **kw)
            torch.cuda.synchronize()
            same_bits(free, {"p_" + n: v.cpu() for n, v in p._asdict().items()}, ["p_" + n for n in free_fields()])


def free_fields():
    import tf_seq2seq_losses_amd as ctc
    return ctc.CtcLongLabelPosterior._fields


@pytest.mark.parametrize("kind", KINDS)
def test_three_label_blocks_and_a_wrapping_ring(kind):
    """U = 2100, T = 2600, frames_per_tile = 64: K = 3 label blocks, J = 41 time blocks, a ring of min(K, J) = 3 blocks that wraps."""
    B, T, V, U = 2, 2600, 8, 2100
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=71)
    ref = oracle("three blocks", kind, 0, x.astype(np.float64), labels, ll, tl, window)
    assert np.isfinite(ref["loss"]).all(), ref["loss"]
    thin = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=True, dense=False, frames_per_tile=64)
    assert "p_label_posterior" not in thin  # label_posterior is None
    check(ref, thin, window, tl, f"{kind} K=3 dense=False")
    full = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=True, dense=True, frames_per_tile=64)
    same_bits(full, thin, thin.keys())  # duration, expected_frame, peak_posterior, peak_frame and the rest: bit for bit
    assert set(POST_KEYS) <= set(thin.keys())
    check(ref, full, window, tl, f"{kind} K=3 dense=True")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 169, 8, 129), (2, 1300, 8, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_one_block_against_the_oracle_and_the_short_form(kind, shape):
    B, T, V, U = shape
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=13 + U)
    ref = oracle(f"one block {shape}", kind, 0, x.astype(np.float64), labels, ll, tl, window)
    short = run_long(kind, 0, x, labels, ll, tl, window, short=True)
    keys = ("loss", "grad", "p_loss", "p_label_posterior", "p_blank_posterior", "p_duration", "p_expected_frame")
    for ck in (False, True):
        got = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck)
        check(ref, got, window, tl, f"{kind} {shape} checkpoint={ck}")
        equal = {n: torch.equal(got[n].view(torch.uint8), short[n].view(torch.uint8)) for n in keys}
        print(f"LONG-WINDOWED {kind} {shape} checkpoint={ck}: bits equal to the short form: {equal}")
        s = short["loss"].numpy().astype(np.float64)
        assert np.all(np.abs(got["loss"].numpy() - s) <= tol(s))
        for n in ("grad", "p_label_posterior", "p_blank_posterior"):
            assert (got[n] - short[n]).abs().max() <= 1e-4, n
        d = short["p_duration"].numpy().astype(np.float64)
        assert np.all(np.abs(got["p_duration"].numpy() - d) <= 1e-4 * np.maximum(1.0, d))


def assert_infeasible(out, b):
    assert out["loss"][b] == float("inf") and out["p_loss"][b] == float("inf")
    assert not out["grad"][b].any() and not out["p_label_posterior"][b].any() and not out["p_blank_posterior"][b].any()
    assert not out["p_duration"][b].any() and torch.all(out["p_expected_frame"][b] == -1)
    assert not out["p_peak_posterior"][b].any() and torch.all(out["p_peak_frame"][b] == -1)


@pytest.mark.parametrize("kind", KINDS)
def test_infeasible_windows_are_infeasible_and_alone(kind):
    x, labels, ll, tl, window = main_input(kind)
    for ck in (False, True):
        good = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck)
        empty = window.copy()
        empty[0, 1024] = (5, 4)  # first > last, in the second label block
        # each non-empty, but no monotonic path: position 100 may only own frames far behind those of position 900
        swapped = window.copy()
        swapped[0, 100], swapped[0, 900] = window[0, 900], window[0, 100]
        assert np.all(swapped[0, [100, 900], 0] <= swapped[0, [100, 900], 1]) and swapped[0, 900, 1] < swapped[0, 100, 0]
        for bad in (empty, swapped):
            got = run_long(kind, 0, x, labels, ll, tl, bad, checkpoint=ck)
            assert_infeasible(got, 0)
            for b in (1, 2):
                same_bits(row(good, b), row(got, b))


@pytest.mark.parametrize("kind", KINDS)
def test_the_pipeline_align_window_train(kind):
    """Align unconstrained, widen by a tolerance, train inside it.  With wildcard_log_weight = 0 the best path lies inside the
    windows and a wildcard frame's summed emission is at least its maximised one, so free loss <= windowed loss <= -score."""
    import tf_seq2seq_losses_amd as ctc
    T, V, U = LONG
    x, labels, ll, tl, _, _ = draw(kind, 2, T, V, U, seed=91)
    loss_fn, post_fn, align_fn, _ = fns(kind, 0)
    lab, xs, l1, l2 = dev(labels), dev(x), dev(ll), dev(tl)
    al = align_fn(lab, xs, l1, l2, 0, max_label_length=U)
    win = ctc.ctc_frame_window(al.first_frame, al.last_frame, l2, before=2, after=3)
    assert win.dtype == torch.int32 and tuple(win.shape) == (2, U, 2)
    for ck in (False, True):
        got = run_long(kind, 0, x, labels, ll, tl, win, weight=0.0, checkpoint=ck, max_label_length=U)
        free = run_long(kind, 0, x, labels, ll, tl, None, weight=0.0, checkpoint=ck, post=False, max_label_length=U)
        loss, lo, hi = (v.numpy().astype(np.float64) for v in (got["loss"], free["loss"], -al.score.cpu()))
        print(f"PIPELINE {kind} checkpoint={ck}: free loss {lo}, windowed loss {loss}, -score {hi}")
        assert np.isfinite(hi).all()
        assert np.all(lo - tol(lo) <= loss) and np.all(loss <= hi + tol(hi))
        assert got["grad"].abs().max() > 0
    # label_index of the alignment owns only frames whose posterior column is non-zero
    index = al.label_index.cpu().numpy()
    post = got["p_label_posterior"].numpy()
    for b in range(2):
        t = np.nonzero(index[b] >= 0)[0]
        assert len(t) >= ll[b] and np.all(post[b, t, index[b, t]] > 0.0), b


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    """int64 windows and time-major strided logits: the bits of int32 windows on contiguous logits.  bfloat16 logits: the oracle on
    the values the kernel reads; the gradient comes back in bfloat16, half a unit in its 8th bit on top of the bar."""
    # U = 1026: two positions in the second label block.  T = 1100 on the simplified lattice; the classic one needs a blank between
    # equal neighbours, about 1130 frames for 1026 random labels over 7 tokens, so it gets 1200
    B, T, V, U = 2, (1200 if kind == "classic" else 1100), 8, 1026
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=21)
    big = torch.zeros((T, B, V + 8), device=DEV)
    big[:, :, :V] = dev(x).transpose(0, 1)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    ref = oracle("formats bfloat16", kind, 0, xb.double().numpy(), labels, ll, tl, window)
    for ck in (False, True):
        base = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck)
        same_bits(base, run_long(kind, 0, x, labels, ll, tl, dev(window.astype(np.int64)), checkpoint=ck))
        same_bits(base, run_long(kind, 0, big[:, :, :V].transpose(0, 1), labels, ll, tl, window, checkpoint=ck))
        got = run_long(kind, 0, xb.to(DEV), labels, ll, tl, window, checkpoint=ck)
        assert got["grad"].dtype == torch.bfloat16
        free = run_long(kind, 0, xb.to(DEV), labels, ll, tl, None, checkpoint=ck, post=False)
        check(ref, got, window, tl, f"{kind} bfloat16 checkpoint={ck}", free["loss"], grad_tol=1e-4 + 2.0 ** -9)


def _raw_calls(kind, x, labels, ll, tl, window, fill, tf=64, blank=0, U=None, window_stride=None, d_loss=None):
    """The three C entry points themselves on outputs and an exact-size workspace prefilled with the byte `fill`.  U, window_stride
    and d_loss as in tests/test_gpu_windowed.py's _raw_calls: the width of `labels` is always the label stride."""
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
            t["win"].data_ptr(), window_stride, ctypes.c_float(WEIGHT), B, T, V, U, tf)

    def buf(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=DEV)[:n].view(dtype).reshape(shape)

    def ws(n):
        assert n > 0
        return torch.full((n,), fill, dtype=torch.uint8, device=DEV)

    out = {}
    for name, call, size in (("", lib.ctc_amd_long_windowed_loss_grad, _lib.long_wildcard_loss_workspace_bytes),
                             ("ckpt_", lib.ctc_amd_long_windowed_loss_grad_ckpt, _lib.long_wildcard_loss_ckpt_workspace_bytes)):
        lg = {name + "loss": buf((B,), torch.float32), name + "grad": buf((B, T, V), torch.float32)}
        w = ws(size(k, B, T, V, U, tf, True))
        rc = call(*lead, None if dl is None else dl.data_ptr(), *(v.data_ptr() for v in lg.values()), 0, T * V, V, w.data_ptr(), w.numel(),
                  None)
        assert rc == 0, lib.ctc_amd_last_error()
        out.update(lg)
    po = dict(p_loss=buf((B,), torch.float32), post=buf((B, T, U), torch.float32), blk=buf((B, T), torch.float32),
              dur=buf((B, U), torch.float32), exf=buf((B, U), torch.float32), peak=buf((B, U), torch.float32),
              peak_frame=buf((B, U), torch.int32))
    w = ws(_lib.long_label_posterior_workspace_bytes(k, B, T, V, U, tf))
    rc = lib.ctc_amd_long_windowed_label_posterior(*lead, *(v.data_ptr() for v in po.values()), w.data_ptr(), w.numel(), None)
    assert rc == 0, lib.ctc_amd_last_error()
    out.update(po)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_prefilled_outputs_do_not_show(kind):
    """Every element of every output has a writer and nothing unwritten is read: 0x00 and 0xFF in the outputs and the workspace
    give the same bits, the infeasible utterance's included."""
    T, V, U = LONG
    x, labels, ll, tl, window, _ = draw(kind, 2, T, V, U, seed=41)
    tl[-1] = max(1, int(ll[-1]) // 2)  # an infeasible utterance: its outputs are written too
    a = _raw_calls(kind, x, labels, ll, tl, window, 0x00)
    b = _raw_calls(kind, x, labels, ll, tl, window, 0xFF)
    same_bits(a, b)
    assert np.isinf(a["loss"].numpy()[-1]) and np.isfinite(a["loss"].numpy()[0])
    same_bits({"loss": a["loss"], "grad": a["grad"]}, {"loss": a["ckpt_loss"], "grad": a["ckpt_grad"]})
    same_bits({"loss": a["loss"]}, {"loss": a["p_loss"]})
    # ... and they are the public calls' bits
    pub = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=True, frames_per_tile=64)
    same_bits({n: a[m] for n, m in (("loss", "loss"), ("grad", "grad"), ("p_label_posterior", "post"), ("p_peak_frame", "peak_frame"))}, pub,
              ["loss", "grad", "p_label_posterior", "p_peak_frame"])


def test_graph_capture_replays():
    """The windowed long-form calls neither synchronise nor allocate outside the graph's pool: one capture, one replay, the eager
    bits."""
    import tf_seq2seq_losses_amd as ctc
    T, V, U = LONG
    x, labels, ll, tl, window, _ = draw("classic", 1, T, V, U, seed=61)
    eager = run_long("classic", 0, x, labels, ll, tl, window, checkpoint=True, max_label_length=U)
    xs, lab, l1, l2, win = dev(x), dev(labels), dev(ll), dev(tl), dev(window)

    def work():
        xg = xs.clone().requires_grad_(True)
        loss = ctc.classic_ctc_long_loss(lab, xg, l1, l2, 0, wildcard_log_weight=WEIGHT, max_label_length=U, checkpoint=True, frame_window=win)
        (g,) = torch.autograd.grad(loss.sum(), xg)
        p = ctc.classic_ctc_long_windowed_label_posterior(lab, xs, l1, l2, 0, wildcard_log_weight=WEIGHT, max_label_length=U,
                                                          frame_window=win)
        return dict(loss=loss.detach(), grad=g, **{"p_" + k: v for k, v in p._asdict().items()})

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
    same_bits(eager, {k: v.cpu() for k, v in out.items()})
