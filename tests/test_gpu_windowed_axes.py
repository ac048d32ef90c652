"""The windowed kernels along the axes that tests/test_gpu_windowed.py and tests/test_gpu_long_windowed.py hold at one point: the
blank index, the vocabulary, d_loss, the label and window strides and float16 logits.  Every `WIN = true` instantiation (short and
long form, loss, gradient, label posteriors, alignment) is compared with tests/tools/window_oracle.py, which
tests/test_window_oracle.py pins at a non-zero blank and with a weighted gradient.  Inputs, bit comparison and checks are those two
modules' own (imported, not copied).

A non-zero blank: the inputs are drawn as there (labels in 1 .. V-1, a feasible path, windows with slack 0..3) and every label
equal to the blank then becomes 0.  The map is injective on the labels, so equal neighbours, segments, windows and feasibility stay
as drawn.  Before any GPU call the host asserts that no label is the blank and that the oracle's loss is finite where it should be.

Bars: those of the two modules, 1e-4 + 1e-6 |loss| on the loss and a path's score, 1e-4 per gradient, posterior, duration or
expected-frame element (duration relative above 1, as there); a weighted gradient 1e-4 max(1, |d_loss[b]|); a float16 gradient 1e-4
plus half a unit in the last place of float16 at magnitude 1, 2^-12 (the bfloat16 bar of those modules is 2^-9 in its place).
float16 logits: every unwindowed counterpart accepts them (tests/test_gpu_wildcard_loss.py, test_gpu_label_posterior.py,
test_gpu_wildcard_alignment.py, test_gpu_long_loss.py, test_gpu_long_loss_ckpt.py, test_gpu_long_label_posterior.py,
test_gpu_long_wildcard_alignment.py), so every windowed call runs on them.

Worst errors measured on an MI355X, both lattices and both input kinds (bar):
  short form, blank 17 / 66     loss 2.7e-5 (1e-4 + 1e-6 |loss|), gradient 7.2e-7, posterior 7.0e-7, blank 7.2e-7, expected frame
                                7.5e-6 (1e-4 each)
  long form, blank 17           loss 1.7e-4 (4.3e-3), gradient 2.1e-6, posterior 2.2e-6, blank 1.8e-6, duration 8.4e-6, expected
                                frame 6.1e-5 (half a float32 unit in the last place at frame 1400; 1e-4 each)
  long form, V = 1028           loss 2.3e-4 (7.1e-3), gradient 2.3e-6 (1e-4)
  d_loss, short / long          gradient 8.4e-7 / 3.9e-6 (1e-4 max(1, |d_loss|)); zero-weight and infeasible rows exactly 0
  float16, short / long         gradient 2.44e-4 / 2.45e-4 (3.44e-4), loss 1.1e-5 / 8.4e-5, posterior 9.0e-7 / 1.2e-6, expected frame
                                7.5e-6 / 6.1e-5
Every bit comparison (padded widths, odd window_stride, C entry points against the public calls, both workspaces, both tile heights)
held exactly.  With one-line mistakes planted in a scratch build, each of these tests failed and no other: the windowed producer of
the short form reading column 0 for the blank (test_nonzero_blank_short_form), the long-form back-trace reporting token 0 on blank
frames (test_nonzero_blank_long_alignment), the infeasible rows written as d_loss * 0 (test_d_loss_short_form), the long-form loss
kernels indexing the window by 2 * U (test_padded_widths_long_form)."""
import numpy as np
import pytest
import torch

from tests import test_gpu_long_windowed as TL
from tests import test_gpu_windowed as TW
from tests.tools import window_oracle as WO

pytestmark = pytest.mark.gpu
KINDS = WO.KINDS
W = WO.WILDCARD
draw, dev, same_bits, tol, run_all = TW.draw, TW.dev, TW.same_bits, TW.tol, TW.run_all
check_sums, check_path, check_owners = TW.check_sums, TW.check_path, TW.check_owners
run_long, oracle, check = TL.run_long, TL.oracle, TL.check
WEIGHT = TL.WEIGHT
SHORT = [((2, 88, 37, 64), 17), ((2, 169, 67, 129), 66)]  # ((B, T, V, U), blank): V odd and no multiple of 4; V beyond a wavefront, NL = 4
LONG_MAIN = (2, 1400, 37, 1030, 17)  # B, T, V, U, blank
PAD = 7
EMPTY = (5, 4)  # first > last


def reblank(labels, blank):
    out = labels.copy()
    out[out == blank] = 0
    return out


def logp(x):
    return torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()


def host_checks(kind, wrt, x64, labels, ll, tl, window, blank, feasible=None):
    """What must hold before a GPU call: no label inside label_length is the blank, and the oracle's loss is finite for every
    utterance meant to be feasible (default: all) and +inf for the others."""
    for b in range(len(ll)):
        L, Tb = int(ll[b]), int(tl[b])
        assert not np.any(labels[b, :L] == blank), b
        loss = WO.posterior_one(kind, labels[b, :L], x64[b, :Tb], window[b, :L], blank, wrt, WEIGHT)[0]
        assert np.isfinite(loss) == (feasible is None or bool(feasible[b])), (b, loss)


def check_expected_frame(got, ref, what):
    e = np.abs(got["p_expected_frame"].numpy() - ref["exf"])
    print(f"{what}: expected frame err {e.max():.3g}")
    assert e.max() <= 1e-4, (what, e.max())


def check_blank_token(got, tl, blank, what):
    """Frames the alignment reports as blank carry the token `blank`, and there are such frames."""
    tokens, index = got["a_tokens"].numpy(), got["a_label_index"].numpy()
    n = 0
    for b in range(len(tl)):
        free = index[b, :tl[b]] < 0
        n += int(free.sum())
        assert np.all(tokens[b, :tl[b]][free] == blank), (what, b)
    assert n > 0, what


_INPUTS = {}


def short_input(kind, case, wrt):
    """The input of SHORT[case] on a lattice: (x, labels, ll, tl, window), drawn once and not changed by anybody."""
    key = ("short", kind, case, wrt)
    if key not in _INPUTS:
        (B, T, V, U), blank = SHORT[case]
        x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=4000 + 10 * U + wrt)
        labels = reblank(labels, blank)
        assert np.any(labels == 0)  # the column a blank of 0 would have taken is a label's
        if wrt:
            x = logp(x)
        _INPUTS[key] = (x, labels, ll, tl, window)
    return _INPUTS[key]


def long_input(kind):
    """T = 1400, V = 37, U = 1030, blank 17: utterance 0 is full length, utterance 1 fits in one label block."""
    key = ("long", kind)
    if key not in _INPUTS:
        B, T, V, U, blank = LONG_MAIN
        x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=4100)
        labels = reblank(labels, blank)
        assert ll[0] == U and tl[0] == T and ll[1] <= 1024
        _INPUTS[key] = (x, labels, ll, tl, window)
    return _INPUTS[key]


def long_ref(kind):
    x, labels, ll, tl, window = long_input(kind)
    ref = oracle("axes long", kind, 0, x.astype(np.float64), labels, ll, tl, window, blank=LONG_MAIN[4])
    assert np.isfinite(ref["loss"]).all(), ref["loss"]
    return ref


def wide_input(kind):
    """T = 1100 (classic: 1200, as test_formats of tests/test_gpu_long_windowed.py explains), V = 1028, U = 1026, blank 1027: two
    column passes of the row stage, the blank in the last column of the second, two positions in the second label block."""
    key = ("wide", kind)
    if key not in _INPUTS:
        T, V, U, blank = (1200 if kind == "classic" else 1100), 1028, 1026, 1027
        x, labels, ll, tl, window, _ = draw(kind, 1, T, V, U, seed=4200)
        labels = reblank(labels, blank)
        # token 0 stands in both label blocks: the drawn path stays a path, a new token only lifts a blank between equal neighbours
        for lo in (0, 1024):
            i = lo + int(np.nonzero(labels[0, lo:] != W)[0][0])
            assert 0 not in labels[0, max(i - 1, 0):i + 2] or labels[0, i] == 0
            labels[0, i] = 0
        assert ll[0] == U and tl[0] == T and np.any(labels[0, :1024] == 0) and np.any(labels[0, 1024:] == 0)
        _INPUTS[key] = (x, labels, ll, tl, window, blank)
    return _INPUTS[key]


def padded(labels, window, blank):
    """labels and window in tensors PAD positions wider, the padding hostile: labels equal to the blank and empty windows."""
    B, U = labels.shape
    lab = np.full((B, U + PAD), blank, np.int32)
    lab[:, :U] = labels
    win = np.empty((B, U + PAD, 2), np.int32)
    win[...] = EMPTY
    win[:, :U] = window
    return lab, win


def odd_stride(window):
    """The pairs of `window` in a flat buffer with window_stride = 2 U + 1: one int32 (an empty window's bound) between utterances."""
    B, U, _ = window.shape
    flat = np.full(B * (2 * U + 1), EMPTY[0], np.int32)
    for b in range(B):
        flat[b * (2 * U + 1):b * (2 * U + 1) + 2 * U] = window[b].reshape(-1)
    return flat, 2 * U + 1


# ---- a. a non-zero blank and a real vocabulary, the short form ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(SHORT)), ids=lambda c: "x".join(map(str, SHORT[c][0])) + f"-blank{SHORT[c][1]}")
def test_nonzero_blank_short_form(kind, case):
    shape, blank = SHORT[case]
    for wrt in (0, 1):
        x, labels, ll, tl, window = short_input(kind, case, wrt)
        x64 = x.astype(np.float64)
        host_checks(kind, wrt, x64, labels, ll, tl, window, blank)
        what = f"{kind} {shape} blank={blank} wrt={wrt}"
        got = run_all(kind, wrt, x, labels, ll, tl, window, blank=blank)
        free = run_all(kind, wrt, x, labels, ll, tl, None, blank=blank)
        ref = check_sums(kind, wrt, x64, labels, ll, tl, window, got, free, WEIGHT, what, blank=blank)
        check_expected_frame(got, ref, what)
        check_path(kind, wrt, x64, labels, ll, tl, window, got, what, blank=blank)
        check_blank_token(got, tl, blank, what)
        assert np.all(got["a_score"].numpy() <= free["a_score"].numpy())


# ---- b. the same for the long form ----

@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_blank_long_form(kind):
    """Against the oracle, and the same bits for frames_per_tile 64 and the default and for both workspaces."""
    B, T, V, U, blank = LONG_MAIN
    x, labels, ll, tl, window = long_input(kind)
    x64 = x.astype(np.float64)
    assert not any(np.any(labels[b, :ll[b]] == blank) for b in range(B))
    ref = long_ref(kind)  # (finite for both utterances: asserted there, before any GPU call)
    free = run_long(kind, 0, x, labels, ll, tl, None, post=False, blank=blank)
    base = run_long(kind, 0, x, labels, ll, tl, window, blank=blank)
    check(ref, base, window, tl, f"{kind} long blank={blank}", free["loss"])
    check_expected_frame(base, ref, f"{kind} long blank={blank}")
    for tf in (64, None):
        for ck in (False, True):
            got = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck, blank=blank, frames_per_tile=tf)
            same_bits(base, got)


@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_blank_long_alignment(kind):
    B, T, V, U, blank = LONG_MAIN
    x, labels, ll, tl, window = long_input(kind)
    x64 = x.astype(np.float64)
    long_ref(kind)
    runs = {tf: run_all(kind, 0, x, labels, ll, tl, window, long_form=True, blank=blank, frames_per_tile=tf) for tf in (64, None)}
    same_bits(runs[64], runs[None], [k for k in runs[64] if k != "a_score"])  # (score: last bits apart, as test_long_form says)
    for tf, got in runs.items():
        what = f"{kind} long alignment blank={blank} frames_per_tile={tf}"
        check_path(kind, 0, x64, labels, ll, tl, window, got, what, blank=blank)
        check_blank_token(got, tl, blank, what)


@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_blank_two_column_passes(kind):
    """V = 1028, blank 1027, the shape of test_two_column_passes_on_the_vector_path in tests/test_gpu_long_scale.py: loss and gradient."""
    x, labels, ll, tl, window, blank = wide_input(kind)
    assert blank not in labels
    ref = oracle("axes wide", kind, 0, x.astype(np.float64), labels, ll, tl, window, blank=blank, post=False)
    assert np.isfinite(ref["loss"]).all(), ref["loss"]
    free = run_long(kind, 0, x, labels, ll, tl, None, post=False, blank=blank)
    got = run_long(kind, 0, x, labels, ll, tl, window, post=False, blank=blank, checkpoint=False)
    check(ref, got, window, tl, f"{kind} V=1028 blank={blank}", free["loss"])


# ---- c. d_loss ----

def check_weighted(kind, x, labels, ll, tl, window, bad_b, bad_i, d, runs, raws, what):
    """`runs(window, d_loss)` and `raws(window, d_loss)` give dicts with loss and grad, the public call and the C entry point(s).
    Utterance bad_b gets an empty window and NaN in d_loss."""
    d = np.asarray(d, np.float32)
    assert np.isnan(d[bad_b]) and bad_i < ll[bad_b]
    bad = window.copy()
    bad[bad_b, bad_i] = EMPTY
    feasible = np.arange(len(ll)) != bad_b
    x64 = x.astype(np.float64)
    host_checks(kind, 0, x64, labels, ll, tl, bad, 0, feasible)
    o_loss, o_grad = WO.loss_and_grad(kind, 0, labels, x64, ll, tl, bad, 0, WEIGHT, d)
    assert not o_grad[bad_b].any() and not np.isnan(o_grad).any()
    got = runs(bad, d)
    loss, grad = got["loss"].numpy(), got["grad"].numpy()
    assert loss[bad_b] == np.inf and np.isfinite(loss[feasible]).all(), (what, loss)
    assert not np.isnan(grad).any(), what
    for b in range(len(ll)):
        e = np.abs(grad[b] - o_grad[b]).max()
        print(f"{what} b={b} d_loss={d[b]}: loss err {abs(loss[b] - o_loss[b]) if feasible[b] else 0.0:.3g} grad err {e:.3g} "
              f"(bar {1e-4 * max(1.0, abs(d[b])) if feasible[b] else 0.0:.3g})")
        if not feasible[b] or d[b] == 0.0:
            assert not grad[b].any(), (what, b)  # exactly zero
        else:
            assert e <= 1e-4 * max(1.0, abs(d[b])), (what, b, e)
            assert grad[b].any(), (what, b)
            assert abs(loss[b] - o_loss[b]) <= tol(o_loss[b]), (what, b)
    # the C entry point with the d_loss pointer: the public call's bits
    for name, raw in raws(bad, d).items():
        same_bits(got, raw, ["loss", "grad"])
    # d_loss does not leak: every other row as in a run where that utterance is feasible (and weighted)
    d2 = d.copy()
    d2[bad_b] = 1.5
    good = runs(window, d2)
    assert np.isfinite(good["loss"].numpy()).all() and good["grad"][bad_b].any()
    for b in np.nonzero(feasible)[0]:
        same_bits({k: v[b] for k, v in got.items()}, {k: v[b] for k, v in good.items()})


@pytest.mark.parametrize("kind", KINDS)
def test_d_loss_short_form(kind):
    B, T, V, U = 4, 88, 8, 64
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=4300)

    def runs(win, d):
        out = run_all(kind, 0, x, labels, ll, tl, win, d_loss=d)
        return {k: out[k] for k in ("loss", "grad")}

    def raws(win, d):
        return {"ctc_amd_windowed_loss_grad": TW._raw_calls(kind, x, labels, ll, tl, win, 0xFF, False, d_loss=d)}

    check_weighted(kind, x, labels, ll, tl, window, 0, int(ll[0]) // 2, [np.nan, -2.0, 0.0, 3.0], runs, raws, f"{kind} d_loss")
    check_weighted(kind, x, labels, ll, tl, window, 3, 0, [0.5, 0.0, -2.0, np.nan], runs, raws, f"{kind} d_loss, the last row")


@pytest.mark.parametrize("kind", KINDS)
def test_d_loss_long_form(kind):
    """The main input of tests/test_gpu_long_windowed.py (B = 3 of LONG) with both workspaces.  Three utterances cannot hold NaN, a
    zero, a negative weight and one above 1 at once, so there are two weight vectors: the infeasible utterance is once the one that
    reaches the second label block (its empty window lies there) and once one that does not."""
    x, labels, ll, tl, window = TL.main_input(kind)

    def raws(win, d):
        raw = TL._raw_calls(kind, x, labels, ll, tl, win, 0xFF, tf=64, d_loss=d)
        return {"ctc_amd_long_windowed_loss_grad": {"loss": raw["loss"], "grad": raw["grad"]},
                "ctc_amd_long_windowed_loss_grad_ckpt": {"loss": raw["ckpt_loss"], "grad": raw["ckpt_grad"]}}

    def runs(win, d):
        a, b = (run_long(kind, 0, x, labels, ll, tl, win, checkpoint=ck, post=False, d_loss=d, frames_per_tile=64) for ck in (False, True))
        same_bits(a, b)
        return a

    check_weighted(kind, x, labels, ll, tl, window, 0, 1024, [np.nan, -2.0, 0.0], runs, raws, f"{kind} long d_loss")
    check_weighted(kind, x, labels, ll, tl, window, 1, int(ll[1]) // 2, [3.0, np.nan, -2.0], runs, raws,
                   f"{kind} long d_loss, one block infeasible")


# ---- d. padded widths: label stride != U, window_stride != 2 U ----

def check_width_follows_labels(base, wide, U):
    """The C entry points called with the padded width as their bound U (the public functions never do that: without
    max_label_length they bound a label tensor wider than 128 by the largest label_length inside, which is U here).  Outputs whose
    last axis is that bound: the unpadded result on [:, :U], and on the padding what include/ctc_amd.h says of positions from
    label_length on: -1 in first_frame, last_frame, expected_frame and peak_frame, -inf in label_score, 0 in label_posterior,
    duration and peak_posterior.  Every other output: the unpadded bits."""
    fill = {"first_frame": -1, "last_frame": -1, "label_score": -np.inf, "post": 0.0, "dur": 0.0, "exf": -1.0, "peak": 0.0,
            "peak_frame": -1}
    assert set(wide) == set(base)
    for k, v in wide.items():
        if k in fill:
            assert v.shape[-1] == U + PAD and base[k].shape[-1] == U, k
            same_bits({k: v[..., :U]}, base, [k])
            assert torch.all(v[..., U:] == fill[k]), k
        else:
            same_bits({k: v}, base, [k])


@pytest.mark.parametrize("kind", KINDS)
def test_padded_widths_short_form(kind):
    (B, T, V, U), blank = SHORT[1]
    for wrt in (0, 1):
        x, labels, ll, tl, window = short_input(kind, 1, wrt)
        host_checks(kind, wrt, x.astype(np.float64), labels, ll, tl, window, blank)
        lab_p, win_p = padded(labels, window, blank)
        base = run_all(kind, wrt, x, labels, ll, tl, window, blank=blank, max_label_length=U)
        assert np.isfinite(base["loss"].numpy()).all() and np.isfinite(base["a_score"].numpy()).all()
        same_bits(base, run_all(kind, wrt, x, labels, ll, tl, window, blank=blank))  # (the bound is the width: the same call)
        got = run_all(kind, wrt, x, lab_p, ll, tl, win_p, blank=blank, max_label_length=U)
        assert set(got) == set(base)
        same_bits(base, got)  # every output, every width as without the padding
        # either of the two alone
        same_bits(base, run_all(kind, wrt, x, lab_p, ll, tl, window, blank=blank, max_label_length=U))
        same_bits(base, run_all(kind, wrt, x, labels, ll, tl, win_p, blank=blank, max_label_length=U))
        same_bits(base, run_all(kind, wrt, x, lab_p, ll, tl, win_p, blank=blank))  # (the bound from the device: max(label_length) = U)
    # the C entry points: label_stride = U + PAD, window_stride = 2 (U + PAD), outputs and workspaces sized for U
    x, labels, ll, tl, window = short_input(kind, 1, 0)
    lab_p, win_p = padded(labels, window, blank)
    raw = TW._raw_calls(kind, x, labels, ll, tl, window, 0xFF, False, blank=blank)
    base = run_all(kind, 0, x, labels, ll, tl, window, blank=blank, max_label_length=U)
    names = dict(loss="loss", grad="grad", post="p_label_posterior", blk="p_blank_posterior", dur="p_duration", exf="p_expected_frame",
                 score="a_score", tokens="a_tokens", label_index="a_label_index", first_frame="a_first_frame", last_frame="a_last_frame",
                 label_score="a_label_score")
    same_bits({n: raw[n] for n in names}, {n: base[m] for n, m in names.items()})
    same_bits(raw, TW._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, False, blank=blank, U=U))
    flat, stride = odd_stride(window)
    same_bits(raw, TW._raw_calls(kind, x, lab_p, ll, tl, flat, 0xFF, False, blank=blank, U=U, window_stride=stride))
    same_bits(raw, TW._raw_calls(kind, x, labels, ll, tl, flat, 0xFF, False, blank=blank, window_stride=stride))
    check_width_follows_labels(raw, TW._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, False, blank=blank), U)


@pytest.mark.parametrize("kind", KINDS)
def test_padded_widths_long_form(kind):
    B, T, V, U, blank = LONG_MAIN
    x, labels, ll, tl, window = long_input(kind)
    long_ref(kind)
    lab_p, win_p = padded(labels, window, blank)
    for ck in (False, True):
        base = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=ck, blank=blank, max_label_length=U)
        assert np.isfinite(base["loss"].numpy()).all()
        got = run_long(kind, 0, x, lab_p, ll, tl, win_p, checkpoint=ck, blank=blank, max_label_length=U)
        assert set(got) == set(base)
        same_bits(base, got)
        thin = run_long(kind, 0, x, lab_p, ll, tl, win_p, checkpoint=ck, dense=False, blank=blank, max_label_length=U)
        assert "p_label_posterior" not in thin and set(TL.POST_KEYS) <= set(thin)
        same_bits(thin, base, thin.keys())
    same_bits(base, run_long(kind, 0, x, lab_p, ll, tl, win_p, checkpoint=True, blank=blank))  # (the bound from the device: U)
    a_base = run_all(kind, 0, x, labels, ll, tl, window, long_form=True, blank=blank, max_label_length=U)
    assert np.isfinite(a_base["a_score"].numpy()).all()
    same_bits(a_base, run_all(kind, 0, x, lab_p, ll, tl, win_p, long_form=True, blank=blank, max_label_length=U))
    same_bits(a_base, run_all(kind, 0, x, lab_p, ll, tl, win_p, long_form=True, blank=blank))
    # the C entry points
    flat, stride = odd_stride(window)
    raw = TL._raw_calls(kind, x, labels, ll, tl, window, 0xFF, blank=blank)
    pub = run_long(kind, 0, x, labels, ll, tl, window, checkpoint=True, blank=blank, frames_per_tile=64)
    names = dict(loss="loss", grad="grad", ckpt_loss="loss", ckpt_grad="grad", p_loss="p_loss", post="p_label_posterior",
                 blk="p_blank_posterior", dur="p_duration", exf="p_expected_frame", peak="p_peak_posterior", peak_frame="p_peak_frame")
    same_bits({n: raw[n] for n in names}, {n: pub[m] for n, m in names.items()})
    same_bits(raw, TL._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, blank=blank, U=U))
    same_bits(raw, TL._raw_calls(kind, x, lab_p, ll, tl, flat, 0xFF, blank=blank, U=U, window_stride=stride))
    a_raw = TW._raw_calls(kind, x, labels, ll, tl, window, 0xFF, True, blank=blank)
    same_bits(a_raw, TW._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, True, blank=blank, U=U))
    same_bits(a_raw, TW._raw_calls(kind, x, lab_p, ll, tl, flat, 0xFF, True, blank=blank, U=U, window_stride=stride))
    check_width_follows_labels(raw, TL._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, blank=blank), U)
    check_width_follows_labels(a_raw, TW._raw_calls(kind, x, lab_p, ll, tl, win_p, 0xFF, True, blank=blank), U)


# ---- e. float16 logits ----

F16_TOL = 1e-4 + 2.0 ** -12


@pytest.mark.parametrize("kind", KINDS)
def test_float16_short_form(kind):
    B, T, V, U = 2, 169, 8, 129
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=4400)
    xh = torch.from_numpy(x).to(torch.float16)
    x64 = xh.double().numpy()  # the values the kernel reads
    host_checks(kind, 0, x64, labels, ll, tl, window, 0)
    got = run_all(kind, 0, xh.to(TW.DEV), labels, ll, tl, window)
    assert got["grad"].dtype == torch.float16
    free = run_all(kind, 0, xh.to(TW.DEV), labels, ll, tl, None)
    ref = check_sums(kind, 0, x64, labels, ll, tl, window, got, free, WEIGHT, f"{kind} float16", grad_tol=F16_TOL)
    check_expected_frame(got, ref, f"{kind} float16")
    check_path(kind, 0, x64, labels, ll, tl, window, got, f"{kind} float16")


@pytest.mark.parametrize("kind", KINDS)
def test_float16_long_form(kind):
    """The shape of test_formats in tests/test_gpu_long_windowed.py: both workspaces, the posteriors and the alignment."""
    B, T, V, U = 2, (1200 if kind == "classic" else 1100), 8, 1026
    x, labels, ll, tl, window, _ = draw(kind, B, T, V, U, seed=21)
    xh = torch.from_numpy(x).to(torch.float16)
    x64 = xh.double().numpy()
    ref = oracle("axes float16", kind, 0, x64, labels, ll, tl, window)
    assert np.isfinite(ref["loss"]).all(), ref["loss"]
    free = run_long(kind, 0, xh.to(TW.DEV), labels, ll, tl, None, post=False)
    for ck in (False, True):
        got = run_long(kind, 0, xh.to(TW.DEV), labels, ll, tl, window, checkpoint=ck)
        assert got["grad"].dtype == torch.float16
        check(ref, got, window, tl, f"{kind} float16 checkpoint={ck}", free["loss"], grad_tol=F16_TOL)
        check_expected_frame(got, ref, f"{kind} float16 checkpoint={ck}")
    al = run_all(kind, 0, xh.to(TW.DEV), labels, ll, tl, window, long_form=True)
    check_path(kind, 0, x64, labels, ll, tl, window, al, f"{kind} float16 long alignment")
