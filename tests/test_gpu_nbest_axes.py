"""The N-best family along the axes that its own modules hold at one point: the vocabulary and the blank index (V up to 2052, where
tests/test_gpu_nbest_loss.py, tests/test_gpu_nbest_loss_grad.py and tests/test_gpu_mwer_loss.py stop at 32), the scale and range
of the weights, and ownership at V > 1024.  N-best loss and gradient, the MWER loss, the prefix scorer and beam search are compared
with the oracles their own modules use (tests/tools/nbest_grad_oracle.py, edit_oracle.py, prefix_oracle.py, beam_oracle.py);
runners, checks and bit comparison are those modules' own and those of tests/_ownership.py (imported, not copied).  Every input is
drawn once per process and kept, read-only, with its oracle result where the check takes one; before any GPU call the host asserts
what the case is about (host_checks).

a. shapes (B, T, V, N, W): utterance 1 has W - 1 frames; hypothesis 0 of every utterance has weight 0, hypothesis 1 a negative
weight; hypothesis 2 of utterance 1 has W labels, one more than its frames, and a NaN weight.  (With N = 3 that leaves utterance 1
one hypothesis that counts: what the host asserts of two hypotheses, it asserts there of utterance 0.)  Where the blank is 1024 the
adjacent pair across the pass boundary is (1023, 1025).

Bars: those of the modules.  Loss 1e-4 + 1e-6 |loss|; gradient 1e-4 max(1, sum |w|) over the feasible hypotheses, a 16-bit gradient
plus 2^-8 |oracle|; MWER, prefix scores and beam search as their modules derive them.  Scale invariance, zero rows and ownership: bits.

Worst errors measured on an MI355X, both lattices, wrt = 0 and 1 (bar; in brackets the worst error as a fraction of its bar):
  a. (2, 30, 37, 9, 10) blank 17      loss 6.4e-6 (1e-4 + 1e-6 |loss|) [0.027], gradient 9.6e-7 (1e-4 max(1, sum |w|)) [0.001]
  a. (2, 30, 67, 5, 10) blank 66      loss 6.3e-6 [0.027], gradient 7.7e-7 [0.002]
  a. (2, 24, 260, 5, 8) blank 259     loss 8.8e-6 [0.036], gradient 2.8e-7 [0.001]
  a. (2, 24, 261, 5, 8) blank 130     loss 8.9e-6 [0.037], gradient 3.4e-7 [0.001]
  a. (2, 24, 1028, 9, 12) blank 1027  loss 9.8e-6 [0.039], gradient 7.7e-7 [0.001]; bfloat16: loss 1.0e-5 [0.039], gradient 7.7e-3
                                      (1e-4 max(1, sum |w|) + 2^-8 |oracle|) [0.82]
  a. (2, 24, 1030, 9, 12) blank 1029  loss 9.7e-6 [0.036], gradient 6.8e-7 [0.001]
  a. (2, 20, 2052, 3, 8) blank 1024   loss 9.5e-6 [0.037], gradient 6.0e-7 [0.003]
  b. weights * 2^12 and * 2^-12       0 of 49440 gradient elements differ in their bits from the unscaled gradient times the scale, wrt = 0
                                      and 1: every term of the row stage is scale-invariant, as the code reads
  b. weights over 2^20                gradient 4.4e-7 against the oracle (1e-4) [0.004]; |wide - zeroed| 2.0e-6 where the oracle's two
                                      gradients differ by 2.0e-6: 0.0012 of the bar beyond the oracle's own difference
  b. zero weights, nothing feasible   +0 in every element with wrt = 0 AND with wrt = 1: both leave through the row stage's early
                                      exit (wmax = 0), so no -0 was seen with wrt = 1 either; the test asserts numeric zero there
  b. C entry points, stride V + 3     gradient 4.2e-7 [0.001]; every bit comparison held, no guard byte changed
  c. MWER V = 67 / 1030               loss 8.9e-7, gradient 9.5e-7 (1e-4 max(1, sum |c|)), log_posterior 2.1e-6 (2 max tol + 1e-6 |.|)
  d. prefix scores V = 1030 / 1028    scores 5.6e-6 [0.033], full_score 1.1e-5 [0.044] (1e-4 + 1e-6 |oracle|)
  d. beam search                      |score - oracle| 6.6e-6 (V = 1030), 3.5e-6 (V = 8192) (1e-4 + 1e-6 |score|); labels exact.  Seeds chosen
                                      with the oracle on the CPU: seed 2 (margin 2.56e-4) and seed 1 (margin 4.73e-3), both lattices alike

With one-line mistakes planted in ctc_nbest.hip in scratch builds, one at a time, the whole of this module and of the three existing
modules (N-best loss, N-best gradient, MWER: 97 cases) was run on each build:
  1. the row stage adds the blank's share only when c0 == 0     12 cases here failed: test_loss_and_gradient_along_v_and_blank at V = 1028,
                                                                1030 and 2052 (all eight), test_weights_that_span_twenty_binary_orders
                                                                and test_unowned_memory_beyond_one_pass_changes_no_bit (both each);
                                                                all 97 existing cases passed
  2. the bins are not zeroed again for the second pass          16 failed: the twelve of 1. and
                                                                test_mwer_explicit_hypotheses_with_a_blank_elsewhere at V = 1030 (all
                                                                four); all 97 existing cases passed
  3. the producer's statistics loop stops after its first       18 failed: test_loss_and_gradient_along_v_and_blank from V = 260 on (twelve),
     stride                                                     the weights, zero-weights and ownership tests.  Not new coverage alone:
                                                                test_committed_hard_cases[r04_case_forward_loss_nl8.npz] of
                                                                tests/test_gpu_nbest_loss.py failed on that build too (96 of 97 passed)
  4. the label filter reads rel <= NBG_CH                       not run: a token equal to c0 + 1024 then adds to slot 1024 of its wavefront's
                                                                1024 bins, that is to bin 0 of the next wavefront's row or, from the last
                                                                wavefront, past the kernel's LDS -- an out-of-bounds write by
                                                                construction, whose effect depends on a race between wavefronts.  The
                                                                inputs that reach it are here (token 1024 at V = 1028 and 1030); no claim
                                                                is made that a test fails on it
"""
import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_beam_search as TB
from tests import test_gpu_mwer_loss as TM
from tests import test_gpu_nbest_loss as F
from tests import test_gpu_nbest_loss_grad as G
from tests import test_gpu_prefix_score as TP
from tests.tools import nbest_grad_oracle as NG

pytestmark = pytest.mark.gpu
KINDS = G.KINDS
DEV = G.DEV
# ((B, T, V, N, W), blank, element type)
GRAD = [((2, 30, 37, 9, 10), 17, torch.float32),      # V odd: the element-wise path; N = 9: two groups of eight
        ((2, 30, 67, 5, 10), 66, torch.float32),      # V beyond one wavefront of the statistics, the blank in the last column
        ((2, 24, 260, 5, 8), 259, torch.float32),     # second stride of the k += 256 loops, vector path
        ((2, 24, 261, 5, 8), 130, torch.float32),     # the same stride, element-wise path
        ((2, 24, 1028, 9, 12), 1027, torch.float32),  # two column passes, vector path
        ((2, 24, 1028, 9, 12), 1027, torch.bfloat16),  # ... and the 16-bit vector stores
        ((2, 24, 1030, 9, 12), 1029, torch.float32),  # two column passes, element-wise path
        ((2, 20, 2052, 3, 8), 1024, torch.float32)]   # three passes, the blank in the first column of the second
WEIGHTS_CASE = 6
CH = 1024  # columns per pass of the gradient's row stage
# V -> (the token behind 1023, a token >= 1024 shared by two hypotheses, the last non-blank token, one more token of the last pass)
PLANT = {1028: (1024, 1025, 1026, 1024), 1030: (1024, 1026, 1028, 1027), 2052: (1025, 1026, 2051, 2050)}
# (B, T, V, W, K, nbest), blank, seed, the smallest oracle margin of the two lattices with that seed
BEAM = [((2, 40, 1030, 8, 8, 4), 1029, 2, 2.55e-4), ((2, 30, 8192, 5, 32, 5), 4096, 1, 4.73e-3)]
GUARD_FILL = 0xA5

_INPUTS, _REFS = {}, {}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def logp(x):
    return torch.log_softmax(torch.tensor(x).double(), -1).float().numpy()


def zero_bits(t):
    """Every element is +0, bit for bit."""
    return not bool(OW.bits(t.contiguous()).any())


def case_id(c):
    shape, blank, dtype = GRAD[c]
    return "x".join(map(str, shape)) + f"-blank{blank}-{str(dtype).split('.')[1]}"


# ---- a. N-best loss and gradient along V and the blank ----

def second_live(N):
    """The hypothesis that holds a positive weight and, at V > 1024, the second set of planted tokens."""
    return 3 if N > 3 else 2


def grad_input(shape, blank):
    """(x, tl, labels, ll, w, meant): float32 logits, the N-best list and its weights; meant[B, N]: the hypotheses meant to be
    feasible.  Tokens of a hypothesis are distinct but for one planted repeat (utterance 0, hypothesis 1, positions 4 and 5)."""
    key = (shape, blank)
    if key not in _INPUTS:
        B, T, V, N, W = shape
        rng = np.random.default_rng(7000 + V)
        x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
        tl = np.asarray([T, W - 1], np.int32)
        toks = np.asarray([c for c in range(V) if c != blank], np.int32)
        labels = np.stack([np.stack([rng.permutation(toks)[:W] for _ in range(N)]) for _ in range(B)]).astype(np.int32)
        ll = rng.integers(1, W + 1, (B, N)).astype(np.int32)
        ll[1] = rng.integers(1, W - 1, N)  # at most W - 2 labels in W - 1 frames
        q = second_live(N)
        ll[0, 0], ll[0, 1], ll[1, 1], ll[:, q] = W, W - 1, W - 2, 4
        if N >= 5:
            ll[0, 4] = 0  # an empty hypothesis that counts
        ll[1, 2] = W  # W labels in W - 1 frames
        if V > CH:
            nxt, hi, last, other = PLANT[V]
            labels[:, 1, :4] = [CH - 1, nxt, hi, other]
            labels[:, q, :4] = [0, hi, last, 3]
        labels[0, 1, 5] = labels[0, 1, 4]
        w = G.weights(rng, B, N)
        w[:, q] = np.abs(w[:, q]) + 0.25
        w[1, 2] = np.nan
        meant = np.ones((B, N), bool)
        meant[1, 2] = False
        _INPUTS[key] = frozen(x, tl, labels, ll, w, meant)
    return _INPUTS[key]


def host_checks(shape, blank, tl, labels, ll, w, meant, want_loss):
    """What must hold of an input of a. before a GPU call."""
    B, T, V, N, W = shape
    assert B == 2 and tl[0] == T and tl[1] < T
    for b in range(B):
        for n in range(N):
            lab = labels[b, n, :ll[b, n]]
            assert lab.size == 0 or (lab.min() >= 0 and lab.max() < V and not np.any(lab == blank)), (b, n)
    assert np.array_equal(np.isfinite(want_loss), meant) and np.all(want_loss[~meant] == np.inf), want_loss
    assert (~meant).any() and np.isnan(w[~meant]).all() and not np.isnan(w[meant]).any()
    for b, n in np.argwhere(~meant):
        assert ll[b, n] > tl[b]  # too long for its frames on either lattice
    live = meant & (np.nan_to_num(w) != 0.0)
    for b in range(B):
        assert np.any(w[b][meant[b]] == 0.0) and np.any(w[b][meant[b]] < 0.0), b
    assert live[0].sum() >= 2 and (N == 3 or live[1].sum() >= 2)
    if V <= CH:
        return
    nxt, hi, last, _ = PLANT[V]
    assert last == (V - 2 if blank == V - 1 else V - 1) and nxt == (CH + 1 if blank == CH else CH) and hi >= CH
    seen = set()
    for b in range(B):
        labs = {n: labels[b, n, :ll[b, n]] for n in range(N) if live[b, n]}
        assert any(np.any((l[:-1] == CH - 1) & (l[1:] == nxt)) for l in labs.values() if l.size > 1), b
        for l in labs.values():
            seen.update(l.tolist())
        if len(labs) < 2:
            continue
        for c0 in range(0, V, CH):  # every pass holds labels of two hypotheses that count
            assert sum(bool(np.any((l >= c0) & (l < c0 + CH))) for l in labs.values()) >= 2, (b, c0)
        signs = {np.sign(w[b, n]) for n, l in labs.items() if np.any(l == hi)}
        assert signs == {-1.0, 1.0}, (b, signs)  # one bin sums weights of both signs
    assert 0 in seen and last in seen


def grad_case(c, kind, wrt):
    """(xv, xt, tl, labels, ll, w, meant, ref) of GRAD[c]: xv the float32 values the kernel reads, xt the CPU tensor in the case's
    element type, ref the oracle's (loss, grad) on xv."""
    shape, blank, dtype = GRAD[c]
    x, tl, labels, ll, w, meant = grad_input(shape, blank)
    key = ("a", c, kind, wrt)
    if key not in _REFS:
        xt = torch.tensor(logp(x) if wrt else x).to(dtype)
        xv = xt.float().numpy()
        _REFS[key] = (xt,) + frozen(xv, *NG.nbest_loss_and_grad(kind, wrt, labels, xv, ll, tl, blank, w))
    xt, xv, want_loss, want = _REFS[key]
    host_checks(shape, blank, tl, labels, ll, w, meant, want_loss)
    return xv, xt, tl, labels, ll, w, meant, (want_loss, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", range(len(GRAD)), ids=case_id)
def test_loss_and_gradient_along_v_and_blank(kind, c):
    shape, blank, dtype = GRAD[c]
    V = shape[2]
    for wrt in (0, 1):
        xv, xt, tl, labels, ll, w, meant, ref = grad_case(c, kind, wrt)
        what = f"a. {kind} {case_id(c)} wrt={wrt}"
        loss, grad, _, want = G.check_all(kind, wrt, labels, xv, ll, tl, blank, w, what, xt=xt.to(DEV), sixteen=dtype != torch.float32, ref=ref)
        assert np.array_equal(np.isfinite(loss), meant)
        for c0 in range(0, V, CH):  # a gradient to speak of in every pass
            assert np.abs(want[:, :, c0:c0 + CH]).max() > 1e-3 and np.abs(grad[:, :, c0:c0 + CH]).max() > 1e-3, (what, c0)
        assert np.abs(want[0, :, blank]).max() > 1e-3


# ---- b. weights ----

def weights_input(kind, wrt):
    xv, xt, tl, labels, ll, w, meant, ref = grad_case(WEIGHTS_CASE, kind, wrt)
    return GRAD[WEIGHTS_CASE][0], GRAD[WEIGHTS_CASE][1], xv, tl, labels, ll, w, meant, ref


@pytest.mark.parametrize("kind", KINDS)
def test_weights_scaled_by_a_power_of_two_scale_the_gradient_exactly(kind):
    """The bins hold the same integers at every scale: fe follows the largest weight, wsum and the blank's share scale exactly."""
    for wrt in (0, 1):
        shape, blank, x, tl, labels, ll, w, meant, _ = weights_input(kind, wrt)
        loss, g_np, g = G.run(kind, wrt, labels, x, ll, tl, blank, w)
        assert np.abs(g_np).max() > 1e-3 and np.abs(g_np[g_np != 0.0]).min() > 2.0 ** -100  # nothing near the subnormal range
        for e in (12, -12):
            s = np.float32(2.0 ** e)
            loss_s, _, g_s = G.run(kind, wrt, labels, x, ll, tl, blank, w * s)
            n = OW.count_diff(g_s.cpu(), g.cpu() * float(s))
            print(f"AXES b. {kind} wrt={wrt} weights * 2^{e}: {n} of {g.numel()} gradient elements differ in their bits", flush=True)
            assert F.same(loss_s, loss) and n == 0, (kind, wrt, e, n)


def range_weights(w, meant):
    """(wide, zeroed): one weight of 1 beside the others scaled by 2^-20, and beside exact zeros."""
    keep = second_live(w.shape[1])
    wide, zeroed = (w * np.float32(2.0 ** -20)).astype(np.float32), np.where(meant, np.float32(0.0), w).astype(np.float32)
    wide[:, keep] = zeroed[:, keep] = 1.0
    return wide, zeroed


@pytest.mark.parametrize("kind", KINDS)
def test_weights_that_span_twenty_binary_orders(kind):
    shape, blank, x, tl, labels, ll, w, meant, _ = weights_input(kind, 0)
    wide, zeroed = range_weights(w, meant)
    key = ("range", kind)
    if key not in _REFS:
        _REFS[key] = frozen(*(NG.nbest_loss_and_grad(kind, 0, labels, x, ll, tl, blank, wide) + NG.nbest_loss_and_grad(kind, 0, labels, x, ll, tl, blank, zeroed)))
    want_loss, want_wide, _, want_zeroed = _REFS[key]
    small = np.abs(wide[meant & (wide != 1.0)])
    assert small.max() <= 4.0 * 2.0 ** -20 and small[small > 0].min() >= 2.0 ** -26 and np.all(meant[:, second_live(shape[3])])
    _, g_wide, _, _ = G.check_all(kind, 0, labels, x, ll, tl, blank, wide, f"b. {kind} weights over 2^20", ref=(want_loss, want_wide))
    _, g_zeroed, _, _ = G.check_all(kind, 0, labels, x, ll, tl, blank, zeroed, f"b. {kind} small weights zeroed", ref=(want_loss, want_zeroed))
    wsum = np.abs(np.where(meant, wide, 0.0)).sum(axis=1)
    bar = 1e-4 * np.maximum(1.0, wsum)[:, None, None]
    diff, odiff = np.abs(g_wide - g_zeroed), np.abs(want_wide - want_zeroed)
    print(f"AXES b. {kind} dynamic range: worst |wide - zeroed| {diff.max():.3e}, the oracle's {odiff.max():.3e}, worst excess over the "
          f"oracle's / bar {((diff - odiff) / bar).max():.3g}", flush=True)
    assert odiff.max() > 0.0 and np.all(diff <= odiff + bar)


def nothing_input(kind):
    """The weights case with every weight of utterance 0 zero and W labels in every hypothesis of utterance 1 (W - 1 frames)."""
    shape, blank, x, tl, labels, ll, w, meant, _ = weights_input(kind, 0)
    key = ("nothing", kind)
    if key not in _REFS:
        ll2, w2 = ll.copy(), w.copy()
        ll2[1] = shape[4]
        w2[0] = 0.0
        w2[1, 0] = 1.5
        xs = frozen(x, logp(x))
        _REFS[key] = frozen(ll2, w2) + (xs, frozen(*(F.oracle(kind, wrt, labels, xs[wrt], ll2, tl, blank) for wrt in (0, 1))))
    ll2, w2, xs, want_loss = _REFS[key]
    for wl in want_loss:
        assert np.all(np.isfinite(wl[0])) and np.all(wl[1] == np.inf)
    assert not w2[0].any() and np.all(w2[1] != 0.0)
    for n in range(shape[3]):
        assert not np.any(labels[1, n, :ll2[1, n]] == blank)
    return blank, xs, tl, labels, ll2, w2, want_loss


@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights_and_nothing_feasible_give_zero(kind):
    """wrt = 0: +0 in every element, the early exit of the row stage.  wrt = 1: numeric zero; the count of -0 is printed."""
    blank, xs, tl, labels, ll, w, want_loss = nothing_input(kind)
    for wrt in (0, 1):
        loss, g_np, g = G.run(kind, wrt, labels, xs[wrt], ll, tl, blank, w)
        F.check(loss, want_loss[wrt], f"b. {kind} nothing counts wrt={wrt}")
        minus = int((OW.bits(g.cpu()) != 0).sum())
        print(f"AXES b. {kind} wrt={wrt} zero weights / nothing feasible: {int((g_np != 0.0).sum())} non-zero elements, {minus} not +0 in their bits", flush=True)
        assert np.all(g_np == 0.0), (kind, wrt)
        if wrt == 0:
            assert zero_bits(g.cpu()), kind


@pytest.mark.parametrize("kind", KINDS)
def test_unowned_memory_beyond_one_pass_changes_no_bit(kind):
    """The C entry points at V = 1030 with a row stride of V + 3 for logits and gradient: NaN between V and the stride, poisoned
    padding frames, label tails of (blank, -1, V + 5, INT32_MIN, INT32_MAX).  The guards are asserted inside the raw calls."""
    shape, blank, x, tl, labels, ll, w, meant, ref = weights_input(kind, 0)
    B, T, V, N, W = shape
    S = V + 3
    lab, llt, tlt, wt = G.dev(labels), G.dev(ll), G.dev(tl), G.dev(w)
    storage, view, owned = OW.strided_storage(G.dev(x), T * S, S)
    assert OW.padding_mask(tl, T).any() and bool((~owned).any()) and np.any(ll < W)

    def both(xin, labin):
        loss, _, grad = G.raw_call(kind, xin, labin, llt, tlt, wt, blank, W, fill=GUARD_FILL, gsb=T * S, gst=S)
        assert OW.same_bits(F.raw_call(kind, xin, labin, llt, tlt, blank, W, fill=GUARD_FILL), loss)
        return loss, grad

    closs, clean = both(view, lab)
    F.check(closs.cpu().numpy(), ref[0], f"b. {kind} C entry points V={V} stride {S}")
    G.check_grad(clean.cpu().numpy(), ref[1], ref[0], w, f"b. {kind} C entry points V={V} stride {S}")
    cycle = (blank, -1, V + 5, OW.INT32_MIN, OW.INT32_MAX)
    poisoned = OW.poison_labels(lab.view(B * N, W), ll.reshape(-1), cycle).view(B, N, W)
    assert not torch.equal(poisoned, lab)
    for value in OW.poison_values(torch.float32):
        pstorage, _, _ = OW.strided_storage(OW.poison_padding(G.dev(x), tl, value), T * S, S)
        pview = OW.poison_gaps(pstorage, owned, float("nan")).as_strided((B, T, V), (T * S, S, 1))
        assert pview.stride() == view.stride() and not OW.same_bits(pview, view) and OW.same_bits(pview[0], view[0])
        loss, grad = both(pview, poisoned)
        assert OW.same_bits(loss, closs) and OW.same_bits(grad, clean), (kind, value)


# ---- c. MWER end to end with a non-zero blank ----

@pytest.mark.parametrize("entry", TM.ENTRIES)
@pytest.mark.parametrize("V,blank", [(67, 66), (1030, 513)])
def test_mwer_explicit_hypotheses_with_a_blank_elsewhere(entry, V, blank):
    x, tl, hyp, hl, score, labels, ll = TM.case(V, blank)
    assert not np.any(hyp == blank) and not np.any(labels == blank) and x.shape[2] == V
    assert hyp.max() == (V - 2 if blank == V - 1 else V - 1) and np.any(hyp == 0) and np.any(labels == 0)
    TM.check_explicit(entry, V, blank)


@pytest.mark.parametrize("entry", TM.ENTRIES)
def test_mwer_own_search_with_the_blank_in_the_last_column(entry):
    V, blank = 1030, 1029
    x, tl, hyp, hl, score, labels, ll = TM.case(V, blank)
    assert not np.any(labels == blank) and x.shape[2] == V
    TM.check_own_search(entry, V, blank)


# ---- d. prefix scores and beam search beyond 1024 columns ----

def prefix_input(T, V, N, blank):
    key = ("prefix", T, V, N, blank)
    if key not in _INPUTS:
        rng = np.random.default_rng(T * 1000 + V + blank)
        x = rng.standard_normal((4, T, V), dtype=np.float32)
        _INPUTS[key] = frozen(x, TP.lengths(T), TP.token_plan(V, blank, N, 6, rng))
    return _INPUTS[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank,dtype", [(1030, 513, torch.float32), (1030, 1029, torch.float32), (1028, 1027, torch.bfloat16)],
                         ids=["V1030-blank513-float32", "V1030-blank1029-float32", "V1028-blank1027-bfloat16"])
def test_prefix_scores_beyond_1024_columns(kind, V, blank, dtype):
    T, N = 20, 9
    x, tl, plan = prefix_input(T, V, N, blank)
    toks = [c for c in range(V) if c != blank]
    assert {toks[0], toks[len(toks) // 2], toks[-1]} <= set(plan[:, :5].ravel().tolist()) and toks[-1] >= CH and blank in plan[:, 2]
    xt = torch.tensor(x).to(dtype).to(DEV)
    # (writable copies of tl and plan: the runner hands them to torch.as_tensor)
    TP.run_plan(kind, xt, np.array(tl), blank, N, np.array(plan), xf=xt.float().cpu().double().numpy(), what=f"d. {kind} T={T} V={V} N={N} blank={blank} {dtype}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", range(len(BEAM)), ids=lambda c: "B%d-T%d-V%d-W%d-K%d-n%d" % BEAM[c][0] + f"-blank{BEAM[c][1]}")
def test_beam_search_beyond_1024_columns(kind, c):
    (B, T, V, W, K, nbest), blank, seed, margin = BEAM[c]
    x, tl = TB.inputs(B, T, V, seed, blank)
    want = TB.reference(kind, B, T, V, W, K, nbest, seed, blank)
    assert tl[0] == T and np.all(want[3] >= 1e-6) and want[3].min() >= 0.99 * margin, want[3]
    tok = want[1][want[1] >= 0]
    assert np.any(tok >= CH) and not np.any(tok == blank) and (blank == V - 1 or (np.any(tok < blank) and np.any(tok > blank)))
    TB.check(TB.run(kind, 0, x, tl, blank, W, K, nbest), want, f"d. {kind} {BEAM[c][0]} blank={blank} seed {seed}")
