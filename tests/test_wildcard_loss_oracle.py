"""Pins the float64 reference of the wildcard CTC loss (tests/tools/wildcard_loss_oracle.py) that the GPU tests compare against:
Z against brute-force enumeration of every state sequence, the gradient against central differences, the plain CTC oracle where
there is no wildcard, the best path as a lower bound, and the closed forms of the definition.  No GPU."""
import itertools

import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import wildcard_loss_oracle as WL
from tests.tools import wildcard_oracle as WB

W = WL.WILDCARD

# labels of at most three positions over tokens 1..3 (blank 0): adjacent wildcards, a wildcard first and last, a repeated label on
# both sides of a wildcard, repeated labels without one, no label at all
LABELS = [[], [W], [1], [W, W], [W, 1], [1, W], [1, 1], [1, 2], [W, 1, W], [1, W, 1], [2, W, 2], [W, W, 1], [1, W, W], [W, W, W],
          [1, 1, W], [W, 2, 2], [1, 2, 3], [2, 2, 2], [3, W, 1]]


def brute_force_z(kind, label, x, blank, wrt, weight):
    """Z by enumeration: every sequence of states of the header's lattice, one per frame, the product of their emissions."""
    lpx, _ = WL.emissions(x, wrt, weight)
    e = np.exp(lpx)
    T, V = x.shape
    L = len(label)
    wild = [k == W for k in label]
    col = [V if w else k for k, w in zip(label, wild)]
    total = 0.0
    if kind == "classic":
        S = 2 * L + 1
        ext = [blank if s % 2 == 0 else col[(s - 1) // 2] for s in range(S)]
        ends = {S - 1, S - 2} if L else {0}

        def step_ok(a, b):  # from state a (-1: before the first frame, which may start in state 0 or 1) to state b
            if a < 0:
                return b in (0, 1)
            if b == a or b == a + 1:
                return True
            if b == a + 2 and b % 2 == 1:
                i = (b - 1) // 2
                return label[i] != label[i - 1] or wild[i] or wild[i - 1]
            return False
        for seq in itertools.product(range(S), repeat=T):
            prev, ok, p = -1, True, 1.0
            for t, s in enumerate(seq):
                if not step_ok(prev, s):
                    ok = False
                    break
                p *= e[t, ext[s]]
                prev = s
            if ok and ((T == 0 and L == 0) or (T > 0 and prev in ends)):
                total += p
        return total
    # simplified: the state is the number of labels emitted; a frame either stays (blank, or e_w behind a wildcard) or enters the next
    for moves in itertools.product((0, 1), repeat=T):
        l, p = 0, 1.0
        for t, m in enumerate(moves):
            if m:
                if l == L:
                    p = 0.0
                    break
                p *= e[t, col[l]]
                l += 1
            else:
                p *= e[t, V if (l > 0 and wild[l - 1]) else blank]
        if l == L:
            total += p
    return total


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", WL.KINDS)
def test_z_equals_the_sum_over_every_state_sequence(kind, wrt):
    rng = np.random.default_rng(5)
    V, worst, feasible, infeasible = 4, 0.0, 0, 0
    for label in LABELS:
        for T in range(0, 7):
            for weight in (0.0, -0.7):
                x = rng.standard_normal((T, V)) * 2.0
                if wrt:
                    x = x - 0.3  # log-"probabilities" that do not sum to one: e_w carries their log-sum-exp
                z = brute_force_z(kind, label, x, 0, wrt, weight)
                loss, gamma, Gamma = WL.posteriors_one(kind, label, x, 0, wrt, weight)
                if z == 0.0:
                    assert loss == np.inf, (label, T)
                    infeasible += 1
                    continue
                feasible += 1
                rel = abs(np.exp(-loss) - z) / z
                worst = max(worst, rel)
                assert rel <= 1e-12, (kind, label, T, weight, rel)
                if T:
                    assert np.abs(gamma.sum(axis=1) + Gamma - 1.0).max() < 1e-12, "sum_k gamma + Gamma = 1"
    print(f"WILDCARD-LOSS-ORACLE {kind} wrt={wrt}: worst relative |Z - brute force| {worst:.3e} over {feasible} cases, {infeasible} infeasible")
    assert feasible > 100 and infeasible > 10


def case():
    rng = np.random.default_rng(3)
    B, T, V, U = 3, 7, 5, 4
    x = rng.standard_normal((B, T, V))
    tl = np.asarray([T, 4, 6], np.int32)
    labels = np.asarray([[W, 2, W, 2], [3, 3, W, W], [1, W, 4, -1]], np.int32)
    ll = np.asarray([4, 4, 3], np.int32)
    d = rng.standard_normal(B)
    return x, tl, labels, ll, d


@pytest.mark.parametrize("weight", [0.0, -0.7])
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", WL.KINDS)
def test_reference_gradient_matches_central_differences(kind, wrt, weight):
    x, tl, labels, ll, d = case()
    if wrt:
        x = O.logit_to_logproba(x, 2) - 0.2
    loss, grad = WL.loss_and_grad(kind, wrt, labels, x, ll, tl, 0, weight, d)
    fin = np.isfinite(loss)
    if kind == "classic":
        assert not fin[1] and fin[0] and fin[2], "3 3 * * needs five frames on the classic lattice (a blank between the equal labels), utterance 1 has four"
    else:
        assert fin.all()
    assert not np.isnan(grad).any()
    assert np.all(grad[1, 4:] == 0.0) and np.all(grad[2, 6:] == 0.0), "zeros beyond T_b"
    d_bad = d.copy()
    d_bad[~fin] = np.nan  # the d_loss of an infeasible utterance is not interpreted
    assert np.array_equal(WL.loss_and_grad(kind, wrt, labels, x, ll, tl, 0, weight, d_bad)[1], grad)

    def objective(xx):
        l, _ = WL.loss_and_grad(kind, wrt, labels, xx, ll, tl, 0, weight)
        return float((d * np.where(fin, l, 0.0))[fin].sum())
    h = 1e-5
    num = np.zeros_like(grad)
    for b in range(x.shape[0]):
        for t in range(int(tl[b])):
            for k in range(x.shape[2]):
                xp, xm = x.copy(), x.copy()
                xp[b, t, k] += h
                xm[b, t, k] -= h
                num[b, t, k] = (objective(xp) - objective(xm)) / (2 * h)
    err = float(np.abs(num - grad).max())
    print(f"WILDCARD-LOSS-ORACLE {kind} wrt={wrt} w={weight}: worst |central difference - reference| {err:.3e}")
    # central differences of step h: truncation h^2 |f'''| / 6 ~ 1e-10, rounding eps |f| / h ~ 1e-16 * 30 / 1e-5 = 3e-10
    assert err < 2e-9, err
    assert np.abs(grad).max() > 0.1, "a gradient to speak of"
    if not wrt:
        assert np.abs(grad.sum(axis=2)).max() < 1e-12, "sum_k grad[t, k] = 0 for logits"


@pytest.mark.parametrize("kind", WL.KINDS)
def test_without_a_wildcard_it_is_the_plain_ctc_oracle(kind):
    inp = O.generate_ctc_loss_inputs(5, 14, 1, 6, max_label_length=5)
    ref = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0)
    gref = O.logits_gradient(ref, inp["logits"])
    for weight in (0.0, -1.5):  # nothing reads the weight
        loss, grad = WL.loss_and_grad(kind, 0, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0, weight)
        fin = np.isfinite(ref.loss)
        assert np.array_equal(np.isfinite(loss), fin) and fin.any()
        assert np.abs(loss[fin] - ref.loss[fin]).max() < 1e-10
        assert np.abs(grad - gref).max() < 1e-10
    lp = O.logit_to_logproba(np.asarray(inp["logits"], np.float64), 2)
    loss1, grad1 = WL.loss_and_grad(kind, 1, inp["labels"], lp, inp["label_length"], inp["logit_length"], 0)
    assert np.abs(loss1[fin] - ref.loss[fin]).max() < 1e-10
    assert np.abs(grad1 - np.where(fin[:, None, None], ref.gradient, 0.0)).max() < 1e-10


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", WL.KINDS)
def test_the_best_path_is_one_of_the_summed_paths(kind, wrt):
    """With w = 0: -loss >= the score of wildcard_oracle.best_path, because m_t <= e_w(t) and the maximum is one term of the sum."""
    rng = np.random.default_rng(11)
    V, n = 5, 0
    for label in LABELS:
        for T in (1, 3, 6, 9):
            x = rng.standard_normal((T, V)) * 3.0
            if wrt:
                x = O.logit_to_logproba(x[None], 2)[0]
            score, _, _ = WB.best_path_one(kind, label, x, 0, wrt)
            loss, _, _ = WL.posteriors_one(kind, label, x, 0, wrt, 0.0)
            assert np.isfinite(score) == np.isfinite(loss), (label, T)
            if np.isfinite(score):
                n += 1
                assert -loss >= score - 1e-12, (kind, label, T, -loss, score)
    assert n > 40


@pytest.mark.parametrize("kind", WL.KINDS)
def test_closed_forms(kind):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 4, 6))
    # a lone wildcard on one frame: the loss is -w exactly, whatever the logits
    for weight in (0.0, -0.7, -3.25):
        loss, grad = WL.loss_and_grad(kind, 0, [[W]] * 3, x, [1, 1, 1], [1, 1, 1], 0, weight)
        assert np.array_equal(loss, np.full(3, -weight)), (loss, weight)
        assert np.all(grad == 0.0), "Gamma = 1: the logits do not matter"
    # ... and on log-probabilities -w - LSE of the row
    lp = x - 0.4
    loss, _ = WL.loss_and_grad(kind, 1, [[W]] * 3, lp, [1, 1, 1], [1, 1, 1], 0, -0.5)
    assert np.abs(loss - (0.5 - np.log(np.exp(lp[:, 0]).sum(axis=-1)))).max() < 1e-14
    # no label: the all-blank path; no frame: 0 for an empty transcript, +inf otherwise; each wildcard needs a frame of its own
    loss, _ = WL.loss_and_grad(kind, 0, [[W, W]] * 3, x, [0, 0, 2], [4, 0, 0], 0)
    lsm = O.logit_to_logproba(x, 2)
    assert abs(loss[0] + lsm[0, :, 0].sum()) < 1e-12 and loss[1] == 0.0 and loss[2] == np.inf
    loss, grad = WL.loss_and_grad(kind, 0, [[W, W, W]] * 3, x, [3, 3, 4], [2, 3, 4], 0)
    assert loss[0] == np.inf and np.isfinite(loss[1]) and loss[2] == np.inf, "too few frames; label_length > U"
    assert np.all(grad[0] == 0.0) and np.all(grad[2] == 0.0)
    # malformed labels: the blank, beyond V, a negative value other than the wildcard; a row of -inf
    for bad in (0, 6, -3, -1):
        loss, grad = WL.loss_and_grad(kind, 0, [[1, bad]] * 3, x, [2, 2, 2], [4, 4, 4], 0)
        assert np.all(loss == np.inf) and np.all(grad == 0.0), bad
    y = x.copy()
    y[1, 2] = -np.inf
    loss, grad = WL.loss_and_grad(kind, 0, [[W, 1]] * 3, y, [2, 2, 2], [4, 4, 4], 0)
    assert loss[1] == np.inf and np.isfinite(loss[[0, 2]]).all() and np.all(grad[1] == 0.0) and not np.isnan(grad).any()
