"""tests/tools/window_oracle.py checked three ways, on the CPU: against an enumeration of every path of tiny lattices written from
the ownership rule alone (no dynamic programme), its gradient against central differences of its own loss, and with windows that
cover every frame against the three unwindowed oracles."""
import itertools

import numpy as np
import pytest

from tests.tools import label_posterior_oracle as PO
from tests.tools import wildcard_loss_oracle as LO
from tests.tools import wildcard_oracle as AO
from tests.tools import window_oracle as WO

W = WO.WILDCARD
BLANK = 0


def owner_sequences(kind, label, T):
    """Every path of the lattice as the frame owners it reports (-1: a blank frame), from the header's words alone."""
    L = len(label)
    wild = [k == W for k in label]
    if kind == "classic":
        # any sequence over {-1, 0 .. L-1} whose owned frames read 0 .. L-1 in contiguous runs, with a blank between two
        # neighbours that hold the same ordinary label
        for seq in itertools.product(range(-1, L), repeat=T):
            runs = [k for k, _ in itertools.groupby(seq)]
            if [k for k in runs if k >= 0] != list(range(L)):
                continue
            ok = True
            for a, b in zip(runs, runs[1:]):
                if a >= 0 and b >= 0 and label[a] == label[b] and not wild[a] and not wild[b]:
                    ok = False
            if ok:
                yield seq
    else:
        # L entry frames in ascending order; every other frame is a stay, owned by the wildcard it is behind, if any
        for entry in itertools.combinations(range(T), L):
            seq, s = [], 0
            for t in range(T):
                if s < L and entry[s] == t:
                    seq.append(s)
                    s += 1
                else:
                    seq.append(s - 1 if s >= 1 and wild[s - 1] else -1)
            yield tuple(seq)


def brute(kind, label, x, window, wrt, weight, blank=BLANK):
    """(Z, posterior[T, L], blank posterior[T], best score, {owners: score} of every path); emissions from first principles."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    lse = np.log(np.exp(x).sum(axis=1))
    lp = x if wrt else x - lse[:, None]
    L = len(label)
    Z, post, blk = 0.0, np.zeros((T, L)), np.zeros(T)
    best, scores = -np.inf, {}
    for seq in owner_sequences(kind, label, T):
        s_sum = s_max = 0.0
        for t, i in enumerate(seq):
            if i < 0:
                e_sum = e_max = lp[t, blank]
            elif not (window[i][0] <= t <= window[i][1]):
                e_sum = e_max = -np.inf
            elif label[i] == W:
                e_sum = weight + (lse[t] if wrt else 0.0)
                e_max = lp[t].max()
            else:
                e_sum = e_max = lp[t, label[i]]
            s_sum += e_sum
            s_max += e_max
        p = np.exp(s_sum)
        Z += p
        for t, i in enumerate(seq):
            if i >= 0:
                post[t, i] += p
            else:
                blk[t] += p
        scores[seq] = s_max
        best = max(best, s_max)
    return Z, post, blk, best, scores


CASES = [  # (label, T, window)
    ([1, 2], 5, [(0, 2), (2, 4)]),
    ([1, 1, 2], 6, [(0, 1), (2, 4), (3, 5)]),          # a repeated label: needs the blank between
    ([2, W, 2], 6, [(0, 3), (1, 4), (2, 5)]),          # a wildcard between two equal labels
    ([W, 3], 4, [(-3, 1), (1, 99)]),                   # bounds beyond the frames act as clipped
    ([1, 2, 3], 6, [(0, 5), (3, 2), (0, 5)]),          # an empty window: infeasible
    ([3], 3, [(1, 1)]),
    ([1, 2], 4, [(0, 0), (3, 3)]),                     # the blank frames between are free
    ([], 3, []),
]


def reblank(label, blank):
    """The labels of a case for another blank: a label equal to it becomes 0, which no case uses.  The map is injective on the
    labels, so equal neighbours, windows and feasibility stay as they are."""
    return [0 if k == blank else k for k in label]


def enumeration_case(kind, wrt, case, blank):
    label, T, window = CASES[case]
    label = reblank(label, blank)
    assert blank not in label
    rng = np.random.default_rng(100 * case + 10 * wrt + (kind == "classic"))
    x = rng.normal(0.0, 2.0, (T, 4))
    if wrt:
        x = x - np.log(np.exp(x).sum(axis=1, keepdims=True)) - rng.uniform(0.0, 0.5, (T, 1))  # sub-normalised log-probabilities
    weight = -0.3
    Z, post, blk, best, scores = brute(kind, label, x, window, wrt, weight, blank)
    win = np.asarray(window, dtype=np.int64).reshape(-1, 2)
    loss, p, q = WO.posterior_one(kind, label, x, win, blank, wrt, weight)
    score, path, index = WO.best_path_one(kind, label, x, win, blank, wrt)
    if Z == 0.0:
        assert case == 4
        assert loss == np.inf and score == -np.inf and path is None and not p.any() and not q.any()
        return
    assert abs(loss + np.log(Z)) < 1e-12 * max(1.0, abs(np.log(Z)))
    np.testing.assert_allclose(p, post / Z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(q, blk / Z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(p.sum(axis=1) + q, 1.0, rtol=0, atol=1e-12)
    assert abs(score - best) < 1e-12 * max(1.0, abs(best))
    # the reported owners are a path of the lattice and attain the maximum (a wildcard frame whose best token is the blank ties
    # with a blank frame, so the maximiser need not be unique; where it is, this pins it)
    assert scores[tuple(int(i) for i in index)] == best
    for t, i in enumerate(index):
        if i >= 0:
            assert window[i][0] <= t <= window[i][1]
            assert path[t] == (np.asarray(x, np.float32)[t].argmax() if label[i] == W else label[i])
        else:
            assert path[t] == blank


@pytest.mark.parametrize("kind", WO.KINDS)
@pytest.mark.parametrize("wrt", (0, 1))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_against_enumeration(kind, wrt, case):
    enumeration_case(kind, wrt, case, BLANK)


@pytest.mark.parametrize("kind", WO.KINDS)
@pytest.mark.parametrize("wrt", (0, 1))
@pytest.mark.parametrize("blank", (3, 2, 1), ids=("blank=V-1", "blank=2", "blank=1"))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_against_enumeration_at_a_nonzero_blank(kind, wrt, blank, case):
    """The same cases and logits with the blank in the last column (V = 4) and in either interior one."""
    enumeration_case(kind, wrt, case, blank)


@pytest.mark.parametrize("kind", WO.KINDS)
@pytest.mark.parametrize("wrt", (0, 1))
def test_gradient_is_the_derivative_of_the_loss(kind, wrt):
    rng = np.random.default_rng(7 + wrt)
    B, T, V, U = 2, 7, 5, 3
    x = rng.normal(0.0, 1.5, (B, T, V))
    labels = np.asarray([[1, W, 1], [2, 2, 4]])
    ll, tl = np.asarray([3, 2]), np.asarray([7, 6])
    window = np.asarray([[(0, 2), (1, 5), (3, 6)], [(0, 3), (2, 5), (0, 0)]])
    d_loss = np.asarray([0.7, -1.3])
    loss, grad = WO.loss_and_grad(kind, wrt, labels, x, ll, tl, window, BLANK, -0.2, d_loss)
    assert np.isfinite(loss).all()
    num = np.zeros_like(x)
    h = 1e-6
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        lp_ = WO.loss_and_grad(kind, wrt, labels, xp, ll, tl, window, BLANK, -0.2)[0]
        lm_ = WO.loss_and_grad(kind, wrt, labels, xm, ll, tl, window, BLANK, -0.2)[0]
        num[idx] = ((lp_ - lm_) * d_loss).sum() / (2 * h)
    np.testing.assert_allclose(grad, num, rtol=0, atol=2e-8)
    assert not grad[1, 6].any()  # beyond logit_length


@pytest.mark.parametrize("kind", WO.KINDS)
def test_weighted_gradient_is_the_derivative_of_the_weighted_loss_at_a_nonzero_blank(kind):
    """loss_and_grad(..., d_loss=d) against central differences of sum(d * loss), d with a zero and a negative entry, the blank in
    the last column (V = 5) and in an interior one."""
    B, T, V, U = 3, 7, 5, 3
    ll, tl = np.asarray([3, 2, 3]), np.asarray([7, 6, 7])
    window = np.asarray([[(0, 2), (1, 5), (3, 6)], [(0, 3), (2, 5), (0, 0)], [(0, 3), (1, 5), (2, 6)]])
    d_loss = np.asarray([0.0, -1.3, 0.7])
    h = 1e-6
    for wrt in (0, 1):
        for blank in (V - 1, 2):
            x = np.random.default_rng(70 + 10 * wrt + blank).normal(0.0, 1.5, (B, T, V))
            labels = np.asarray([reblank(r, blank) for r in ([1, W, 1], [2, 2, 4], [4, 3, W])])
            assert not (labels == blank).any()
            loss, grad = WO.loss_and_grad(kind, wrt, labels, x, ll, tl, window, blank, -0.2, d_loss)
            assert np.isfinite(loss).all()
            num = np.zeros_like(x)
            for idx in np.ndindex(*x.shape):
                xp, xm = x.copy(), x.copy()
                xp[idx] += h
                xm[idx] -= h
                lp_ = WO.loss_and_grad(kind, wrt, labels, xp, ll, tl, window, blank, -0.2)[0]
                lm_ = WO.loss_and_grad(kind, wrt, labels, xm, ll, tl, window, blank, -0.2)[0]
                num[idx] = ((lp_ - lm_) * d_loss).sum() / (2 * h)
            np.testing.assert_allclose(grad, num, rtol=0, atol=2e-8)
            assert not grad[0].any() and grad[1].any() and grad[2].any()  # the zero weight: exactly zero
            assert not grad[1, 6].any()  # beyond logit_length


@pytest.mark.parametrize("kind", WO.KINDS)
@pytest.mark.parametrize("wrt", (0, 1))
def test_all_covering_windows_are_the_unwindowed_oracles(kind, wrt):
    rng = np.random.default_rng(31 + wrt)
    B, T, V, U = 4, 11, 6, 4
    x = rng.normal(0.0, 2.0, (B, T, V))
    labels = np.asarray([[1, 2, 2, 3], [W, 4, W, 0], [5, 5, 5, 5], [1, W, W, 2]])
    ll, tl = np.asarray([4, 3, 4, 4]), np.asarray([11, 9, 6, 3])  # (the third: too few frames on the classic lattice; the last: too few)
    full = WO.full_window(B, U, T)
    for window in (None, full):
        loss, grad = WO.loss_and_grad(kind, wrt, labels, x, ll, tl, window, BLANK, -0.4)
        rl, rg = LO.loss_and_grad(kind, wrt, labels, x, ll, tl, BLANK, -0.4)
        np.testing.assert_allclose(loss, rl, rtol=1e-13, atol=0)
        np.testing.assert_allclose(grad, rg, rtol=0, atol=1e-13)
        got = WO.label_posterior(kind, wrt, labels, x, ll, tl, window, BLANK, -0.4)
        ref = PO.label_posterior(kind, wrt, labels, x, ll, tl, BLANK, -0.4)
        for g, r in zip(got, ref):
            np.testing.assert_allclose(g, r, rtol=1e-12, atol=1e-13)
        score, paths, indices = WO.best_path(kind, labels, x, ll, tl, window, BLANK, wrt)
        rs, rp, ri = AO.best_path(kind, labels, x, ll, tl, BLANK, wrt)
        np.testing.assert_allclose(score, rs, rtol=1e-13, atol=0)
        for a, b, c, d in zip(paths, rp, indices, ri):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a, b) and np.array_equal(c, d)
    assert np.isinf(loss).any() and np.isfinite(loss).any()
