"""Pins tests/tools/optional_wildcard_oracle.py by the equivalence of include/ctc_amd.h: the state sequences of a transcript with
optional wildcards are the disjoint union, over all subsets of the optional positions, of those of the transcript with that
subset deleted and the remaining optional wildcards made mandatory.  So Z is the sum of the reduced transcripts' Z and gradients
and posteriors are the Z-weighted mixtures -- computed here with the EXISTING oracles of the mandatory wildcard.  CPU only."""
import itertools

import numpy as np
import pytest

from tests.tools import label_posterior_oracle as PO
from tests.tools import optional_wildcard_oracle as OO
from tests.tools import wildcard_loss_oracle as WO
from tests.tools import wildcard_oracle as VO

W, Q = OO.WILDCARD, OO.OPTIONAL
TOL = 1e-10  # loss, gradient and posteriors
TOL_SCORE = 1e-12  # the best path's score


def _x(T, V, seed, wrt):
    x = np.random.default_rng(seed).normal(0.0, 2.0, (T, V))
    return x - 0.3 if wrt else x  # (log-probabilities used as they stand need not be normalised)


def _mixture(kind, label, x, blank, wrt, weight):
    """(loss, grad[T, V], label_posterior[T, L], blank_posterior[T]) from the existing oracles over all subsets."""
    T, V = x.shape
    L = len(label)
    opts = [i for i, k in enumerate(label) if k == Q]
    terms = []
    for r in range(len(opts) + 1):
        for drop in itertools.combinations(opts, r):
            keep = [i for i in range(L) if i not in drop]
            red = np.asarray([W if label[i] == Q else label[i] for i in keep], dtype=np.int64)
            loss, grad = WO.loss_and_grad(kind, wrt, red[None, :], x[None], [len(keep)], [T], blank, weight)
            l2, p, q, _, _ = PO.posterior_one(kind, red, x, blank, wrt, weight)
            assert (np.isinf(loss[0]) and np.isinf(l2)) or abs(loss[0] - l2) < 1e-12
            post = np.zeros((T, L))
            if np.isfinite(l2) and T:
                post[:, keep] = p
            terms.append((loss[0], grad[0], post, q))
    logz = np.logaddexp.reduce([-t[0] for t in terms])
    if not np.isfinite(logz):
        return np.inf, np.zeros((T, V)), np.zeros((T, L)), np.zeros(T)
    w = [np.exp(-t[0] - logz) for t in terms]
    return (-logz, sum(wi * t[1] for wi, t in zip(w, terms)), sum(wi * t[2] for wi, t in zip(w, terms)),
            sum(wi * t[3] for wi, t in zip(w, terms)))


def _check(kind, label, T, V, wrt, weight, seed=0, blank=0):
    x = _x(T, V, seed, wrt)
    lab = np.asarray(label, dtype=np.int64)
    ref_loss, ref_grad, ref_post, ref_blk = _mixture(kind, list(label), x, blank, wrt, weight)
    loss, grad = OO.loss_and_grad(kind, wrt, lab[None, :], x[None], [len(label)], [T], blank, weight)
    l2, post, blk, dur, exf = OO.label_posterior(kind, wrt, lab[None, :], x[None], [len(label)], [T], blank, weight)
    if np.isinf(ref_loss):
        assert np.isinf(loss[0]) and np.isinf(l2[0]) and not grad.any() and not post.any()
        return False
    assert abs(loss[0] - ref_loss) < TOL and abs(l2[0] - ref_loss) < TOL
    assert np.abs(grad[0] - ref_grad).max(initial=0.0) < TOL
    assert np.abs(post[0] - ref_post).max(initial=0.0) < TOL
    assert np.abs(blk[0] - ref_blk).max(initial=0.0) < TOL
    if T:
        assert np.abs(post[0].sum(axis=1) + blk[0] - 1.0).max() < TOL  # a frame's values sum to 1
    assert ((dur[0] >= 0) & (dur[0] <= T + TOL)).all()
    assert ((exf[0] == -1.0) == (dur[0] == 0.0)).all()
    return True


CASES = {
    "first": ([Q, 1, 2], 6),
    "last": ([1, 2, Q], 6),
    "between_equal": ([2, Q, 2], 6),
    "beside_mandatory_before": ([1, W, Q, 2], 7),
    "beside_mandatory_behind": ([1, Q, W, 2], 7),
    "lone": ([Q], 4),
    "both_ends_and_middle": ([Q, 1, 1, Q, 3, Q], 8),
    "stc": ([Q, 1, Q, 2, Q, 2, Q, 3, Q], 7),  # T < 2L + 1 for the four labels' 9 positions
    "six_optional": ([Q, 1, Q, 1, Q, 2, Q, W, Q, 3, Q], 9),
}


@pytest.mark.parametrize("weight", [0.0, -0.7])
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_mixture_over_subsets(name, kind, wrt, weight):
    label, T = CASES[name]
    assert _check(kind, label, T, 5, wrt, weight, seed=len(name))


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", OO.KINDS)
def test_no_frames(kind, wrt):
    """T = 0 is feasible, with loss 0, for an empty label and for a single optional wildcard; for nothing else."""
    for label, ok in (([], True), ([Q], True), ([W], False), ([1], False), ([Q, 1], False), ([1, Q], False)):
        loss, _ = OO.loss_and_grad(kind, wrt, np.asarray(label, dtype=np.int64).reshape(1, -1), np.zeros((1, 0, 4)), [len(label)], [0])
        assert (loss[0] == 0.0) if ok else np.isinf(loss[0]), label
        assert _check(kind, label, 0, 4, wrt, 0.0) == ok


@pytest.mark.parametrize("kind", OO.KINDS)
def test_one_frame_short_of_feasible(kind):
    """The frames an utterance needs do not count optional wildcards: [1, ?, 1] needs 2 on the simplified lattice (1 1) and 3 on
    the classic one (1 blank 1, or 1 ? 1 with the star used): one frame fewer is infeasible, in the mixture as well."""
    need = 3 if kind == "classic" else 2
    assert _check(kind, [1, Q, 1], need, 4, 0, 0.0)
    assert not _check(kind, [1, Q, 1], need - 1, 4, 0, 0.0)
    assert _check(kind, [Q, 1, Q, 2, Q], 2, 4, 0, -0.7)
    assert not _check(kind, [Q, 1, Q, 2, Q], 1, 4, 0, -0.7)


@pytest.mark.parametrize("kind", OO.KINDS)
def test_adjacent_optional_wildcards_are_infeasible(kind):
    for label in ([Q, Q], [1, Q, Q, 2], [Q, Q, 1]):
        loss, grad = OO.loss_and_grad(kind, 0, np.asarray([label]), _x(8, 5, 1, 0)[None], [len(label)], [8])
        assert np.isinf(loss[0]) and not grad.any()
    loss, _ = OO.loss_and_grad(kind, 0, np.asarray([[1, Q, W, Q, 2]]), _x(8, 5, 1, 0)[None], [5], [8])
    assert np.isfinite(loss[0])  # a mandatory wildcard between them separates them


@pytest.mark.parametrize("weight", [0.0, -0.7])
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", OO.KINDS)
def test_without_an_optional_wildcard_it_is_the_existing_oracle(kind, wrt, weight):
    x = _x(9, 6, 3, wrt)
    lab = np.asarray([[W, 1, 1, 2, W, 3]])
    a = WO.loss_and_grad(kind, wrt, lab, x[None], [6], [9], 0, weight)
    b = OO.loss_and_grad(kind, wrt, lab, x[None], [6], [9], 0, weight)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for u, v in zip(PO.label_posterior(kind, wrt, lab, x[None], [6], [9], 0, weight), OO.label_posterior(kind, wrt, lab, x[None], [6], [9], 0, weight)):
        assert np.array_equal(u, v)


def test_non_zero_blank_and_bad_labels():
    assert _check("classic", [Q, 0, 1, Q], 6, 4, 0, -0.7, blank=3)
    assert _check("simplified", [0, Q, 0], 5, 4, 1, 0.0, blank=2)
    for bad in ([1, 0, Q], [1, 7, Q], [1, -4, Q]):
        assert np.isinf(OO.loss_and_grad("classic", 0, np.asarray([bad]), _x(6, 5, 0, 0)[None], [3], [6])[0][0])


def _check_path(kind, label, T, V, wrt, seed=0, blank=0):
    """The best path: its score is the best over the reduced transcripts (existing wildcard_oracle), the path is admissible for the
    reduced transcript that its own used positions name and worth what it claims, and the per-label outputs add up."""
    x = _x(T, V, seed, wrt)
    L = len(label)
    opts = [i for i, k in enumerate(label) if k == Q]
    best = -np.inf
    for r in range(len(opts) + 1):
        for drop in itertools.combinations(opts, r):
            red = [W if label[i] == Q else label[i] for i in range(L) if i not in drop]
            best = max(best, VO.best_path_one(kind, np.asarray(red, dtype=np.int64), x, blank, wrt)[0])
    score, path, index, first, last, lscore = OO.best_path_one(kind, label, x, blank, wrt)
    if np.isinf(best):
        assert np.isinf(score) and path is None
        return False
    assert abs(score - best) <= TOL_SCORE
    lp = VO._lp(x, wrt)
    assert abs(sum(lp[t, path[t]] for t in range(T)) - score) <= 1e-10
    used = [i for i in range(L) if first[i] >= 0]
    assert all(label[i] == Q for i in range(L) if i not in used)
    assert all(lscore[i] == 0.0 and last[i] == -1 for i in range(L) if i not in used)
    assert abs(sum(lscore) + sum(lp[t, blank] for t in range(T) if index[t] < 0) - score) <= 1e-10
    # the same path through the existing oracle's eyes: the reduced transcript of the used positions scores no less
    red = np.asarray([W if label[i] == Q else label[i] for i in used], dtype=np.int64)
    assert VO.best_path_one(kind, red, x, blank, wrt)[0] >= score - TOL_SCORE
    order = [i for t, i in enumerate(index) if i >= 0 and (t == 0 or index[t - 1] != i)]
    assert order == used  # every used position once, in order
    return True


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_best_path_is_the_best_over_subsets(name, kind, wrt):
    label, T = CASES[name]
    for seed in range(3):
        assert _check_path(kind, label, T, 5, wrt, seed=seed)


@pytest.mark.parametrize("kind", OO.KINDS)
def test_best_path_edges(kind):
    need = 3 if kind == "classic" else 2
    assert _check_path(kind, [1, Q, 1], need, 4, 0) and not _check_path(kind, [1, Q, 1], need - 1, 4, 0)
    assert _check_path(kind, [], 0, 4, 0) and _check_path(kind, [Q], 0, 4, 0) and not _check_path(kind, [1, Q], 0, 4, 0)
    assert OO.best_path_one(kind, [Q], np.zeros((0, 4)))[5][0] == 0.0
    for label in ([Q, Q], [1, Q, Q, 2]):
        assert np.isinf(OO.best_path_one(kind, label, _x(8, 5, 1, 0))[0])
    assert _check_path(kind, [Q, 0, 1, Q], 6, 4, 0, blank=3)
    x, lab = _x(9, 6, 3, 0), [W, 1, 1, 2, W, 3]  # no optional wildcard: the existing oracle exactly
    a, b = VO.best_path_one(kind, np.asarray(lab), x), OO.best_path_one(kind, lab, x)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", OO.KINDS)
def test_weighted_gradient_at_the_last_blank(kind, wrt):
    """blank = V - 1 and a d_loss with a zero and a negative value: the gradient is d_loss[b] times the unweighted mixture over
    subsets (the GPU tests of d_loss rest on the oracle's weighted gradient)."""
    V, T, blank, weight = 5, 8, 4, -0.7
    labs = ([Q, 0, 1, Q, 3], [2, Q, 2, W, 0], [0, 1, Q])
    d_loss = np.asarray([0.0, -1.5, 2.5])
    x = np.stack([_x(T, V, 40 + b, wrt) for b in range(3)])
    labels = np.full((3, 5), 1, dtype=np.int64)
    for b, lab in enumerate(labs):
        labels[b, :len(lab)] = lab
    ll = [len(lab) for lab in labs]
    loss, grad = OO.loss_and_grad(kind, wrt, labels, x, ll, [T] * 3, blank, weight, d_loss)
    plain = OO.loss_and_grad(kind, wrt, labels, x, ll, [T] * 3, blank, weight)
    assert np.array_equal(loss, plain[0])  # the loss is unaffected by d_loss
    for b, lab in enumerate(labs):
        ref_loss, ref_grad, _, _ = _mixture(kind, lab, x[b], blank, wrt, weight)
        assert np.isfinite(ref_loss) and abs(loss[b] - ref_loss) < TOL and np.abs(ref_grad).max() > 1e-3
        assert np.abs(grad[b] - d_loss[b] * ref_grad).max() < TOL
    assert not grad[0].any()
