"""The float64 oracle of the star that excludes the label behind it (tests/tools/star_exclusion_oracle.py), pinned three ways: by
enumeration of every state sequence at T <= 6, U <= 3, V = 4; by central differences of its own loss; and by equality with the
existing oracles when nothing is excluded.  No GPU."""
import itertools

import numpy as np
import pytest

from tests.tools import optional_wildcard_oracle as OO
from tests.tools import star_exclusion_oracle as SO

W, O = SO.WILDCARD, SO.OPTIONAL
V, BLANK = 4, 0
TRANSCRIPTS = [[W, 2], [2, W, 2], [W, W, 1], [1, W], [O, 2], [3, O, 3], [W, O, 2], [O, 1, W], [2, 2], [W]]


def _emissions(label, lp, weight):
    """Per position of the ORIGINAL transcript: (sum emission[T], max emission[T]), the wildcard's over the tokens it may emit."""
    out = []
    for i, k in enumerate(label):
        if k >= 0:
            out.append((lp[:, k], lp[:, k]))
            continue
        nxt = label[i + 1] if i + 1 < len(label) else -1
        keep = [q for q in range(V) if not (nxt >= 0 and q == nxt)]
        out.append((weight + np.log(np.exp(lp[:, keep]).sum(axis=1)), lp[:, keep].max(axis=1)))
    return out


def _paths(kind, kept, label, T):
    """Every state sequence of the transcript made of the positions `kept` (all mandatory): per frame the position that owns it,
    -1 for the blank."""
    n = len(kept)
    if kind == "simplified":  # the frames at which the positions are entered; a wildcard owns the stays behind it too
        for enter in itertools.combinations(range(T), n):
            own, cur = [], -1
            for t in range(T):
                if cur + 1 < n and enter[cur + 1] == t:
                    cur += 1
                    own.append(kept[cur])
                else:
                    own.append(kept[cur] if cur >= 0 and label[kept[cur]] < 0 else -1)
            yield own
        return
    for own in itertools.product(range(-1, n), repeat=T):
        seen = [q for q, _ in itertools.groupby(own) if q >= 0]
        if seen != list(range(n)):
            continue
        ok = True
        for t in range(1, T):  # open -> open of the next position: only if the labels differ or either is a wildcard
            a, b = own[t - 1], own[t]
            if a >= 0 and b == a + 1 and label[kept[a]] == label[kept[b]] and label[kept[a]] >= 0:
                ok = False
        if ok:
            yield [kept[q] if q >= 0 else -1 for q in own]


def _enumerate(kind, label, lp, weight):
    """(-ln Z, label_posterior[T, L], best score) over the disjoint union, over the subsets of optional positions, of the paths."""
    T, L = lp.shape[0], len(label)
    em = _emissions(label, lp, weight)
    opts = [i for i, k in enumerate(label) if k == O]
    z, post, best = 0.0, np.zeros((T, L)), -np.inf
    for r in range(len(opts) + 1):
        for gone in itertools.combinations(opts, r):
            kept = [i for i in range(L) if i not in gone]
            for own in _paths(kind, kept, label, T):
                w = np.exp(sum(em[i][0][t] if i >= 0 else lp[t, BLANK] for t, i in enumerate(own)))
                best = max(best, sum(em[i][1][t] if i >= 0 else lp[t, BLANK] for t, i in enumerate(own)))
                z += w
                for t, i in enumerate(own):
                    if i >= 0:
                        post[t, i] += w
    return -np.log(z), post / z, best


@pytest.mark.parametrize("kind", SO.KINDS)
@pytest.mark.parametrize("label", TRANSCRIPTS, ids=str)
def test_enumeration(kind, label):
    rng = np.random.default_rng(len(label) * 7 + sum(label) % 5)
    for T in (3, 6):
        x = rng.normal(size=(T, V)) * 2.0
        lp = SO.log_probs(x, 0)
        loss, post, best = _enumerate(kind, label, lp, -0.3)
        got = SO.posteriors_one(kind, label, x, BLANK, 0, -0.3)
        assert abs(got[0] - loss) < 1e-10
        assert np.abs(got[3] - post).max() < 1e-10
        assert np.abs(got[3].sum(axis=1) + got[4] - 1.0).max() < 1e-12
        assert abs(SO.best_path_one(kind, label, x, BLANK, 0)[0] - best) < 1e-10


@pytest.mark.parametrize("wrt", (0, 1))
@pytest.mark.parametrize("kind", SO.KINDS)
def test_gradient_is_the_derivative_of_the_loss(kind, wrt):
    rng = np.random.default_rng(3)
    labels = np.asarray([[W, 2, W, 2], [O, 1, W, 3], [2, W, W, 1]])
    ll, tl = np.asarray([4, 4, 4]), np.asarray([7, 6, 7])
    x = rng.normal(size=(3, 7, V)) * 1.5
    x[0, 1, 2] += 9.0  # a confident frame of the excluded token
    if wrt:
        x = x - np.log(np.exp(x).sum(axis=-1, keepdims=True)) - 0.2  # (not normalised on purpose)
    d = np.asarray([1.0, -0.5, 2.0])
    _, grad = SO.loss_and_grad(kind, wrt, labels, x, ll, tl, BLANK, -0.2, d)
    f = lambda z: float((SO.loss_and_grad(kind, wrt, labels, z, ll, tl, BLANK, -0.2)[0] * d).sum())
    num = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        e = np.zeros_like(x)
        e[idx] = 1e-6
        num[idx] = (f(x + e) - f(x - e)) / 2e-6
    assert np.abs(grad - num).max() < 1e-7
    assert np.all(grad[1, 6:] == 0.0)


@pytest.mark.parametrize("wrt", (0, 1))
@pytest.mark.parametrize("kind", SO.KINDS)
def test_nothing_excluded_is_the_existing_oracle(kind, wrt):
    rng = np.random.default_rng(5)
    labels = np.asarray([[W, 2, O, 1], [3, W, W, 0], [1, O, W, 0], [2, 3, W, 0]])  # (the stars of rows 1.. have no ordinary successor)
    ll, tl = np.asarray([4, 3, 3, 3]), np.asarray([8, 8, 5, 8])
    x = rng.normal(size=(4, 8, V))
    for exclude, rows in ((False, slice(0, 4)), (True, slice(1, 4))):
        a = SO.loss_and_grad(kind, wrt, labels[rows], x[rows], ll[rows], tl[rows], BLANK, -0.1, exclude=exclude)
        b = OO.loss_and_grad(kind, wrt, labels[rows], x[rows], ll[rows], tl[rows], BLANK, -0.1)
        assert np.abs(a[0] - b[0]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12
        a = SO.label_posterior(kind, wrt, labels[rows], x[rows], ll[rows], tl[rows], BLANK, -0.1, exclude=exclude)
        b = OO.label_posterior(kind, wrt, labels[rows], x[rows], ll[rows], tl[rows], BLANK, -0.1)
        assert all(np.abs(p - q).max() < 1e-12 for p, q in zip(a, b))
        sa, ra = SO.best_path(kind, labels[rows], x[rows], ll[rows], tl[rows], BLANK, wrt, exclude=exclude)
        sb, rb = OO.best_path(kind, labels[rows], x[rows], ll[rows], tl[rows], BLANK, wrt)
        assert np.abs(sa - sb).max() < 1e-12
        assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[2], q[2]) for p, q in zip(ra, rb))
