"""tests/tools/wildcard_oracle.py against brute force, against the wildcard-free Viterbi oracle and against the greedy oracle.
CPU only.

Brute force: every path in [0, V)^T (T <= 6, V <= 3) whose admissibility an independent recursive acceptor decides, written from the
prose of include/ctc_amd.h (ctc_amd_wildcard_best_path) and sharing nothing with the oracle's lattice.  A wildcard accepts any
tokens, so the maximum over admissible paths is what the definition calls the score (sum of row maxima on wildcard frames)."""
import itertools
from functools import lru_cache

import numpy as np
import pytest

from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO
from tests.tools import wildcard_oracle as WO

W = WO.WILDCARD


def accepts(kind, path, label, blank):
    """Does `path` (a tuple of tokens) spell `label` (tokens and wildcards) on the lattice `kind`?"""
    T, L = len(path), len(label)

    @lru_cache(maxsize=None)
    def rec(t, done, is_open):
        """Frames t.. remain; positions 0..done-1 are entered; is_open: frame t-1 belonged to position done-1."""
        if t == T:
            return done == L
        k = path[t]
        cur = label[done - 1] if done else None
        if kind == "classic":
            # one more frame of the open position: the same token again, or anything for a wildcard
            if is_open and (cur == W or k == cur) and rec(t + 1, done, True):
                return True
            # a blank outside any label (it also closes the open position)
            if k == blank and rec(t + 1, done, False):
                return True
            # the first frame of the next position; straight from an open one only if the two differ or one is a wildcard
            if done < L:
                nxt = label[done]
                if (nxt == W or k == nxt) and not (is_open and cur != W and nxt != W and cur == nxt):
                    if rec(t + 1, done + 1, True):
                        return True
            return False
        # simplified: a wildcard owns every frame from its entry until the next label's frame; elsewhere only blanks lie between
        if done and cur == W:
            if rec(t + 1, done, True):
                return True
        elif k == blank and rec(t + 1, done, False):
            return True
        if done < L:
            nxt = label[done]
            if (nxt == W or k == nxt) and rec(t + 1, done + 1, True):
                return True
        return False

    return rec(0, 0, False)


def brute_force(kind, label, lp, blank):
    T, V = lp.shape
    best = -np.inf
    for path in itertools.product(range(V), repeat=T):
        if accepts(kind, path, tuple(label), blank):
            best = max(best, float(sum(lp[t, k] for t, k in enumerate(path))))
    return best


def label_lists(V, blank):
    tok = [k for k in range(V) if k != blank]
    a, b = tok[0], tok[-1]
    return [[], [a], [a, b], [a, a], [b, a, b],                       # no wildcard
            [W], [W, a], [a, W], [a, W, b], [a, W, a], [a, a, W],      # one: lone, first, last, between equal and different labels
            [W, W], [W, a, W], [a, W, W], [W, W, a], [a, W, W, b], [W, a, a, W]]  # two: adjacent, both ends, all-wildcard


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("T,V", [(1, 3), (3, 3), (5, 3), (6, 3), (6, 2)])
def test_oracle_equals_brute_force(T, V, kind, blank):
    if blank >= V:
        blank = V - 1
    rng = np.random.default_rng(100 * T + 10 * V + blank)
    x = rng.standard_normal((T, V)).astype(np.float32)
    for wrt in (0, 1):
        xin = VO.log_softmax64(x).astype(np.float32) if wrt else x
        lp = np.asarray(xin, np.float64) if wrt else VO.log_softmax64(xin)
        for label in label_lists(V, blank):
            want = brute_force(kind, label, lp, blank)
            score, path, index = WO.best_path_one(kind, label, xin, blank, wrt)
            if want == -np.inf:
                assert score == -np.inf and path is None, (label, score)
                continue
            assert abs(score - want) <= 1e-12, (kind, label, score, want)
            assert accepts(kind, tuple(int(k) for k in path), tuple(label), blank), (kind, label, path)
            assert abs(WO.path_score(xin, path, wrt) - score) <= 1e-12
            for i, k in enumerate(label):  # every label has frames, contiguous, in order
                fr = np.nonzero(index == i)[0]
                assert len(fr) >= 1 and np.all(np.diff(fr) == 1)
                if k != W:
                    assert np.all(path[fr] == k)
            seq = index[index >= 0]
            assert np.all(np.diff(seq) >= 0) and np.all(path[index < 0] == blank)


@pytest.mark.parametrize("kind", VO.KINDS)
def test_without_wildcards_it_is_the_viterbi_oracle(kind):
    rng = np.random.default_rng(3)
    B, T, V, U = 6, 30, 7, 8
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, V, (B, U))
    ll = rng.integers(0, U + 1, B)
    tl = rng.integers(20, T + 1, B)
    ll[0], tl[1] = U + 1, 3  # beyond the tensor's width; too few frames
    for wrt in (0, 1):
        xin = VO.log_softmax64(x).astype(np.float32) if wrt else x
        vs, vp = VO.best_path(kind, labels, xin, ll, tl, 0, wrt)
        ws, wp, wi = WO.best_path(kind, labels, xin, ll, tl, 0, wrt)
        for b in range(B):
            if vp[b] is None:
                assert wp[b] is None and ws[b] == -np.inf
                continue
            assert abs(ws[b] - vs[b]) <= 1e-12
            assert abs(VO.path_score(xin[b, :tl[b]], wp[b], wrt) - VO.path_score(xin[b, :tl[b]], vp[b], wrt)) <= 1e-12
            assert VO.reduces_to(kind, wp[b], 0) == list(labels[b, :ll[b]])


@pytest.mark.parametrize("blank", [0, 4])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_lone_wildcard_is_the_greedy_path(kind, blank):
    rng = np.random.default_rng(5)
    B, T, V = 4, 25, 6
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tl = np.asarray([T, 1, 17, 9])
    labels = np.full((B, 1), W)
    for wrt in (0, 1):
        xin = VO.log_softmax64(x).astype(np.float32) if wrt else x
        dec = GO.decode(kind, xin, tl, blank, wrt)
        ws, wp, wi = WO.best_path(kind, labels, xin, np.ones(B, int), tl, blank, wrt)
        for b in range(B):
            assert abs(ws[b] - dec.score[b]) <= 1e-12
            assert np.array_equal(wp[b], dec.tokens[b, :tl[b]])


def test_infeasible_by_the_contract():
    x = np.zeros((4, 3), np.float32)
    for kind in VO.KINDS:
        assert WO.best_path_one(kind, [W, 1, W, 2, W], x)[0] == -np.inf        # five positions, four frames
        assert WO.best_path_one(kind, [W, 1, W, 2], x)[0] > -np.inf
        for bad in (0, -1, -3, 3):
            assert WO.best_path_one(kind, [W, bad], x)[0] == -np.inf
        assert WO.best_path_one(kind, [], x[:0])[0] == 0.0 and WO.best_path_one(kind, [W], x[:0])[0] == -np.inf
        y = x.copy()
        y[2] = -np.inf
        assert WO.best_path_one(kind, [W], y)[0] == -np.inf and WO.best_path_one(kind, [W], y, 0, 1)[0] == -np.inf
