"""The prefix beam search oracle (tests/tools/beam_oracle.py) against what it must equal when nothing is pruned: brute force over
all V^T paths, and -loss of the float64 loss oracle.  Plus one hand-computed case per lattice and the effect of the token cut.
No GPU."""
import itertools
import math

import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import beam_oracle as BO
from tests.tools.viterbi_oracle import KINDS, log_softmax64, reduces_to


def brute_force(kind, x, blank):
    """{labelling: summed probability of the paths that give it} over all V^T paths of x[T, V]."""
    T, V = x.shape
    p = np.exp(log_softmax64(x)) if T else None
    out = {}
    for path in itertools.product(range(V), repeat=T):
        m = 1.0
        for t, k in enumerate(path):
            m *= p[t, k]
        y = tuple(reduces_to(kind, path, blank))
        out[y] = out.get(y, 0.0) + m
    return out


@pytest.mark.parametrize("blank", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", [0, 1, 2, 3, 4, 5])
def test_unpruned_search_is_the_sum_over_all_paths(kind, T, blank):
    V = 3
    x = np.random.default_rng(10 * T + blank).standard_normal((T, V)).astype(np.float32) * 2.0
    want = brute_force(kind, x, blank)
    W = len(want)  # every prefix of a labelling is a labelling of this T, so no beam is ever larger
    res = BO.search_one(kind, x, blank, 0, W, V - 1, W)
    got = {h.labels: h.score for h in res.hyps}
    assert len(res.hyps) == len(got) and set(got) == set(want)
    for y, m in want.items():
        assert abs(got[y] - math.log(m)) <= 1e-12 * max(1.0, abs(math.log(m))), (y, got[y], math.log(m))
    scores = [h.score for h in res.hyps]
    assert scores == sorted(scores, reverse=True)
    # ... and -loss of the loss oracle, labelling by labelling
    ys = [h.labels for h in res.hyps]
    U = max(1, max(len(y) for y in ys))
    labels = np.full((len(ys), U), (blank + 1) % V, np.int32)
    for i, y in enumerate(ys):
        labels[i, :len(y)] = y
    ll = np.asarray([len(y) for y in ys], np.int32)
    xb = np.broadcast_to(x if T else np.zeros((1, V), np.float32), (len(ys), max(T, 1), V))
    loss = O.ctc_loss(kind, labels, xb, ll, np.full(len(ys), T, np.int32), blank).loss
    assert np.abs(-np.asarray(loss) - np.asarray(scores)).max() <= 1e-10, (loss, scores)


def test_hand_computed_classic():
    """T = 2, V = 3, blank 0, p = [[.5, .3, .2], [.4, .4, .2]]:
    ()     blank,blank                          .5*.4                      = .20
    (1)    1,blank + blank,1 + 1,1              .3*.4 + .5*.4 + .3*.4      = .44
    (2)    2,blank + blank,2 + 2,2              .2*.4 + .5*.2 + .2*.2      = .22
    (1,2)  1,2                                  .3*.2                      = .06
    (2,1)  2,1                                  .2*.4                      = .08
    (1,1) and (2,2) need a blank between the two labels: impossible in two frames."""
    x = np.log(np.asarray([[.5, .3, .2], [.4, .4, .2]])).astype(np.float32)
    res = BO.search_one("classic", x, 0, 1, 64, 2, 64)
    want = [((1,), .44), ((2,), .22), ((), .20), ((2, 1), .08), ((1, 2), .06)]
    assert [h.labels for h in res.hyps] == [y for y, _ in want]
    for h, (_, m) in zip(res.hyps, want):
        assert abs(h.score - math.log(m)) < 1e-6  # (the float32 logarithms above)
    assert abs(res.margin - (math.log(.22) - math.log(.20))) < 1e-6


def test_hand_computed_simplified():
    """The same p on the simplified lattice: every non-blank frame is a label.
    () .20;  (1) .3*.4 + .5*.4 = .32;  (2) .2*.4 + .5*.2 = .18;  (1,1) .12;  (1,2) .06;  (2,1) .08;  (2,2) .04"""
    x = np.log(np.asarray([[.5, .3, .2], [.4, .4, .2]])).astype(np.float32)
    res = BO.search_one("simplified", x, 0, 1, 64, 2, 64)
    want = [((1,), .32), ((), .20), ((2,), .18), ((1, 1), .12), ((2, 1), .08), ((1, 2), .06), ((2, 2), .04)]
    assert [h.labels for h in res.hyps] == [y for y, _ in want]
    for h, (_, m) in zip(res.hyps, want):
        assert abs(h.score - math.log(m)) < 1e-6


def test_the_beam_prunes_and_reports_its_margin():
    x = np.log(np.asarray([[.5, .3, .2], [.4, .4, .2]])).astype(np.float32)
    # W = 2: after frame 0 the beam is {(): .5, (1): .3} ((2): .2 is dropped, margin ln .3 - ln .2); frame 1 then gives
    # () .2, (1) .5*.4 + .3*.4 + .3*.4 = .44, (2) .5*.2 = .10, (1,2) .06 -> kept (1), (); margin ln .2 - ln .1
    res = BO.search_one("classic", x, 0, 1, 2, 2, 2)
    assert [h.labels for h in res.hyps] == [(1,), ()]
    assert abs(res.hyps[0].score - math.log(.44)) < 1e-6 and abs(res.hyps[1].score - math.log(.20)) < 1e-6
    assert abs(res.margin - (math.log(.3) - math.log(.2))) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_a_last_label_outside_the_cut_is_not_repeated(kind):
    """V = 4, K = 1.  Frame 0: token 1 is the one non-blank candidate.  Frame 1: token 2 is, so prefix (1) can neither repeat its
    label (classic) nor be extended by 1; token 3 is never considered."""
    p = np.asarray([[.4, .5, .05, .05], [.3, .2, .4, .1]])
    x = np.log(p).astype(np.float32)
    res = BO.search_one(kind, x, 0, 1, 64, 1, 64)
    got = {h.labels: math.exp(h.score) for h in res.hyps}
    want = {(): .4 * .3, (1,): .5 * .3, (2,): .4 * .4, (1, 2): .5 * .4}
    assert set(got) == set(want)
    for y in want:
        assert abs(got[y] - want[y]) < 1e-6, y
    full = {h.labels: math.exp(h.score) for h in BO.search_one(kind, x, 0, 1, 64, 3, 64).hyps}
    assert full[(1,)] > got[(1,)] + 0.05  # with the whole vocabulary (1) also takes blank,1 (and 1,1 on the classic lattice)


def test_ties_go_to_the_lowest_index_and_the_blank_is_no_candidate():
    row = np.asarray([9.0, 1.0, 2.0, 2.0, 2.0, -np.inf], np.float32)
    assert BO.candidates(row, 0, 2) == [2, 3]
    assert BO.candidates(row, 0, 32) == [2, 3, 4, 1, 5]
    assert BO.candidates(row, 3, 2) == [0, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_batch_form_lengths_and_missing_hypotheses(kind):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 6, 5)).astype(np.float32)
    x[3, 2, :] = -np.inf  # kills utterance 3's beam
    tl = np.asarray([6, 0, 9, 6], np.int32)
    score, labels, length, margin = BO.search(kind, x, tl, 0, 0, 8, 4, 3)
    assert score.shape == (4, 3) and labels.shape == (4, 3, 6) and length.shape == (4, 3) and margin.shape == (4,)
    assert score[1].tolist() == [0.0, -np.inf, -np.inf] and length[1].tolist() == [0, 0, 0] and np.all(labels[1] == -1)
    assert np.all(np.isneginf(score[3])) and np.all(labels[3] == -1) and np.all(length[3] == 0)
    assert np.all(np.isfinite(score[0])) and np.all(np.diff(score[0]) <= 0) and margin[0] > 0
    for n in range(3):
        assert np.all(labels[0, n, length[0, n]:] == -1) and np.all(labels[0, n, :length[0, n]] > 0)
    # a hypothesis' mass inside the beam is a lower bound of its labelling's probability
    loss = O.ctc_loss(kind, labels[0].clip(min=1), np.broadcast_to(x[0], (3, 6, 5)), length[0], np.full(3, 6, np.int32), 0).loss
    assert np.all(score[0] <= -np.asarray(loss) + 1e-12)
