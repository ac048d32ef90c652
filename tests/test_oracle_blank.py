"""The blank index of the float64 oracles themselves (CPU only): the yardstick of tests/test_gpu_blank.py.

The reference's known answers pin the blank at column 0 and at a few other places.  Here every blank position is tied back to
column 0 without trusting the blank handling under test:
  * the C restatement against the NumPy oracle, blank in {0, 1, V//2, V-1};
  * column-permutation equivariance of each oracle on its own: with logits'[..., pi(k)] = logits[..., k], labels' = pi(labels),
    blank' = pi(blank) the loss is unchanged and grad'[..., pi(k)] = grad[..., k] -- for a random pi and for the transposition that
    swaps the blank with column 0;
  * the same for the best-path and the greedy oracle, on continuous random logits (no ties: "the lowest token" is not
    permutation-invariant).

Bound.  Both sides of every comparison are float64 sums of the same terms in another order.  Largest deviations measured over all
cases of this file (every test prints its own, pytest -s): C against NumPy 3.6e-15 on a loss and 6.1e-15 on a gradient entry;
permutation equivariance of either oracle 7.1e-15 on a loss and 7.55e-15 on a gradient entry; best-path scores 3.6e-15, greedy
scores 1.8e-15.  BOUND = 100 x the largest = 7.6e-13, absolute, on losses (up to ~40 nats here), gradient entries and scores
alike; integer results (paths, tokens, labels, frames) are compared exactly."""
import functools

import numpy as np
import pytest

from oracle import c_oracle as C
from oracle import ctc_oracle as O
from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO

KINDS = ["classic", "simplified"]
BOUND = 7.6e-13
T, U = 12, 5
VOCAB_BLANK = [(V, blank) for V in (5, 12) for blank in (0, 1, V // 2, V - 1)]


@functools.lru_cache(maxsize=None)
def case(V, blank):
    """Five utterances, ragged: 0 full with token 0 (blank != 0) and the blank's two neighbours, 1 a run of repeats, 2 an empty
    label, 3 infeasible (fewer frames than labels), 4 short.  Labels (padding included) never equal the blank."""
    rng = np.random.default_rng(100 * V + blank)
    logits = rng.standard_normal((5, T, V)).astype(np.float32)
    labels = rng.integers(0, V - 1, (5, U)).astype(np.int32)
    labels[labels >= blank] += 1
    others = [k for k in range(V) if k != blank]
    labels[0, 0] = others[0]  # token 0 whenever the blank is elsewhere
    labels[0, 1] = others[max(blank - 1, 0)]  # the column right before the blank (blank = 0: the first token)
    labels[0, 2] = others[min(blank, V - 2)]  # the column right after it (blank = V - 1: the last token)
    labels[1, :3] = labels[1, 0]
    ll = np.array([U, 4, 0, U, 2], np.int32)
    tl = np.array([T, T - 2, 7, U - 1, 5], np.int32)
    for a in (logits, labels, ll, tl):
        a.flags.writeable = False
    return logits, labels, ll, tl


def numpy_loss_grad(kind, labels, logits, ll, tl, blank):
    ref = O.ctc_loss(kind, labels, logits, ll, tl, blank)
    return ref.loss, O.logits_gradient(ref, logits)


ORACLES = {"numpy": numpy_loss_grad, "c": C.loss_grad}


def permutations(V, blank, rng):
    """pi as an array (pi[k] = new column of token k): a random one, and the transposition of the blank and column 0."""
    swap = np.arange(V)
    swap[[0, blank]] = swap[[blank, 0]]
    return [("random", rng.permutation(V)), ("blank<->0", swap)]


def permuted(logits, pi):
    out = np.empty_like(logits)
    out[..., pi] = logits
    return out


def deviation(a, b):
    """max |a - b| with equal infinities counting as 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    same = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    with np.errstate(invalid="ignore"):
        d = np.where(same, 0.0, np.abs(a - b))
    return float(d.max()) if d.size else 0.0


def check_loss_grad(got, want, what):
    (l1, g1), (l0, g0) = got, want
    assert np.array_equal(np.isfinite(l1), np.isfinite(l0)), (what, l1, l0)
    assert np.array_equal(np.isfinite(l0), [True, True, True, False, True]) and l0[3] == np.inf, (what, l0)
    dl, dg = deviation(l1, l0), deviation(g1, g0)
    print(f"ORACLE-BLANK {what}: loss deviation {dl:.3e}, gradient deviation {dg:.3e} (bound {BOUND:.1e})", flush=True)
    assert dl <= BOUND and dg <= BOUND, (what, dl, dg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank", VOCAB_BLANK)
def test_c_oracle_matches_numpy_oracle_at_every_blank(kind, V, blank):
    logits, labels, ll, tl = case(V, blank)
    assert blank == 0 or 0 in labels[0]
    want = numpy_loss_grad(kind, labels, logits, ll, tl, blank)
    got = C.loss_grad(kind, labels, logits, ll, tl, blank)
    check_loss_grad(got, want, f"C vs NumPy {kind} V={V} blank={blank}")
    assert np.all(want[1][3] == 0) and np.all(got[1][3] == 0)  # the infeasible utterance
    for b in range(5):  # nothing beyond logit_length
        assert np.all(want[1][b, tl[b]:] == 0) and np.all(got[1][b, tl[b]:] == 0)
    assert np.abs(want[1][0]).max() > 1e-3  # (the comparison is not one of zeros)


@pytest.mark.parametrize("oracle", list(ORACLES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank", VOCAB_BLANK)
def test_loss_and_gradient_are_equivariant_under_column_permutations(oracle, kind, V, blank):
    logits, labels, ll, tl = case(V, blank)
    fn = ORACLES[oracle]
    loss, grad = fn(kind, labels, logits, ll, tl, blank)
    for name, pi in permutations(V, blank, np.random.default_rng(V + blank)):
        loss_p, grad_p = fn(kind, pi[labels].astype(np.int32), permuted(logits, pi), ll, tl, int(pi[blank]))
        check_loss_grad((loss_p, grad_p[..., pi]), (loss, grad), f"{oracle} {kind} V={V} blank={blank} -> {int(pi[blank])} ({name})")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank", VOCAB_BLANK)
def test_best_path_oracle_is_equivariant(kind, V, blank):
    logits, labels, ll, tl = case(V, blank)
    score, paths = VO.best_path(kind, labels, logits, ll, tl, blank)
    assert [p is None for p in paths] == [False, False, False, True, False]
    for b, p in enumerate(paths):
        assert p is None or VO.reduces_to(kind, p, blank) == labels[b, :ll[b]].tolist()
    for name, pi in permutations(V, blank, np.random.default_rng(V + blank)):
        score_p, paths_p = VO.best_path(kind, pi[labels].astype(np.int32), permuted(logits, pi), ll, tl, int(pi[blank]))
        d = deviation(score_p, score)
        print(f"ORACLE-BLANK best path {kind} V={V} blank={blank} ({name}): score deviation {d:.3e} (bound {BOUND:.1e})", flush=True)
        assert d <= BOUND
        for p, q in zip(paths, paths_p):
            assert (p is None) == (q is None)
            assert p is None or np.array_equal(pi[p], q)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank", VOCAB_BLANK)
def test_greedy_oracle_is_equivariant(kind, V, blank):
    logits, _, _, tl = case(V, blank)
    logits = logits.copy()
    logits[..., blank] += 1.0  # blanks do occur on the argmax path
    want = GO.decode(kind, logits, tl, blank)
    assert (want.tokens == blank).any() and want.label_length.max() > 0
    for name, pi in permutations(V, blank, np.random.default_rng(V + blank)):
        got = GO.decode(kind, permuted(logits, pi), tl, int(pi[blank]))
        pad = lambda a: np.where(a >= 0, pi[np.maximum(a, 0)], -1)
        assert np.array_equal(got.tokens, pad(want.tokens)) and np.array_equal(got.labels, pad(want.labels))
        assert np.array_equal(got.label_length, want.label_length) and np.array_equal(got.frames, want.frames)
        d, dl = deviation(got.score, want.score), deviation(got.label_score, want.label_score)
        print(f"ORACLE-BLANK greedy {kind} V={V} blank={blank} ({name}): score deviation {d:.3e}, label score deviation {dl:.3e} "
              f"(bound {BOUND:.1e})", flush=True)
        assert d <= BOUND and dl <= BOUND
