"""The CTC prefix score oracle (tests/tools/prefix_oracle.py) against enumeration of all V^T paths, and its full score against
-loss of the float64 loss oracle.  No GPU."""
import itertools
import math

import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import prefix_oracle as PO

KINDS = ("classic", "simplified")


def close(log_got, mass_want):
    """ln of a mass against the mass: -inf and 0 count as equal."""
    if mass_want == 0.0:
        return log_got == -np.inf
    return abs(math.exp(log_got) - mass_want) <= 1e-9


def same_log(a, b):
    return (a == -np.inf and b == -np.inf) or abs(a - b) <= 1e-9


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 4, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_every_prefix_against_enumeration(kind, T, blank):
    V = 3
    rng = np.random.default_rng(100 * T + blank)
    lp = PO.log_softmax(rng.standard_normal((T, V)) * 2.0)
    seqs = PO.enumerate_sequences(kind, lp, T, blank)
    assert abs(sum(seqs.values()) - 1.0) < 1e-12
    tokens = [c for c in range(V) if c != blank]
    for m in range(0, 5):
        for g in itertools.product(tokens, repeat=m):
            st = PO.state_of(kind, lp, T, blank, g)
            assert close(PO.full_score(st), seqs.get(g, 0.0)), (g, "full score")
            sc = PO.scores(kind, lp, T, blank, st)
            assert sc[blank] == -np.inf
            for c in tokens:
                assert close(sc[c], PO.prefix_mass(seqs, g + (c,))), (g, c, "psi")
            # psi(g) = P(g) + sum_c psi(g . c); psi of the empty prefix is 1
            if m == 0:
                psi_g = 0.0
            else:
                psi_g = PO.scores(kind, lp, T, blank, PO.state_of(kind, lp, T, blank, g[:-1]))[g[-1]]
            assert same_log(psi_g, PO.lse(PO.full_score(st), *sc)), (g, "identity")


@pytest.mark.parametrize("kind", KINDS)
def test_impossible_candidates_and_no_frames(kind):
    lp = PO.log_softmax(np.random.default_rng(1).standard_normal((4, 5)))
    st = PO.state_of(kind, lp, 4, 0, (2,))
    for c in (0, -1, 5):
        assert PO.extend(kind, lp, 4, 0, st, c) is None
    assert (PO.scores(kind, lp, 4, 0, None) == -np.inf).all() and PO.full_score(None) == -np.inf
    e = PO.empty_state(lp, 0, 0)
    assert PO.full_score(e) == 0.0 and (PO.scores(kind, lp, 0, 0, e) == -np.inf).all()
    assert PO.full_score(PO.extend(kind, lp, 0, 0, e, 3)) == -np.inf


@pytest.mark.parametrize("kind", KINDS)
def test_full_score_is_minus_loss(kind):
    inp = O.generate_ctc_loss_inputs(6, 14, 7, 6, max_label_length=5)
    ref = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0).loss
    for b in range(6):
        Tb, L = int(inp["logit_length"][b]), int(inp["label_length"][b])
        lp = PO.log_softmax(inp["logits"][b])
        got = PO.full_score(PO.state_of(kind, lp, Tb, 0, [int(c) for c in inp["labels"][b, :L]]))
        if np.isfinite(ref[b]):
            assert abs(got + ref[b]) < 1e-9 * max(1.0, abs(ref[b])), b
        else:
            assert got == -np.inf, b


@pytest.mark.parametrize("kind", KINDS)
def test_rows_of_minus_infinity(kind):
    """A frame that is -inf everywhere has no mass: nothing is NaN, prefixes that start before it keep their prefix score (the
    definition sums over the entry frame alone) and no full score survives it."""
    x = np.random.default_rng(3).standard_normal((6, 4))
    x[3, :] = -np.inf
    x[1, 2] = -np.inf
    lp = PO.log_softmax(x)
    assert not np.isnan(lp).any() and (lp[3] == -np.inf).all()
    st = PO.state_of(kind, lp, 6, 0, (1,))
    sc = PO.scores(kind, lp, 6, 0, st)
    assert not np.isnan(sc).any() and np.isfinite(sc[3]) and PO.full_score(st) == -np.inf
    # (the identity psi(g) = P(g) + sum_c psi(g . c) needs frames that sum to one and does not hold here)
