"""Float64 NumPy oracle of the CTC prefix scores (include/ctc_amd.h "CTC prefix scores"), and the
brute-force enumeration that pins it.  Natural logarithms; one utterance at a time; log(0) is a true -inf.

A state is the pair (rn, rb) of arrays over the frames t < Tb plus the prefix's tokens; None is the dead state."""
import itertools

import numpy as np

NINF = -np.inf


def log_softmax(x):
    """Rows of float64 log-probabilities; a row of -inf stays -inf everywhere (no NaN)."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    dead = ~np.isfinite(m)
    m = np.where(dead, 0.0, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dead, NINF, x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def lse(*a):
    a = np.asarray(a, dtype=np.float64)
    m = a.max()
    if m == NINF:
        return NINF
    return float(m + np.log(np.exp(a - m).sum()))


class State:
    def __init__(self, rn, rb, tokens):
        self.rn, self.rb, self.tokens = rn, rb, tuple(tokens)


def empty_state(lp, Tb, blank):
    return State(np.full(Tb, NINF), np.cumsum(lp[:Tb, blank]), ())


def emits(c, V, blank):
    return 0 <= c < V and c != blank


def entry_weight(kind, st, c, Tb):
    """phi[t], t < Tb."""
    phi = np.full(Tb, NINF)
    if Tb > 0 and len(st.tokens) == 0:
        phi[0] = 0.0
    if Tb > 1:
        if kind == "classic" and st.tokens and c == st.tokens[-1]:
            phi[1:] = st.rb[:-1]
        else:
            with np.errstate(invalid="ignore"):  # (numpy warns about logaddexp(-inf, -inf), which is -inf)
                phi[1:] = np.logaddexp(st.rb[:-1], st.rn[:-1])
    return phi


def lse_columns(a):
    """Log-sum-exp over axis 0 of a [Tb, V] array; -inf where a column is -inf throughout."""
    m = a.max(axis=0)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(m == NINF, NINF, m0 + np.log(np.exp(a - m0).sum(axis=0)))


def scores(kind, lp, Tb, blank, st):
    """ln psi(g . c) for every c < V."""
    V = lp.shape[1]
    out = np.full(V, NINF)
    if st is None or Tb == 0:
        return out
    out = lse_columns(entry_weight(kind, st, -1, Tb)[:, None] + lp[:Tb])
    if kind == "classic" and st.tokens:
        c = st.tokens[-1]
        out[c] = lse(*(entry_weight(kind, st, c, Tb) + lp[:Tb, c]))
    out[blank] = NINF
    return out


def extend(kind, lp, Tb, blank, st, c):
    V = lp.shape[1]
    if st is None or not emits(c, V, blank):
        return None
    phi = entry_weight(kind, st, c, Tb)
    rn, rb = np.full(Tb, NINF), np.full(Tb, NINF)
    pn, pb = NINF, NINF
    for t in range(Tb):
        rn[t] = (lse(pn, phi[t]) if kind == "classic" else phi[t]) + lp[t, c]
        rb[t] = lse(pb, pn) + lp[t, blank]
        pn, pb = rn[t], rb[t]
    return State(rn, rb, st.tokens + (c,))


def full_score(st):
    if st is None:
        return NINF
    if len(st.rn) == 0:
        return 0.0 if not st.tokens else NINF
    return lse(st.rn[-1], st.rb[-1])


def state_of(kind, lp, Tb, blank, tokens):
    """The state after extending the empty prefix by `tokens` in turn (None once an extension is impossible)."""
    st = empty_state(lp, Tb, blank)
    for c in tokens:
        st = extend(kind, lp, Tb, blank, st, c)
    return st


def collapse(kind, path, blank):
    out, prev = [], None
    for k in path:
        if k != blank and (kind == "simplified" or k != prev):
            out.append(k)
        prev = k
    return tuple(out)


def enumerate_sequences(kind, lp, Tb, blank):
    """{label sequence: probability} from all V^Tb paths."""
    V = lp.shape[1]
    p = np.exp(lp[:Tb])
    out = {}
    for path in itertools.product(range(V), repeat=Tb):
        w = 1.0
        for t, k in enumerate(path):
            w *= p[t, k]
        seq = collapse(kind, path, blank)
        out[seq] = out.get(seq, 0.0) + w
    return out


def prefix_mass(seqs, prefix):
    n = len(prefix)
    return sum(w for s, w in seqs.items() if s[:n] == tuple(prefix))
