"""Loss and gradient oracle for CTC with wildcard labels on both lattices: pure NumPy, float64, forward-backward, written from
the definition in include/ctc_amd.h (ctc_amd_wildcard_loss_grad).

A label equal to WILDCARD (-2) stands for any non-empty run of frames with any tokens on them.  With lp = log_softmax(x)
(wrt == 1: x as it stands) and w = wildcard_log_weight <= 0 a wildcard frame emits e_w(t) = w + ln sum_k exp(lp[t, k]).
    classic     the textbook extended label sequence (blank, l_1, blank, l_2, ..., blank: 2L + 1 states).  A wildcard's state emits
                e_w; the skip s-2 -> s is allowed when the two labels differ or one of them is a wildcard; ends S-1 and S-2.
    simplified  the number of labels emitted (L + 1 states).  Entering a wildcard costs e_w, and so does staying in the state
                behind it (where an ordinary label's state costs the blank).
Z = the sum over all state sequences of the product of their emissions, loss = -ln Z (a sum over lattice paths, not a probability:
it may be negative).  gamma_t(k): posterior that frame t sits in an ordinary state emitting k; Gamma_t: that it sits in a wildcard
emission.  Neither state layout is the HIP kernel's (csrc/ctc_wild_loss.hip keeps open / closed pairs per label position)."""
import numpy as np

from tests.tools.viterbi_oracle import log_softmax64

WILDCARD = -2
KINDS = ("classic", "simplified")


def _lse(*a):
    out = a[0]
    for b in a[1:]:
        out = np.logaddexp(out, b)
    return out


def emissions(x, wrt, weight):
    """(lpx[T, V + 1], lse[T]): lp with e_w as column V, the column a wildcard reads, and ln sum_k exp(lp[t, k])."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    if T == 0:
        return np.zeros((0, V + 1)), np.zeros(0)
    if wrt:
        lp = x
        with np.errstate(divide="ignore", invalid="ignore"):
            m = lp.max(axis=-1)
            ms = np.where(np.isfinite(m), m, 0.0)
            lse = ms + np.log(np.exp(lp - ms[:, None]).sum(axis=-1))
    else:
        lp = log_softmax64(x)
        dead = np.isneginf(x.max(axis=-1))  # a row that is -inf throughout: log_softmax64 leaves nan there
        lp = np.where(np.isnan(lp), -np.inf, lp)
        lse = np.where(dead, -np.inf, 0.0)
    return np.concatenate([lp, (weight + lse)[:, None]], axis=1), lse


def posteriors_one(kind, label, x, blank=0, wrt=0, weight=0.0):
    """One utterance: label (1-D, cut to its length), x[T, V] (cut to its length).  Returns (loss, gamma[T, V], Gamma[T]);
    (inf, zeros, zeros) when no path of finite value exists."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    label = [int(k) for k in label]
    L = len(label)
    none = (np.inf, np.zeros((T, V)), np.zeros(T))
    if any(k != WILDCARD and (k == blank or k < 0 or k >= V) for k in label):
        return none
    lpx, _ = emissions(x, wrt, weight)
    wild = [k == WILDCARD for k in label]
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    NI = -np.inf
    if kind == "classic":
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)  # the column every state emits
        ext[1::2] = col
        skip = np.zeros(S, dtype=bool)  # s-2 -> s
        for s in range(3, S, 2):
            i = (s - 1) // 2
            skip[s] = label[i] != label[i - 1] or wild[i] or wild[i - 1]
        ends = (S - 1, S - 2) if L else (0,)
        if T == 0:
            return (0.0, np.zeros((0, V)), np.zeros(0)) if L == 0 else none
        E = lpx[:, ext]  # [T, S]
        alpha = np.full((T, S), NI)
        v = np.full(S, NI)
        v[0] = 0.0
        for t in range(T):
            a1 = np.concatenate([[NI], v[:-1]])
            a2 = np.concatenate([[NI, NI], v[:-2]])[:S] if S >= 2 else np.full(S, NI)
            a2 = np.where(skip, a2, NI)
            v = _lse(v, a1, a2) + E[t]
            alpha[t] = v
        beta = np.full((T, S), NI)
        w_ = np.full(S, NI)
        for s in ends:
            w_[s] = 0.0
        beta[T - 1] = w_
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + E[t + 1]
            b1 = np.concatenate([nxt[1:], [NI]])
            b2 = np.concatenate([np.where(skip, nxt, NI)[2:], [NI, NI]])[:S] if S >= 2 else np.full(S, NI)
            beta[t] = _lse(nxt, b1, b2)
        logz = _lse(*[alpha[T - 1, s] for s in ends])
        if not np.isfinite(logz):
            return none
        post = np.exp(alpha + beta - logz)  # [T, S]
        gamma = np.zeros((T, V))
        Gamma = np.zeros(T)
        for s in range(S):
            if ext[s] == V:
                Gamma += post[:, s]
            else:
                gamma[:, ext[s]] += post[:, s]
        return float(-logz), gamma, Gamma
    # simplified: posteriors sit on the edges (stay in l / enter l), alpha before the frame, beta behind it
    S = L + 1
    enter = np.concatenate([[blank], col]).astype(np.int64)
    stay = np.asarray([blank] + [V if w else blank for w in wild], dtype=np.int64)
    if T == 0:
        return (0.0, np.zeros((0, V)), np.zeros(0)) if L == 0 else none
    Es, Ee = lpx[:, stay], lpx[:, enter]
    Ee[:, 0] = NI  # nothing enters state 0
    before = np.full((T + 1, S), NI)
    before[0, 0] = 0.0
    for t in range(T):
        v = before[t]
        before[t + 1] = _lse(v + Es[t], np.concatenate([[NI], v[:-1]]) + Ee[t])
    behind = np.full((T + 1, S), NI)  # behind[t]: the mass of frames t.. given the state before frame t
    behind[T, S - 1] = 0.0
    for t in range(T - 1, -1, -1):
        w_ = behind[t + 1]
        behind[t] = _lse(Es[t] + w_, np.concatenate([(Ee[t] + w_)[1:], [NI]]))
    logz = before[T, S - 1]
    if not np.isfinite(logz):
        return none
    p_stay = np.exp(before[:T] + Es + behind[1:] - logz)
    p_enter = np.exp(np.concatenate([np.full((T, 1), NI), before[:T, :-1]], axis=1) + Ee + behind[1:] - logz)
    gamma = np.zeros((T, V))
    Gamma = np.zeros(T)
    for l in range(S):
        for p, c in ((p_stay[:, l], stay[l]), (p_enter[:, l], enter[l])):
            if c == V:
                Gamma += p
            else:
                gamma[:, c] += p
    return float(-logz), gamma, Gamma


def loss_and_grad(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, d_loss=None):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B], d_loss[B] or None (ones).  Returns (loss[B] float64, grad[B, T, V] float64):
        grad = d_loss * ((1 - Gamma_t) softmax(x)[k] - gamma_t(k))       wrt == 0
             = d_loss * (-gamma_t(k) - Gamma_t exp(x[t, k] - LSE_t))     wrt == 1
    zero beyond T_b and for an infeasible utterance, whose d_loss is not interpreted.  Lengths by the input contract of DESIGN.md
    section 5.8 with U = the width of `labels`."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    loss = np.full(B, np.inf)
    grad = np.zeros((B, T, V))
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        Lb = max(int(ll[b]), 0)
        if Lb > labels.shape[1]:
            continue
        loss[b], gamma, Gamma = posteriors_one(kind, labels[b, :Lb], x[b, :Tb], blank, wrt, weight)
        if not np.isfinite(loss[b]) or Tb == 0:
            continue
        lpx, lse = emissions(x[b, :Tb], wrt, weight)
        share = np.exp(lpx[:, :V] - lse[:, None])  # softmax(x) for logits, exp(x - LSE) for log-probabilities
        g = ((1.0 - Gamma) if not wrt else -Gamma)[:, None] * share - gamma
        grad[b, :Tb] = g * (1.0 if d_loss is None else float(d_loss[b]))
    return loss, grad
