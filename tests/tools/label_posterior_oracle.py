"""Label-posterior oracle for both CTC lattices, wildcard labels included: pure NumPy, float64, forward-backward, written from the
definition in include/ctc_amd.h (ctc_amd_label_posterior).  Self-contained: nothing here is shared with the other oracles.

With lp = log_softmax(x) (wrt == 1: x as it stands) and w = wildcard_log_weight <= 0, a label equal to WILDCARD (-2) marks a
position whose frames emit e_w(t) = w + ln sum_k exp(lp[t, k]).
    classic     states 0 .. 2L: even ones emit the blank (state 0: nothing emitted yet; state 2i + 2: "closed", labels 0..i done),
                the odd state 2i + 1 is the open state of position i and emits label i (or e_w).  Steps s -> s, s -> s + 1 and, into
                an open state whose label differs from the previous one or where either is a wildcard, s -> s + 2; the first frame
                sits in state 0 or 1, the last in one of the last two.
                label_posterior[t, i] = P(state after frame t = 2i + 1);  blank_posterior[t] = sum over even states.
    simplified  states 0 .. L, the number of labels emitted so far.  Frame t either enters position i (state i -> i + 1, emits
                label i or e_w) or stays (emits the blank, or e_w in the state behind a wildcard).
                label_posterior[t, i] = P(frame t enters i) + [i is a wildcard] P(frame t stays behind i);
                blank_posterior[t] = sum of P(stay) over the stays that emit the blank.
duration[i] = sum_t label_posterior[t, i], expected_frame[i] = sum_t t label_posterior[t, i] / duration[i]; here both come from the
float64 posteriors (the library reduces the float32 values it returns)."""
import numpy as np

WILDCARD = -2
KINDS = ("classic", "simplified")
NI = -np.inf


def _lse(*a):
    out = a[0]
    for b in a[1:]:
        out = np.logaddexp(out, b)
    return out


def _shift(v, n=1):
    """v moved n states up: out[s] = v[s - n], -inf below."""
    return np.concatenate([np.full(n, NI), v])[:len(v)]


def _unshift(v, n=1):
    """out[s] = v[s + n], -inf above."""
    return np.concatenate([v, np.full(n, NI)])[n:]


def emissions(x, wrt, weight):
    """lpx[T, V + 1]: lp, and e_w as column V (the column a wildcard reads).  A row that is -inf throughout emits nothing."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        m = x.max(axis=-1) if T else np.zeros(0)
        ms = np.where(np.isfinite(m), m, 0.0)
        lse = ms + np.log(np.exp(x - ms[:, None]).sum(axis=-1))  # -inf for a dead row
    if wrt:
        lp, ew = x, weight + lse
    else:
        lp = np.where(np.isneginf(lse)[:, None], NI, x - np.where(np.isneginf(lse), 0.0, lse)[:, None])
        ew = np.where(np.isneginf(lse), NI, weight)
    return np.concatenate([lp, ew[:, None]], axis=1)


def posterior_one(kind, label, x, blank=0, wrt=0, weight=0.0):
    """One utterance: label (1-D, cut to its length L), x[T, V] (cut to its length).  Returns (loss, label_posterior[T, L],
    blank_posterior[T], duration[L], expected_frame[L]); (inf, zeros, zeros, zeros, -1) when no path of finite value exists."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    label = [int(k) for k in label]
    L = len(label)
    none = (np.inf, np.zeros((T, L)), np.zeros(T), np.zeros(L), np.full(L, -1.0))
    if any(k != WILDCARD and (k == blank or k < 0 or k >= V) for k in label):
        return none
    if T == 0:
        return (0.0,) + none[1:] if L == 0 else none
    lpx = emissions(x, wrt, weight)
    wild = np.asarray([k == WILDCARD for k in label], dtype=bool)
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    if kind == "classic":
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)
        ext[1::2] = col
        skip = np.zeros(S, dtype=bool)  # s - 2 -> s
        for i in range(1, L):
            skip[2 * i + 1] = label[i] != label[i - 1] or wild[i] or wild[i - 1]
        E = lpx[:, ext]
        alpha = np.full((T, S), NI)  # the mass of frames 0..t that ends in state s after frame t
        v = np.full(S, NI)
        v[0] = 0.0
        for t in range(T):
            v = _lse(v, _shift(v), np.where(skip, _shift(v, 2), NI)) + E[t]  # (t == 0: one step from state 0 gives states 0 and 1)
            alpha[t] = v
        beta = np.full((T, S), NI)  # the mass of frames t+1.. given state s after frame t
        beta[T - 1, S - 1] = 0.0
        if L:
            beta[T - 1, S - 2] = 0.0
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + E[t + 1]
            beta[t] = _lse(nxt, _unshift(nxt), _unshift(np.where(skip, nxt, NI), 2))
        logz = _lse(*alpha[T - 1, (S - 2 if L else S - 1):])
        if not np.isfinite(logz):
            return none
        post = np.exp(alpha + beta - logz)
        lab_post = post[:, 1::2]
        blk_post = post[:, 0::2].sum(axis=1)
    else:
        S = L + 1
        Es = lpx[:, np.concatenate([[blank], np.where(wild, V, blank)]).astype(np.int64)]  # staying in state l
        Ee = np.concatenate([np.full((T, 1), NI), lpx[:, col]], axis=1)                      # entering state l (= position l - 1)
        before = np.full((T + 1, S), NI)  # the mass of frames 0..t-1 that ends in state l
        before[0, 0] = 0.0
        for t in range(T):
            before[t + 1] = _lse(before[t] + Es[t], _shift(before[t]) + Ee[t])
        behind = np.full((T + 1, S), NI)  # the mass of frames t.. given state l before frame t
        behind[T, S - 1] = 0.0
        for t in range(T - 1, -1, -1):
            behind[t] = _lse(Es[t] + behind[t + 1], _unshift(Ee[t] + behind[t + 1]))
        logz = before[T, S - 1]
        if not np.isfinite(logz):
            return none
        p_stay = np.exp(before[:T] + Es + behind[1:] - logz)                                              # [T, S]
        p_enter = np.exp(np.stack([_shift(before[t]) for t in range(T)]) + Ee + behind[1:] - logz)        # [T, S], column 0 empty
        lab_post = p_enter[:, 1:] + np.where(wild[None, :], p_stay[:, 1:], 0.0)
        blk_post = p_stay[:, 0] + np.where(wild[None, :], 0.0, p_stay[:, 1:]).sum(axis=1)
    duration = lab_post.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = np.where(duration > 0.0, (np.arange(T)[:, None] * lab_post).sum(axis=0) / duration, -1.0)
    return float(-logz), lab_post, blk_post, duration, expected


def label_posterior(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, U=None):
    """Batch: labels[B, W], x[B, T, V], ll[B], tl[B]; U bounds the label lengths (default W).  Returns float64 (loss[B],
    label_posterior[B, T, U], blank_posterior[B, T], duration[B, U], expected_frame[B, U]) padded as the header says: 0 for frames
    from T_b on and positions from L on, -1 in expected_frame there; an infeasible utterance +inf, zeros and -1."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    U = labels.shape[1] if U is None else int(U)
    loss = np.full(B, np.inf)
    post, blk = np.zeros((B, T, U)), np.zeros((B, T))
    dur, exf = np.zeros((B, U)), np.full((B, U), -1.0)
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        Lb = max(int(ll[b]), 0)
        if Lb > U:
            continue
        lab = [int(labels[b, i]) if i < labels.shape[1] else blank for i in range(Lb)]  # (a position beyond the row: infeasible)
        loss[b], p, q, d, e = posterior_one(kind, lab, x[b, :Tb], blank, wrt, weight)
        if np.isfinite(loss[b]):
            post[b, :Tb, :Lb], blk[b, :Tb], dur[b, :Lb], exf[b, :Lb] = p, q, d, e
    return loss, post, blk, dur, exf
