"""Oracle for CTC with frame windows per label position on both lattices, wildcard labels included: pure NumPy, float64, written
from the text in include/ctc_amd.h ("Frame windows per label").  Self-contained: nothing here is shared with the other oracles.

window[i] = (first, last), both inclusive: position i may OWN frame t -- be what label_index[t] reports -- only if
first <= t <= last; outside, its emission is -inf.  Blank frames are never constrained.  With lp = log_softmax(x) (wrt == 1: x as
it stands) a label equal to WILDCARD (-2) marks a position whose frames emit
    summed lattice (loss, gradient, posteriors)   e_w(t) = w + ln sum_k exp(lp[t, k]),  w = wildcard_log_weight <= 0
    maximised lattice (alignment)                 m_t = max_k lp[t, k], reported as the lowest k that holds the float32 row's maximum
    classic     states 0 .. 2L.  Even states emit the blank; the odd state 2i + 1 is the open state of position i, emits label i (or
                the wildcard's emission) and owns its frames.  Steps s -> s, s -> s + 1 and, into an open state whose label differs
                from the previous one or where either is a wildcard, s -> s + 2.  Ends in one of the last two states.
    simplified  states 0 .. L, the number of labels emitted so far.  A frame either enters position i (owned by i, emits label i or
                the wildcard's emission) or stays: behind a wildcard the stay emits the wildcard's emission and is owned by it,
                otherwise it emits the blank and is owned by nobody.
Ties of the maximised lattice go to the earlier of (stay, step, skip), as in tests/tools/wildcard_oracle.py."""
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
    return np.concatenate([np.full(n, NI), v])[:len(v)]


def _unshift(v, n=1):
    return np.concatenate([v, np.full(n, NI)])[n:]


def full_window(B, U, T):
    """Windows that cover every frame."""
    w = np.zeros((B, U, 2), dtype=np.int64)
    w[..., 1] = max(T - 1, 0)
    return w


def _rows(x, wrt):
    """(lp[T, V], lse[T] = ln sum_k exp(lp), share[T, V] = exp(lp - lse)); a row that is -inf throughout emits nothing."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = x.max(axis=-1) if T else np.zeros(0)
        ms = np.where(np.isfinite(m), m, 0.0)
        xl = ms + np.log(np.exp(x - ms[:, None]).sum(axis=-1))  # -inf for a dead row
    dead = np.isneginf(xl)
    share = np.where(dead[:, None], 0.0, np.exp(x - np.where(dead, 0.0, xl)[:, None]))
    if wrt:
        return x, xl, share
    lp = np.where(dead[:, None], NI, x - np.where(dead, 0.0, xl)[:, None])
    return lp, np.where(dead, NI, 0.0), share


def _lattice(kind, label, lp, wild_emission, window, blank):
    """The emission of every state (classic: E[T, S]) or step (simplified: Es, Ee [T, S]) with the windows applied, or None when a
    label is no emission at all."""
    T, V = lp.shape
    L = len(label)
    if any(k != WILDCARD and (k == blank or k < 0 or k >= V) for k in label):
        return None
    wild = np.asarray([k == WILDCARD for k in label], dtype=bool)
    lpx = np.concatenate([lp, wild_emission[:, None]], axis=1)
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    t = np.arange(T)[:, None]
    win = np.asarray(window, dtype=np.int64).reshape(-1, 2)[:L]
    inside = (t >= win[None, :, 0]) & (t <= win[None, :, 1])  # [T, L]
    own = np.where(inside, lpx[:, col], NI)                   # the emission of position i when it owns frame t
    if kind == "classic":
        S = 2 * L + 1
        E = np.repeat(lp[:, blank:blank + 1], S, axis=1)
        E[:, 1::2] = own
        skip = np.zeros(S, dtype=bool)
        for i in range(1, L):
            skip[2 * i + 1] = label[i] != label[i - 1] or wild[i] or wild[i - 1]
        return dict(E=E, skip=skip, wild=wild, ends=(S - 1, S - 2) if L else (0,))
    Es = np.repeat(lp[:, blank:blank + 1], L + 1, axis=1)
    Es[:, 1:] = np.where(wild[None, :], own, Es[:, 1:])  # the stay behind a wildcard is the wildcard's frame
    Ee = np.concatenate([np.full((T, 1), NI), own], axis=1)
    return dict(Es=Es, Ee=Ee, wild=wild)


def posterior_one(kind, label, x, window, blank=0, wrt=0, weight=0.0):
    """One utterance (label, x and window cut to their lengths).  Returns (loss, label_posterior[T, L], blank_posterior[T]);
    (inf, zeros, zeros) when no path of finite value exists."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    label = [int(k) for k in label]
    L = len(label)
    none = (np.inf, np.zeros((T, L)), np.zeros(T))
    if T == 0:
        return (0.0,) + none[1:] if L == 0 else none
    lp, lse, _ = _rows(x, wrt)
    lat = _lattice(kind, label, lp, weight + lse, window, blank)
    if lat is None:
        return none
    if kind == "classic":
        E, skip = lat["E"], lat["skip"]
        S = E.shape[1]
        alpha = np.full((T, S), NI)
        v = np.full(S, NI)
        v[0] = 0.0
        for t in range(T):
            v = _lse(v, _shift(v), np.where(skip, _shift(v, 2), NI)) + E[t]
            alpha[t] = v
        beta = np.full((T, S), NI)
        for s in lat["ends"]:
            beta[T - 1, s] = 0.0
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + E[t + 1]
            beta[t] = _lse(nxt, _unshift(nxt), _unshift(np.where(skip, nxt, NI), 2))
        logz = _lse(*[alpha[T - 1, s] for s in lat["ends"]])
        if not np.isfinite(logz):
            return none
        post = np.exp(alpha + beta - logz)
        return float(-logz), post[:, 1::2], post[:, 0::2].sum(axis=1)
    Es, Ee, wild = lat["Es"], lat["Ee"], lat["wild"]
    S = L + 1
    before = np.full((T + 1, S), NI)
    before[0, 0] = 0.0
    for t in range(T):
        before[t + 1] = _lse(before[t] + Es[t], _shift(before[t]) + Ee[t])
    behind = np.full((T + 1, S), NI)
    behind[T, S - 1] = 0.0
    for t in range(T - 1, -1, -1):
        behind[t] = _lse(Es[t] + behind[t + 1], _unshift(Ee[t] + behind[t + 1]))
    logz = before[T, S - 1]
    if not np.isfinite(logz):
        return none
    p_stay = np.exp(before[:T] + Es + behind[1:] - logz)
    p_enter = np.exp(np.stack([_shift(before[t]) for t in range(T)]) + Ee + behind[1:] - logz)
    lab_post = p_enter[:, 1:] + np.where(wild[None, :], p_stay[:, 1:], 0.0)
    blk_post = p_stay[:, 0] + np.where(wild[None, :], 0.0, p_stay[:, 1:]).sum(axis=1)
    return float(-logz), lab_post, blk_post


def best_path_one(kind, label, x, window, blank=0, wrt=0):
    """One utterance.  Returns (score, path[T], label_index[T]); (-inf, None, None) when no path of finite value exists."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    label = [int(k) for k in label]
    L = len(label)
    lp, _, _ = _rows(x, wrt)
    with np.errstate(invalid="ignore"):
        top = lp.max(axis=-1) if T else np.zeros(0)
    lat = _lattice(kind, label, lp, top, window, blank)
    if lat is None:
        return -np.inf, None, None
    arg = np.asarray(x, dtype=np.float32).argmax(axis=-1) if T else np.zeros(0, np.int64)
    wild = lat["wild"]
    S = 2 * L + 1 if kind == "classic" else L + 1
    v = np.full(S, NI)
    v[0] = 0.0
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        cand = np.full((3, S), NI)
        if kind == "classic":
            cand[0] = v
            cand[1] = _shift(v)
            cand[2] = np.where(lat["skip"], _shift(v, 2), NI)
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)] + lat["E"][t]
        else:
            cand[0] = v + lat["Es"][t]
            cand[1] = _shift(v) + lat["Ee"][t]
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)]
        back[t] = k
    ends = lat["ends"] if kind == "classic" else (S - 1,)
    s = max(ends, key=lambda q: v[q])
    score = float(v[s])
    if not score > NI:
        return -np.inf, None, None
    path = np.zeros(T, dtype=np.int64)
    index = np.full(T, -1, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        k = int(back[t, s])
        if kind == "classic":
            i = (s - 1) // 2 if s % 2 else -1
        else:
            i = s - 1 if (k == 1 or (s >= 1 and wild[s - 1])) else -1
        if i >= 0:
            path[t] = arg[t] if wild[i] else label[i]
            index[t] = i
        else:
            path[t] = blank
        s -= k
    assert s == 0
    return score, path, index


def _cut(labels, x, ll, tl, window, b, U):
    T = x.shape[1]
    Tb = min(max(int(tl[b]), 0), T)
    Lb = max(int(ll[b]), 0)
    if Lb > U:
        return None
    lab = [int(labels[b, i]) if i < labels.shape[1] else 0 for i in range(Lb)]
    win = full_window(1, Lb, Tb)[0] if window is None else np.asarray(window)[b, :Lb]
    return lab, x[b, :Tb], win, Tb, Lb


def label_posterior(kind, wrt, labels, x, ll, tl, window=None, blank=0, weight=0.0, U=None):
    """Batch: labels[B, W], x[B, T, V], ll[B], tl[B], window[B, U, 2] or None (no constraint).  Returns float64 (loss[B],
    label_posterior[B, T, U], blank_posterior[B, T], duration[B, U], expected_frame[B, U]), padded as the header says."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, _ = x.shape
    U = labels.shape[1] if U is None else int(U)
    loss = np.full(B, np.inf)
    post, blk = np.zeros((B, T, U)), np.zeros((B, T))
    dur, exf = np.zeros((B, U)), np.full((B, U), -1.0)
    for b in range(B):
        c = _cut(labels, x, ll, tl, window, b, U)
        if c is None:
            continue
        lab, xb, win, Tb, Lb = c
        loss[b], p, q = posterior_one(kind, lab, xb, win, blank, wrt, weight)
        if np.isfinite(loss[b]):
            post[b, :Tb, :Lb], blk[b, :Tb] = p, q
            d = p.sum(axis=0)
            dur[b, :Lb] = d
            with np.errstate(divide="ignore", invalid="ignore"):
                exf[b, :Lb] = np.where(d > 0.0, (np.arange(Tb)[:, None] * p).sum(axis=0) / d, -1.0)
    return loss, post, blk, dur, exf


def loss_and_grad(kind, wrt, labels, x, ll, tl, window=None, blank=0, weight=0.0, d_loss=None):
    """Batch.  Returns (loss[B], grad[B, T, V]) in float64.  With gamma_t(k) the posterior that frame t emits token k from an
    ordinary position or the blank, and Gamma_t that it is a wildcard's:
        grad = d_loss * ((1 - Gamma_t) softmax(x)[k] - gamma_t(k))       wrt == 0
             = d_loss * (-gamma_t(k) - Gamma_t exp(x[t, k] - LSE_t))     wrt == 1
    zero beyond T_b and for an infeasible utterance."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    loss = np.full(B, np.inf)
    grad = np.zeros((B, T, V))
    for b in range(B):
        c = _cut(labels, x, ll, tl, window, b, labels.shape[1])
        if c is None:
            continue
        lab, xb, win, Tb, Lb = c
        loss[b], p, q = posterior_one(kind, lab, xb, win, blank, wrt, weight)
        if not np.isfinite(loss[b]) or Tb == 0:
            continue
        gamma = np.zeros((Tb, V))
        Gamma = np.zeros(Tb)
        gamma[:, blank] += q
        for i, k in enumerate(lab):
            if k == WILDCARD:
                Gamma += p[:, i]
            else:
                gamma[:, k] += p[:, i]
        share = _rows(xb, wrt)[2]
        g = ((1.0 - Gamma) if not wrt else -Gamma)[:, None] * share - gamma
        grad[b, :Tb] = g * (1.0 if d_loss is None else float(d_loss[b]))
    return loss, grad


def best_path(kind, labels, x, ll, tl, window=None, blank=0, wrt=0):
    """Batch.  Returns (score[B] float64, [path or None] * B, [label_index or None] * B)."""
    labels, x = np.asarray(labels), np.asarray(x)
    B = x.shape[0]
    scores, paths, indices = np.full(B, -np.inf), [], []
    for b in range(B):
        c = _cut(labels, x, ll, tl, window, b, labels.shape[1])
        if c is None:
            paths.append(None); indices.append(None)
            continue
        lab, xb, win, _, _ = c
        scores[b], p, i = best_path_one(kind, lab, xb, win, blank, wrt)
        paths.append(p); indices.append(i)
    return scores, paths, indices
