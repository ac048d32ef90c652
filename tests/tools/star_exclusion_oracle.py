"""Oracle for star temporal classification's exclusion of the following label (ctc_amd_star_loss_grad / _label_posterior /
_best_path): pure NumPy, float64, written from the contract in include/ctc_amd.h.

A wildcard position i (WILDCARD, or OPTIONAL where optional wildcards are on) whose position i + 1 is an ordinary, valid label y
excludes y on each of its frames: its emission is weight + ln sum_{k != y} exp lp[t, k], formed here as a log-sum-exp over the
other V - 1 columns, never as 1 - p.  Everything else is the lattice of optional_wildcard_oracle.py, restated as one dynamic
programme over explicit states with one emission column per label position: classic, the 2L + 1 states (blank, l_0, blank, ...);
simplified, L + 1 states with an emission for entering a state and one for staying in it.  `exclude=False` is the lattice without
the exclusion; `optional=False` makes OPTIONAL a malformed label.  Nothing here is the HIP kernels' layout."""
import numpy as np

WILDCARD = -2
OPTIONAL = -3
KINDS = ("classic", "simplified")
NI = -np.inf


def _lse(*a):
    out = a[0]
    for b in a[1:]:
        out = np.logaddexp(out, b)
    return out


def _lse_rows(m):
    """ln sum_k exp m[t, k] of every row; -inf for a row of -inf (or of no columns)."""
    if m.shape[1] == 0:
        return np.full(m.shape[0], NI)
    top = m.max(axis=1)
    ref = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        return ref + np.log(np.exp(m - ref[:, None]).sum(axis=1))


def _below(v, k):
    return np.concatenate([np.full(k, NI), v])[:len(v)]


def _above(v, k):
    return np.concatenate([v, np.full(k, NI)])[k:]


def log_probs(x, wrt):
    """lp[T, V] float64: x itself for log-probabilities, its log-softmax for logits (a row of -inf stays -inf)."""
    x = np.asarray(x, dtype=np.float64)
    if wrt or x.shape[0] == 0:
        return x
    with np.errstate(invalid="ignore"):
        lp = x - _lse_rows(x)[:, None]
    return np.where(np.isnan(lp), NI, lp)


def excluded_tokens(label, V, blank, optional, exclude):
    """(wild[L], y[L]): which positions are wildcards, and the token each excludes (-1: none)."""
    L = len(label)
    wild = [k == WILDCARD or (optional and k == OPTIONAL) for k in label]
    y = [-1] * L
    for i in range(L - 1):
        k = label[i + 1]
        if exclude and wild[i] and not wild[i + 1] and 0 <= k < V and k != blank:
            y[i] = k
    return wild, y


def _lattice(kind, label, wild, opt):
    """reach[k][s] (the step s - k -> s exists), end states, and the label position a state emits for (-1: the blank)."""
    L = len(label)
    differ = lambda a, b: label[a] != label[b] or wild[a] or wild[b]
    last_opt = L > 0 and opt[L - 1]
    if kind == "classic":
        S = 2 * L + 1
        reach = {k: np.zeros(S, dtype=bool) for k in (1, 2, 3, 4)}
        reach[1][1:] = True
        for i in range(1, L):
            s = 2 * i + 1
            reach[2][s] = differ(i, i - 1)
            if opt[i - 1]:
                reach[3][s] = True
                reach[4][s] = i >= 2 and differ(i, i - 2)
        ends = [S - 1] + ([S - 2] if L else [])
        if last_opt:
            ends += [S - 3] + ([S - 4] if L >= 2 else [])
        return S, reach, ends
    S = L + 1
    reach = {1: np.ones(S, dtype=bool), 2: np.zeros(S, dtype=bool)}
    reach[1][0] = False
    for l in range(2, S):
        reach[2][l] = opt[l - 2]
    return S, reach, [S - 1] + ([S - 2] if last_opt else [])


def _valid(label, V, blank, optional):
    if any(not (k == WILDCARD or (optional and k == OPTIONAL)) and (k == blank or k < 0 or k >= V) for k in label):
        return False
    return not any(label[i] == OPTIONAL and label[i + 1] == OPTIONAL for i in range(len(label) - 1))


def posteriors_one(kind, label, x, blank=0, wrt=0, weight=0.0, optional=True, exclude=True):
    """One utterance: label (cut to its length L), x[T, V] (cut to its length).  Returns (loss, gamma[T, V], Gw[T, L],
    label_posterior[T, L], blank_posterior[T], rest[T, L]): gamma_t(k) the posterior that frame t emits token k in an ordinary
    state (the blank included), Gw[t, i] the posterior of wildcard position i (0 for an ordinary one), rest[t, i] = 1 - p_t(y_i)
    (1 where nothing is excluded).  No path of finite value: (inf, zeros...)."""
    lp = log_probs(x, wrt)
    T, V = lp.shape
    label = [int(k) for k in label]
    L = len(label)
    none = (np.inf, np.zeros((T, V)), np.zeros((T, L)), np.zeros((T, L)), np.zeros(T), np.ones((T, L)))
    if not _valid(label, V, blank, optional):
        return none
    wild, y = excluded_tokens(label, V, blank, optional, exclude)
    opt = [optional and k == OPTIONAL for k in label]
    if T == 0:
        return ((0.0,) + none[1:]) if (L == 0 or (L == 1 and opt[0])) else none
    lse = _lse_rows(lp)
    # one emission column per label position; ln(1 - p_t(y)) from the sum over the other columns
    E = np.full((T, L), NI)
    rest = np.ones((T, L))
    for i in range(L):
        if not wild[i]:
            E[:, i] = lp[:, label[i]]
        elif y[i] < 0:
            E[:, i] = weight + lse
        else:
            others = _lse_rows(np.delete(lp, y[i], axis=1))
            E[:, i] = weight + others
            with np.errstate(invalid="ignore"):
                rest[:, i] = np.where(np.isfinite(lse), np.exp(others - lse), 0.0)
    eb = lp[:, blank]
    S, reach, ends = _lattice(kind, label, wild, opt)
    wl = np.asarray(wild, dtype=bool)
    if kind == "classic":
        Es = np.empty((T, S))
        Es[:, 0::2] = eb[:, None]
        Es[:, 1::2] = E
        inflow = lambda v: _lse(v, *[np.where(reach[k], _below(v, k), NI) for k in (1, 2, 3, 4)])
        alpha, v = np.full((T, S), NI), np.full(S, NI)
        v[0] = 0.0
        for t in range(T):
            v = inflow(v) + Es[t]
            alpha[t] = v
        beta = np.full((T, S), NI)
        beta[T - 1, ends] = 0.0
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + Es[t + 1]
            beta[t] = _lse(nxt, *[_above(np.where(reach[k], nxt, NI), k) for k in (1, 2, 3, 4)])
        logz = _lse(*[alpha[T - 1, s] for s in ends])
        if not np.isfinite(logz):
            return none
        post = np.exp(alpha + beta - logz)
        lab_post, blk_post = post[:, 1::2], post[:, 0::2].sum(axis=1)
    else:
        Est = np.concatenate([eb[:, None], np.where(wl[None, :], E, eb[:, None])], axis=1)  # staying in state l
        Een = np.concatenate([np.full((T, 1), NI), E], axis=1)                              # entering state l
        inflow = lambda v: _lse(*[np.where(reach[k], _below(v, k), NI) for k in (1, 2)])
        before = np.full((T + 1, S), NI)
        before[0, 0] = 0.0
        for t in range(T):
            before[t + 1] = _lse(before[t] + Est[t], inflow(before[t]) + Een[t])
        behind = np.full((T + 1, S), NI)
        behind[T, ends] = 0.0
        for t in range(T - 1, -1, -1):
            into = Een[t] + behind[t + 1]
            behind[t] = _lse(Est[t] + behind[t + 1], *[_above(np.where(reach[k], into, NI), k) for k in (1, 2)])
        logz = _lse(*[before[T, l] for l in ends])
        if not np.isfinite(logz):
            return none
        p_stay = np.exp(before[:T] + Est + behind[1:] - logz)
        p_enter = np.exp(np.stack([inflow(before[t]) for t in range(T)]) + Een + behind[1:] - logz)
        lab_post = p_enter[:, 1:] + np.where(wl[None, :], p_stay[:, 1:], 0.0)
        blk_post = p_stay[:, 0] + np.where(wl[None, :], 0.0, p_stay[:, 1:]).sum(axis=1)
    gamma = np.zeros((T, V))
    gamma[:, blank] = blk_post
    for i in range(L):
        if not wild[i]:
            gamma[:, label[i]] += lab_post[:, i]
    return float(-logz), gamma, np.where(wl[None, :], lab_post, 0.0), lab_post, blk_post, rest


def _rows(labels, ll, tl, T, U, blank):
    for b in range(len(ll)):
        Tb, Lb = min(max(int(tl[b]), 0), T), max(int(ll[b]), 0)
        yield b, Tb, Lb, None if Lb > U else [int(labels[b, i]) if i < labels.shape[1] else blank for i in range(Lb)]


def loss_and_grad(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, d_loss=None, optional=True, exclude=True):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B], d_loss[B] or None (ones).  Returns (loss[B], grad[B, T, V]) float64 by the
    header's formula, c_i = Gw[t, i] / (1 - p_t(y_i)) (0 where Gw is 0), C = sum_i c_i, D(k) = sum_{i: y_i = k} c_i:
        grad = d_loss * (p_k (1 - (C - D(k))) - gamma_t(k))       wrt == 0
             = d_loss * (-gamma_t(k) - p_k (C - D(k)))            wrt == 1
    zero beyond T_b and for an infeasible utterance."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    loss, grad = np.full(B, np.inf), np.zeros((B, T, V))
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, labels.shape[1], blank):
        if lab is None:
            continue
        loss[b], gamma, Gw, _, _, rest = posteriors_one(kind, lab, x[b, :Tb], blank, wrt, weight, optional, exclude)
        if not np.isfinite(loss[b]) or Tb == 0:
            continue
        lp = log_probs(x[b, :Tb], wrt)
        p = np.exp(lp - _lse_rows(lp)[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(Gw > 0.0, Gw / rest, 0.0)
        _, y = excluded_tokens(lab, V, blank, optional, exclude)
        CD = np.repeat(c.sum(axis=1)[:, None], V, axis=1)
        for i, k in enumerate(y):
            if k >= 0:
                CD[:, k] -= c[:, i]
        g = p * ((1.0 - CD) if not wrt else -CD) - gamma
        grad[b, :Tb] = g * (1.0 if d_loss is None else float(d_loss[b]))
    return loss, grad


def label_posterior(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, U=None, optional=True, exclude=True):
    """Batch: float64 (loss[B], label_posterior[B, T, U], blank_posterior[B, T], duration[B, U], expected_frame[B, U]);
    expected_frame is -1 where duration is 0."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    U = labels.shape[1] if U is None else int(U)
    loss = np.full(B, np.inf)
    post, blk = np.zeros((B, T, U)), np.zeros((B, T))
    dur, exf = np.zeros((B, U)), np.full((B, U), -1.0)
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, U, blank):
        if lab is None:
            continue
        loss[b], _, _, p, q, _ = posteriors_one(kind, lab, x[b, :Tb], blank, wrt, weight, optional, exclude)
        if np.isfinite(loss[b]):
            post[b, :Tb, :Lb], blk[b, :Tb] = p, q
            d = p.sum(axis=0)
            dur[b, :Lb] = d
            with np.errstate(divide="ignore", invalid="ignore"):
                exf[b, :Lb] = np.where(d > 0.0, (np.arange(Tb)[:, None] * p).sum(axis=0) / d, -1.0)
    return loss, post, blk, dur, exf


def best_path_one(kind, label, x, blank=0, wrt=0, optional=True, exclude=True):
    """One utterance.  Returns (score, path[T], label_index[T], first_frame[L], last_frame[L], label_score[L]) -- a skipped optional
    position has first = last = -1 and label_score 0.0 -- or (-inf, None...) when no path of finite value exists.  A wildcard
    frame scores and reports the best token other than the excluded one, the lowest on ties (of the float32 row)."""
    lp = log_probs(x, wrt)
    T, V = lp.shape
    label = [int(k) for k in label]
    L = len(label)
    none = (-np.inf, None, None, None, None, None)
    if not _valid(label, V, blank, optional):
        return none
    wild, y = excluded_tokens(label, V, blank, optional, exclude)
    opt = [optional and k == OPTIONAL for k in label]
    x32 = np.asarray(x, dtype=np.float32).reshape(T, V)
    tok = np.zeros((T, L), dtype=np.int64)  # the token position i emits on frame t
    for i in range(L):
        if not wild[i]:
            tok[:, i] = label[i]
        else:
            row = x32.copy()
            if y[i] >= 0:
                row[:, y[i]] = -np.inf
                if V == 1:
                    continue
            tok[:, i] = row.argmax(axis=1) if T else 0
    E = np.take_along_axis(lp, tok, axis=1) if L else np.zeros((T, 0))
    for i in range(L):  # a wildcard whose every other token is -inf (or that has no other token) emits -inf
        if wild[i] and y[i] >= 0:
            E[:, i] = np.where(tok[:, i] == y[i], NI, E[:, i])
    eb = lp[:, blank]
    S, reach, ends = _lattice(kind, label, wild, opt)
    steps = (0, 1, 2, 3, 4) if kind == "classic" else (0, 1, 2)
    if kind == "classic":
        position = lambda s, k: (s - 1) // 2 if s % 2 else -1
    else:
        position = lambda s, k: s - 1 if (k > 0 or (s >= 1 and wild[s - 1])) else -1
    v = np.full(S, NI)
    v[0] = 0.0
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        if kind == "classic":
            emit = np.empty(S)
            emit[0::2], emit[1::2] = eb[t], E[t]
            stay, enter = np.zeros(S), np.zeros(S)
        else:
            emit = np.zeros(S)
            stay = np.concatenate([[eb[t]], np.where(wild, E[t], eb[t])]) if L else np.asarray([eb[t]])
            enter = np.concatenate([[NI], E[t]])
        cand = np.full((len(steps), S), NI)
        cand[0] = v + stay
        for k in steps[1:]:
            cand[k] = np.where(reach[k], _below(v, k), NI) + enter
        k = cand.argmax(axis=0)
        v = cand[k, np.arange(S)] + emit
        back[t] = k
    s = max(ends, key=lambda q: v[q])
    score = float(v[s])
    if not score > NI:
        return none
    path, index = np.zeros(T, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        k = int(back[t, s])
        i = position(s, k)
        path[t], index[t] = (tok[t, i], i) if i >= 0 else (blank, -1)
        s -= k
    assert s == 0
    first, last = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    lscore = np.full(L, NI)
    for i in range(L):
        t = np.nonzero(index == i)[0]
        if len(t):
            first[i], last[i] = t[0], t[-1]
            lscore[i] = sum(lp[q, path[q]] for q in t)
        else:
            assert opt[i]
            lscore[i] = 0.0
    return score, path, index, first, last, lscore


def best_path(kind, labels, x, ll, tl, blank=0, wrt=0, optional=True, exclude=True):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B].  Returns (score[B] float64, [the rest of best_path_one or None] * B)."""
    labels, x = np.asarray(labels), np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    scores, rest = np.full(B, NI), []
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, labels.shape[1], blank):
        r = none = (-np.inf, None)
        if lab is not None:
            r = best_path_one(kind, lab, x[b, :Tb], blank, wrt, optional, exclude)
        scores[b] = r[0]
        rest.append(None if r[1] is None else r[1:])
    return scores, rest
