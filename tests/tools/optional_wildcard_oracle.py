"""Oracle for optional wildcards (ctc_amd_optional_wildcard_loss_grad / _label_posterior): pure NumPy, float64, written from the
contract in include/ctc_amd.h as a direct dynamic programme on the 2L + 1 (classic) / L + 1 (simplified) states.

OPTIONAL (-3) is a wildcard position that may take no frame at all.  On the extended label sequence of the classic lattice
(blank, l_0, blank, l_1, ..., blank; label position i is state 2i + 1, the blank behind it 2i + 2) skipping position i adds
    2i     -> 2i + 3     the blank before i (the start state for i = 0) straight into the open state of i + 1
    2i - 1 -> 2i + 3     the open state of i - 1 into that of i + 1, when the two labels differ or either is a wildcard
and, when i is the last position, makes 2i and 2i - 1 end states.  The blank behind i (2i + 2) is still entered from i alone.
On the simplified lattice (state l = l labels emitted) state i + 2 may also be entered from state i, at the cost of label i + 1;
when i is last, state i is an end state too.  Two adjacent optional wildcards make the utterance infeasible.
Nothing here is the HIP kernel's layout (csrc/ctc_wild_loss.hip keeps open / closed pairs per position, lanes and masks).
The best path (ctc_amd_optional_wildcard_best_path) is the same programme in (max, +) on the log-probabilities with m_t as a
wildcard's emission; candidates in the header's order (stay, one back, the skip over two, then the two sources over an optional
position; numpy's argmax keeps the first maximum, which is a strict comparison)."""
import numpy as np

from tests.tools.wildcard_loss_oracle import emissions
from tests.tools.wildcard_oracle import _lp, argmax_tokens

WILDCARD = -2
OPTIONAL = -3
KINDS = ("classic", "simplified")
NI = -np.inf


def _lse(*a):
    out = a[0]
    for b in a[1:]:
        out = np.logaddexp(out, b)
    return out


def _from_below(v, k):
    """out[s] = v[s - k], -inf where there is no such state."""
    return np.concatenate([np.full(k, NI), v])[:len(v)]


def _from_above(v, k):
    """out[s] = v[s + k], -inf where there is no such state."""
    return np.concatenate([v, np.full(k, NI)])[k:]


def _none(T, V, L):
    return np.inf, np.zeros((T, V)), np.zeros(T), np.zeros((T, L)), np.zeros(T)


def posteriors_one(kind, label, x, blank=0, wrt=0, weight=0.0):
    """One utterance: label (1-D, cut to its length L; may hold WILDCARD and OPTIONAL), x[T, V] (cut to its length).  Returns
    (loss, gamma[T, V], Gamma[T], label_posterior[T, L], blank_posterior[T]): gamma_t(k) the posterior that frame t emits token k
    in an ordinary state (the blank included), Gamma_t that it sits in a wildcard emission of either kind.  No path of finite
    value: (inf, zeros...)."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    label = [int(k) for k in label]
    L = len(label)
    none = _none(T, V, L)
    if any(k not in (WILDCARD, OPTIONAL) and (k == blank or k < 0 or k >= V) for k in label):
        return none
    opt = [k == OPTIONAL for k in label]
    if any(opt[i] and opt[i + 1] for i in range(L - 1)):
        return none
    wild = [k in (WILDCARD, OPTIONAL) for k in label]
    last_opt = L > 0 and opt[L - 1]
    if T == 0:  # no frame: feasible when the start state is an end state
        return ((0.0,) + none[1:]) if (L == 0 or (L == 1 and last_opt)) else none
    lpx, _ = emissions(x, wrt, weight)
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    differ = lambda a, b: label[a] != label[b] or wild[a] or wild[b]
    if kind == "classic":
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)
        ext[1::2] = col
        # reach[k][s]: the step s - k -> s exists
        reach = {k: np.zeros(S, dtype=bool) for k in (1, 2, 3, 4)}
        reach[1][1:] = True
        for i in range(L):
            s = 2 * i + 1
            if i >= 1 and differ(i, i - 1):
                reach[2][s] = True
            if i >= 1 and opt[i - 1]:          # position i - 1 may be skipped
                reach[3][s] = True             # from the blank before it
                if i >= 2 and differ(i, i - 2):
                    reach[4][s] = True         # from the open state before it
        ends = [S - 1] + ([S - 2] if L else [])
        if last_opt:
            ends += [S - 3] + ([S - 4] if L >= 2 else [])
        E = lpx[:, ext]
        alpha = np.full((T, S), NI)
        v = np.full(S, NI)
        v[0] = 0.0
        for t in range(T):
            v = _lse(v, *[np.where(reach[k], _from_below(v, k), NI) for k in (1, 2, 3, 4)]) + E[t]
            alpha[t] = v
        beta = np.full((T, S), NI)
        beta[T - 1, ends] = 0.0
        for t in range(T - 2, -1, -1):
            nxt = beta[t + 1] + E[t + 1]
            beta[t] = _lse(nxt, *[_from_above(np.where(reach[k], nxt, NI), k) for k in (1, 2, 3, 4)])
        logz = _lse(*[alpha[T - 1, s] for s in ends])
        if not np.isfinite(logz):
            return none
        post = np.exp(alpha + beta - logz)
        lab_post = post[:, 1::2]
        blk_post = post[:, 0::2].sum(axis=1)
        gamma, Gamma = np.zeros((T, V)), np.zeros(T)
        gamma[:, blank] = blk_post
        for i in range(L):
            if wild[i]:
                Gamma += lab_post[:, i]
            else:
                gamma[:, label[i]] += lab_post[:, i]
        return float(-logz), gamma, Gamma, lab_post, blk_post
    S = L + 1
    wl = np.asarray(wild, dtype=bool)
    Es = lpx[:, np.concatenate([[blank], np.where(wl, V, blank)]).astype(np.int64)]  # staying in state l
    Ee = np.concatenate([np.full((T, 1), NI), lpx[:, col]], axis=1)                   # entering state l (= position l - 1)
    over = np.zeros(S, dtype=bool)  # over[l]: state l may be entered from l - 2, over the optional position l - 2
    for l in range(2, S):
        over[l] = opt[l - 2]
    ends = [S - 1] + ([S - 2] if last_opt else [])
    inflow = lambda v: _lse(_from_below(v, 1), np.where(over, _from_below(v, 2), NI))
    before = np.full((T + 1, S), NI)  # the mass of frames 0..t-1 that ends in state l
    before[0, 0] = 0.0
    for t in range(T):
        before[t + 1] = _lse(before[t] + Es[t], inflow(before[t]) + Ee[t])
    behind = np.full((T + 1, S), NI)  # the mass of frames t.. given state l before frame t
    behind[T, ends] = 0.0
    for t in range(T - 1, -1, -1):
        into = Ee[t] + behind[t + 1]  # entering state l with frame t and what follows
        behind[t] = _lse(Es[t] + behind[t + 1], _from_above(into, 1), _from_above(np.where(over, into, NI), 2))
    logz = _lse(*[before[T, l] for l in ends])
    if not np.isfinite(logz):
        return none
    p_stay = np.exp(before[:T] + Es + behind[1:] - logz)
    p_enter = np.exp(np.stack([inflow(before[t]) for t in range(T)]) + Ee + behind[1:] - logz)
    lab_post = p_enter[:, 1:] + np.where(wl[None, :], p_stay[:, 1:], 0.0)
    blk_post = p_stay[:, 0] + np.where(wl[None, :], 0.0, p_stay[:, 1:]).sum(axis=1)
    gamma, Gamma = np.zeros((T, V)), np.zeros(T)
    gamma[:, blank] = blk_post
    for i in range(L):
        if wild[i]:
            Gamma += lab_post[:, i]
        else:
            gamma[:, label[i]] += lab_post[:, i]
    return float(-logz), gamma, Gamma, lab_post, blk_post


def _rows(labels, ll, tl, T, U, blank):
    for b in range(len(ll)):
        Tb = min(max(int(tl[b]), 0), T)
        Lb = max(int(ll[b]), 0)
        if Lb > U:
            yield b, Tb, Lb, None
            continue
        yield b, Tb, Lb, [int(labels[b, i]) if i < labels.shape[1] else blank for i in range(Lb)]


def loss_and_grad(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, d_loss=None):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B], d_loss[B] or None (ones).  Returns (loss[B], grad[B, T, V]) float64 by the
    gradient formula of wildcard_loss_oracle.loss_and_grad:
        grad = d_loss * ((1 - Gamma_t) softmax(x)[k] - gamma_t(k))       wrt == 0
             = d_loss * (-gamma_t(k) - Gamma_t exp(x[t, k] - LSE_t))     wrt == 1
    zero beyond T_b and for an infeasible utterance."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    loss = np.full(B, np.inf)
    grad = np.zeros((B, T, V))
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, labels.shape[1], blank):
        if lab is None:
            continue
        loss[b], gamma, Gamma, _, _ = posteriors_one(kind, lab, x[b, :Tb], blank, wrt, weight)
        if not np.isfinite(loss[b]) or Tb == 0:
            continue
        lpx, lse = emissions(x[b, :Tb], wrt, weight)
        share = np.exp(lpx[:, :V] - lse[:, None])
        g = ((1.0 - Gamma) if not wrt else -Gamma)[:, None] * share - gamma
        grad[b, :Tb] = g * (1.0 if d_loss is None else float(d_loss[b]))
    return loss, grad


def label_posterior(kind, wrt, labels, x, ll, tl, blank=0, weight=0.0, U=None):
    """Batch, padded as label_posterior_oracle.label_posterior pads: float64 (loss[B], label_posterior[B, T, U],
    blank_posterior[B, T], duration[B, U], expected_frame[B, U]); expected_frame is -1 where duration is 0."""
    labels, x = np.asarray(labels), np.asarray(x, dtype=np.float64)
    B, T, V = x.shape
    U = labels.shape[1] if U is None else int(U)
    loss = np.full(B, np.inf)
    post, blk = np.zeros((B, T, U)), np.zeros((B, T))
    dur, exf = np.zeros((B, U)), np.full((B, U), -1.0)
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, U, blank):
        if lab is None:
            continue
        loss[b], _, _, p, q = posteriors_one(kind, lab, x[b, :Tb], blank, wrt, weight)
        if np.isfinite(loss[b]):
            post[b, :Tb, :Lb], blk[b, :Tb] = p, q
            d = p.sum(axis=0)
            dur[b, :Lb] = d
            with np.errstate(divide="ignore", invalid="ignore"):
                exf[b, :Lb] = np.where(d > 0.0, (np.arange(Tb)[:, None] * p).sum(axis=0) / d, -1.0)
    return loss, post, blk, dur, exf


def best_path_one(kind, label, x, blank=0, wrt=0):
    """One utterance.  Returns (score, path[T], label_index[T], first_frame[L], last_frame[L], label_score[L]) -- a skipped optional
    position has first = last = -1 and label_score 0.0 -- or (-inf, None, None, None, None, None) when no path of finite value exists."""
    lp = _lp(x, wrt)
    T, V = lp.shape
    label = [int(k) for k in label]
    L = len(label)
    none = (-np.inf, None, None, None, None, None)
    if any(k not in (WILDCARD, OPTIONAL) and (k == blank or k < 0 or k >= V) for k in label):
        return none
    opt = [k == OPTIONAL for k in label]
    if any(opt[i] and opt[i + 1] for i in range(L - 1)):
        return none
    wild = [k in (WILDCARD, OPTIONAL) for k in label]
    last_opt = L > 0 and opt[L - 1]
    with np.errstate(invalid="ignore"):
        top = lp.max(axis=-1) if T else np.zeros(0)
    if not wrt and T:  # a row that is -inf throughout: log_softmax64 leaves nan there
        top = np.where(np.isneginf(np.asarray(x, dtype=np.float64).max(axis=-1)), NI, top)
        lp = np.where(np.isnan(lp), NI, lp)
    arg = argmax_tokens(x)
    lpx = np.concatenate([lp, top[:, None]], axis=1) if T else np.zeros((0, V + 1))
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    differ = lambda a, b: label[a] != label[b] or wild[a] or wild[b]
    if kind == "classic":
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)
        ext[1::2] = col
        reach = {k: np.zeros(S, dtype=bool) for k in (1, 2, 3, 4)}
        reach[1][1:] = True
        for i in range(1, L):
            reach[2][2 * i + 1] = differ(i, i - 1)
            if opt[i - 1]:
                reach[3][2 * i + 1] = True
                reach[4][2 * i + 1] = i >= 2 and differ(i, i - 2)
        ends = [S - 1] + ([S - 2] if L else [])
        if last_opt:
            ends += [S - 3] + ([S - 4] if L >= 2 else [])
        steps = (0, 1, 2, 3, 4)
        position = lambda s, k: (s - 1) // 2 if s % 2 else -1
    else:
        S = L + 1
        enter = np.concatenate([[blank], col]).astype(np.int64)
        stay = np.asarray([blank] + [V if w else blank for w in wild], dtype=np.int64)
        reach = {1: np.ones(S, dtype=bool), 2: np.zeros(S, dtype=bool)}
        reach[1][0] = False
        for l in range(2, S):
            reach[2][l] = opt[l - 2]
        ends = [S - 1] + ([S - 2] if last_opt else [])
        steps = (0, 1, 2)
        position = lambda s, k: s - 1 if (k > 0 or (s >= 1 and wild[s - 1])) else -1
    v = np.full(S, NI)
    v[0] = 0.0
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        cand = np.full((len(steps), S), NI)
        for k in steps:
            if k == 0:
                cand[0] = v if kind == "classic" else v + lpx[t, stay]
            else:
                cand[k] = np.where(reach[k], _from_below(v, k), NI) + (0.0 if kind == "classic" else lpx[t, enter])
        k = cand.argmax(axis=0)
        v = cand[k, np.arange(S)] + (lpx[t, ext] if kind == "classic" else 0.0)
        back[t] = k
    s = max(ends, key=lambda q: v[q])
    score = float(v[s])
    if not score > NI:
        return none
    path = np.zeros(T, dtype=np.int64)
    index = np.full(T, -1, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        k = int(back[t, s])
        i = position(s, k)
        if i >= 0:
            path[t] = arg[t] if wild[i] else label[i]
            index[t] = i
        else:
            path[t] = blank
        s -= k
    assert s == 0
    first, last = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    lscore = np.full(L, NI)
    for i in range(L):
        t = np.nonzero(index == i)[0]
        if len(t):
            first[i], last[i] = t[0], t[-1]
            assert np.array_equal(t, np.arange(t[0], t[-1] + 1))  # a label's frames are contiguous
            lscore[i] = sum(lp[q, path[q]] for q in t)
        else:
            assert opt[i]
            lscore[i] = 0.0
    return score, path, index, first, last, lscore


def best_path(kind, labels, x, ll, tl, blank=0, wrt=0):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B].  Returns (score[B] float64, [the rest of best_path_one or None] * B)."""
    labels, x = np.asarray(labels), np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    scores, rest = np.full(B, NI), []
    for b, Tb, Lb, lab in _rows(labels, ll, tl, T, labels.shape[1], blank):
        if lab is None:
            rest.append(None)
            continue
        r = best_path_one(kind, lab, x[b, :Tb], blank, wrt)
        scores[b] = r[0]
        rest.append(None if r[1] is None else r[1:])
    return scores, rest
