"""Best-path (Viterbi) oracle for both CTC lattices: pure NumPy, float64, written from the definition.

A path is pi in [0, V)^T with value sum_t lp[t, pi_t], lp = log_softmax(x) (wrt == 1: x as it stands).
    classic:    maximise over the paths that give the label after collapsing repeats and then dropping blanks
    simplified: maximise over the paths that give the label after dropping blanks only
Classic runs on the textbook extended label sequence (blank, l_1, blank, l_2, ..., blank: 2L + 1 states), simplified on the
number of labels emitted (L + 1 states) -- neither is the state layout of the HIP kernel (csrc/ctc_align.hip)."""
import numpy as np

KINDS = ("classic", "simplified")


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _lp(x, wrt):
    return np.asarray(x, dtype=np.float64) if wrt else log_softmax64(x)


def reduces_to(kind, path, blank):
    """The label a path stands for: classic collapses repeats and then drops blanks, simplified drops blanks only."""
    out, prev = [], None
    for k in path:
        k = int(k)
        if kind == "classic":
            if k != blank and k != prev:
                out.append(k)
            prev = k
        elif k != blank:
            out.append(k)
    return out


def path_score(x, path, wrt=0):
    """Value of `path` (one token per row of x[T, V]) in float64."""
    lp = _lp(x, wrt)
    path = np.asarray(path, dtype=np.int64)
    assert path.shape == (lp.shape[0],)
    return float(lp[np.arange(lp.shape[0]), path].sum()) if len(path) else 0.0


def best_path_one(kind, label, x, blank=0, wrt=0):
    """One utterance: label (1-D, cut to its length), x[T, V] (cut to its length).  Returns (score, path); (-inf, None) when
    no path of finite value exists."""
    lp = _lp(x, wrt)
    T, V = lp.shape
    label = [int(k) for k in label]
    L = len(label)
    if any(k == blank or k < 0 or k >= V for k in label):
        return -np.inf, None
    if kind == "classic":
        ext = np.full(2 * L + 1, blank, dtype=np.int64)
        ext[1::2] = label
        S = 2 * L + 1
        skip = np.zeros(S, dtype=bool)  # s-2 -> s: onto a label that differs from the previous label
        for s in range(3, S, 2):
            skip[s] = ext[s] != ext[s - 2]
        ends = (S - 1, S - 2) if L else (0,)
    else:
        ext = np.asarray([blank] + label, dtype=np.int64)  # state l = labels emitted; entering l emits label[l-1], staying emits blank
        S = L + 1
        ends = (S - 1,)
    v = np.full(S, -np.inf)
    v[0] = 0.0
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        cand = np.full((3, S), -np.inf)
        if kind == "classic":
            e = lp[t, ext]
            cand[0] = v
            cand[1, 1:] = v[:-1]
            cand[2, 2:] = np.where(skip[2:], v[:-2], -np.inf)
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)] + e
        else:
            cand[0] = v + lp[t, blank]
            cand[1, 1:] = v[:-1] + lp[t, ext[1:]]
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)]
        back[t] = k
    s = max(ends, key=lambda q: v[q])
    score = float(v[s])
    if not score > -np.inf:
        return -np.inf, None
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        k = int(back[t, s])
        if kind == "classic":
            path[t] = ext[s]
        else:
            path[t] = ext[s] if k == 1 else blank
        s -= k
    assert s == 0
    return score, path


def best_path(kind, labels, x, ll, tl, blank=0, wrt=0):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B].  Returns (score[B] float64, [path or None] * B).  Lengths and labels are
    read by the input contract of DESIGN.md section 5.8, with U = the width of `labels`: logit_length clamped to [0, T], a negative
    label_length as 0, label_length > U infeasible, a label outside [0, V) or equal to the blank infeasible (best_path_one)."""
    labels, x = np.asarray(labels), np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    scores, paths = np.full(B, -np.inf), []
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        Lb = max(int(ll[b]), 0)
        if Lb > labels.shape[1]:
            paths.append(None)
            continue
        scores[b], p = best_path_one(kind, labels[b, :Lb], x[b, :Tb], blank, wrt)
        paths.append(p)
    return scores, paths
