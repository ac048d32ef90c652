"""Best-path oracle for forced alignment with wildcard labels on both CTC lattices: pure NumPy, float64, written from the
definition in include/ctc_amd.h (ctc_amd_wildcard_best_path).

A label equal to WILDCARD (-2) stands for any non-empty run of frames with any tokens on them.  With lp = log_softmax(x)
(wrt == 1: x as it stands) such a run is worth sum_t max_k lp[t, k], and the tokens reported for it are the lowest k holding the
maximum of the float32 row the kernel reads.
    classic     the textbook extended label sequence (blank, l_1, blank, l_2, ..., blank: 2L + 1 states).  A wildcard's state emits
                the row maximum; the skip s-2 -> s is allowed when the two labels differ or one of them is a wildcard.
    simplified  the number of labels emitted (L + 1 states).  Entering a wildcard costs the row maximum, and so does staying in the
                state behind it (where an ordinary label's state costs the blank).
Neither is the state layout of the HIP kernel (csrc/ctc_align_wild.hip)."""
import numpy as np

from tests.tools.viterbi_oracle import KINDS, log_softmax64  # noqa: F401

WILDCARD = -2


def _lp(x, wrt):
    return np.asarray(x, dtype=np.float64) if wrt else log_softmax64(x)


def argmax_tokens(x):
    """a_t: the lowest index holding the maximum of every float32 row."""
    x32 = np.asarray(x, dtype=np.float32)
    return x32.argmax(axis=-1).astype(np.int64) if x32.shape[0] else np.zeros(0, np.int64)


def path_score(x, path, wrt=0):
    """Value of `path` (one token per row of x[T, V]) in float64, summed in time order."""
    lp = _lp(x, wrt)
    s = 0.0
    for t, k in enumerate(path):
        s += float(lp[t, int(k)])
    return s


def best_path_one(kind, label, x, blank=0, wrt=0):
    """One utterance: label (1-D, cut to its length), x[T, V] (cut to its length).  Returns (score, path, label_index);
    (-inf, None, None) when no path of finite value exists."""
    lp = _lp(x, wrt)
    T, V = lp.shape
    label = [int(k) for k in label]
    L = len(label)
    if any(k != WILDCARD and (k == blank or k < 0 or k >= V) for k in label):
        return -np.inf, None, None
    with np.errstate(invalid="ignore"):
        top = lp.max(axis=-1) if T else np.zeros(0)
    if not wrt and T:  # a row that is -inf throughout: log_softmax64 leaves nan there
        top = np.where(np.isneginf(np.asarray(x, dtype=np.float64).max(axis=-1)), -np.inf, top)
        lp = np.where(np.isnan(lp), -np.inf, lp)
    arg = argmax_tokens(x)
    wild = [k == WILDCARD for k in label]

    # lpx: lp with the row maximum as column V, the column a wildcard reads
    lpx = np.concatenate([lp, top[:, None]], axis=1) if T else np.zeros((0, V + 1))
    col = np.asarray([V if w else k for k, w in zip(label, wild)], dtype=np.int64)
    if kind == "classic":
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)  # the column every state emits
        ext[1::2] = col
        pos = [(s - 1) // 2 if s % 2 else -1 for s in range(S)]  # label position of an odd state
        skip = np.zeros(S, dtype=bool)  # s-2 -> s: onto a label that differs from the previous one, or beside a wildcard
        for s in range(3, S, 2):
            i = pos[s]
            skip[s] = label[i] != label[i - 1] or wild[i] or wild[i - 1]
        ends = (S - 1, S - 2) if L else (0,)
    else:
        S = L + 1
        enter = np.concatenate([[blank], col]).astype(np.int64)  # entering state l emits label l - 1
        stay = np.asarray([blank] + [V if w else blank for w in wild], dtype=np.int64)  # staying behind a wildcard costs the maximum
        ends = (S - 1,)
    v = np.full(S, -np.inf)
    v[0] = 0.0
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(T):
        cand = np.full((3, S), -np.inf)
        if kind == "classic":
            cand[0] = v
            cand[1, 1:] = v[:-1]
            cand[2, 2:] = np.where(skip[2:], v[:-2], -np.inf)
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)] + lpx[t, ext]
        else:
            cand[0] = v + lpx[t, stay]
            cand[1, 1:] = v[:-1] + lpx[t, enter[1:]]
            k = cand.argmax(axis=0)
            v = cand[k, np.arange(S)]
        back[t] = k
    s = max(ends, key=lambda q: v[q])
    score = float(v[s])
    if not score > -np.inf:
        return -np.inf, None, None
    path = np.zeros(T, dtype=np.int64)
    index = np.full(T, -1, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        k = int(back[t, s])
        if kind == "classic":
            i = pos[s]
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


def best_path(kind, labels, x, ll, tl, blank=0, wrt=0):
    """Batch: labels[B, U], x[B, T, V], ll[B], tl[B].  Returns (score[B] float64, [path or None] * B, [label_index or None] * B).
    Lengths by the input contract of DESIGN.md section 5.8 with U = the width of `labels` (tests/tools/viterbi_oracle.best_path)."""
    labels, x = np.asarray(labels), np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    scores, paths, indices = np.full(B, -np.inf), [], []
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        Lb = max(int(ll[b]), 0)
        if Lb > labels.shape[1]:
            paths.append(None); indices.append(None)
            continue
        scores[b], p, i = best_path_one(kind, labels[b, :Lb], x[b, :Tb], blank, wrt)
        paths.append(p); indices.append(i)
    return scores, paths, indices
