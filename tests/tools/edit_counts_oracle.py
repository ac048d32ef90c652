"""Reference of ctc_amd_edit_counts: the lexicographic minimum of (distance, substitutions, insertions)
over all alignments of a hypothesis with a reference.  Rows are hypothesis tokens, columns reference tokens; a move up is an
insertion (1, 0, 1), a move left a deletion (1, 0, 0), a diagonal move a hit (0, 0, 0) or a substitution (1, 1, 0).

edit_counts:       the recurrence on Python tuples (tuples compare lexicographically), boundaries (j, 0, 0) and (i, 0, i).
edit_counts_rows:  the same a row at a time in NumPy on the packed word d * 2^42 + S * 2^21 + I, for strings of tens of thousands
                   of tokens: cur[j] = min(c[j], cur[j - 1] + DEL) unrolls to cur[j] = j * DEL + min_{k <= j} (c[k] - k * DEL).
edit_counts_paths: a memoised recursion over all alignments that names no table: for tiny inputs.
edit_counts_batch: counts[B, N, 4] = (distance, substitutions, insertions, deletions) with the lengths read as the C ABI reads
                   them (clamped to the tensor's width; a reference longer than R gives -1 four times)."""
import functools

import numpy as np

DEL, SUB, INS = 1 << 42, (1 << 42) + (1 << 21), (1 << 42) + 1
FIELD = (1 << 21) - 1


def edit_counts(a, b):
    """(d, S, I) on Python ints."""
    a, b = [int(t) for t in a], [int(t) for t in b]
    prev = [(j, 0, 0) for j in range(len(b) + 1)]
    for i, x in enumerate(a, 1):
        cur = [(i, 0, i)]
        for j, y in enumerate(b, 1):
            up, left, diag = prev[j], cur[j - 1], prev[j - 1]
            cur.append(min((up[0] + 1, up[1], up[2] + 1), (left[0] + 1, left[1], left[2]),
                           diag if x == y else (diag[0] + 1, diag[1] + 1, diag[2])))
        prev = cur
    return prev[-1]


def unpack(w):
    w = int(w)
    return w >> 42, (w >> 21) & FIELD, w & FIELD


def edit_counts_rows(a, b):
    """(d, S, I), one NumPy operation per row; lengths up to 2^20 (each field fits 21 bits, the word a signed int64)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    assert len(a) <= 1 << 20 and len(b) <= 1 << 20
    jd = np.arange(len(b) + 1, dtype=np.int64) * DEL
    prev = jd.copy()
    for i, x in enumerate(a, 1):
        c = np.empty_like(prev)
        c[0] = i * INS
        c[1:] = np.minimum(prev[1:] + INS, prev[:-1] + np.where(b != x, SUB, 0))
        prev = np.minimum.accumulate(c - jd) + jd
    return unpack(prev[-1])


def edit_counts_paths(a, b):
    """(d, S, I) as the minimum over all alignments, by recursion on the suffixes still to align."""
    a, b = tuple(int(t) for t in a), tuple(int(t) for t in b)

    @functools.lru_cache(maxsize=None)
    def best(i, j):  # the cheapest way to align a[i:] with b[j:]
        if i == len(a):
            return (len(b) - j, 0, 0)
        if j == len(b):
            return (len(a) - i, 0, len(a) - i)
        t = best(i + 1, j)
        cands = [(t[0] + 1, t[1], t[2] + 1)]
        t = best(i, j + 1)
        cands.append((t[0] + 1, t[1], t[2]))
        t = best(i + 1, j + 1)
        cands.append(t if a[i] == b[j] else (t[0] + 1, t[1] + 1, t[2]))
        return min(cands)

    return best(0, 0)


def edit_counts_batch(hyp, hyp_length, ref, ref_length, R=None, one=edit_counts):
    """counts[B, N, 4] int32.  hyp [B, N, W], hyp_length [B, N], ref [B, Wr], ref_length [B]; R defaults to Wr."""
    hyp, hyp_length, ref, ref_length = np.asarray(hyp), np.asarray(hyp_length), np.asarray(ref), np.asarray(ref_length)
    B, N, W = hyp.shape
    Wr = ref.shape[1]
    R = Wr if R is None else R
    out = np.zeros((B, N, 4), np.int32)
    for b in range(B):
        r = min(max(int(ref_length[b]), 0), Wr)
        for n in range(N):
            h = min(max(int(hyp_length[b, n]), 0), W)
            if r > R:
                out[b, n] = -1
            else:
                d, s, i = one(hyp[b, n, :h], ref[b, :r])
                out[b, n] = (d, s, i, d - s - i)
    return out
