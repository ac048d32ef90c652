"""Greedy CTC decoding oracle: pure NumPy, float64, written from the definition (include/ctc_amd.h, ctc_amd_greedy_decode).

Per frame the LOWEST token index holding the row maximum of the float32 values the kernel reads; lp = log_softmax(x) in float64
(wrt == 1: x as it stands); score = sum of lp over the frames inside logit_length; the path collapsed with
viterbi_oracle.reduces_to; per decoded label its first frame and the lp of its run (classic: the unbroken repeat of the token
that starts there; simplified: that one frame)."""
from typing import NamedTuple

import numpy as np

from tests.tools.viterbi_oracle import KINDS, log_softmax64, reduces_to  # noqa: F401


class Decoding(NamedTuple):
    score: np.ndarray         # [B] float64
    tokens: np.ndarray        # [B, T] int32, -1 beyond logit_length
    labels: np.ndarray        # [B, T] int32, -1 beyond label_length
    label_length: np.ndarray  # [B] int32
    frames: np.ndarray        # [B, T] int32, -1 padding
    label_score: np.ndarray   # [B, T] float64, -inf padding


def decode_one(kind, x, blank=0, wrt=0):
    """One utterance, x[T, V] cut to its length.  Returns (score, tokens[T], labels, frames, label_score) with Python lists for
    the three per-label results."""
    x32 = np.asarray(x, dtype=np.float32)
    T = x32.shape[0]
    tokens = x32.argmax(axis=-1).astype(np.int32) if T else np.zeros(0, np.int32)  # (numpy: the first maximum, i.e. the lowest index)
    lp = np.asarray(x32, dtype=np.float64) if wrt else log_softmax64(x32)
    with np.errstate(invalid="ignore"):
        plp = lp[np.arange(T), tokens] if T else np.zeros(0)
    if not wrt:  # a row whose maximum is -inf has log-probability -inf (log_softmax64 leaves x - 0 - log(0) = nan there)
        plp = np.where(np.isneginf(x32.max(axis=-1)) if T else np.zeros(0, bool), -np.inf, plp)
    score = 0.0
    for v in plp:  # time order
        score += float(v)
    labels, frames, label_score = [], [], []
    t = 0
    while t < T:
        k = int(tokens[t])
        e = t + 1
        if kind == "classic":
            while e < T and int(tokens[e]) == k:
                e += 1
        if k != blank:
            labels.append(k)
            frames.append(t)
            s = 0.0
            for u in range(t, e):
                s += float(plp[u])
            label_score.append(s)
        t = e
    assert labels == reduces_to(kind, tokens, blank)
    return score, tokens, labels, frames, label_score


def decode(kind, x, tl, blank=0, wrt=0):
    """Batch: x[B, T, V], tl[B] (clamped to [0, T] as the loss does)."""
    x = np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    out = Decoding(np.zeros(B), np.full((B, T), -1, np.int32), np.full((B, T), -1, np.int32), np.zeros(B, np.int32),
                   np.full((B, T), -1, np.int32), np.full((B, T), -np.inf))
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        score, tokens, labels, frames, label_score = decode_one(kind, x[b, :Tb], blank, wrt)
        n = len(labels)
        out.score[b] = score
        out.tokens[b, :Tb] = tokens
        out.labels[b, :n] = labels
        out.label_length[b] = n
        out.frames[b, :n] = frames
        out.label_score[b, :n] = label_score
    return out
