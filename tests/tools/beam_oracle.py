"""Prefix beam search oracle: NumPy / Python float64, written from the definition (include/ctc_amd.h, ctc_amd_beam_search).

Prefixes are tuples in a dict, so contributions to the same prefix add wherever they come from.  Masses are linear-domain float64
under lp = log_softmax(x) in float64 (wrt == 1: x as it stands), rescaled by a power of two per frame (exact) so that long
utterances do not underflow.  Candidates of a frame: the blank, and the min(K, V - 1) non-blank tokens with the largest float32
values, ties to the lowest index.

Besides the hypotheses the search returns its MARGIN: the smallest difference in ln(total mass) over every pruning decision (last
kept against first dropped) and every pair of neighbours of the returned list (the first hypothesis behind it included).  A second
implementation whose masses differ from these by less than the margin must return the same hypotheses in the same order."""
import math
from typing import List, NamedTuple, Tuple

import numpy as np

from tests.tools.viterbi_oracle import KINDS, log_softmax64  # noqa: F401


class Hypothesis(NamedTuple):
    labels: Tuple[int, ...]
    score: float  # ln of the total mass


class BeamResult(NamedTuple):
    hyps: List[Hypothesis]  # at most nbest, best first
    margin: float           # +inf when no decision was taken


def candidates(x32_row, blank, K):
    """Non-blank tokens of one frame inside the cut: the min(K, V - 1) largest float32 values, ties to the lowest index."""
    V = x32_row.shape[0]
    idx = [k for k in range(V) if k != blank]
    idx.sort(key=lambda k: (-float(x32_row[k]), k))  # (stable; -inf sorts last, NaN rows are unspecified)
    return idx[:min(K, V - 1)]


def search_one(kind, x, blank, wrt, W, K, nbest):
    """One utterance, x[T_b, V] cut to its length."""
    classic = kind == "classic"
    x32 = np.asarray(x, dtype=np.float32)
    T = x32.shape[0]
    if T:
        if wrt:
            lp = x32.astype(np.float64)
        else:
            with np.errstate(invalid="ignore"):
                lp = log_softmax64(x32)
            lp[np.isneginf(x32.max(axis=-1))] = -np.inf  # a row of -inf: every probability is 0
        with np.errstate(under="ignore"):
            prob = np.exp(lp)
    beam = {(): (1.0, 0.0)}  # prefix -> (pb, pnb); simplified keeps its one mass in pb
    scale = 0                # true mass = mass * 2^scale
    margin = math.inf
    for t in range(T):
        cand = candidates(x32[t], blank, K)
        p = prob[t]
        new = {}

        def add(y, pb, pnb):
            a = new.get(y, (0.0, 0.0))
            new[y] = (a[0] + pb, a[1] + pnb)

        for y, (pb, pnb) in beam.items():
            tot = pb + pnb
            add(y, tot * p[blank], 0.0)
            if classic and y and y[-1] in cand:
                add(y, 0.0, pnb * p[y[-1]])
            for c in cand:
                m = (pb if (classic and y and c == y[-1]) else tot) * p[c]
                if classic:
                    add(y + (c,), 0.0, m)
                else:
                    add(y + (c,), m, 0.0)
        ranked = sorted(((pb + pnb, y) for y, (pb, pnb) in new.items() if pb + pnb > 0.0), key=lambda e: -e[0])
        if len(ranked) > W:
            margin = min(margin, math.log(ranked[W - 1][0]) - math.log(ranked[W][0]))
            ranked = ranked[:W]
        beam = {y: new[y] for _, y in ranked}
        if ranked:
            e = math.frexp(ranked[0][0])[1]
            beam = {y: (math.ldexp(pb, -e), math.ldexp(pnb, -e)) for y, (pb, pnb) in beam.items()}
            scale += e
    ranked = sorted(((pb + pnb, y) for y, (pb, pnb) in beam.items()), key=lambda e: -e[0])
    for a, b in zip(ranked[:nbest], ranked[1:nbest + 1]):
        margin = min(margin, math.log(a[0]) - math.log(b[0]))
    return BeamResult([Hypothesis(y, math.log(m) + scale * math.log(2.0)) for m, y in ranked[:nbest]], margin)


def search(kind, x, tl, blank=0, wrt=0, beam_width=16, top_k=16, nbest=1):
    """Batch: x[B, T, V], tl[B] (clamped to [0, T]).  Returns (score[B, nbest] float64 with -inf for missing hypotheses,
    labels[B, nbest, T] int32 with -1 padding, label_length[B, nbest] int32, margin[B])."""
    x = np.asarray(x)
    B, T = x.shape[0], x.shape[1]
    score = np.full((B, nbest), -np.inf)
    labels = np.full((B, nbest, T), -1, np.int32)
    length = np.zeros((B, nbest), np.int32)
    margin = np.full(B, np.inf)
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        res = search_one(kind, x[b, :Tb], blank, wrt, beam_width, top_k, nbest)
        margin[b] = res.margin
        for n, h in enumerate(res.hyps):
            score[b, n] = h.score
            labels[b, n, :len(h.labels)] = h.labels
            length[b, n] = len(h.labels)
    return score, labels, length, margin
