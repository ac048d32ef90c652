"""The greedy-decoding oracle (tests/tools/greedy_oracle.py) against brute force and a direct restatement: no GPU.

For T <= 5 and V <= 3 every one of the V^T paths is scored; the oracle's path must have the maximal score (the frame-wise
argmax is the unconstrained optimum) and be the lexicographically lowest among the maximal ones (ties to the lowest token)."""
import itertools

import numpy as np
import pytest

from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO


def restate(kind, tokens, plp, blank):
    """decoded / frames / label_score straight from the wording of the header."""
    labels, frames, scores = [], [], []
    for t, k in enumerate(tokens):
        k = int(k)
        if k == blank:
            continue
        if kind == "classic":
            if t > 0 and int(tokens[t - 1]) == k:
                scores[-1] += float(plp[t])  # the unbroken repeat goes on
                continue
        labels.append(k); frames.append(t); scores.append(float(plp[t]))
    return labels, frames, scores


def cases():
    rng = np.random.default_rng(0)
    out = []
    for T in range(0, 6):
        for V in (1, 2, 3):
            for blank in sorted({0, V - 1}):
                out.append((f"T{T}-V{V}-blank{blank}-random", rng.standard_normal((T, V)).astype(np.float32), blank))
                out.append((f"T{T}-V{V}-blank{blank}-halves", (rng.integers(0, 3, (T, V)) / 2).astype(np.float32), blank))  # many ties
    out.append(("all-ties", np.zeros((5, 3), np.float32), 0))
    out.append(("all-ties-blank2", np.zeros((5, 3), np.float32), 2))
    out.append(("nonzero-blank", np.asarray([[0, 2, 1], [0, 2, 1], [3, 0, 0], [0, 0, 3], [0, 0, 3]], np.float32), 1))
    return out


CASES = cases()


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("name,x,blank", CASES, ids=[c[0] for c in CASES])
def test_oracle_path_is_the_optimum_of_all_paths(name, x, blank, kind, wrt):
    T, V = x.shape
    score, tokens, labels, frames, label_score = GO.decode_one(kind, x, blank, wrt)
    best, best_path = -np.inf, None
    for path in itertools.product(range(V), repeat=T):  # lexicographic order: the first maximum has the lowest tokens
        s = VO.path_score(x, path, wrt)
        if s > best + 1e-12:
            best, best_path = s, path
    assert abs(score - best) <= 1e-12 * max(1.0, abs(best))
    assert abs(VO.path_score(x, tokens, wrt) - best) <= 1e-12 * max(1.0, abs(best))
    # ties to the lowest index, frame by frame
    for t in range(T):
        assert x[t, tokens[t]] == x[t].max() and not np.any(x[t, :tokens[t]] == x[t].max())
    if T:
        exact_ties_only = all(np.sum(np.isclose(x[t], x[t].max(), atol=1e-6)) == np.sum(x[t] == x[t].max()) for t in range(T))
        if exact_ties_only and wrt == 1:
            assert tuple(int(k) for k in tokens) == best_path
    lp = np.asarray(x, np.float64) if wrt else VO.log_softmax64(x)
    plp = lp[np.arange(T), tokens] if T else np.zeros(0)
    want = restate(kind, tokens, plp, blank)
    assert labels == want[0] == VO.reduces_to(kind, tokens, blank)
    assert frames == want[1]
    assert np.allclose(label_score, want[2], rtol=0, atol=1e-12)
    if kind == "simplified":
        assert len(labels) == int(np.sum(tokens != blank))
        assert np.allclose(label_score, plp[tokens != blank], rtol=0, atol=0)
    # blank frames count towards the score only
    if wrt == 0:  # (log-probabilities are <= 0, so the blank frames can only lower the score)
        assert score <= sum(label_score) + 1e-9


def test_named_examples():
    # all ties: token 0 everywhere; with blank 0 nothing is decoded, with blank 2 one label (classic) or five (simplified)
    z = np.zeros((5, 3), np.float32)
    assert GO.decode_one("classic", z, 0)[2] == [] and GO.decode_one("simplified", z, 0)[2] == []
    s, tok, lab, frm, ls = GO.decode_one("classic", z, 2)
    assert list(tok) == [0] * 5 and lab == [0] and frm == [0] and abs(ls[0] - 5 * np.log(1 / 3)) < 1e-12 and abs(s - ls[0]) < 1e-12
    s, tok, lab, frm, ls = GO.decode_one("simplified", z, 2)
    assert lab == [0] * 5 and frm == [0, 1, 2, 3, 4] and np.allclose(ls, np.log(1 / 3))
    # a non-zero blank between two runs of the same token
    x = np.asarray([[5, 0, 0], [0, 5, 0], [5, 0, 0], [5, 0, 0]], np.float32)
    assert GO.decode_one("classic", x, 1)[2:4] == ([0, 0], [0, 2])
    assert GO.decode_one("simplified", x, 1)[2:4] == ([0, 0, 0], [0, 2, 3])
    assert GO.decode_one("classic", x, 2)[2:4] == ([0, 1, 0], [0, 1, 2])


def test_batch_layout_and_padding():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, 6, 3)).astype(np.float32)
    tl = np.asarray([6, 0, 3, 9])
    d = GO.decode("classic", x, tl, blank=0)
    assert d.tokens.shape == d.labels.shape == d.frames.shape == d.label_score.shape == (4, 6)
    assert d.score[1] == 0.0 and d.label_length[1] == 0 and np.all(d.tokens[1] == -1)
    assert np.all(d.tokens[2, 3:] == -1) and np.all(d.tokens[3] >= 0)  # a length beyond T is clamped
    for b in range(4):
        n = d.label_length[b]
        assert np.all(d.labels[b, n:] == -1) and np.all(d.frames[b, n:] == -1) and np.all(np.isneginf(d.label_score[b, n:]))
        assert np.all(d.labels[b, :n] > 0) and np.all(np.diff(d.frames[b, :n]) > 0)
    # an all -inf row of log-probabilities: score -inf, token 0 there
    lp = VO.log_softmax64(x).astype(np.float32)
    lp[0, 2, :] = -np.inf
    d = GO.decode("simplified", lp, tl, blank=0, wrt=1)
    assert d.score[0] == -np.inf and d.tokens[0, 2] == 0 and np.isfinite(d.score[2])
    d = GO.decode("simplified", lp, tl, blank=0, wrt=0)  # the same row as logits
    assert d.score[0] == -np.inf and d.tokens[0, 2] == 0
