"""The best-path oracle (tests/tools/viterbi_oracle.py) against the definition: exhaustive enumeration of every path, the
closed form for uniform logits, and the bound score <= -loss (one path is at most the sum over all of them).  CPU only."""
import itertools

import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests._cases import load_known_answers, case_inputs
from tests.tools import viterbi_oracle as VO

KA = load_known_answers()


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("V", [2, 3, 4])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_oracle_against_every_path(T, V, wrt):
    rng = np.random.default_rng(100 * T + 10 * V + wrt)
    blank = int(rng.integers(0, V))
    x = rng.standard_normal((T, V)) * 2.0
    lp = x if wrt else VO.log_softmax64(x)
    best = {kind: {} for kind in VO.KINDS}  # label -> best value over the paths that reduce to it
    for path in itertools.product(range(V), repeat=T):
        val = float(lp[np.arange(T), list(path)].sum())
        for kind in VO.KINDS:
            key = tuple(VO.reduces_to(kind, path, blank))
            if val > best[kind].get(key, -np.inf):
                best[kind][key] = val
    tokens = [k for k in range(V) if k != blank]
    for n in range(0, 4):
        for label in itertools.product(tokens, repeat=n):
            for kind in VO.KINDS:
                score, path = VO.best_path_one(kind, label, x, blank, wrt)
                want = best[kind].get(tuple(label), -np.inf)
                if want == -np.inf:
                    assert score == -np.inf and path is None, (kind, label)
                    continue
                assert abs(score - want) <= 1e-12 * max(1.0, abs(want)), (kind, label, score, want)
                assert VO.reduces_to(kind, path, blank) == list(label), (kind, label, path)
                assert abs(VO.path_score(x, path, wrt) - want) <= 1e-12 * max(1.0, abs(want)), (kind, label, path)


def _uniform_cases():
    out = []
    for c in KA["cases"]:
        if "logits" in c:
            inp = case_inputs(c)
            if np.all(np.ptp(inp["logits"], axis=2) == 0):
                out.append((c["id"], c["kind"], inp))
    for c in KA["shape_cases"]:
        if "labels" in c:
            B, T, V = c["logits_shape"]
            out.append((c["id"], c["kind"], dict(
                labels=np.asarray(c["labels"], np.int32), logits=np.full((B, T, V), c.get("logits_fill", 0.0), np.float32),
                label_length=np.asarray(c["label_length"], np.int32), logit_length=np.asarray(c["logit_length"], np.int32),
                blank=int(c.get("blank", 0)))))
    return out


UNIFORM = _uniform_cases()


@pytest.mark.parametrize("cid,kind,inp", UNIFORM, ids=[u[0] for u in UNIFORM])
def test_uniform_logits(cid, kind, inp):
    """Every path has the value -T_b ln V, so that is the score of every feasible label; loss = +inf <=> score = -inf."""
    assert len(UNIFORM) >= 8
    x = inp["logits"]
    B, T, V = x.shape
    loss = O.ctc_loss(kind, inp["labels"], x, inp["label_length"], inp["logit_length"], inp["blank"]).loss
    score, paths = VO.best_path(kind, inp["labels"], x, inp["label_length"], inp["logit_length"], inp["blank"], 0)
    for b in range(B):
        Tb = min(int(inp["logit_length"][b]), T)
        if np.isinf(loss[b]):
            assert score[b] == -np.inf and paths[b] is None
        else:
            assert abs(score[b] + Tb * np.log(V)) <= 1e-12 * max(1, Tb)
            assert VO.reduces_to(kind, paths[b], inp["blank"]) == list(inp["labels"][b, :inp["label_length"][b]])
            assert len(paths[b]) == Tb


def test_uniform_cases_cover_the_infeasible_ones():
    ids = {u[0] for u in UNIFORM}
    assert {"classic_too_short_logit", "simplified_label_longer_than_logit", "simplified_zero_logit_length", "readme_example"} <= ids


@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("seed,T,V,U", [(0, 12, 6, 4), (1, 30, 5, 12), (2, 25, 17, 25), (3, 8, 3, 8)])
def test_score_is_at_most_minus_the_loss(kind, seed, T, V, U):
    inp = O.generate_ctc_loss_inputs(6, T, seed, V, max_label_length=U)
    loss = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0).loss
    score, paths = VO.best_path(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0, 0)
    for b in range(6):
        assert np.isinf(loss[b]) == (score[b] == -np.inf), (b, loss[b], score[b])
        if np.isfinite(loss[b]):
            assert score[b] <= -loss[b] + 1e-9 * max(1.0, abs(loss[b]))
            x = inp["logits"][b, :inp["logit_length"][b]]
            assert abs(VO.path_score(x, paths[b], 0) - score[b]) <= 1e-9 * max(1.0, abs(score[b]))
            assert VO.reduces_to(kind, paths[b], 0) == list(inp["labels"][b, :inp["label_length"][b]])
