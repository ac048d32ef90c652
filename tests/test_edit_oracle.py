"""The references of tests/tools/edit_oracle.py: the edit distance on known answers and on the properties of a metric, the MWER
reference against central differences of itself.  No GPU."""
import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import edit_oracle as E


def test_known_answers():
    assert E.edit_distance(b"kitten", b"sitting") == 3
    assert E.edit_distance(b"sitting", b"kitten") == 3
    assert E.edit_distance([], []) == 0
    for k in (1, 2, 7, 100):
        assert E.edit_distance([], range(k)) == k == E.edit_distance(range(k), [])
        assert E.edit_distance(range(k), range(k)) == 0
    base = [5, 1, 4, 1, 5, 9, 2, 6]
    for pos in (0, 3, len(base) - 1):
        assert E.edit_distance(base[:pos] + base[pos + 1:], base) == 1, "one deletion"
        assert E.edit_distance(base[:pos] + [77] + base[pos:], base) == 1, "one insertion"
        assert E.edit_distance(base[:pos] + [77] + base[pos + 1:], base) == 1, "one substitution"
    assert E.edit_distance(base + [77], base) == 1
    assert E.edit_distance([1, 2, 3], [4, 5, 6, 7]) == 4, "disjoint alphabets: max(h, r)"
    assert E.edit_distance([-1, 2 ** 31 - 1], [2 ** 31 - 1, -1]) == 2, "any int32 is a token"


@pytest.mark.parametrize("alphabet", [2, 50])
def test_metric_properties(alphabet):
    rng = np.random.default_rng(alphabet)
    strings = [rng.integers(0, alphabet, int(n)).tolist() for n in rng.integers(0, 14, 24)]
    d = [[E.edit_distance(a, b) for b in strings] for a in strings]
    for i, a in enumerate(strings):
        assert d[i][i] == 0
        for j, b in enumerate(strings):
            assert d[i][j] == d[j][i], "symmetry"
            assert abs(len(a) - len(b)) <= d[i][j] <= max(len(a), len(b))
            assert (d[i][j] == 0) == (a == b)
            for k in range(len(strings)):
                assert d[i][k] <= d[i][j] + d[j][k], "triangle inequality"


def test_row_form_equals_the_plain_one():
    rng = np.random.default_rng(11)
    for alphabet in (2, 50):
        for _ in range(60):
            a = rng.integers(0, alphabet, int(rng.integers(0, 40)))
            b = rng.integers(0, alphabet, int(rng.integers(0, 40)))
            assert E.edit_distance_rows(a, b) == E.edit_distance(a, b)
    assert E.edit_distance_rows([], []) == 0 and E.edit_distance_rows([3], []) == 1 and E.edit_distance_rows([], [3, 4]) == 2
    assert E.edit_distance_rows([-1, 2 ** 31 - 1], [2 ** 31 - 1, -1]) == 2


def test_batched_form_reads_lengths_as_the_abi_does():
    hyp = np.asarray([[[1, 2, 3, -1], [1, 2, 3, 4]], [[7, 7, 7, 7], [9, 9, 9, 9]]], np.int32)
    hl = np.asarray([[3, 9], [-2, 1]], np.int32)          # beyond the width: clamped; negative: empty
    ref = np.asarray([[1, 2, 4], [7, 8, 9]], np.int32)
    rl = np.asarray([3, 2], np.int32)
    assert E.edit_distances(hyp, hl, ref, rl).tolist() == [[1, 1], [2, 2]]
    assert E.edit_distances(hyp, hl, ref, rl, R=2).tolist() == [[-1, -1], [2, 2]]
    assert E.edit_distances(hyp, hl, ref, np.asarray([5, -1])).tolist() == [[1, 1], [0, 1]]


def case():
    rng = np.random.default_rng(5)
    B, T, V, N, W = 3, 7, 5, 4, 4
    x = rng.standard_normal((B, T, V))
    tl = np.asarray([T, 5, 2], np.int32)
    hyp = rng.integers(1, V, (B, N, W)).astype(np.int32)
    hl = np.asarray([[2, 0, 3, 2], [4, 1, 2, 3], [3, 4, 3, 0]], np.int32)
    hyp[0, 3] = hyp[0, 0]      # a duplicate
    hyp[1, 0] = 2              # four equal labels: infeasible in five frames on the classic lattice
    hyp[:, :, 3:] = -1
    hyp[1, 0, 3] = 2
    mask = np.ones((B, N), bool)
    mask[0, 2] = False
    mask[2, 3] = False         # utterance 2: two frames, three hypotheses of 3 or 4 labels and a masked empty one -- nothing is used
    ref = rng.integers(1, V, (B, 3)).astype(np.int32)
    rl = np.asarray([3, 2, 1], np.int32)
    return x, tl, hyp, hl, mask, ref, rl


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", ["classic", "simplified"])
def test_mwer_reference_matches_central_differences(kind, wrt):
    x, tl, hyp, hl, mask, ref, rl = case()
    if wrt:
        x = O.logit_to_logproba(x, 2)
    out = E.mwer_reference(kind, wrt, hyp, hl, mask, x, tl, 0, ref, rl)
    assert np.array_equal(out["risk"], E.edit_distances(hyp, hl, ref, rl))
    used = mask & np.isfinite(out["hyp_loss"])
    assert not used[2].any() and out["loss"][2] == 0.0 and np.all(out["grad"][2] == 0.0), "an utterance without a used hypothesis"
    assert used[0].sum() == 3 and (kind == "simplified" or not used[1, 0])
    assert np.array_equal(np.isneginf(out["log_posterior"]), ~used)
    assert np.allclose(np.exp(out["log_posterior"]).sum(axis=1), [1.0, 1.0, 0.0], atol=1e-12)
    assert not np.isnan(out["grad"]).any()

    def objective(xx):
        return float(E.mwer_reference(kind, wrt, hyp, hl, mask, xx, tl, 0, ref, rl)["loss"].sum())

    h = 1e-5
    num = np.zeros_like(x)
    for b in range(x.shape[0]):
        for t in range(int(tl[b])):
            for k in range(x.shape[2]):
                xp, xm = x.copy(), x.copy()
                xp[b, t, k] += h
                xm[b, t, k] -= h
                num[b, t, k] = (objective(xp) - objective(xm)) / (2 * h)
    err = float(np.abs(num - out["grad"]).max())
    print(f"MWER-ORACLE {kind} wrt={wrt}: worst |central difference - reference| {err:.3e}, largest |grad| {np.abs(out['grad']).max():.3g}")
    # central differences of step h: truncation h^2 |f'''| / 6 ~ 1e-10, rounding eps |f| / h ~ 1e-16 * 30 / 1e-5 = 3e-10
    # (the bound of tests/test_nbest_grad_oracle.py for the same losses)
    assert err < 2e-9, err
    assert np.abs(out["grad"]).max() > 0.01, "a gradient to speak of"
