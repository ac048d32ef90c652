"""The float64 reference of the N-best gradient (tests/tools/nbest_grad_oracle.py) against central differences of
sum_n weight[b, n] * loss[b, n] over the feasible hypotheses, on both lattices and for both `wrt`: pins the sign and the softmax
convention of the helper that the GPU tests compare against.  No GPU."""
import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import nbest_grad_oracle as NG


def case():
    rng = np.random.default_rng(2)
    B, T, V, N, W = 2, 7, 5, 3, 4
    x = rng.standard_normal((B, T, V))
    tl = np.asarray([T, 5], np.int32)
    labels = rng.integers(1, V, (B, N, W)).astype(np.int32)
    ll = np.asarray([[2, 0, 3], [4, 1, 2]], np.int32)
    labels[1, 0] = 2          # four equal labels need 7 frames on the classic lattice, 4 on the simplified: utterance 1 has 5
    labels[:, :, 3:] = -1     # padding as a beam search writes it ...
    labels[1, 0, 3] = 2       # ... except where the label is that long
    w = rng.standard_normal((B, N))
    return x, tl, labels, ll, w


def objective(kind, wrt, labels, x, ll, tl, w, fin):
    loss, _ = NG.nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, 0, np.zeros_like(w))
    return float(np.where(fin, w * np.where(fin, loss, 0.0), 0.0).sum())


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", ["classic", "simplified"])
def test_reference_gradient_matches_central_differences(kind, wrt):
    x, tl, labels, ll, w = case()
    if wrt:
        x = O.logit_to_logproba(x, 2)
    loss, grad = NG.nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, 0, w)
    fin = np.isfinite(loss)
    if kind == "classic":
        assert not fin[1, 0] and fin.sum() == fin.size - 1, "one infeasible hypothesis"
    assert not np.isnan(grad).any()
    assert np.all(grad[1, 5:] == 0.0), "zeros beyond T_b"
    w_bad = w.copy()
    w_bad[~fin] = np.nan      # the weight of an infeasible hypothesis is not interpreted
    assert np.array_equal(NG.nbest_grad(kind, wrt, labels, x, ll, tl, 0, w_bad), grad)
    h = 1e-5
    num = np.zeros_like(grad)
    for b in range(x.shape[0]):
        for t in range(int(tl[b])):
            for k in range(x.shape[2]):
                xp, xm = x.copy(), x.copy()
                xp[b, t, k] += h
                xm[b, t, k] -= h
                num[b, t, k] = (objective(kind, wrt, labels, xp, ll, tl, w, fin) - objective(kind, wrt, labels, xm, ll, tl, w, fin)) / (2 * h)
    err = float(np.abs(num - grad).max())
    print(f"NBEST-GRAD-ORACLE {kind} wrt={wrt}: worst |central difference - reference| {err:.3e}")
    # central differences of step h: truncation h^2 |f'''| / 6 ~ 1e-10, rounding eps |f| / h ~ 1e-16 * 30 / 1e-5 = 3e-10
    assert err < 2e-9, err
    assert np.abs(grad).max() > 0.1, "a gradient to speak of"
