"""Float64 reference of ctc_amd_nbest_loss_grad: the gradient of sum_n weight[b, n] * loss[b, n] with
respect to the shared logits (wrt = 0) or log-probabilities (wrt = 1), one hypothesis at a time from the project's own oracle:

    sum_n where(isfinite(loss_n), O.logits_gradient(O.ctc_loss(kind, labels[:, n], x64, ll[:, n], tl, blank), x64, d_loss=w[:, n]), 0)

and, for wrt = 1, w[:, n] * data.gradient of O.LOSS_DATA[kind] on the input as it stands.  A hypothesis whose loss is not finite
contributes exactly zero and its weight is not looked at (it may be NaN or infinite).  Padding labels (outside [0, V)) are
replaced by a valid token, as tests/test_gpu_nbest_loss.py::oracle does: the oracle indexes a row with every label position but
reads nothing of the padding into its result."""
import numpy as np

from oracle import ctc_oracle as O


def nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, blank, weight):
    """(loss[B, N], grad[B, T, V]) in float64.  labels [B, N, W], ll [B, N], tl [B], weight [B, N]."""
    labels, ll, weight = np.asarray(labels), np.asarray(ll), np.asarray(weight, np.float64)
    x64 = np.asarray(x, np.float64)
    B, T, V = x64.shape
    safe = np.where((labels < 0) | (labels >= V), (blank + 1) % V, labels)
    grad = np.zeros((B, T, V), np.float64)
    losses = []
    with np.errstate(all="ignore"):
        for n in range(labels.shape[1]):
            if wrt:
                data = O.LOSS_DATA[kind](safe[:, n], x64, ll[:, n], tl, blank, np.float64)
            else:
                data = O.ctc_loss(kind, safe[:, n], x64, ll[:, n], tl, blank)
            loss = np.asarray(data.loss, np.float64)
            fin = np.isfinite(loss)
            w = np.where(fin, weight[:, n], 0.0)  # not interpreted where the loss is not finite
            g = np.asarray(data.gradient, np.float64) * w[:, None, None] if wrt else O.logits_gradient(data, x64, d_loss=w)
            grad += np.where(fin[:, None, None], np.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0), 0.0)
            losses.append(loss)
    grad[np.arange(T)[None, :] >= np.clip(np.asarray(tl), 0, T)[:, None]] = 0.0
    return np.stack(losses, axis=1), grad


def nbest_grad(kind, wrt, labels, x, ll, tl, blank, weight):
    return nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, blank, weight)[1]
