"""Reference of ctc_amd_edit_distance and of the MWER loss.

edit_distance / edit_distances: the textbook dynamic programme on Python ints, unit cost for insertion, deletion and substitution,
with the lengths read as the C ABI reads them (clamped to the tensor's width; a reference longer than R gives -1).
edit_distance_rows: the same recurrence a row at a time in NumPy, for strings of a thousand tokens.

mwer_reference: float64 NumPy.  With loss_n the oracle's loss of hypothesis n (oracle.ctc_oracle, through
tests/tools/nbest_grad_oracle.py), F the hypotheses that are unmasked and have a finite loss, p_n = exp(-loss_n) / sum_{m in F}
exp(-loss_m) and W the mean of risk_n over F:
    loss[b] = sum_{n in F} p_n * (risk_n - W)
    dL/dx   = sum_{n in F} c_n * d loss_n / dx,    c_n = -p_n * (risk_n - sum_{m in F} p_m * risk_m)
(d p_n / d loss_m = -p_n * (delta_nm - p_m); W drops out because sum_n p_n = 1).  An utterance whose F is empty has loss 0 and a
zero gradient."""
import numpy as np

from tests.tools import nbest_grad_oracle as NG


def edit_distance(a, b) -> int:
    a, b = [int(t) for t in a], [int(t) for t in b]
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def edit_distance_rows(a, b) -> int:
    """The same number, one NumPy operation per row (for the long strings of the GPU tests; tests/test_edit_oracle.py holds it equal
    to edit_distance).  cur[j] = min(c[j], cur[j - 1] + 1) unrolls to cur[j] = j + min_{k <= j} (c[k] - k)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(len(b) + 1, dtype=np.int64)
    prev = j.copy()
    for i, x in enumerate(a, 1):
        c = np.empty_like(prev)
        c[0] = i
        c[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != x))
        prev = np.minimum.accumulate(c - j) + j
    return int(prev[-1])


def edit_distances(hyp, hyp_length, ref, ref_length, R=None, one=edit_distance):
    """distance[B, N] int32.  hyp [B, N, W], hyp_length [B, N], ref [B, Wr], ref_length [B]; R defaults to Wr."""
    hyp, hyp_length, ref, ref_length = np.asarray(hyp), np.asarray(hyp_length), np.asarray(ref), np.asarray(ref_length)
    B, N, W = hyp.shape
    Wr = ref.shape[1]
    R = Wr if R is None else R
    out = np.zeros((B, N), np.int32)
    for b in range(B):
        r = min(max(int(ref_length[b]), 0), Wr)
        for n in range(N):
            h = min(max(int(hyp_length[b, n]), 0), W)
            out[b, n] = -1 if r > R else one(hyp[b, n, :h], ref[b, :r])
    return out


def mwer_terms(loss, mask, risk):
    """(mwer[B], log_posterior[B, N], c[B, N]) in float64 from the hypotheses' losses [B, N], the mask and the risks."""
    loss, risk = np.asarray(loss, np.float64), np.asarray(risk, np.float64)
    used = np.asarray(mask, bool) & np.isfinite(loss)
    B, N = loss.shape
    mwer, logp, c = np.zeros(B), np.full((B, N), -np.inf), np.zeros((B, N))
    for b in range(B):
        f = used[b]
        if not f.any():
            continue
        nl = -loss[b, f]
        lse = nl.max() + np.log(np.exp(nl - nl.max()).sum())
        logp[b, f] = nl - lse
        p = np.exp(logp[b, f])
        mwer[b] = (p * (risk[b, f] - risk[b, f].mean())).sum()
        c[b, f] = -p * (risk[b, f] - (p * risk[b, f]).sum())
    return mwer, logp, c


def mwer_reference(kind, wrt, hyp, hyp_length, mask, x, logit_length, blank, ref, ref_length):
    """dict(loss[B], risk[B, N], log_posterior[B, N], grad[B, T, V], c[B, N]); hyp [B, N, W], hyp_length [B, N], mask [B, N] bool."""
    risk = edit_distances(hyp, hyp_length, ref, ref_length).astype(np.float64)
    zeros = np.zeros(np.asarray(hyp_length).shape)
    hyp_loss, _ = NG.nbest_loss_and_grad(kind, wrt, hyp, x, hyp_length, logit_length, blank, zeros)
    mwer, logp, c = mwer_terms(hyp_loss, mask, risk)
    _, grad = NG.nbest_loss_and_grad(kind, wrt, hyp, x, hyp_length, logit_length, blank, c)
    return dict(loss=mwer, risk=risk, log_posterior=logp, grad=grad, c=c, hyp_loss=hyp_loss)
