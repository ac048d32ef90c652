"""The MWER loss (classic_ctc_mwer_loss, simplified_ctc_mwer_loss, ctc_mwer_loss_from_logproba) against the
float64 reference of tests/tools/edit_oracle.py, at B = 3, T = 12, V = 6, N = 4, U <= 4.

Tolerances (derived, not measured).  `risk` is an integer: exact.  The loss and the gradient are linear combinations of the
hypotheses' losses and gradients with the coefficients c_n of the reference, so the project's 1e-4 for a hypothesis loss and
gradient against the oracle (tests/test_gpu_nbest_loss_grad.py) carries through as 1e-4 * max(1, sum_n |c_n|) per utterance.
log_posterior = -loss_n - logsumexp(-loss): every loss is within tol = 1e-4 + 1e-6 |loss| of the oracle
(tests/test_gpu_nbest_loss.py) and a log-sum-exp moves by at most the largest move of its arguments, so 2 * max_n tol, plus the
float32 rounding of the result, 1e-6 |log_posterior|.  Every worst figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from oracle import ctc_oracle as O
from tests.tools import edit_oracle as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ENTRIES = ("classic", "simplified", "classic-logproba", "simplified-logproba")


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a, dtype), device=DEV)


def call(entry, labels, x, ll, tl, blank=0, **kw):
    import tf_seq2seq_losses_amd as ctc
    kind = entry.split("-")[0]
    if entry.endswith("logproba"):
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        return ctc.ctc_mwer_loss_from_logproba(labels, x, ll, tl, blank, cls, **kw)
    return (ctc.classic_ctc_mwer_loss if kind == "classic" else ctc.simplified_ctc_mwer_loss)(labels, x, ll, tl, blank, **kw)


@functools.lru_cache(maxsize=None)
def case(V=6, blank=0):
    """Explicit lists with a duplicate, a masked entry, an entry infeasible for the lattice and an utterance without a feasible entry.
    Another V or blank: new logits, and the same lists on five tokens spread from the first to the last non-blank column (token i
    of the default draw becomes the i-th of them), so that the risks are those of the default draw; those five columns and the
    blank's are raised by ln(V / 6), so that the list's posterior is spread as it is at V = 6 (unbiased, one entry holds all of it
    up to 1e-15, and the loss and its gradient vanish)."""
    rng = np.random.default_rng(12)
    B, T, N = 3, 12, 4
    x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([12, 3, 1], np.int32)
    hyp = np.full((B, N, T), -1, np.int32)
    hl = np.asarray([[3, 4, 3, 2], [2, 4, 1, 0], [2, 3, 2, 4]], np.int32)
    ll = np.asarray([4, 2, 3], np.int32)
    if (V, blank) == (6, 0):
        for b in range(B):
            for n in range(N):
                hyp[b, n, :hl[b, n]] = rng.integers(1, V, hl[b, n])
        hyp[0, 2] = hyp[0, 0]                       # a duplicate
        hyp[1, 0, :2] = (3, 3)                      # needs 3 frames on the classic lattice, 2 on the simplified: feasible in 3
        labels = rng.integers(1, V, (B, 4)).astype(np.int32)
    else:
        toks = [c for c in range(V) if c != blank]
        spread = np.asarray([-1] + [toks[(i * (len(toks) - 1)) // 4] for i in range(5)], np.int32)
        x[..., spread[1:].tolist() + [blank]] += np.float32(np.log(V / 6.0))
        _, _, hyp6, _, _, labels6, _ = case()
        hyp, labels = spread[np.maximum(hyp6, 0)], spread[labels6]
    score = np.zeros((B, N), np.float32) - np.arange(N, dtype=np.float32)
    score[0, 3] = -np.inf                       # masked
    score[1, 2] = -np.inf                       # masked
    # utterance 1: three frames, entry 1 has four labels (infeasible on both lattices)
    # utterance 2: one frame, every entry has two labels or more (nothing is feasible)
    for a in (x, tl, hyp, hl, score, labels, ll):
        a.setflags(write=False)
    return x, tl, hyp, hl, score, labels, ll


@pytest.mark.parametrize("entry", ENTRIES)
def test_explicit_hypotheses_against_the_reference(entry):
    check_explicit(entry)


def check_explicit(entry, V=6, blank=0):
    """case(V, blank) through `entry` against the reference."""
    import tf_seq2seq_losses_amd as ctc
    kind, wrt = entry.split("-")[0], int(entry.endswith("logproba"))
    x, tl, hyp, hl, score, labels, ll = case(V, blank)
    if wrt:
        x = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    mask = np.isfinite(score)
    want = E.mwer_reference(kind, wrt, hyp, hl, mask, x, tl, blank, labels, ll)
    used = mask & np.isfinite(want["hyp_loss"])
    assert used[0].sum() == 3 and not used[1, 1] and used[1, 0] and used[1, 3] and not used[2].any(), used

    xt = dev(x).requires_grad_(True)
    beam = ctc.CtcBeamDecoding(dev(score), dev(hyp), dev(hl))
    out = call(entry, dev(labels), xt, dev(ll), dev(tl), blank, hypotheses=beam)
    assert isinstance(out, ctc.CtcMwerLoss) and out.hypotheses.labels is beam.labels
    assert out.loss.shape == (3,) and out.risk.shape == (3, 4) == out.log_posterior.shape
    assert out.loss.dtype == out.risk.dtype == out.log_posterior.dtype == torch.float32
    assert out.loss.requires_grad and out.log_posterior.requires_grad and not out.risk.requires_grad
    out.loss.sum().backward()
    torch.cuda.synchronize()
    loss, risk, logp, grad = (t.detach().cpu().numpy() for t in (out.loss, out.risk, out.log_posterior, xt.grad))

    assert np.array_equal(risk, want["risk"].astype(np.float32)), "risk is exact"
    assert np.array_equal(np.isneginf(logp), ~used) and not np.isnan(logp).any()
    bound = 1e-4 * np.maximum(1.0, np.abs(want["c"]).sum(axis=1))
    lerr = np.abs(loss - want["loss"])
    gerr = np.abs(grad - want["grad"]).max(axis=(1, 2))
    hl_tol = 1e-4 + 1e-6 * np.abs(np.where(used, want["hyp_loss"], 0.0))
    pbound = 2.0 * hl_tol.max(axis=1, keepdims=True) + 1e-6 * np.abs(np.where(used, want["log_posterior"], 0.0))
    perr = np.abs(np.where(used, logp, 0.0) - np.where(used, want["log_posterior"], 0.0))
    print(f"MWER-MEASURE {entry} V={V} blank={blank}: loss {loss.tolist()} reference {want['loss'].tolist()}; worst |loss - reference| {lerr.max():.3e}, "
          f"worst |grad - reference| {gerr.max():.3e}, bound per utterance {bound.tolist()}, sum |c| "
          f"{np.abs(want['c']).sum(axis=1).tolist()}, worst |log_posterior - reference| {perr.max():.3e} (bound {pbound.min():.3e}), "
          f"largest |grad| {np.abs(want['grad']).max():.3g}", flush=True)
    assert not np.isnan(loss).any() and np.isfinite(grad).all()
    assert np.all(lerr <= bound), lerr
    assert np.all(gerr <= bound), gerr
    assert np.all(perr <= pbound), perr
    assert loss[2] == 0.0 and np.all(grad[2] == 0.0), "an utterance without a feasible entry: loss 0, a zero gradient"
    assert np.all(grad[1, 3:] == 0.0), "rows beyond logit_length"
    assert np.abs(want["grad"][0]).max() > 1e-3 and np.abs(want["loss"][0]) > 1e-3, "a loss and a gradient to speak of"


@pytest.mark.parametrize("entry", ENTRIES)
def test_own_beam_search_equals_the_explicit_call(entry):
    """The same functions on the same inputs: equal bits.  The labels of utterance 1 are its best hypothesis (four frames: at most
    four labels), so that its list holds risk 0 beside risks >= 1 and the gradient compared is not a tensor of zeros."""
    check_own_search(entry)


def check_own_search(entry, V=6, blank=0):
    import tf_seq2seq_losses_amd as ctc
    kind, wrt = entry.split("-")[0], int(entry.endswith("logproba"))
    x, _, _, _, _, labels, ll = case(V, blank)
    tl = np.asarray([12, 4, 1], np.int32)
    if wrt:
        x = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    kw = dict(beam_width=8, top_k=5, nbest=4)
    x2 = dev(x).requires_grad_(True)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        beam = ctc.ctc_beam_search_from_logproba(x2, dev(tl), blank, cls, **kw)
    else:
        beam = (ctc.classic_ctc_beam_search if kind == "classic" else ctc.simplified_ctc_beam_search)(x2, dev(tl), blank, **kw)
    labels, ll = labels.copy(), ll.copy()
    ll[1] = int(beam.label_length[1, 0])
    labels[1, :ll[1]] = beam.labels[1, 0, :ll[1]].cpu().numpy()
    explicit = call(entry, dev(labels), x2, dev(ll), dev(tl), blank, hypotheses=beam)
    explicit.loss.sum().backward()

    x1 = dev(x).requires_grad_(True)
    own = call(entry, dev(labels), x1, dev(ll), dev(tl), blank, **kw)
    # the search leaves the logits' graph alone: a leaf without a gradient yet, detached hypotheses
    assert x1.is_leaf and x1.grad is None and x1.requires_grad
    assert not own.hypotheses.score.requires_grad and not own.hypotheses.labels.requires_grad
    own.loss.sum().backward()
    torch.cuda.synchronize()
    for a, b in zip(own.hypotheses, beam):
        assert torch.equal(a, b)
    assert torch.equal(own.loss, explicit.loss) and torch.equal(own.risk, explicit.risk)
    assert torch.equal(own.log_posterior, explicit.log_posterior)
    assert torch.equal(x1.grad, x2.grad)
    assert torch.isfinite(own.loss).all() and torch.isfinite(x1.grad).all()
    want_risk = E.edit_distances(beam.labels.cpu().numpy(), beam.label_length.cpu().numpy(), labels, ll)
    risk = own.risk.cpu().numpy()
    print(f"MWER-MEASURE own search {entry} V={V} blank={blank}: risk {risk.tolist()} loss {own.loss.tolist()} largest |grad| per utterance "
          f"{x1.grad.abs().amax(dim=(1, 2)).tolist()}", flush=True)
    assert np.array_equal(risk, want_risk.astype(np.float32))
    assert ll[1] <= 4 and risk[1, 0] == 0.0 and risk[1, 1] >= 1.0 and bool(torch.isfinite(beam.score[1, 1]))
    assert float(x1.grad[1].abs().max()) > 0.0 and float(own.loss[1].detach().abs()) > 0.0


def test_gradient_reaches_a_producer_and_detached_logits_give_a_detached_loss():
    import tf_seq2seq_losses_amd as ctc
    x, tl, hyp, hl, score, labels, ll = case()
    beam = ctc.CtcBeamDecoding(dev(score), dev(hyp), dev(hl))
    w = dev(x).requires_grad_(True)
    out = ctc.classic_ctc_mwer_loss(dev(labels), w * 1.0, dev(ll), dev(tl), 0, hypotheses=beam)
    out.loss.sum().backward()
    leaf = dev(x).requires_grad_(True)
    ref = ctc.classic_ctc_mwer_loss(dev(labels), leaf, dev(ll), dev(tl), 0, hypotheses=beam)
    ref.loss.sum().backward()
    assert torch.equal(w.grad, leaf.grad) and torch.equal(out.loss, ref.loss)
    plain = ctc.classic_ctc_mwer_loss(dev(labels), dev(x), dev(ll), dev(tl), 0, hypotheses=beam)
    assert not plain.loss.requires_grad and torch.equal(plain.loss, ref.loss.detach())
