"""The per-utterance input contract (csrc/ctc_common.h) on every entry point and tier, both lattices.

One batch has one row per rule:
    0  well formed                       4  label_length = U + 2 (U is the static bound the call passes)
    1  label_length = -3   (counts as 0)  5  a label inside label_length equal to V + 3
    2  logit_length = T + 5 (clamped: T)  6  a label inside label_length equal to -2
    3  logit_length = -2   (clamped: 0; its label_length is 0, so that the expected loss is the finite 0 and not +inf)
and a second call passes a labels tensor two columns narrower than U with one row whose label_length reaches past the tensor:
those positions read as the blank, an impossible emission.

Expected: the well-formed rows give what the float64 oracles give on the SANITISED lengths, at the project's 1e-4; the others give
loss +inf, an exactly zero gradient / Hessian / Hessian-vector product, -inf log posteriors, alignment score -inf and frames -1.
The Hessian-vector product has no closed-form oracle at V = 256 (the dense oracle Hessian is 0.5 GB per utterance): its reference is
the central difference of the float64 oracle gradient with eps = 1e-3, whose own truncation error is O(eps^2 |d3 loss|) ~ 1e-6
at T = 30, two orders inside the bound.  Every figure is printed before it is asserted (pytest -s)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import ctc_oracle as O
from tests.test_gpu_alignment import check_against_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = ["classic", "simplified"]
SMALL = (7, 12, 8, 5)    # the log-domain entry points: Hessian, alpha / beta, log posterior
FUSED = (7, 30, 256, 6)  # the fused tiers: loss + gradient, Hessian-vector product


def _t(a):
    return torch.tensor(a, device=torch.device("cuda:0"))  # (a copy: the shared inputs are read-only arrays)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def _case(shape, narrow):
    """Raw inputs, sanitised lengths, and which rows are well formed (good) / infeasible (bad)."""
    B, T, V, U = shape
    rng = np.random.default_rng(T + V)
    logits = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    if not narrow:
        ll = np.array([U, -3, U - 2, 0, U + 2, U - 1, U - 1], np.int32)
        tl = np.array([T - 1, T, T + 5, -2, T, T, T - 2], np.int32)
        labels[5, 1] = V + 3
        labels[6, 0] = -2
        good, bad = [0, 1, 2, 3], [4, 5, 6]
    else:
        logits, labels = logits[:3].copy(), labels[:3, :U - 2].copy()
        ll = np.array([U - 2, U - 1, U - 3], np.int32)  # row 1: one position past the tensor, inside the bound U
        tl = np.array([T, T, T - 1], np.int32)
        good, bad = [0, 2], [1]
    ll_s, tl_s = np.maximum(ll, 0), np.clip(tl, 0, T)
    _frozen(logits, labels, ll, tl, ll_s, tl_s)
    return SimpleNamespace(shape=(len(ll), T, V, U), logits=logits, labels=labels, ll=ll, tl=tl, ll_s=ll_s, tl_s=tl_s, good=good, bad=bad)


def _prepared(c):
    from tf_seq2seq_losses_amd import ops
    return ops.Prepared(_t(c.labels), _t(c.logits), _t(c.ll), _t(c.tl), 0, U=c.shape[3])


@functools.lru_cache(maxsize=None)
def _ref_loss_grad(shape, narrow, kind):
    c = _case(shape, narrow)
    g = c.good
    return _frozen(*C.loss_grad(kind, c.labels[g], c.logits[g], c.ll_s[g], c.tl_s[g], 0))


@functools.lru_cache(maxsize=None)
def _ref_data(narrow, kind):
    """The NumPy oracle's loss data of the well-formed rows of the small shape (alpha, beta, log posterior, Hessian)."""
    c = _case(SMALL, narrow)
    g = c.good
    return O.ctc_loss(kind, c.labels[g], c.logits[g], c.ll_s[g], c.tl_s[g], 0)


def _check_loss(c, loss, ref_loss, what):
    got = loss.cpu().numpy().astype(np.float64)
    assert np.all(got[c.bad] == np.inf), (what, got)
    fin = np.isfinite(ref_loss)
    assert np.array_equal(np.isfinite(got[c.good]), fin), (what, got, ref_loss)
    err = (np.abs(got[c.good][fin] - ref_loss[fin]) / np.maximum(1, np.abs(ref_loss[fin]))).max()
    print(f"CONTRACT {what}: loss error {err:.3e}", flush=True)
    assert err < TOL, (what, err)


def _check_rows(c, got, ref, what):
    """good rows against the reference (absolute), bad rows exactly zero"""
    got = got.cpu().numpy()
    assert np.all(got[c.bad] == 0), what
    err = np.abs(got[c.good] - ref).max()
    print(f"CONTRACT {what}: error {err:.3e}", flush=True)
    assert err < TOL, (what, err)


@pytest.mark.parametrize("narrow", [False, True], ids=["rules", "narrow"])
@pytest.mark.parametrize("kind", KINDS)
def test_loss_and_gradient_in_every_pipeline(kind, narrow):
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = _case(FUSED, narrow), ops.KINDS[kind]
    assert _lib.pipeline_name(k, 0, *c.shape, True) == "fused6"
    rl, rg = _ref_loss_grad(FUSED, narrow, kind)
    p = _prepared(c)
    for pipeline in ("", "fused5", "v1"):
        _lib.debug_override("pipeline", pipeline)
        try:
            loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True)
            loss_only, _ = ops.loss_grad(k, _lib.WRT_LOGITS, p, False)
            loss2, ws = ops.loss_forward(k, _lib.WRT_LOGITS, p, keep_always=True)
            grad2 = ops.grad_resume(k, _lib.WRT_LOGITS, p, ws)
        finally:
            _lib.debug_override("pipeline", "")
        what = f"{kind} pipeline '{pipeline}'"
        _check_loss(c, loss, rl, what + " loss+gradient")
        _check_loss(c, loss_only, rl, what + " loss only")
        _check_loss(c, loss2, rl, what + " loss_forward")
        _check_rows(c, grad, rg, what + " gradient")
        _check_rows(c, grad2, rg, what + " grad_resume")


@pytest.mark.parametrize("narrow", [False, True], ids=["rules", "narrow"])
@pytest.mark.parametrize("kind", KINDS)
def test_hessian_vector_product_on_both_tiers(kind, narrow):
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = _case(FUSED, narrow), ops.KINDS[kind]
    _lib.hvp_flags_offset(k, *c.shape)  # (raises unless the shape runs the fused kernel)
    g, eps = c.good, 1e-3
    v = np.random.default_rng(5).standard_normal(c.logits.shape)
    xp = (c.logits.astype(np.float64) + eps * v).astype(np.float32)
    xm = (c.logits.astype(np.float64) - eps * v).astype(np.float32)
    v = ((xp.astype(np.float64) - xm.astype(np.float64)) / (2 * eps)).astype(np.float32)  # the direction actually taken
    fd = (C.loss_grad(kind, c.labels[g], xp[g], c.ll_s[g], c.tl_s[g], 0)[1] -
          C.loss_grad(kind, c.labels[g], xm[g], c.ll_s[g], c.tl_s[g], 0)[1]) / (2 * eps)
    rl, _ = _ref_loss_grad(FUSED, narrow, kind)
    p = _prepared(c)
    for tier in ("", "v1"):
        _lib.debug_override("hvp", tier)
        try:
            loss, _, out = ops.hvp(k, _lib.WRT_LOGITS, p, _t(v))
        finally:
            _lib.debug_override("hvp", "")
        what = f"{kind} hvp '{tier}'"
        _check_loss(c, loss, rl, what)
        outn = out.cpu().numpy()
        assert np.all(outn[c.bad] == 0), what
        err = np.abs(outn[g] - fd).max()  # (absolute, like the gradient: max|Hv| is about 1 here)
        print(f"CONTRACT {what}: error {err:.3e}, max|Hv| = {np.abs(fd).max():.3e}", flush=True)
        assert err < TOL, (what, err)


@pytest.mark.parametrize("narrow", [False, True], ids=["rules", "narrow"])
@pytest.mark.parametrize("kind", KINDS)
def test_hessian_both_kernels(kind, narrow):
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = _case(SMALL, narrow), ops.KINDS[kind]
    rl, rg = _ref_loss_grad(SMALL, narrow, kind)
    rh = O.logits_hessian(_ref_data(narrow, kind), c.logits[c.good])
    p = _prepared(c)
    for kernel in ("", "slab"):
        _lib.debug_override("hessian", kernel)
        try:
            loss, grad, hess = ops.hessian(k, _lib.WRT_LOGITS, p)
        finally:
            _lib.debug_override("hessian", "")
        what = f"{kind} hessian '{kernel}'"
        _check_loss(c, loss, rl, what)
        _check_rows(c, grad, rg, what + " gradient")
        _check_rows(c, hess, rh, what)


@pytest.mark.parametrize("narrow", [False, True], ids=["rules", "narrow"])
@pytest.mark.parametrize("kind", KINDS)
def test_alpha_beta_and_log_posterior(kind, narrow):
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = _case(SMALL, narrow), ops.KINDS[kind]
    rl, _ = _ref_loss_grad(SMALL, narrow, kind)
    ref = _ref_data(narrow, kind)
    p = _prepared(c)
    loss, alpha, beta = ops.alpha_beta(k, _lib.WRT_LOGITS, p)
    _check_loss(c, loss, rl, f"{kind} alpha_beta")
    for name, got in (("alpha", alpha), ("beta", beta)):
        full = got.cpu().numpy().astype(np.float64)
        for b in c.bad:  # label_length > U: every state of every frame is -inf (the other infeasible rows: through the loss above)
            assert c.ll_s[b] <= c.shape[3] or np.all(full[b] == -np.inf), (name, b)
        a, r = full[c.good], getattr(ref, name)
        Lo = r.shape[2]  # the oracle sizes the label axis by max(label_length), the call by U: what lies beyond is unreachable
        assert a.shape[:2] == r.shape[:2] and Lo <= a.shape[2]
        assert np.all(a[:, :, Lo:] == -np.inf), name
        a = a[:, :, :Lo]
        assert np.array_equal(np.isfinite(a), np.isfinite(r)), name
        m = np.isfinite(r)
        err = (np.abs(a[m] - r[m]) / np.maximum(1, np.abs(r[m]))).max()
        print(f"CONTRACT {kind} {name}: error {err:.3e}", flush=True)
        assert err < TOL, (name, err)
    loss, lg = ops.log_posterior(k, _lib.WRT_LOGITS, p)
    _check_loss(c, loss, rl, f"{kind} log_posterior")
    lgn, r = lg.cpu().numpy().astype(np.float64), ref.logarithmic_logproba_gradient
    assert np.all(lgn[c.bad] == -np.inf)
    assert np.array_equal(np.isfinite(lgn[c.good]), np.isfinite(r))
    m = np.isfinite(r)
    err = (np.abs(lgn[c.good][m] - r[m]) / np.maximum(1, np.abs(r[m]))).max()
    print(f"CONTRACT {kind} log posterior: error {err:.3e}", flush=True)
    assert err < TOL, err


@pytest.mark.parametrize("narrow", [False, True], ids=["rules", "narrow"])
@pytest.mark.parametrize("shape", [SMALL, FUSED], ids=["small", "fused"])
@pytest.mark.parametrize("kind", KINDS)
def test_best_path(kind, shape, narrow):
    from tf_seq2seq_losses_amd import ops, _lib
    c = _case(shape, narrow)
    score, tokens, index = ops.best_path(ops.KINDS[kind], _lib.WRT_LOGITS, _prepared(c))
    got = (score.cpu().numpy(), tokens.cpu().numpy(), index.cpu().numpy())
    assert np.all(got[0][c.bad] == -np.inf) and np.all(got[1][c.bad] == -1) and np.all(got[2][c.bad] == -1)
    assert np.all(np.isfinite(got[0][c.good]))
    # (the oracle finds the bad rows infeasible by itself; the sanitised lengths are what the checker slices labels and frames with)
    check_against_oracle(kind, 0, c.logits, c.labels, c.ll_s, c.tl_s, got, what=f"contract {kind} {shape}")


def test_check_labels_reports_rows_5_and_6_only():
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    c = _case(SMALL, False)
    B, _, V, U = c.shape
    st = torch.cuda.current_stream().cuda_stream

    llt = _t(c.ll)

    def run(labels):
        lt = _t(labels)  # (kept alive over the call, like llt: a temporary's memory would be handed to the next tensor)
        return lib.ctc_amd_check_labels(lt.data_ptr(), U, llt.data_ptr(), 0, B, V, U, st)

    assert run(c.labels) == _lib.ELABEL and b"2 label" in lib.ctc_amd_last_error()
    fixed = c.labels.copy()
    fixed[5, 1] = 1
    assert run(fixed) == _lib.ELABEL and b"1 label" in lib.ctc_amd_last_error()
    fixed[6, 0] = 1
    assert run(fixed) == 0
    fixed[1, 0] = fixed[4, 0] = V + 3  # a row without labels (-3) and a row beyond the bound: their labels are not read
    assert run(fixed) == 0
