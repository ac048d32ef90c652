"""Gradient of N-best rescoring from block checkpoints (ctc_amd_nbest_loss_grad_ckpt) against the float64
reference of tests/tools/nbest_grad_oracle.py, with the bars of tests/test_gpu_nbest_loss_grad.py (its check_grad, as it stands):
|grad - oracle| <= 1e-4 max(1, sum of the feasible |w_n|), + 2^-8 |oracle| for 16 bits; the loss has the bits of ops.nbest_loss."""
import numpy as np
import pytest
import torch

from oracle import ctc_oracle as O
from tests import _ownership as OW
from tests import test_gpu_nbest_loss as F
from tests import test_gpu_nbest_loss_grad as G
from tests.tools import nbest_grad_oracle as NG

pytestmark = pytest.mark.gpu

DEV = G.DEV
KINDS = G.KINDS


def run(kind, wrt, labels, x, ll, tl, blank, w, U=None, grad_dtype=None):
    from tf_seq2seq_losses_amd import ops
    loss, grad = ops.nbest_loss_grad_ckpt(G.KIND_ID[kind], wrt, G.dev(labels, np.int32), torch.tensor(x, device=DEV), G.dev(ll, np.int32),
                                          G.dev(tl, np.int32), blank, G.dev(w, np.float32), U, grad_dtype)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), grad.float().cpu().numpy()


def check_all(kind, wrt, labels, x, ll, tl, blank, w, what, U=None, grad_dtype=None):
    """Loss bit for bit against ops.nbest_loss, gradient against the oracle, rows beyond T_b exactly zero."""
    want_loss, want = NG.nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, blank, w)
    loss, grad = run(kind, wrt, labels, x, ll, tl, blank, w, U, grad_dtype)
    F.check(loss, want_loss, what)
    assert F.same(loss, G.forward_loss(kind, wrt, labels, x, ll, tl, blank, U)), (what, "the bits of ctc_amd_nbest_loss")
    G.check_grad(grad, want, want_loss, w, what, sixteen=grad_dtype in (torch.bfloat16, torch.float16))
    T = grad.shape[1]
    pad = np.arange(T)[None, :] >= np.clip(np.asarray(tl), 0, T)[:, None]
    assert np.all(grad[pad] == 0.0), (what, "rows beyond T_b")
    return loss, grad


def case(seed, B, T, V, N, W, blank=0, max_len=None):
    rng = np.random.default_rng(seed)
    x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
    labels = F.draw_labels(rng, (B, N, W), V, blank)
    ll = rng.integers(0, min(W, T if max_len is None else max_len) + 1, (B, N)).astype(np.int32)
    ll[:, 0] = 1
    return x, labels, ll, G.weights(rng, B, N)


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("U,T", [(64, 1), (64, 15), (64, 16), (64, 17), (64, 33), (129, 3), (129, 4), (129, 5), (129, 9)])
def test_block_edges(U, T, kind, wrt):
    x, labels, ll, w = case(1000 * U + T, 3, T, 8, 3, U, max_len=6)
    if wrt:
        x = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    tl = np.asarray([T, 0, max(T - 2, 1)], np.int32)
    _, grad = check_all(kind, wrt, labels, x, ll, tl, 0, w, f"block edges U={U} T={T} {kind} wrt={wrt}", U=U)
    assert np.abs(grad[0]).max() > 1e-3 and np.all(grad[1] == 0.0)


@pytest.mark.parametrize("U", [64, 65, 129, 256])
def test_label_tiers(U):
    x, tl, labels, ll = F.tier_case(U)
    rng = np.random.default_rng(U + 1)
    for kind in KINDS:
        w = G.weights(rng, *ll.shape)
        w[:, 0] = 1.0 + np.abs(w[:, 1])
        if kind == "classic":
            w[:, 2] = np.nan  # one frame short: infeasible, its weight is not interpreted
        loss, _ = check_all(kind, 0, labels, x, ll, tl, 0, w, f"tier U={U} T={x.shape[1]} {kind}", U=U)
        assert np.all(np.isfinite(loss[:, :2])) and np.array_equal(np.isposinf(loss[:, 2]), np.full(2, kind == "classic"))


@pytest.mark.parametrize("kind", KINDS)
def test_above_256_labels_is_the_three_launch_call(kind):
    from tf_seq2seq_losses_amd import _lib
    x, tl, labels, ll = F.tier_case(257)
    w = G.weights(np.random.default_rng(5), *ll.shape)
    loss, grad = run(kind, 0, labels, x, ll, tl, 0, w, 257)
    loss0, grad0, _ = G.run(kind, 0, labels, x, ll, tl, 0, w, 257)
    assert F.same(loss, loss0) and F.same(grad, grad0)
    shape = (G.KIND_ID[kind], 2, x.shape[1], 8, 257, 3)
    assert _lib.nbest_loss_grad_ckpt_workspace_bytes(*shape) == _lib.nbest_loss_grad_workspace_bytes(*shape)


@pytest.mark.parametrize("N,grad_dtype", [(1, None), (7, None), (8, None), (9, None), (17, None), (17, torch.bfloat16)])
def test_groups(N, grad_dtype):
    x, labels, ll, w = case(100 + N, 2, 37, 8, N, 10)
    for kind in KINDS:
        check_all(kind, 0, labels, x, ll, np.asarray([37, 17], np.int32), 0, w, f"groups N={N} {grad_dtype} {kind}", grad_dtype=grad_dtype)


@pytest.mark.parametrize("V", [5, 1030])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_vocabulary_and_blank(V, where):
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    x, labels, ll, w = case(V + blank, 2, 19, V, 9, 7, blank=blank)
    labels[:, :, 0] = np.where(blank == V - 1, V - 2, V - 1)  # a token of the second column pass
    for kind in KINDS:
        check_all(kind, 0, labels, x, ll, np.asarray([19, 11], np.int32), blank, w, f"V={V} blank={blank} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_zero_rule(kind):
    rng = np.random.default_rng(77)
    B, T, V, N, W = 3, 20, 6, 9, 12
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tl = np.asarray([T, 4, 9], np.int32)
    labels = F.draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(1, 7, (B, N)).astype(np.int32)
    ll[1] = np.arange(5, 5 + N)   # utterance 1 (4 frames): nothing fits
    ll[0, 1] = W + 1              # too long
    ll[2, 4] = 12                 # 12 labels in 9 frames
    w = G.weights(rng, B, N)
    w[0, 1], w[2, 4], w[1, 0], w[1, 1] = np.nan, np.inf, -np.inf, np.nan
    lab_o, ll_o = labels.copy(), ll.copy()
    ll_o[0, 1] = 1                # the oracle's stand-in for the hypothesis that is too long: weight 0, loss +inf by contract
    dead = np.zeros((B, N), bool)
    dead[0, 1] = True
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, lab_o, x, ll_o, tl, 0, np.where(dead, 0.0, w))
    want_loss = np.where(dead, np.inf, want_loss)
    loss, grad = run(kind, 0, labels, x, ll, tl, 0, w, W)
    F.check(loss, want_loss, f"zero rule {kind}")
    assert np.isposinf(loss[0, 1]) and np.isposinf(loss[2, 4]) and np.all(np.isposinf(loss[1]))
    G.check_grad(grad, want, want_loss, w, f"zero rule {kind}")
    assert np.all(grad[1] == 0.0), "an utterance without a feasible hypothesis"
    assert np.all(grad[2, 9:] == 0.0), "rows beyond T_b"


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_on_every_run(kind):
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, N, W = 2, 37, 8, 9, 10
    xs, labs, lls, ws_ = case(9, B, T, V, N, W)
    x, labels, ll, w = G.dev(xs), G.dev(labs, np.int32), G.dev(lls, np.int32), G.dev(ws_)
    tl = G.dev([T, 21], np.int32)
    need = _lib.nbest_loss_grad_ckpt_workspace_bytes(G.KIND_ID[kind], B, T, V, W, N)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss = torch.zeros((B, N), device=DEV)
    grad = torch.zeros((B, T, V), device=DEV)

    def call():
        rc = lib.ctc_amd_nbest_loss_grad_ckpt(G.KIND_ID[kind], _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), W,
                                              ll.data_ptr(), tl.data_ptr(), 0, B, T, V, W, N, w.data_ptr(), loss.data_ptr(), grad.data_ptr(),
                                              _lib.F32, T * V, V, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def prefilled(byte, go):
        ws.fill_(byte)
        loss.view(torch.uint8).fill_(byte)
        grad.view(torch.uint8).fill_(byte)
        go()
        torch.cuda.synchronize()
        return loss.clone(), grad.clone()

    first = prefilled(0x00, call)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for got in (prefilled(0xFF, call), prefilled(0x00, g.replay), prefilled(0xFF, g.replay)):
        assert OW.same_bits(got[0], first[0]) and OW.same_bits(got[1], first[1])
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, labs, xs, lls, np.asarray([T, 21]), 0, ws_)
    G.check_grad(first[1].cpu().numpy(), want, want_loss, ws_, f"determinism {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_expected_risk_through_the_checkpointed_backward(kind):
    import tf_seq2seq_losses_amd as ctc
    fn = ctc.classic_ctc_nbest_loss if kind == "classic" else ctc.simplified_ctc_nbest_loss
    xs, labs, lls, _ = case(21, 2, 37, 8, 5, 10)
    xs, lls = 0.3 * xs, np.full_like(lls, 3)  # flat logits, equal lengths: no hypothesis takes the whole posterior
    tl = G.dev([37, 30], np.int32)
    risk = G.dev(np.random.default_rng(3).integers(0, 5, lls.shape), np.float32)
    grads = []
    for checkpoint in (False, True):
        x = G.dev(xs).requires_grad_(True)
        out = fn(G.dev(labs, np.int32), x, G.dev(lls, np.int32), tl, 0, differentiable=True, checkpoint=checkpoint)
        (out.log_posterior.exp() * risk).sum().backward()
        grads.append(x.grad.cpu().numpy())
    bound = 1e-4  # the bar's floor: 1e-4 max(1, sum |w_n|) with w = d objective / d loss
    err = np.abs(grads[1] - grads[0]).max()
    print(f"NBEST-CKPT-MEASURE public route {kind}: worst |checkpoint - plain| {err:.3e}, bound {bound:.1e}", flush=True)
    assert np.abs(grads[0]).max() > 1e-3 and err <= bound
