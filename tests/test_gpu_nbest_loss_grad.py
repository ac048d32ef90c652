"""Gradient of N-best rescoring (ctc_amd_nbest_loss_grad) against the float64 reference of
tests/tools/nbest_grad_oracle.py: sum over the feasible hypotheses of weight[b, n] * d loss[b, n] / d x.

Tolerances (derived, not measured).  The project's bound for a gradient is "every element within 1e-4 of the float64 oracle"
(tests/test_gpu_parity.py) and this gradient is linear in the weights, so per element
    |grad - oracle| <= 1e-4 * max(1, sum_n |weight[b, n]|)        (the sum over the feasible hypotheses: the others' weights are not read)
for a float32 gradient; a 16-bit gradient adds 2^-8 * |oracle|, the resolution term of tests/test_gpu_formats.py.  The loss has
the tolerance of tests/test_gpu_nbest_loss.py, and the bits of ops.nbest_loss.  Every worst figure is printed before it is asserted."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ctc_oracle as O
from tests import _ownership as OW
from tests import test_gpu_nbest_loss as F  # the forward tests' shapes, loss oracle and loss check
from tests.tools import nbest_grad_oracle as NG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KINDS = ("classic", "simplified")
KIND_ID = {"classic": 0, "simplified": 1}
GUARD = 64


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a, dtype), device=DEV)


def run(kind, wrt, labels, x, ll, tl, blank, w, U=None, grad_dtype=None):
    """ops.nbest_loss_grad.  x: a NumPy array or a device tensor (taken as it stands).  Returns (loss[B, N], grad[B, T, V] float32
    NumPy arrays, the gradient tensor as it came back)."""
    from tf_seq2seq_losses_amd import ops
    xt = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=DEV)
    loss, grad = ops.nbest_loss_grad(KIND_ID[kind], wrt, dev(labels, np.int32), xt, dev(ll, np.int32), dev(tl, np.int32), blank,
                                     dev(w, np.float32), U, grad_dtype)
    torch.cuda.synchronize()
    assert loss.shape == tuple(np.asarray(ll).shape) and loss.dtype == torch.float32
    assert grad.shape == xt.shape and grad.dtype == (grad_dtype or (xt.dtype if xt.dtype in (torch.bfloat16, torch.float16) else torch.float32))
    return loss.cpu().numpy(), grad.float().cpu().numpy(), grad


def forward_loss(kind, wrt, labels, x, ll, tl, blank, U=None):
    from tf_seq2seq_losses_amd import ops
    xt = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=DEV)
    out = ops.nbest_loss(KIND_ID[kind], wrt, dev(labels, np.int32), xt, dev(ll, np.int32), dev(tl, np.int32), blank, U)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_grad(got, want, want_loss, w, what, sixteen=False):
    """got, want [B, T, V]; want_loss [B, N] (the oracle's: which hypotheses count); w [B, N]."""
    assert not np.isnan(want).any(), (what, "the oracle has no answer here")
    assert not np.isnan(got).any(), (what, "NaN in the gradient")
    fin = np.isfinite(want_loss)
    wsum = np.where(fin, np.abs(np.where(fin, w, 0.0)), 0.0).sum(axis=1)
    bound = 1e-4 * np.maximum(1.0, wsum)[:, None, None] + (2.0 ** -8 * np.abs(want) if sixteen else 0.0)
    err = np.abs(got - want)
    print(f"NBEST-GRAD-MEASURE {what}: worst |grad - oracle| {float(err.max()) if err.size else 0.0:.3e}, worst error / bound "
          f"{float((err / bound).max()) if err.size else 0.0:.3f}, largest |oracle| {float(np.abs(want).max()) if want.size else 0.0:.4g}, "
          f"largest sum |w| {float(wsum.max()) if wsum.size else 0.0:.4g}, {int((~fin).sum())} of {fin.size} infeasible", flush=True)
    assert np.all(err <= bound), (what, float(err.max()))


def check_all(kind, wrt, labels, x, ll, tl, blank, w, what, U=None, xt=None, grad_dtype=None, sixteen=False, ref=None):
    """Loss against the oracle and bit for bit against ops.nbest_loss, gradient against the oracle, rows beyond T_b exactly zero.
    ref: the oracle's (loss, grad) on these inputs where the caller has it already."""
    want_loss, want = NG.nbest_loss_and_grad(kind, wrt, labels, x, ll, tl, blank, w) if ref is None else ref
    src = x if xt is None else xt
    loss, grad, _ = run(kind, wrt, labels, src, ll, tl, blank, w, U, grad_dtype)
    F.check(loss, want_loss, what)
    assert F.same(loss, forward_loss(kind, wrt, labels, src, ll, tl, blank, U)), (what, "the bits of ctc_amd_nbest_loss")
    check_grad(grad, want, want_loss, w, what, sixteen)
    T = grad.shape[1]
    pad = np.arange(T)[None, :] >= np.clip(np.asarray(tl), 0, T)[:, None]
    assert np.all(grad[pad] == 0.0), (what, "rows beyond T_b")
    return loss, grad, want_loss, want


def weights(rng, B, N):
    """N(0, 1) with one exact zero and one negative weight per utterance (N >= 2), float32 values."""
    w = rng.standard_normal((B, N)).astype(np.float32)
    if N >= 2:
        w[:, 0] = 0.0
        w[:, 1] = -np.abs(w[:, 1]) - 0.25
    return w


# ---- 1. parity (4. loss bits, 5. rows beyond T_b) ----
@pytest.mark.parametrize("blank", [0, 1, 5])
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(kind, wrt, blank):
    x, tl, labels, ll = F.small(blank)
    if wrt:
        x = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    w = weights(np.random.default_rng(41 + blank), *ll.shape)
    loss, grad, want_loss, _ = check_all(kind, wrt, labels, x, ll, tl, blank, w, f"parity {kind} wrt={wrt} blank={blank}")
    assert np.isfinite(loss[0]).sum() >= 2 and np.abs(grad[0]).max() > 1e-2
    assert np.all(grad[1] == 0.0), "an utterance without frames"


# ---- 2. label tiers ----
def c_oracle_grad(kind, labels, x, ll, tl, w):
    """The same reference from the C restatement of the oracle (float64 sweeps; wrt = 0), for the one size NumPy takes too long for."""
    from oracle import c_oracle as C
    grad = np.zeros(x.shape, np.float64)
    losses = []
    for n in range(labels.shape[1]):
        loss, g = C.loss_grad(kind, labels[:, n], x, ll[:, n], tl, 0)
        fin = np.isfinite(loss)
        grad += np.where(fin[:, None, None], np.where(fin, w[:, n], 0.0)[:, None, None] * np.nan_to_num(g), 0.0)
        losses.append(loss)
    grad[np.arange(x.shape[1])[None, :] >= np.asarray(tl)[:, None]] = 0.0
    return np.stack(losses, axis=1), grad


@pytest.mark.parametrize("U", [64, 65, 129, 257, 513, 1024])
def test_label_tiers(U):
    x, tl, labels, ll = F.tier_case(U)
    rng = np.random.default_rng(U + 1)
    for kind in KINDS:
        w = weights(rng, *ll.shape)
        w[:, 0] = 1.0 + np.abs(w[:, 1])
        if kind == "classic":
            w[:, 2] = np.nan  # one frame short: infeasible, its weight is not interpreted
        what = f"tier U={U} T={x.shape[1]} {kind}"
        if U < 1024:
            loss, grad, want_loss, _ = check_all(kind, 0, labels, x, ll, tl, 0, w, what, U=U)
        else:
            want_loss, want = c_oracle_grad(kind, labels, x, ll, tl, w)
            loss, grad, _ = run(kind, 0, labels, x, ll, tl, 0, w, U)
            F.check(loss, want_loss, what)
            assert F.same(loss, forward_loss(kind, 0, labels, x, ll, tl, 0, U)), what
            check_grad(grad, want, want_loss, w, what)
            assert np.all(grad[1, int(tl[1]):] == 0.0)
        assert np.all(np.isfinite(loss[:, :2]))
        assert np.array_equal(np.isposinf(loss[:, 2]), np.full(2, kind == "classic"))


# ---- 3. group and block edges ----
@pytest.mark.parametrize("N", [1, 7, 8, 9, 17, 64])
def test_group_and_block_edges(N):
    rng = np.random.default_rng(100 + N)
    B, T, V, W = 2, 37, 8, 10
    FB = 16  # frames per block of the one-position-per-lane tier (W <= 64)
    x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
    labels = F.draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(0, W + 1, (B, N)).astype(np.int32)
    ll[:, 0] = 1
    w = weights(rng, B, N)
    for tl in ((0, 1), (FB - 1, FB), (FB + 1, T)):
        for kind in KINDS:
            check_all(kind, 0, labels, x, ll, np.asarray(tl, np.int32), 0, w, f"edges N={N} T_b={tl} {kind}")


# ---- 5. the zero-contribution rule ----
@pytest.mark.parametrize("kind", KINDS)
def test_infeasible_hypotheses_contribute_nothing(kind):
    rng = np.random.default_rng(77)
    B, T, V, N, W = 3, 20, 6, 5, 12
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tl = np.asarray([T, 4, 9], np.int32)
    labels = F.draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(1, 7, (B, N)).astype(np.int32)
    ll[1] = [5, 6, 7, 8, 12]      # utterance 1 (4 frames): nothing fits
    ll[0, 1] = W + 1              # too long
    labels[0, 2, 0] = 0           # a blank inside the label
    labels[2, 3, 1] = V           # out of the vocabulary
    ll[2, 4] = 12                 # 12 labels in 9 frames
    w = weights(rng, B, N)
    w[0, 3], w[2, 0] = 0.7, -1.3
    what = f"zero contribution {kind}"
    # the oracle knows nothing of malformed hypotheses: it scores benign stand-ins with weight 0, and their loss is +inf by contract
    malformed = np.zeros((B, N), bool)
    malformed[0, 1] = malformed[0, 2] = malformed[2, 3] = True
    lab_o, ll_o = labels.copy(), ll.copy()
    lab_o[0, 2, 0], lab_o[2, 3, 1], ll_o[0, 1] = 1, 1, 1
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, lab_o, x, ll_o, tl, 0, np.where(malformed, 0.0, w))
    want_loss = np.where(malformed, np.inf, want_loss)
    loss, grad, _ = run(kind, 0, labels, x, ll, tl, 0, w, W)
    F.check(loss, want_loss, what)
    assert F.same(loss, forward_loss(kind, 0, labels, x, ll, tl, 0, W)), (what, "the bits of ctc_amd_nbest_loss")
    check_grad(grad, want, want_loss, w, what)
    assert np.all(grad[1, 4:] == 0.0) and np.all(grad[2, 9:] == 0.0), "rows beyond T_b"
    inf = np.isposinf(loss)
    assert inf[1].all() and inf[0, 1] and inf[0, 2] and inf[2, 3] and (inf[2, 4] or kind == "simplified") and not inf[0, 3] and not inf[2, 0]
    assert np.all(grad[1] == 0.0), "no feasible hypothesis: a zero gradient"
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy()
        w2[inf] = bad
        loss2, grad2, _ = run(kind, 0, labels, x, ll, tl, 0, w2, W)
        assert F.same(loss2, loss) and F.same(grad2, grad), bad


# ---- 6. determinism, 9. ownership: the C ABI with every buffer under the test's control ----
def raw_call(kind, x, labels, ll, tl, w, blank, U, fill=0xA5, ws_pattern=0x00, wrt=0, gdtype=torch.float32, gsb=None, gst=None):
    """Returns (loss[B, N], the gradient's storage, its [B, T, V] view).  Guards around the losses and behind the gradient; the gaps
    between V and the gradient's strides must keep the prefill."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = x.shape
    N, W = labels.shape[1], labels.shape[2]
    gst = V if gst is None else gst
    gsb = T * gst if gsb is None else gsb
    span = (B - 1) * gsb + (T - 1) * gst + V
    lbuf = OW.filled((GUARD + B * N + GUARD,), torch.float32, fill, DEV)
    gbuf = OW.filled((span + GUARD,), gdtype, fill, DEV)
    need = _lib.nbest_loss_grad_workspace_bytes(KIND_ID[kind], B, T, V, U, N)
    ws = OW.workspace(need + GUARD, ws_pattern)
    rc = lib.ctc_amd_nbest_loss_grad(KIND_ID[kind], wrt, x.data_ptr(), OW._dt(x), x.stride(0), x.stride(1), labels.data_ptr(), W,
                                     ll.data_ptr(), tl.data_ptr(), blank, B, T, V, U, N, w.data_ptr(), lbuf[GUARD:].data_ptr(),
                                     gbuf.data_ptr(), OW._dt(gbuf), gsb, gst, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    assert bool(OW.keeps_prefill(lbuf[:GUARD], fill).all()) and bool(OW.keeps_prefill(lbuf[GUARD + B * N:], fill).all()), "loss guards"
    assert bool(OW.keeps_prefill(gbuf[span:], fill).all()), "gradient guard"
    assert bool((ws[need:] == ws_pattern).all()), "workspace guard"
    view = gbuf.as_strided((B, T, V), (gsb, gst, 1))
    owned = torch.zeros(span + GUARD, dtype=torch.bool, device=DEV)
    owned.as_strided((B, T, V), (gsb, gst, 1)).fill_(True)
    assert bool(OW.keeps_prefill(gbuf[~owned], fill).all()), "the gaps between V and the gradient's strides are not written"
    return lbuf[GUARD:GUARD + B * N].clone().view(B, N), gbuf, view.clone()


def parity_inputs(V=8):
    x, tl, labels, ll = F.small(0, V)
    w = weights(np.random.default_rng(9), *ll.shape)
    return x, tl, labels, ll, w


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_on_every_run(kind):
    x, tl, labels, ll, w = parity_inputs()
    W = labels.shape[2]
    xt, lab, llt, tlt, wt = dev(x), dev(labels), dev(ll), dev(tl), dev(w)
    runs = [raw_call(kind, xt, lab, llt, tlt, wt, 0, W, fill=f, ws_pattern=p) for f, p in ((0x00, 0x00), (0xA5, 0xFF), (0xFF, 0xA5))]
    for loss, _, g in runs[1:]:
        assert OW.same_bits(loss, runs[0][0]) and OW.same_bits(g, runs[0][2])
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, labels, x, ll, tl, 0, w)
    check_grad(runs[0][2].cpu().numpy(), want, want_loss, w, f"determinism {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_unowned_memory_changes_no_bit(kind):
    x, tl, labels, ll, w = parity_inputs()
    B, T, V = x.shape
    N, W = labels.shape[1], labels.shape[2]
    xt, lab, llt, tlt, wt = dev(x), dev(labels), dev(ll), dev(tl), dev(w)
    closs, _, clean = raw_call(kind, xt, lab, llt, tlt, wt, 0, W, fill=0x00)

    def unchanged(out, what):
        assert OW.same_bits(out[0], closs) and OW.same_bits(out[2], clean), what
    for value in OW.poison_values(torch.float32):
        unchanged(raw_call(kind, OW.poison_padding(xt, tl, value), lab, llt, tlt, wt, 0, W), ("padding frames", value))
    poisoned = OW.poison_labels(lab.view(B * N, W), ll.reshape(-1), OW.label_poison_cycle(V, 0)).view(B, N, W)
    unchanged(raw_call(kind, xt, poisoned, llt, tlt, wt, 0, W), "label tails")
    for sb, st in ((T * (V + 3) + 5, V + 3), (V + 4, B * (V + 4))):  # padded rows; time-major with padded rows
        storage, view, owned = OW.strided_storage(xt, sb, st)
        for value in OW.poison_values(torch.float32):
            gaps = OW.poison_gaps(storage, owned, value).as_strided((B, T, V), (sb, st, 1))
            unchanged(raw_call(kind, gaps, lab, llt, tlt, wt, 0, W), ("logits gaps", sb, st, value))
        unchanged(raw_call(kind, xt, lab, llt, tlt, wt, 0, W, gsb=sb, gst=st), ("gradient strides", sb, st))
    for pattern in OW.BYTE_PATTERNS:  # the outputs' and the workspace's contents on entry
        unchanged(raw_call(kind, xt, lab, llt, tlt, wt, 0, W, fill=pattern, ws_pattern=pattern), pattern)


# ---- 7. formats ----
@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    for V in (6, 8):  # 6: every access element-wise; 8: vector accesses where strides and bases allow them
        x, tl, labels, ll, w = parity_inputs(V)
        B, T, _ = x.shape
        W = labels.shape[2]
        xt = torch.tensor(x, device=DEV)
        _, ref32, want_loss, want = check_all(kind, 0, labels, x, ll, tl, 0, w, f"formats {kind} V={V} float32")
        for dt in (torch.bfloat16, torch.float16):
            xh = xt.to(dt)
            xv = xh.float().cpu().numpy()  # the values the element type converts to
            _, gh, _, _ = check_all(kind, 0, labels, xv, ll, tl, 0, w, f"formats {kind} V={V} {dt}", xt=xh, sixteen=True)
            odd = torch.zeros(B * T * V + 1, dtype=dt, device=DEV)[1:].view(B, T, V)  # 2 bytes off: no 8-byte rows
            odd.copy_(xh)
            assert F.same(run(kind, 0, labels, odd, ll, tl, 0, w)[1], gh), (V, dt, "odd base")
            g32 = run(kind, 0, labels, xh, ll, tl, 0, w, grad_dtype=torch.float32)[1]  # 16-bit logits, float32 gradient
            check_grad(g32, NG.nbest_grad(kind, 0, labels, xv, ll, tl, 0, w), want_loss, w, f"formats {kind} V={V} {dt} -> float32")
            assert F.same(g32.astype(np.float32), run(kind, 0, labels, odd, ll, tl, 0, w, grad_dtype=torch.float32)[1])
        x_tm = xt.transpose(0, 1).contiguous()
        assert F.same(run(kind, 0, labels, x_tm.transpose(0, 1), ll, tl, 0, w)[1], ref32), (V, "time-major")
        for sb, st in ((T * (V + 3) + 5, V + 3), (T * (V + 4), V + 4)):  # padded rows: element-wise, and (V = 8) vector accesses
            _, view, _ = OW.strided_storage(xt, sb, st, 0xFF)
            assert F.same(run(kind, 0, labels, view, ll, tl, 0, w)[1], ref32), (V, sb, st)
        odd = torch.zeros(B * T * V + 1, device=DEV)[1:].view(B, T, V)  # 4 bytes off a 16-byte boundary: the element-wise path
        odd.copy_(xt)
        assert odd.data_ptr() % 16 != 0 and xt.data_ptr() % 16 == 0
        assert F.same(run(kind, 0, labels, odd, ll, tl, 0, w)[1], ref32), (V, "odd base")
        # the gradient's own formats through the C ABI: strided and 16-bit gradients, vector and element-wise stores, the same bits
        lab, llt, tlt, wt = dev(labels), dev(ll), dev(tl), dev(w)
        for gdt in (torch.float32, torch.bfloat16, torch.float16):
            _, _, plain = raw_call(kind, xt, lab, llt, tlt, wt, 0, W, gdtype=gdt)
            if gdt == torch.float32:
                assert F.same(plain.cpu().numpy(), ref32)
            else:
                check_grad(plain.float().cpu().numpy(), want, want_loss, w, f"formats {kind} V={V} gradient {gdt}", sixteen=True)
            for sb, st in ((T * (V + 3) + 5, V + 3), (T * (V + 4), V + 4), (V + 4, B * (V + 4))):
                _, _, strided = raw_call(kind, xt, lab, llt, tlt, wt, 0, W, gdtype=gdt, gsb=sb, gst=st)
                assert OW.same_bits(strided, plain), (V, gdt, sb, st)


# ---- 8. sharp and extreme inputs ----
@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits(kind):
    rng = np.random.default_rng(17)
    B, T, V, N, U = 2, 300, 32, 4, 40
    x = (6.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([T, 211], np.int32)
    labels = F.draw_labels(rng, (B, N, U), V, 0)
    ll = np.asarray([[40, 17, 3, 0], [25, 40, 1, 8]], np.int32)
    check_all(kind, 0, labels, x, ll, tl, 0, weights(rng, B, N), f"sharp N(0, 6^2) {kind}", U=U)


@pytest.mark.parametrize("kind", KINDS)
def test_minus_infinity_and_huge_logits(kind):
    rng = np.random.default_rng(23)
    B, T, V, N, W = 3, 24, 6, 4, 8
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tl = np.asarray([T, T, 15], np.int32)
    labels = F.draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(0, 7, (B, N)).astype(np.int32)
    w = weights(rng, B, N)
    xi = x.copy()
    xi[0, 3, 2] = -np.inf                 # single elements: no trouble
    xi[0, 9, 0] = -np.inf                 # ... the blank's among them
    xi[2, :, 4] = -np.inf                 # a token that is never possible: its hypotheses are infeasible
    xi[1, 7, :] = -np.inf                 # a frame that is -inf everywhere: the utterance has no feasible hypothesis
    loss, grad, _ = run(kind, 0, labels, xi, ll, tl, 0, w)
    assert not np.isnan(grad).any() and np.all(np.isposinf(loss[1])) and np.all(grad[1] == 0.0)
    rows = [0, 2]
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, labels[rows], xi[rows], ll[rows], tl[rows], 0, w[rows])
    F.check(loss[rows], want_loss, f"-inf {kind}")
    check_grad(grad[rows], want, want_loss, w[rows], f"-inf {kind}")
    xh = x.copy()
    xh[0] = 1e10                          # a uniform row of 1e10
    xh[1, :, 2] += 1e10                   # one token 1e10 above the rest
    xh[2] += 1e10                         # (float32: multiples of 1024 around 1e10)
    check_all(kind, 0, labels, xh, ll, tl, 0, w, f"1e10 {kind}")


@pytest.mark.parametrize("name", ["r04_case_forward_loss_dwell.npz", "soak_case_endloss_u128.npz"])
def test_committed_hard_cases(name):
    """Two of the cases on which float32 linear-domain sweeps lost mass: the true label as hypothesis 0, two perturbed copies beside it."""
    d = np.load(os.path.join(F.GOLDEN, name), allow_pickle=True)
    x, lab0, L, tl = d["x"], d["labels"], int(d["ll"][0]), d["tl"]
    V = x.shape[2]
    rng = np.random.default_rng(len(name))
    labels = np.repeat(lab0[:, None, :L], 3, axis=1).astype(np.int32)
    for n in (1, 2):  # one label replaced by another token
        i = int(rng.integers(0, L))
        labels[0, n, i] = 1 + (labels[0, n, i] + n - 1) % (V - 1)
    ll = np.full((1, 3), L, np.int32)
    w = np.asarray([[1.0, -0.5, 0.25]], np.float32)
    for kind in KINDS:
        check_all(kind, 0, labels, x, ll, tl, 0, w, f"{name} {kind} T_b={int(tl[0])} V={V} L={L}", U=L)


# ---- 10. autograd ----
@pytest.mark.parametrize("kind", KINDS)
def test_expected_risk_differentiates_end_to_end(kind):
    import tf_seq2seq_losses_amd as ctc
    x, tl, labels, ll = F.small(0, 8)
    B, N = ll.shape
    rng = np.random.default_rng(13)
    risk = rng.integers(0, 5, (B, N)).astype(np.float64)
    mask = np.ones((B, N), bool)
    mask[0, 2] = False  # one hypothesis removed
    fn = ctc.classic_ctc_nbest_loss if kind == "classic" else ctc.simplified_ctc_nbest_loss
    args = (dev(labels), None, dev(ll), dev(tl), 0)
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    out = fn(args[0], xt, *args[2:], hypothesis_mask=dev(mask), differentiable=True)
    assert out.loss.requires_grad and out.log_posterior.requires_grad
    lp = torch.where(torch.isfinite(out.log_posterior), out.log_posterior, torch.zeros_like(out.log_posterior))
    objective = (torch.where(torch.isfinite(out.log_posterior), lp.exp(), torch.zeros_like(lp)) * dev(risk, np.float32)).sum()
    (g,) = torch.autograd.grad(objective, xt)
    torch.cuda.synchronize()
    # float64: p = softmax(-loss) over the feasible, unmasked hypotheses; d sum_n p_n r_n / d loss_m = -p_m (r_m - sum_n p_n r_n)
    want_loss = F.oracle(kind, 0, labels, x, ll, tl, 0)
    live = np.isfinite(want_loss) & mask
    with np.errstate(all="ignore"):
        a = np.where(live, -want_loss, -np.inf)
        m = np.where(live.any(axis=1, keepdims=True), a.max(axis=1, keepdims=True), 0.0)
        p = np.exp(a - m)
        p = p / np.maximum(p.sum(axis=1, keepdims=True), 1e-300)
    wgt = np.where(live, -p * (risk - (p * risk).sum(axis=1, keepdims=True)), 0.0)
    want = NG.nbest_grad(kind, 0, labels, x, ll, tl, 0, wgt)
    got = g.cpu().numpy()
    # the weights reach the kernel as float32 results of float32 softmax arithmetic: a relative 1e-6 of |w| <= max risk, inside the bound
    check_grad(got, want, np.where(live, want_loss, np.inf), wgt, f"expected risk {kind}")
    assert np.abs(want).max() > 1e-3
    # differentiable=False on the same inputs: detached, the same bits
    plain = fn(args[0], xt, *args[2:], hypothesis_mask=dev(mask))
    torch.cuda.synchronize()
    assert not plain.loss.requires_grad and not plain.log_posterior.requires_grad
    assert OW.same_bits(plain.loss, out.loss.detach()) and OW.same_bits(plain.log_posterior, out.log_posterior.detach())
    # logits that do not require grad: nothing to attach
    off = fn(args[0], xt.detach(), *args[2:], hypothesis_mask=dev(mask), differentiable=True)
    assert not off.loss.requires_grad and OW.same_bits(off.loss, plain.loss)


def test_from_logproba_differentiates():
    import tf_seq2seq_losses_amd as ctc
    x, tl, labels, ll = F.small(0, 8)
    lp_in = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    w = weights(np.random.default_rng(3), *ll.shape)
    for kind in KINDS:
        xt = torch.tensor(lp_in, device=DEV, requires_grad=True)
        out = ctc.ctc_nbest_loss_from_logproba(dev(labels), xt, dev(ll), dev(tl), 0, F.data_cls(kind), differentiable=True)
        fin = torch.isfinite(out.loss)
        (g,) = torch.autograd.grad((torch.where(fin, out.loss, torch.zeros_like(out.loss)) * dev(w)).sum(), xt)
        torch.cuda.synchronize()
        want_loss, want = NG.nbest_loss_and_grad(kind, 1, labels, lp_in, ll, tl, 0, w)
        check_grad(g.cpu().numpy(), want, want_loss, w, f"from_logproba {kind}")


# ---- 11. graph capture ----
@pytest.mark.parametrize("kind", KINDS)
def test_nbest_loss_grad_in_a_hip_graph(kind):
    """Three launches on one stream: captured once and replayed twice on new inputs in the same buffers, the bits of the eager call."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    xs, tls, labs, lls, ws_ = parity_inputs()
    B, T, V = xs.shape
    N, W = labs.shape[1], labs.shape[2]
    x = torch.zeros((B, T, V), device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    labels = torch.ones((B, N, W), dtype=torch.int32, device=DEV)
    ll = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    w = torch.zeros((B, N), device=DEV)
    loss = torch.zeros((B, N), device=DEV)
    grad = torch.zeros((B, T, V), device=DEV)
    need = _lib.nbest_loss_grad_workspace_bytes(KIND_ID[kind], B, T, V, W, N)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_nbest_loss_grad(KIND_ID[kind], _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), W, ll.data_ptr(),
                                         tl.data_ptr(), 0, B, T, V, W, N, w.data_ptr(), loss.data_ptr(), grad.data_ptr(), _lib.F32, T * V, V,
                                         ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for dst, a in zip((x, tl, labels, ll, w), (xs, tls, labs, lls, ws_)):
        dst.copy_(torch.from_numpy(np.array(a)))
    replays = []
    for _ in range(2):
        loss.zero_()
        grad.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        replays.append((loss.clone(), grad.clone()))
    loss.zero_()
    grad.fill_(7.0)
    call()
    torch.cuda.synchronize()
    for l, gr in replays:
        assert OW.same_bits(l, loss) and OW.same_bits(gr, grad)
    want_loss, want = NG.nbest_loss_and_grad(kind, 0, labs, xs, lls, tls, 0, ws_)
    F.check(loss.cpu().numpy(), want_loss, f"graph replay {kind}")
    check_grad(grad.cpu().numpy(), want, want_loss, ws_, f"graph replay {kind}")
