"""A non-zero blank in every kernel tier, format and entry point, against the float64 oracles called with the same blank
(tests/test_oracle_blank.py ties their blank handling back to column 0).  Benign N(0,1) logits and small shapes: this file is
about indexing -- the per-lane blank mask of the fused tiers, the direct reads by `blank` of every kernel, "beyond the labels
tensor reads as the blank" -- not about range.

Every loss + gradient case has four utterances: 0 full length with a run of repeated labels and token 0, 1 ragged with token 0 and
the blank's two neighbouring columns, 2 an empty label, 3 infeasible (fewer frames than labels).  Labels come from
[0, V) \\ {blank}.  Asserted: where the loss is finite and that it is +inf elsewhere, loss and gradient against the oracle,
exactly zero gradient rows beyond logit_length and for the infeasible utterance, the loss-only call against the loss + gradient
call, and the name of the pipeline (ops.pipeline_of) the case was written for.

Tolerances are the project's: 1e-4 on the loss (relative, floor 1) and on gradient entries (absolute) for float32; bfloat16 as
test_gpu_formats.py::test_bfloat16_against_oracle (loss 1e-4 * max(1, max|loss|), gradient 2^-8), float16 as
test_gpu_formats2.py::test_float16_logits_and_gradient (loss the same, gradient 1e-3), the oracle on the rounded inputs.

Which instantiation a shape selects (csrc/ctc_fused6.hip launch6 and its entry table, the same table in ctc_fused5.hip,
fused_eligible in ctc_capi.hip): NL = 1 / 2 / 4 / 8 label positions per lane for U <= 64 / 128 / 256 / 512; VPL = 1 / 2 / 4 row
segments per lane for V <= 256 / 512 / 1024 (NL >= 4: V <= 512 only); XT = 0 for aligned contiguous float32 with V == 256 VPL,
1 for float32 whose V and strides are multiples of 4, 3 for any other float32, 2 for bfloat16."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import ctc_oracle as O
from tests.test_gpu_alignment import check_against_oracle
from tests.test_gpu_alignment import run as run_best_path
from tests.test_gpu_greedy_decode import check as check_decoding
from tests.test_gpu_greedy_decode import run as run_greedy
from tests.tools import greedy_oracle as GO

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = ["classic", "simplified"]
DEV = torch.device("cuda:0")
TORCH_DTYPE = {"f32": torch.float32, "tm": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GRAD_TOL = {"f32": TOL, "tm": TOL, "bf16": 2.0 ** -8, "f16": 1e-3}


def _t(a):
    return torch.tensor(a, device=DEV)  # (a copy: the shared inputs are read-only arrays)


def nl_for(U):
    nl = 1
    while 64 * nl < U:
        nl *= 2
    return nl


@functools.lru_cache(maxsize=None)
def case(V, blank, U, T=None, fmt="f32"):
    """Shared by the tests of one shape, never modified.  `x` is what the kernel reads as float32 (rounded for bfloat16 / float16)."""
    T = U + 25 if T is None else T
    B, W = 4, max(U, 1)
    rng = np.random.default_rng(1000003 * V + 1009 * blank + 17 * U + T)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if fmt in ("bf16", "f16"):
        x = torch.from_numpy(x).to(TORCH_DTYPE[fmt]).float().numpy()
    labels = rng.integers(0, V - 1, (B, W)).astype(np.int32)
    labels[labels >= blank] += 1
    labels[0, :min(max(U // 2, 1), 12)] = labels[0, 0]  # a run of repeats: the classic lattice needs the blanks in between
    if blank != 0:
        labels[0, W - 1] = 0
        labels[1, 0] = 0
    if U >= 3:
        labels[1, 1] = blank - 1 if blank > 0 else 1
        labels[1, 2] = blank + 1 if blank < V - 1 else V - 2
    ll = np.array([U, max(min(U, 3), U // 2), 0, U], np.int32)
    tl = np.array([T, min(T, max(T - 7, ll[1] + 3)), T - 3, max(U - 1, 0)], np.int32)
    assert not (labels == blank).any() and (blank == 0 or (0 in labels[0] and 0 in labels[1, :ll[1]]))
    for a in (x, labels, ll, tl):
        a.flags.writeable = False
    return SimpleNamespace(V=V, blank=blank, U=U, T=T, B=B, fmt=fmt, x=x, labels=labels, ll=ll, tl=tl)


@functools.lru_cache(maxsize=None)
def reference(kind, V, blank, U, T=None, fmt="f32"):
    c = case(V, blank, U, T, fmt)
    rl, rg = C.loss_grad(kind, c.labels, c.x, c.ll, c.tl, blank)
    assert np.array_equal(np.isfinite(rl), [True, True, True, False]), rl  # (the case is what its docstring says)
    rl.flags.writeable = rg.flags.writeable = False
    return rl, rg


def device_logits(c):
    x = _t(c.x).to(TORCH_DTYPE[c.fmt])
    if c.fmt == "tm":  # [T,B,V] storage, passed as a [B,T,V] view
        x = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not x.is_contiguous()
    return x


def prepared(c, x=None, **kw):
    from tf_seq2seq_losses_amd import ops
    x = device_logits(c) if x is None else x
    p = ops.Prepared(_t(c.labels), x, _t(c.ll), _t(c.tl), c.blank, U=max(c.U, 1), keep_format=c.fmt != "f32", **kw)
    assert p.native == (c.fmt != "f32") and p.blank == c.blank
    return p


def check_loss(c, loss, rl, what):
    got = loss.detach().cpu().numpy().astype(np.float64)
    fin = np.isfinite(rl)
    assert np.array_equal(np.isfinite(got), fin), (what, got, rl)
    assert np.all(got[~fin] == np.inf), (what, got)
    if c.fmt in ("bf16", "f16"):
        err, bound = np.abs(got[fin] - rl[fin]).max(), TOL * max(1.0, np.abs(rl[fin]).max())
    else:
        err, bound = (np.abs(got[fin] - rl[fin]) / np.maximum(1.0, np.abs(rl[fin]))).max(), TOL
    print(f"BLANK {what}: loss error {err:.3e} (bound {bound:.1e})", flush=True)
    assert err < bound, (what, err)


def check_grad(c, grad, rg, what, d_loss=None):
    """Utterance by utterance against d_loss * oracle; exactly zero beyond logit_length and for the infeasible utterance."""
    got = grad.detach().float().cpu().numpy().astype(np.float64)
    assert got.shape == rg.shape and np.isfinite(got).all(), what
    worst = 0.0
    for b in range(c.B):
        w = 1.0 if d_loss is None else float(d_loss[b])
        assert np.all(got[b, c.tl[b]:] == 0), (what, b)
        if not c.tl[b] >= c.ll[b]:
            assert np.all(got[b] == 0), (what, b)
        err = np.abs(got[b] - w * rg[b]).max() / max(1.0, abs(w))
        worst = max(worst, err)
        assert err < GRAD_TOL[c.fmt], (what, b, err)
    print(f"BLANK {what}: gradient error {worst:.3e} (bound {GRAD_TOL[c.fmt]:.1e})", flush=True)


def run_loss_grad(kind, c, pipeline, override=""):
    """One loss + gradient call and one loss-only call, all of the file's assertions."""
    from tf_seq2seq_losses_amd import ops, _lib
    k = ops.KINDS[kind]
    rl, rg = reference(kind, c.V, c.blank, c.U, c.T, c.fmt)
    p = prepared(c)
    _lib.debug_override("pipeline", override)
    try:
        assert ops.pipeline_of(k, _lib.WRT_LOGITS, p) == pipeline
        loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True)
        loss_only, none = ops.loss_grad(k, _lib.WRT_LOGITS, p, False)
    finally:
        _lib.debug_override("pipeline", "")
    what = f"{kind} {pipeline} V={c.V} blank={c.blank} U={c.U} {c.fmt}"
    assert none is None and grad.dtype == TORCH_DTYPE[c.fmt] and grad.stride() == p.x.stride()
    check_loss(c, loss, rl, what)
    # same pipeline: identical; loss + gradient on a fused tier, loss only on another: last-ulp differences (test_gpu_sweep.py)
    assert torch.allclose(loss, loss_only, rtol=1e-6, atol=0, equal_nan=False), (what, loss, loss_only)
    check_grad(c, grad, rg, what)


# ---- a. the fused tiers: (V, format, U, blank), with the instantiation (NL, VPL, XT) the launch tables give it ----
def _rows(V, fmt, vpl, xt, pairs):
    return [pytest.param(V, fmt, U, blank, id=f"V{V}-{fmt}-U{U}-blank{blank}-NL{nl_for(U)}-VPL{vpl}-XT{xt}") for U, blank in pairs]


FUSED6 = (
    _rows(256, "f32", 1, 0, [(5, 255), (5, 131), (70, 255), (130, 131), (260, 255)])
    + _rows(512, "f32", 2, 0, [(5, 256), (5, 511), (130, 256), (260, 511)])
    + _rows(1024, "f32", 4, 0, [(5, 513), (5, 768), (5, 1023), (70, 768), (70, 1023)])
    + _rows(60, "f32", 1, 1, [(5, 59)])                         # one segment, masked beyond V
    + _rows(300, "f32", 2, 1, [(70, 256), (70, 299)])           # the last segment partial
    + _rows(256, "tm", 1, 1, [(5, 255)])                        # time-major view: the row stride is not V
    + _rows(253, "f32", 1, 3, [(5, 252)])
    + _rows(257, "f32", 2, 3, [(5, 256)])                       # 256: the only column of the second segment
    + _rows(1021, "f32", 4, 3, [(5, 1020)])
    + _rows(300, "bf16", 2, 2, [(5, 299), (130, 256)])
    + _rows(512, "bf16", 2, 2, [(5, 511), (130, 256)])
)
# the log-domain twin: one case per (NL, VPL) pair, every XT among them
FUSED5 = (
    _rows(256, "f32", 1, 0, [(5, 255), (70, 255), (130, 131), (260, 255)])
    + _rows(257, "f32", 2, 3, [(5, 256)])
    + _rows(300, "f32", 2, 1, [(70, 299)])
    + _rows(512, "bf16", 2, 2, [(130, 256)])
    + _rows(512, "f32", 2, 0, [(260, 511)])
    + _rows(1024, "f32", 4, 0, [(5, 768), (70, 1023)])
)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,fmt,U,blank", FUSED6)
def test_fused6_loss_and_gradient(kind, V, fmt, U, blank):
    run_loss_grad(kind, case(V, blank, U, None, fmt), "fused6")


@pytest.mark.parametrize("V,fmt,U,blank", FUSED5)
def test_fused5_loss_and_gradient(V, fmt, U, blank):
    for kind in KINDS:
        run_loss_grad(kind, case(V, blank, U, None, fmt), "fused5", override="fused5")


def test_three_kernel_pipeline_at_a_fused_shape():
    for kind in KINDS:
        run_loss_grad(kind, case(300, 299, 70), "v1", override="v1")


# ---- b. utterances that leave the linear-domain format, redone inside the fused6 launch ----
@pytest.mark.parametrize("kind", KINDS)
def test_flagged_utterances_inside_fused6(kind):
    """Utterances 0 and 1 benign; 2 has a -inf column that no label uses (test_gpu_fused.py::test_fused_neg_inf_logits); 3 has a
    single 1e10 logit (test_gpu_hvp.py::test_fused_hvp_hands_flagged_utterances_to_the_log_domain_pipeline), for which -- as in
    test_gpu_parity.py::test_extreme_logits -- only the loss and the finiteness of the gradient are asserted."""
    from tf_seq2seq_losses_amd import ops, _lib
    B, T, V, U, blank = 4, 120, 256, 40, 255
    rng = np.random.default_rng(41)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    labels = rng.integers(2, V - 1, (B, U)).astype(np.int32)  # neither the blank nor columns 0 / 1 ...
    labels[labels == 7] = 8
    labels[:, 0] = 0                                           # ... but for token 0 in front, in every utterance
    labels[1, 3:9] = labels[1, 3]
    x[2, :, 7] = -np.inf
    x[3, 7, 1] = 1e10
    ll = np.array([U, U - 9, U, U], np.int32)
    tl = np.array([T, T - 20, T, T], np.int32)
    k = ops.KINDS[kind]
    p = ops.Prepared(_t(labels), _t(x), _t(ll), _t(tl), blank, U=U)
    assert ops.pipeline_of(k, _lib.WRT_LOGITS, p) == "fused6"
    ws = torch.zeros(_lib.workspace_bytes(_lib.WS_LOSS_GRAD_LOGITS, k, B, T, V, U), dtype=torch.uint8, device=DEV)
    loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True, workspace=ws)
    flags = ops.fused_flags(ws, k, p).cpu().numpy()
    print(f"BLANK flagged {kind}: flag words {flags.tolist()}", flush=True)
    assert flags[0] == 0 and flags[1] == 0 and (flags[2:] != 0).any(), flags
    rl, rg = C.loss_grad(kind, labels, x, ll, tl, blank)
    lossn, gradn = loss.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(rl).all() and np.isfinite(lossn).all() and np.isfinite(gradn).all()
    err = np.abs(lossn[:3] - rl[:3]) / np.maximum(1.0, np.abs(rl[:3]))
    gerr = [np.abs(gradn[b] - rg[b]).max() for b in range(3)]
    print(f"BLANK flagged {kind}: loss errors {err.tolist()}, gradient errors {gerr}, 1e10 utterance: loss {lossn[3]!r}, oracle {rl[3]!r}", flush=True)
    assert err.max() < TOL and max(gerr) < TOL
    assert np.all(gradn[1, tl[1]:] == 0)
    assert abs(lossn[3] - rl[3]) / max(1.0, abs(rl[3])) < 1e-6


# ---- c. the two-call form and the public functions ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,U,blank", [(256, 70, 255), (300, 5, 299)])
def test_loss_forward_then_grad_resume(kind, V, U, blank):
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = case(V, blank, U), ops.KINDS[kind]
    rl, rg = reference(kind, V, blank, U)
    w = np.array([0.5, -2.0, 0.0, 3.0], np.float32)  # (utterance 2, the empty label, gets 0; the infeasible one a weight that must not show)
    p = prepared(c)
    assert ops.pipeline_of(k, _lib.WRT_LOGITS, p) == "fused6"
    loss1, _ = ops.loss_grad(k, _lib.WRT_LOGITS, p, True)
    loss2, ws = ops.loss_forward(k, _lib.WRT_LOGITS, p)
    assert ws is not None
    grad2 = ops.grad_resume(k, _lib.WRT_LOGITS, p, ws, d_loss=_t(w))
    what = f"{kind} two-call V={V} blank={blank} U={U}"
    check_loss(c, loss2, rl, what)
    print(f"BLANK {what}: forward loss bit-identical to the one-call loss: {torch.equal(loss1, loss2)}", flush=True)
    assert torch.allclose(loss1, loss2, rtol=1e-6, atol=0), (what, loss1, loss2)
    check_grad(c, grad2, rg, what, d_loss=w)
    assert np.all(grad2[2].cpu().numpy() == 0)  # weight 0
    # the same through the public functions: blank_index as an integer and as a scalar tensor
    fn = ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss
    for blank_index in (blank, torch.tensor(blank), torch.tensor(blank, device=DEV)):
        xt = _t(c.x).requires_grad_(True)
        loss = fn(_t(c.labels), xt, _t(c.ll), _t(c.tl), blank_index=blank_index)
        (g,) = torch.autograd.grad(loss, xt, grad_outputs=_t(w))
        check_loss(c, loss, rl, what + " public")
        check_grad(c, g, rg, what + " public", d_loss=w)


# ---- d. the three-kernel pipeline: vocabularies beyond the fused tiers (gradient in 1024-column passes), log-probabilities, float16 ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank", [(2048, 1023), (2048, 1024), (2050, 2049)])
def test_wide_vocabulary(kind, V, blank):
    run_loss_grad(kind, case(V, blank, 9, 30), "v1")


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_with_respect_to_log_probabilities(kind):
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = case(300, 299, 9, 30), ops.KINDS[kind]
    lp = torch.log_softmax(_t(c.x), dim=2)
    p = ops.Prepared(_t(c.labels), lp, _t(c.ll), _t(c.tl), c.blank, U=c.U)
    assert ops.pipeline_of(k, _lib.WRT_LOGPROBS, p) == "v1"
    loss, grad = ops.loss_grad(k, _lib.WRT_LOGPROBS, p, True)
    loss_only, _ = ops.loss_grad(k, _lib.WRT_LOGPROBS, p, False)
    ref = O.LOSS_DATA[kind](c.labels, lp.cpu().numpy().astype(np.float64), c.ll, c.tl, c.blank)
    what = f"{kind} wrt log-probabilities V=300 blank=299"
    check_loss(c, loss, ref.loss, what)
    assert torch.allclose(loss, loss_only, rtol=1e-6, atol=0)
    check_grad(c, grad, ref.gradient, what)


@pytest.mark.parametrize("kind", KINDS)
def test_float16_logits(kind):
    """float16 is read by the three-kernel pipeline only (fused_eligible); pipeline_name speaks of float32 calls, so the call is
    made under the override that names that pipeline."""
    run_loss_grad(kind, case(300, 299, 9, 30, "f16"), "v1", override="v1")


# ---- e. packed batches ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank,fmt", [(257, 256, "f32"), (2052, 2051, "f32"), (260, 259, "bf16")])
def test_packed_batches(kind, V, blank, fmt):
    """The layout of test_gpu_formats2.py::test_packed_batches: a gap between utterances and a row stride wider than V.  (A packed
    batch always runs the three kernels -- fused_eligible -- and ctc_amd_pipeline_name has no packed form to ask.)"""
    from tf_seq2seq_losses_amd import ops, _lib
    c = case(V, blank, 9, 30, fmt)
    rl, rg = reference(kind, V, blank, 9, 30, fmt)
    gap, off, total = 3, np.zeros(c.B, np.int64), 0
    for b in range(c.B):
        off[b] = total + gap
        total = int(off[b]) + int(c.tl[b])
    dtype = TORCH_DTYPE[fmt]
    store = torch.full((total + gap, V + 4), 7.0, dtype=dtype, device=DEV)
    packed, xpad = store[:, :V], _t(c.x).to(dtype)
    owned = torch.zeros(total + gap, dtype=torch.bool, device=DEV)
    for b in range(c.B):
        packed[off[b]:off[b] + c.tl[b]] = xpad[b, :c.tl[b]]
        owned[off[b]:off[b] + c.tl[b]] = True
    loss, grad = ops.loss_grad_packed(ops.KINDS[kind], _lib.WRT_LOGITS, _t(c.labels), packed, _t(off), _t(c.ll), _t(c.tl), blank, c.T, U=c.U)
    what = f"{kind} packed V={V} blank={blank} {fmt}"
    check_loss(c, loss, rl, what)
    assert grad.dtype == dtype and not grad[~owned].any()  # rows no utterance owns
    padded = torch.zeros((c.B, c.T, V), dtype=dtype, device=DEV)
    for b in range(c.B):
        padded[b, :c.tl[b]] = grad[off[b]:off[b] + c.tl[b]]
    check_grad(c, padded, rg, what)


# ---- f. the log-domain entry points ----
@functools.lru_cache(maxsize=None)
def reference_data(kind, V, blank, U, T):
    c = case(V, blank, U, T)
    return O.ctc_loss(kind, c.labels, c.x, c.ll, c.tl, blank)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank,U,T", [(37, 36, 7, 20), (300, 299, 70, 90)])
def test_alpha_beta_and_log_posterior(kind, V, blank, U, T):
    """The comparison of test_gpu_parity.py::_compare / test_gpu_contract.py: the same entries finite, those within 1e-4 relative, floor 1."""
    from tf_seq2seq_losses_amd import ops, _lib
    c, k = case(V, blank, U, T), ops.KINDS[kind]
    ref = reference_data(kind, V, blank, U, T)
    assert np.array_equal(np.isfinite(ref.loss), [True, True, True, False])
    p = prepared(c)
    loss, alpha, beta = ops.alpha_beta(k, _lib.WRT_LOGITS, p)
    check_loss(c, loss, ref.loss, f"{kind} alpha_beta V={V}")
    for name, got in (("alpha", alpha), ("beta", beta)):
        a, r = got.cpu().numpy().astype(np.float64), getattr(ref, name)
        assert a.shape == r.shape, (name, a.shape, r.shape)
        assert np.array_equal(np.isfinite(a), np.isfinite(r)), name
        m = np.isfinite(r)
        err = (np.abs(a[m] - r[m]) / np.maximum(1, np.abs(r[m]))).max()
        print(f"BLANK {kind} {name} V={V} blank={blank}: error {err:.3e}", flush=True)
        assert err < TOL, (name, err)
    loss, lg = ops.log_posterior(k, _lib.WRT_LOGITS, p)
    check_loss(c, loss, ref.loss, f"{kind} log_posterior V={V}")
    lgn, r = lg.cpu().numpy().astype(np.float64), ref.logarithmic_logproba_gradient
    assert lgn.shape == r.shape
    assert np.array_equal(np.isfinite(lgn), np.isfinite(r))
    assert np.all(lgn[~np.isfinite(r)] == -np.inf)
    m = np.isfinite(r)
    err = (np.abs(lgn[m] - r[m]) / np.maximum(1, np.abs(r[m]))).max()
    # the blank column has a code path of its own (`if (k == p.blank) v = lblank`): finite wherever the oracle's is, -inf nowhere else
    bl, rb = lgn[..., blank], r[..., blank]
    assert np.array_equal(np.isfinite(bl), np.isfinite(rb)) and np.isfinite(rb[:3]).any()
    assert np.all(np.isfinite(rb[2, :c.tl[2]]))  # the empty label: every frame emits the blank
    mb = np.isfinite(rb)
    berr = (np.abs(bl[mb] - rb[mb]) / np.maximum(1, np.abs(rb[mb]))).max()
    print(f"BLANK {kind} log posterior V={V} blank={blank}: error {err:.3e}, blank column {berr:.3e}", flush=True)
    assert err < TOL and berr < TOL


@pytest.mark.parametrize("kind", KINDS)
def test_hessian_both_kernels_both_spaces(kind):
    from tf_seq2seq_losses_amd import ops, _lib
    V, blank, U, T = 13, 12, 3, 8  # (the oracle is O(T^2 L^2))
    c, k = case(V, blank, U, T), ops.KINDS[kind]
    ref = reference_data(kind, V, blank, U, T)
    lp = torch.log_softmax(_t(c.x), dim=2)
    refd = O.LOSS_DATA[kind](c.labels, lp.cpu().numpy().astype(np.float64), c.ll, c.tl, blank)
    want = {_lib.WRT_LOGITS: (O.logits_gradient(ref, c.x), O.logits_hessian(ref, c.x)), _lib.WRT_LOGPROBS: (refd.gradient, refd.hessian)}
    assert np.abs(want[_lib.WRT_LOGITS][1]).max() > 1e-2
    for kernel in ("", "slab"):
        _lib.debug_override("hessian", kernel)
        try:
            got = {wrt: ops.hessian(k, wrt, prepared(c, x=(lp if wrt else None))) for wrt in want}
        finally:
            _lib.debug_override("hessian", "")
        for wrt, (loss, grad, hess) in got.items():
            what = f"{kind} hessian '{kernel}' wrt={wrt} blank={blank}"
            check_loss(c, loss, ref.loss, what)
            check_grad(c, grad, want[wrt][0], what)
            h = hess.cpu().numpy().astype(np.float64)
            err = np.abs(h - want[wrt][1]).max()
            print(f"BLANK {what}: Hessian error {err:.3e}", flush=True)
            assert err < TOL, (what, err)


@pytest.mark.parametrize("kind", KINDS)
def test_hvp_with_respect_to_log_probabilities(kind):
    """Against the contraction of this library's dense Hessian (held to the oracle above), as in
    test_gpu_hvp.py::test_hvp_across_lane_tilings and with its bound: 1e-3 of max(1, max|Hv|) -- the dense float32 Hessian sums
    T * V entries per output and carries ~5e-4 itself at this T."""
    from tf_seq2seq_losses_amd import ops, _lib
    V, blank, U, T = 60, 59, 70, 100
    c, k = case(V, blank, U, T), ops.KINDS[kind]
    p = prepared(c, x=torch.log_softmax(_t(c.x), dim=2))
    v = _t(np.random.default_rng(3).standard_normal((c.B, T, V)).astype(np.float32))
    loss, _, out = ops.hvp(k, _lib.WRT_LOGPROBS, p, v)
    check_loss(c, loss, reference(kind, V, blank, U, T)[0], f"{kind} hvp wrt log-probabilities")
    _, _, hess = ops.hessian(k, _lib.WRT_LOGPROBS, p, want_grad=False)
    want = torch.einsum("btkuj,buj->btk", hess.double(), v.double()).cpu().numpy()
    del hess
    outn = out.cpu().numpy().astype(np.float64)
    err = np.abs(outn - want).max() / max(1.0, np.abs(want).max())
    print(f"BLANK {kind} hvp wrt log-probabilities blank={blank}: error {err:.3e}, max|Hv| {np.abs(want).max():.3e}", flush=True)
    assert np.isfinite(outn).all() and np.abs(want).max() > 1e-2 and err < 1e-3
    assert np.all(outn[3] == 0) and np.abs(outn[0, :, blank]).max() > 1e-3


# ---- g. a labels tensor narrower than the labels ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,pipelines", [(256, ("fused6", "fused5", "v1")), (2050, ("v1",))])
def test_positions_beyond_the_labels_tensor_read_as_the_blank(kind, V, pipelines):
    """The tensor is `stride` wide, the call's bound is U = stride + 3 and utterance 1 has label_length = stride + 2: its last two
    positions read as the blank (csrc/ctc_common.h label_at), an impossible emission -- loss +inf, zero gradient.  With
    blank = V - 1 that differs from reading token 0, which is made a cheap continuation here (+6 on column 0 of that utterance); a
    kernel reading on into the next row of the tensor would find ordinary labels there.  Either mistake gives a finite loss.
    (test_gpu_contract.py asserts the same rule with blank = 0, where "the blank" and "0" cannot be told apart.)"""
    from tf_seq2seq_losses_amd import ops, _lib
    stride, T, blank = 5, 30, V - 1
    rng = np.random.default_rng(V)
    x = rng.standard_normal((3, T, V)).astype(np.float32)
    x[1, :, 0] += 6.0
    labels = rng.integers(1, V - 1, (3, stride)).astype(np.int32)
    labels[0, 0] = 0
    ll, tl = np.array([stride, stride + 2, stride - 2], np.int32), np.array([T, T, T - 4], np.int32)
    good = [0, 2]
    k = ops.KINDS[kind]
    # the mistakes this would catch do give a finite loss: token 0 twice / the next row's first two labels
    for tail in ([0, 0], labels[2, :2].tolist()):
        wide = np.concatenate([labels[1], np.int32(tail)])[None]
        assert np.isfinite(C.loss_grad(kind, wide, x[1:2], ll[1:2], tl[1:2], blank)[0][0])
    rl, rg = C.loss_grad(kind, labels[good], x[good], ll[good], tl[good], blank)
    assert np.isfinite(rl).all()
    p = ops.Prepared(_t(labels), _t(x), _t(ll), _t(tl), blank, U=stride + 3)
    assert p.stride == stride and p.U == stride + 3
    for pipeline in pipelines:
        override = "" if pipeline == pipelines[0] else pipeline
        _lib.debug_override("pipeline", override)
        try:
            assert ops.pipeline_of(k, _lib.WRT_LOGITS, p) == pipeline
            loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True)
            loss_only, _ = ops.loss_grad(k, _lib.WRT_LOGITS, p, False)
        finally:
            _lib.debug_override("pipeline", "")
        lossn, gradn = loss.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
        assert lossn[1] == np.inf and loss_only[1].item() == float("inf"), (pipeline, lossn)
        assert np.all(gradn[1] == 0), pipeline
        err = (np.abs(lossn[good] - rl) / np.maximum(1.0, np.abs(rl))).max()
        gerr = np.abs(gradn[good] - rg).max()
        print(f"BLANK narrow labels {kind} {pipeline} V={V}: loss error {err:.3e}, gradient error {gerr:.3e}", flush=True)
        assert err < TOL and gerr < TOL, (pipeline, err, gerr)
        assert torch.allclose(loss, loss_only, rtol=1e-6, atol=0)


# ---- h. alignment and decoding ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank,fmt", [(512, 511, "f32"), (300, 299, "f16"), (300, 299, "tm")])
def test_best_path(kind, V, blank, fmt):
    c = case(V, blank, 20, 45, fmt)
    got = run_best_path(kind, 0, device_logits(c), c.labels, c.ll, c.tl, blank)
    assert np.isfinite(got[0][:3]).all() and got[0][3] == -np.inf
    assert (got[1][0] == blank).any() and (got[1][0] == 0).any()  # the repeats need blanks; token 0 is the last label
    assert np.all(got[1][2, :c.tl[2]] == blank)                   # the empty label: the all-blank path
    check_against_oracle(kind, 0, c.x, c.labels, c.ll, c.tl, got, blank, what=f"{kind} V={V} blank={blank} {fmt}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V,blank,fmt", [(2050, 2049, "f32"), (256, 255, "bf16")])
def test_greedy_decode_and_the_tie_between_the_blank_and_token_0(kind, V, blank, fmt):
    """Frames where the blank and token 0 share the row maximum go to token 0 (the lowest index), which is a label here."""
    B, T = 4, 70
    rng = np.random.default_rng(V)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    x[..., blank] += 2.0  # blanks between the labels
    ties = [(0, 0), (0, 5), (0, 6), (0, 64), (2, 3), (3, T - 1)]
    for b, t in ties:
        x[b, t, 0] = x[b, t, blank] = 9.0
    xt = _t(x).to(TORCH_DTYPE[fmt])
    x = xt.float().cpu().numpy()
    tl = np.array([T, 0, T - 5, T], np.int32)
    want = GO.decode(kind, x, tl, blank, 0)
    got = run_greedy(kind, 0, xt, tl, blank)
    check_decoding(got, want, f"{kind} V={V} blank={blank} {fmt}")
    for b, t in ties:
        assert want.tokens[b, t] == 0 and got[1][b, t] == 0, (b, t)
        assert kind == "classic" or t in got[4][b, :got[3][b]].tolist(), (b, t)  # (simplified: every such frame is a label of its own)
    assert (got[1][0, :T] == blank).any() and 0 in got[2][0, :got[3][0]].tolist()


# ---- i. graph capture ----
@pytest.mark.parametrize("kind", KINDS)
def test_fused6_in_a_hip_graph(kind):
    """One launch, a single serial branch (tests/test_gpu_graph.py): captured once, replayed twice on new logits and labels."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    V, blank, U, T = 256, 255, 5, 30
    k = ops.KINDS[kind]
    c0 = case(V, blank, U, T)
    B = c0.B
    assert _lib.pipeline_name(k, _lib.WRT_LOGITS, B, T, V, U, True) == "fused6"
    x = torch.zeros((B, T, V), device=DEV)
    labels = torch.zeros((B, U), dtype=torch.int32, device=DEV)
    ll = torch.zeros(B, dtype=torch.int32, device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    loss = torch.zeros(B, device=DEV)
    grad = torch.zeros((B, T, V), device=DEV)
    ws = torch.zeros(_lib.workspace_bytes(_lib.WS_LOSS_GRAD, k, B, T, V, U), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_loss_grad(k, _lib.WRT_LOGITS, x.data_ptr(), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), blank,
                                   B, T, V, U, loss.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(c, seed):
        h = np.random.default_rng(seed).standard_normal((B, T, V)).astype(np.float32)
        x.copy_(torch.from_numpy(h)); labels.copy_(_t(c.labels)); ll.copy_(_t(c.ll)); tl.copy_(_t(c.tl))
        return h

    fill(c0, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    c = c0
    for seed in (2, 3):
        h = fill(c, seed)
        loss.zero_(); grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        got_l, got_g = loss.clone(), grad.clone()
        loss.zero_(); grad.zero_()
        call()
        torch.cuda.synchronize()
        assert torch.equal(got_l, loss) and torch.equal(got_g, grad)
        rl, rg = C.loss_grad(kind, c.labels, h, c.ll, c.tl, blank)
        cc = SimpleNamespace(**{**vars(c), "fmt": "f32"})
        check_loss(cc, got_l, rl, f"{kind} graph replay seed {seed}")
        check_grad(cc, got_g, rg, f"{kind} graph replay seed {seed}")
