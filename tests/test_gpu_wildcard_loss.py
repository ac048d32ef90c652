"""CTC loss and gradient with wildcard labels on the GPU (ctc_amd_wildcard_loss_grad, csrc/ctc_wild_loss.hip) against the float64
oracle tests/tools/wildcard_loss_oracle.py, which tests/test_wildcard_loss_oracle.py pins without a GPU.

Bars, from the project:
  loss      |loss - oracle| <= 1e-4 + 1e-6 * |loss|                       (tests/test_gpu_alignment.py)
  gradient  |grad - oracle| <= 1e-4 * max(1, |d_loss[b]|) per element, plus 2^-8 * |oracle| for a 16-bit gradient
  row sums  |sum_k grad[t, k]| <= the same 1e-4 bar, for logits (16-bit gradients: V roundings of 2^-9 relative are added)
The oracle reads the float32 value of every element the kernel reads (a 16-bit input is converted first).
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests.tools import wildcard_loss_oracle as WL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = WL.WILDCARD
KINDS = ("classic", "simplified")
GRID = [(4, 12, 5, 3), (3, 40, 6, 10), (2, 88, 8, 64), (2, 89, 8, 65), (2, 169, 8, 129), (2, 329, 8, 257), (2, 649, 8, 513),
        (2, 1288, 8, 1024)]


def loss_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def nl_for(U):
    nl = 1
    while 64 * nl < U:
        nl *= 2
    return nl


def needed_frames(kind, label):
    label = list(label)
    return len(label) + (sum(a == b and a != W for a, b in zip(label, label[1:])) if kind == "classic" else 0)


def make_inputs(kind, B, T, V, U, seed, blank=0, wild=True, scale=1.0, adjacent=True):
    """Ragged and feasible.  label_length in [U/2, U] (utterance 0: U), logit_length from what the label needs up to T (utterance
    0: T).  Wildcards (the rule of tests/test_gpu_wildcard_alignment.py): about one position in five; in every even utterance also
    position 0, the last position, both sides of lane boundaries (positions k * NL - 1 and k * NL) and an adjacent pair in the
    middle.  adjacent=False: every second of a run of wildcards becomes an ordinary label again."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    toks = np.asarray([k for k in range(V) if k != blank])
    labels = toks[rng.integers(0, len(toks), (B, U))].astype(np.int32)
    plain = labels.copy()
    ll = rng.integers(U // 2, U + 1, B).astype(np.int32)
    ll[0] = U
    NL = nl_for(U)
    for b in range(B):
        L = int(ll[b])
        if not wild or L == 0:
            continue
        labels[b, :L][rng.random(L) < 0.2] = W
        if b % 2 == 0:
            forced = [0, L - 1, L // 2, L // 2 + 1] + [k * NL + d for k in (1, 2, 31, 63) for d in (-1, 0)]
            for i in forced:
                if 0 <= i < L:
                    labels[b, i] = W
        if not adjacent:
            for i in range(1, L):
                if labels[b, i] == W and labels[b, i - 1] == W:
                    labels[b, i] = plain[b, i]
    tl = np.zeros(B, np.int32)
    for b in range(B):
        need = needed_frames(kind, labels[b, :ll[b]])
        assert need <= T, (need, T)
        tl[b] = rng.integers(need, T + 1)
    tl[0] = T
    return x, labels, ll, tl


def logprobs32(x):
    from tests.tools.viterbi_oracle import log_softmax64
    return log_softmax64(x).astype(np.float32)


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=DEV, dtype=dtype) if dtype is not None else t.to(DEV)


def kind_id(kind):
    return KINDS.index(kind)


def run(kind, wrt, x, labels, ll, tl, blank=0, d_loss=None, weight=0.0, want_grad=True, grad_dtype=None, U=None):
    """ops.wildcard_loss_grad on device copies; x may be a tensor in any format.  Returns (loss, grad) as device tensors."""
    from tf_seq2seq_losses_amd import ops
    loss, grad = ops.wildcard_loss_grad(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank,
                                        None if d_loss is None else dev(d_loss, torch.float32), U, grad_dtype, weight, want_grad)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (len(ll),)
    return loss, grad


@functools.lru_cache(maxsize=None)
def _oracle_cached(kind, wrt, key, blank, weight):
    x, labels, ll, tl, d_loss = _ORACLE_INPUTS[key]
    return WL.loss_and_grad(kind, wrt, labels, x, ll, tl, blank, weight, d_loss)


_ORACLE_INPUTS = {}


def oracle(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, d_loss=None, key=None):
    """The float64 reference, computed once per `key` and left unchanged."""
    if key is None:
        return WL.loss_and_grad(kind, wrt, labels, x, ll, tl, blank, weight, d_loss)
    _ORACLE_INPUTS.setdefault(key, (x, labels, ll, tl, d_loss))
    return _oracle_cached(kind, wrt, key, blank, weight)


def compare(what, got_loss, got_grad, ref_loss, ref_grad, d_loss=None, wrt=0, sixteen=False, V=None):
    """Prints every figure, then asserts the three bars of the module docstring."""
    loss = got_loss.detach().float().cpu().numpy().astype(np.float64)
    fin = np.isfinite(ref_loss)
    assert np.array_equal(np.isfinite(loss), fin), (what, loss, ref_loss)
    assert np.all(loss[~fin] == np.inf), (what, loss)
    lerr = np.abs(loss[fin] - ref_loss[fin])
    lbar = loss_tol(ref_loss[fin])
    print(f"WILDCARD-LOSS {what}: loss worst |gpu - oracle| {lerr.max() if lerr.size else 0.0:.3e} (bar {lbar.min() if lbar.size else 0.0:.3e})"
          f" losses {np.round(ref_loss, 3)}")
    if got_grad is None:
        assert np.all(lerr <= lbar), (what, lerr, lbar)
        return
    grad = got_grad.detach().float().cpu().numpy().astype(np.float64)
    assert not np.isnan(grad).any(), what
    B = grad.shape[0]
    dl = np.ones(B) if d_loss is None else np.where(fin, np.nan_to_num(np.asarray(d_loss, np.float64)), 0.0)
    bar = 1e-4 * np.maximum(1.0, np.abs(dl))[:, None, None] + (2.0 ** -8 * np.abs(ref_grad) if sixteen else 0.0)
    gerr = np.abs(grad - ref_grad)
    rows = np.abs(grad.sum(axis=2))
    rbar = 1e-4 * np.maximum(1.0, np.abs(dl))[:, None] + (2.0 ** -9 * np.abs(ref_grad).sum(axis=2) if sixteen else 0.0)
    print(f"WILDCARD-LOSS {what}: gradient worst |gpu - oracle| {gerr.max():.3e}, worst error / bar {(gerr / bar).max():.3f}, "
          f"largest |oracle| {np.abs(ref_grad).max():.3f}" + ("" if wrt else f", worst |row sum| {rows.max():.3e}"))
    assert np.all(lerr <= lbar), (what, lerr, lbar)
    assert np.all(gerr <= bar), (what, float(gerr.max()))
    assert np.all(grad[~fin] == 0.0), (what, "an infeasible utterance has an exactly zero gradient")
    if not wrt:
        assert np.all(rows <= rbar), (what, float(rows.max()))


# ---- the grid ----

@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_grid_logits(kind, shape):
    B, T, V, U = shape
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=U)
    assert (labels == W).any()
    ref = oracle(kind, 0, x, labels, ll, tl, key=("grid", kind, shape))
    assert np.isfinite(ref[0]).all(), "ragged and feasible"
    loss, grad = run(kind, 0, x, labels, ll, tl)
    assert grad.dtype == torch.float32 and grad.is_contiguous()
    compare(f"{kind} {shape} logits", loss, grad, *ref)
    for b in range(B):
        assert torch.all(grad[b, int(tl[b]):] == 0), "zeros beyond T_b"
    # the forward-only launch gives the same loss, bit for bit
    loss0, none = run(kind, 0, x, labels, ll, tl, want_grad=False)
    assert none is None and OW.same_bits(loss0, loss)


@pytest.mark.parametrize("shape", [GRID[0], GRID[3], GRID[5]], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_grid_logprobs(kind, shape):
    B, T, V, U = shape
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=U + 1)
    lp = logprobs32(x) - np.float32(0.25)  # not normalised: e_w carries the rows' log-sum-exp
    ref = oracle(kind, 1, lp, labels, ll, tl, key=("grid-lp", kind, shape))
    loss, grad = run(kind, 1, lp, labels, ll, tl)
    compare(f"{kind} {shape} log-probabilities", loss, grad, *ref, wrt=1)


# ---- single cases ----

SINGLE = (2, 169, 8, 129)


@pytest.mark.parametrize("kind", KINDS)
def test_wildcard_weight(kind):
    x, labels, ll, tl = make_inputs(kind, *SINGLE, seed=7)
    for wrt, xx in ((0, x), (1, logprobs32(x))):
        ref = oracle(kind, wrt, xx, labels, ll, tl, weight=-0.7)
        ref0 = oracle(kind, wrt, xx, labels, ll, tl, weight=0.0)
        assert np.abs(ref[0] - ref0[0]).min() > 1.0, "the penalty is felt"
        loss, grad = run(kind, wrt, xx, labels, ll, tl, weight=-0.7)
        compare(f"{kind} w=-0.7 wrt={wrt}", loss, grad, *ref, wrt=wrt)


@pytest.mark.parametrize("kind", KINDS)
def test_last_token_as_blank(kind):
    B, T, V, U = SINGLE
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=8, blank=V - 1)
    ref = oracle(kind, 0, x, labels, ll, tl, blank=V - 1)
    loss, grad = run(kind, 0, x, labels, ll, tl, blank=V - 1)
    compare(f"{kind} blank=V-1", loss, grad, *ref)


@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits(kind):
    x, labels, ll, tl = make_inputs(kind, *SINGLE, seed=9, scale=4.0)
    ref = oracle(kind, 0, x, labels, ll, tl)
    loss, grad = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} N(0, 4^2) logits", loss, grad, *ref)


@pytest.mark.parametrize("kind", KINDS)
def test_random_d_loss_and_nan_for_the_infeasible(kind):
    B, T, V, U = 4, 40, 6, 10
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=10)
    tl[2] = int(ll[2]) - 1  # too few frames
    d = np.random.default_rng(1).standard_normal(B).astype(np.float32) * 3
    d[2] = np.nan
    ref = oracle(kind, 0, x, labels, ll, tl, d_loss=d)
    assert ref[0][2] == np.inf and np.isfinite(ref[0][[0, 1, 3]]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl, d_loss=d)
    compare(f"{kind} random d_loss, NaN for the infeasible", loss, grad, *ref, d_loss=d)
    assert torch.all(grad[2] == 0)


# ---- formats ----

FMT = (3, 90, 260, 20)


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    B, T, V, U = FMT
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=20)
    xt = dev(x)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("fmt", kind))
    loss_c, grad_c = run(kind, 0, xt, labels, ll, tl)
    compare(f"{kind} {FMT} float32", loss_c, grad_c, *ref)
    # 16-bit logits and gradient: the oracle reads what the kernel reads
    for dt in (torch.bfloat16, torch.float16):
        xh = xt.to(dt)
        refh = oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl, key=("fmt", kind, str(dt)))
        loss, grad = run(kind, 0, xh, labels, ll, tl)
        assert grad.dtype == dt
        compare(f"{kind} {FMT} {dt}", loss, grad, *refh, sixteen=True)
        _, grad32 = run(kind, 0, xh, labels, ll, tl, grad_dtype=torch.float32)
        compare(f"{kind} {FMT} {dt} logits, float32 gradient", loss, grad32, *refh)
    # time-major: read in place, the gradient comes back in the same layout, the same bits
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)
    assert xtm.stride() == (V, B * V, 1)
    loss, grad = run(kind, 0, xtm, labels, ll, tl)
    assert grad.stride() == xtm.stride()
    assert OW.same_bits(loss, loss_c) and OW.same_bits(grad.contiguous(), grad_c)
    # an offset base pointer: the element-wise accesses give identical bits
    flat = torch.zeros(B * T * V + 1, dtype=torch.float32, device=DEV)
    xo = flat[1:].view(B, T, V)
    xo.copy_(xt)
    assert xo.data_ptr() % 16 == 4
    loss, grad = run(kind, 0, xo, labels, ll, tl)
    assert OW.same_bits(loss, loss_c) and OW.same_bits(grad, grad_c)


def raw_call(kind, wrt, x, labels, ll, tl, blank, weight, U, d_loss, loss, grad, ws):
    """The C entry point with every buffer under the caller's control; x and grad are [B, T, V] views with any strides."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V = x.shape
    rc = lib.ctc_amd_wildcard_loss_grad(
        kind_id(kind), wrt, x.data_ptr(), ops._DTYPES[x.dtype], x.stride(0), x.stride(1), labels.data_ptr(), labels.shape[1],
        ll.data_ptr(), tl.data_ptr(), blank, weight, B, T, V, U, None if d_loss is None else d_loss.data_ptr(), loss.data_ptr(),
        None if grad is None else grad.data_ptr(), ops._DTYPES[(x if grad is None else grad).dtype],
        T * V if grad is None else grad.stride(0), V if grad is None else grad.stride(1),
        None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_wildcard_loss_grad")


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_strides_beyond_v_leave_the_gaps_alone(kind, pad):
    """Row strides of V + 3 (element-wise accesses) and V + 4 (vector accesses) for logits and gradient: the same bits as the
    contiguous call, and every element of the gradient's buffer that no row owns keeps its prefill."""
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = FMT
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=20)
    loss_c, grad_c = run(kind, 0, x, labels, ll, tl)
    st, sb = V + pad, (V + pad) * T + 8
    for dt in (torch.float32, torch.bfloat16):
        xs = dev(x).to(dt)
        _, xv, _ = OW.strided_storage(xs, sb, st, pattern=0x7F)
        gstore, gv, owned = OW.strided_storage(torch.zeros((B, T, V), dtype=dt, device=DEV), sb, st, pattern=0xA5)
        gv.copy_(OW.filled((B, T, V), dt, 0xA5, DEV))
        loss = OW.filled((B,), torch.float32, 0xA5, DEV)
        ws = OW.byte_fill(_lib.wildcard_loss_workspace_bytes(kind_id(kind), B, T, V, U), 0xA5, DEV)
        raw_call(kind, 0, xv, dev(labels), dev(ll), dev(tl), 0, 0.0, U, None, loss, gv, ws)
        torch.cuda.synchronize()
        assert bool(OW.keeps_prefill(gstore, 0xA5)[~owned].all()), "elements between V and the stride are untouched"
        assert not bool(OW.keeps_prefill(gv.contiguous(), 0xA5).all())
        if dt == torch.float32:
            assert OW.same_bits(loss, loss_c) and OW.same_bits(gv.contiguous(), grad_c)
        else:
            lossh, gradh = run(kind, 0, xs, labels, ll, tl)
            assert OW.same_bits(loss, lossh) and OW.same_bits(gv.contiguous(), gradh)


@pytest.mark.parametrize("kind", KINDS)
def test_a_vocabulary_of_more_than_one_column_pass(kind):
    B, T, V, U = 2, 20, 1030, 6
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=30)
    labels[0, 1], labels[0, 3], labels[1, 1] = 1029, 1029, 1024  # tokens of the second pass, one of them twice
    ref = oracle(kind, 0, x, labels, ll, tl)
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} V=1030", loss, grad, *ref)


# ---- edges ----

@pytest.mark.parametrize("kind", KINDS)
def test_edges(kind):
    """Every degenerate utterance gives its documented loss, +inf and a zero gradient where it is infeasible, and the other
    utterances keep the bits of a run without it."""
    B, T, V, U = 3, 24, 6, 5
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=40)
    loss_c, grad_c = run(kind, 0, x, labels, ll, tl)
    ref_c = oracle(kind, 0, x, labels, ll, tl)
    compare(f"{kind} edges: clean", loss_c, grad_c, *ref_c)

    def variant(name, want, **change):
        xx, lab, l2, t2 = x.copy(), labels.copy(), ll.copy(), tl.copy()
        for k, v in change.items():
            {"x": xx, "labels": lab, "ll": l2, "tl": t2}[k][v[0]] = v[1]
        ref = oracle(kind, 0, xx, lab, l2, t2)
        loss, grad = run(kind, 0, xx, lab, l2, t2)
        compare(f"{kind} edge {name}", loss, grad, *ref)
        if want is not None:
            assert float(loss[1]) == want, (name, float(loss[1]))
        if want == np.inf:
            assert torch.all(grad[1] == 0)
        for b in (0, 2):
            assert OW.same_bits(loss[b], loss_c[b]) and OW.same_bits(grad[b], grad_c[b]), (name, b)
        return loss, grad, ref

    variant("T_b = 0, a transcript", np.inf, tl=(1, 0))
    variant("T_b = 0, no transcript", 0.0, tl=(1, 0), ll=(1, 0))
    loss, _, _ = variant("L = 0", None, ll=(1, 0))
    lp = logprobs32(x[1, :tl[1]]).astype(np.float64)
    want = -lp[:, 0].sum()
    print(f"WILDCARD-LOSS {kind} L = 0: loss {float(loss[1]):.6f}, -sum lp[t, blank] {want:.6f}")
    assert abs(float(loss[1]) - want) <= loss_tol(want)
    variant("negative label_length", None, ll=(1, -3))
    variant("too few frames", np.inf, tl=(1, int(ll[1]) - 1))
    variant("a label equal to the blank", np.inf, labels=((1, 1), 0))
    variant("a label >= V", np.inf, labels=((1, 0), V))
    variant("a label of -3", np.inf, labels=((1, 1), -3))
    variant("label_length > U", np.inf, ll=(1, U + 1))
    variant("a row of -inf", np.inf, x=((1, 0), -np.inf))


# ---- against the rest of the library ----

@pytest.mark.parametrize("kind", KINDS)
def test_without_a_wildcard_it_is_the_plain_loss(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = SINGLE
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=50, wild=False)
    assert not (labels == W).any()
    xt = dev(x).requires_grad_(True)
    fn = ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss
    plain = fn(dev(labels), xt, dev(ll), dev(tl), 0)
    (gplain,) = torch.autograd.grad(plain.sum(), xt)
    loss, grad = run(kind, 0, x, labels, ll, tl)
    lerr = (loss - plain.detach()).abs().cpu().numpy()
    gerr = float((grad - gplain).abs().max())
    print(f"WILDCARD-LOSS {kind} no wildcard: worst |loss - plain| {lerr.max():.3e}, worst |grad - plain| {gerr:.3e}")
    assert np.all(lerr <= 2 * loss_tol(plain.detach().cpu().numpy()))  # the sum of both calls' bars
    assert gerr <= 2e-4
    loss_w, grad_w = run(kind, 0, x, labels, ll, tl, weight=-2.5)  # nothing reads the weight: not a bit changes
    assert OW.same_bits(loss_w, loss) and OW.same_bits(grad_w, grad)


@pytest.mark.parametrize("kind", KINDS)
def test_the_best_path_is_a_lower_bound(kind):
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = make_inputs(kind, *SINGLE, seed=51)
    align = (ctc.classic_ctc_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_wildcard_alignment)(
        dev(labels), dev(x), dev(ll), dev(tl), 0)
    loss, _ = run(kind, 0, x, labels, ll, tl, want_grad=False)
    score = align.score.cpu().numpy().astype(np.float64)
    neg = -loss.cpu().numpy().astype(np.float64)
    print(f"WILDCARD-LOSS {kind}: -loss {neg}, best-path score {score}")
    assert np.all(neg >= score - (1e-4 + 1e-6 * np.abs(score)))


def test_the_caller_side_route():
    """Classic lattice, float32, no adjacent wildcards, w = 0: log_softmax, a zero column (ln sum_k p_k = 0) as token V, the plain
    loss on the [B, T, V + 1] log-probabilities with the wildcard mapped to V, backward through autograd."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = SINGLE
    x, labels, ll, tl = make_inputs("classic", B, T, V, U, seed=52, adjacent=False)
    assert (labels == W).any()
    xt = dev(x).requires_grad_(True)
    lp = torch.cat([torch.log_softmax(xt, dim=2), torch.zeros((B, T, 1), device=DEV)], dim=2)
    mapped = np.where(labels == W, V, labels).astype(np.int32)
    route = ctc.ctc_loss_from_logproba(dev(mapped), lp, dev(ll), dev(tl), 0, ctc.ClassicCtcLossData)
    (groute,) = torch.autograd.grad(route.sum(), xt)
    loss, grad = run("classic", 0, x, labels, ll, tl)
    lerr = (loss - route.detach()).abs().cpu().numpy()
    gerr = float((grad - groute).abs().max())
    print(f"WILDCARD-LOSS caller-side route: worst |loss - route| {lerr.max():.3e}, worst |grad - route| {gerr:.3e}, losses {loss.cpu().numpy()}")
    assert np.all(lerr <= 2 * loss_tol(route.detach().cpu().numpy()))
    assert gerr <= 2e-4


# ---- determinism ----

@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_whatever_the_buffers_held_and_under_graph_capture(kind):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = SINGLE
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=60)
    tl[1] = int(ll[1]) - 1  # one infeasible utterance: its zeros are written, not left over
    xt, lt, llt, tlt = dev(x), dev(labels), dev(ll), dev(tl)
    d = dev(np.asarray([1.5, np.nan], np.float32))
    n = _lib.wildcard_loss_workspace_bytes(kind_id(kind), B, T, V, U)
    outs = []
    for pattern in (0x00, 0xFF):
        ws = OW.byte_fill(n, pattern, DEV)
        loss = OW.filled((B,), torch.float32, pattern, DEV)
        grad = OW.filled((B, T, V), torch.float32, pattern, DEV)
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, d, loss, grad, ws)
        torch.cuda.synchronize()
        outs.append((loss, grad))
    assert OW.same_bits(outs[0][0], outs[1][0]) and OW.same_bits(outs[0][1], outs[1][1])
    assert float(outs[0][0][1]) == np.inf and torch.all(outs[0][1][1] == 0) and torch.isfinite(outs[0][1]).all()
    # capture on one stream, replay twice
    ws = OW.byte_fill(n, 0x5A, DEV)
    loss = OW.filled((B,), torch.float32, 0x5A, DEV)
    grad = OW.filled((B, T, V), torch.float32, 0x5A, DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, d, loss, grad, ws)
    for _ in range(2):
        loss.fill_(7.0)
        grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert OW.same_bits(loss, outs[0][0]) and OW.same_bits(grad, outs[0][1])


# ---- the autograd surface ----

@pytest.mark.parametrize("kind", KINDS)
def test_autograd_surface(kind, monkeypatch):
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops
    B, T, V, U = 3, 40, 6, 10
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=70)
    ref = oracle(kind, 0, x, labels, ll, tl, weight=-0.3)
    fn = ctc.classic_ctc_wildcard_loss if kind == "classic" else ctc.simplified_ctc_wildcard_loss
    calls = []
    real = ops.wildcard_loss_grad

    def spy(*a, **kw):
        calls.append(kw.get("want_grad", a[11] if len(a) > 11 else True))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "wildcard_loss_grad", spy)

    # requires_grad=False: the forward-only launch, a detached result
    loss = fn(dev(labels), dev(x), dev(ll), dev(tl), 0, wildcard_log_weight=-0.3)
    assert calls == [False] and not loss.requires_grad and loss.dtype == torch.float32
    compare(f"{kind} public, forward only", loss, None, *ref)
    # backward fills logits.grad in the logits' dtype
    for dt in (torch.float32, torch.bfloat16):
        xt = dev(x).to(dt).requires_grad_(True)
        refd = ref if dt == torch.float32 else oracle(kind, 0, xt.detach().float().cpu().numpy(), labels, ll, tl, weight=-0.3)
        del calls[:]
        loss = fn(dev(labels), xt, dev(ll), dev(tl), 0, wildcard_log_weight=-0.3)
        loss.sum().backward()
        torch.cuda.synchronize()
        assert calls == [False, True], "forward is the forward-only launch, backward the one call with a gradient"
        assert xt.grad is not None and xt.grad.dtype == dt and xt.grad.shape == xt.shape
        compare(f"{kind} public {dt}", loss, xt.grad, *refd, sixteen=dt != torch.float32)
    # log-probabilities, the lattice by class (classic by default)
    lp = dev(logprobs32(x)).requires_grad_(True)
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    loss = ctc.ctc_wildcard_loss_from_logproba(dev(labels), lp, dev(ll), dev(tl), 0, cls if kind != "classic" else None)
    loss.sum().backward()
    compare(f"{kind} public from_logproba", loss, lp.grad, *oracle(kind, 1, logprobs32(x), labels, ll, tl), wrt=1)
    # a second derivative raises
    xt = dev(x).requires_grad_(True)
    loss = fn(dev(labels), xt, dev(ll), dev(tl), 0)
    (g,) = torch.autograd.grad(loss.sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
    # a positive weight is refused
    with pytest.raises(ValueError):
        fn(dev(labels), dev(x), dev(ll), dev(tl), 0, wildcard_log_weight=0.1)
