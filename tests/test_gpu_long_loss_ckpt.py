"""The long-form CTC gradient from tile checkpoints on the GPU (ctc_amd_long_wildcard_loss_grad_ckpt, csrc/ctc_loss_long.hip; DESIGN.md
section 5.21) against the existing, unchanged call ctc_amd_long_wildcard_loss_grad on the same inputs: the chain step, the posteriors
and the row stage are the same code and a tile starts from the same float64 state, so loss and gradient are compared with
OW.same_bits, never with a tolerance.  One comparison per lattice goes through the float64 oracle at the bars of
tests/test_gpu_long_loss.py, whose helpers and inputs are used.  V = 32 unless a case says otherwise."""
import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_long_loss as LL
from tests import test_gpu_wildcard_loss as WLT

pytestmark = pytest.mark.gpu

DEV = LL.DEV
W = LL.W
KINDS = LL.KINDS
dev, compare, oracle, kind_id, make, same = LL.dev, LL.compare, LL.oracle, LL.kind_id, LL.make, LL.same


def run(kind, wrt, x, labels, ll, tl, blank=0, d_loss=None, weight=0.0, grad_dtype=None, U=None, tf=0, checkpoint=True):
    """ops.long_wildcard_loss_grad with a gradient, checkpointed or not, on device copies; (loss, grad) as device tensors."""
    from tf_seq2seq_losses_amd import ops
    loss, grad = ops.long_wildcard_loss_grad(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank,
                                             None if d_loss is None else dev(d_loss, torch.float32), U, grad_dtype, weight, True, tf,
                                             checkpoint=checkpoint)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (len(ll),)
    return loss, grad


def both(kind, wrt, x, labels, ll, tl, **kw):
    """(checkpointed, existing) on the same inputs, after asserting that they are the same bits."""
    got, want = run(kind, wrt, x, labels, ll, tl, **kw), run(kind, wrt, x, labels, ll, tl, checkpoint=False, **kw)
    assert got[1].dtype == want[1].dtype and got[1].stride() == want[1].stride()
    assert same(got, want), (kind, {k: v for k, v in kw.items() if k != "d_loss"},
                             float((got[1].float() - want[1].float()).abs().max()), got[0].tolist(), want[0].tolist())
    return got, want


def ws_bytes(kind, x, U, tf=0):
    from tf_seq2seq_losses_amd import _lib
    B, T, V = x.shape
    return _lib.long_wildcard_loss_ckpt_workspace_bytes(kind_id(kind), B, T, V, U, tf, True)


def raw_call(kind, wrt, x, labels, ll, tl, blank, weight, U, tf, d_loss, loss, grad, ws_ptr, ws_n):
    """The C entry point with every buffer under the caller's control."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V = x.shape
    rc = lib.ctc_amd_long_wildcard_loss_grad_ckpt(
        kind_id(kind), wrt, x.data_ptr(), ops._DTYPES[x.dtype], x.stride(0), x.stride(1), labels.data_ptr(), labels.shape[1],
        ll.data_ptr(), tl.data_ptr(), blank, weight, B, T, V, U, tf, None if d_loss is None else d_loss.data_ptr(), loss.data_ptr(),
        grad.data_ptr(), ops._DTYPES[grad.dtype], grad.stride(0), grad.stride(1), ws_ptr, ws_n, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_long_wildcard_loss_grad_ckpt")


# ---- 1: three blocks and a wrapping ring ----

@pytest.mark.parametrize("kind", KINDS)
def test_three_blocks_and_a_wrapping_ring(kind):
    """K = 3.  tf = 128 / 64: J = 21 / 41, the ring of R = 3 wraps; tf = 4: J = 650, it wraps over 200 times; tf = 1300: J = 2 < K,
    R = J and every time block has its own slot."""
    x, labels, ll, tl = make(2, 2600, 32, 2100, (2100, 1500), (2600, 2300), seed=2, random_wild=0.05)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long2", kind))
    assert np.isfinite(ref[0]).all()
    first = None
    for tf in (128, 64, 4, 1300):
        got, want = both(kind, 0, x, labels, ll, tl, tf=tf)
        assert torch.all(got[1][1, 2300:] == 0)
        if first is None:
            first = got
            compare(f"long checkpointed {kind} U=2100 T=2600 tf={tf}", *got, *ref)
        assert same(got, first), f"tf={tf}: the bits of tf=128"


# ---- 2: a ragged batch beside a three-block utterance ----

@pytest.mark.parametrize("tf", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch(kind, tf):
    """Beside the three-block utterance 0: more labels than frames (+inf, an exactly zero gradient, NaN in its d_loss); no labels; no
    frames; no frames and no labels; one label block only (blocks beyond the labels); so few frames that whole trailing time blocks
    have no tile; more labels than U."""
    U, T = 2100, 2300
    ll = (2100, 1500, 0, 5, 0, 700, 1100, 2101)
    tl = (2300, 1400, 900, 0, 0, 2300, 1150, 2300)
    x, labels, ll, tl = make(8, T, 32, U, ll, tl, seed=21, random_wild=0.03)
    d = (np.random.default_rng(3).standard_normal(8) * 2).astype(np.float32)
    d[[1, 3, 7]] = np.nan
    got, want = both(kind, 0, x, labels, ll, tl, d_loss=d, tf=tf)
    loss, grad = got
    assert np.array_equal(torch.isfinite(loss).cpu().numpy(), [True, False, True, False, True, True, True, False]), loss.tolist()
    for b in (1, 3, 7):
        assert float(loss[b]) == np.inf and torch.all(grad[b] == 0), b
    assert float(loss[4]) == 0.0 and torch.all(grad[4] == 0)
    assert torch.isfinite(grad).all()
    for b, t in ((2, 900), (6, 1150)):
        assert torch.all(grad[b, t:] == 0) and bool((grad[b, :t] != 0).any()), b
    # the three-block utterance alone: the others change nothing in it
    alone = run(kind, 0, x[:1], labels[:1], ll[:1], tl[:1], d_loss=d[:1], tf=tf)
    assert same(alone, (loss[:1], grad[:1]))


# ---- 3: the block boundary ----

@pytest.mark.parametrize("weight", [-0.5, 0.0])
@pytest.mark.parametrize("kind", KINDS)
def test_wildcards_at_the_block_boundary(kind, weight):
    x, labels, ll, tl = make(4, 1300, 32, 1030, (1025, 1027, 1030, 1028), (1300, 1250, 1300, 1290), seed=3,
                             wild=((1023,), (1024,), (1023, 1024), (0, 1023, 1024, 1027)))
    both(kind, 0, x, labels, ll, tl, weight=weight)


def test_repeated_label_across_the_block_boundary():
    x, labels, ll, tl = make(2, 1300, 32, 1026, (1026, 1025), (1300, 1300), seed=4)
    labels[0, 1024] = labels[0, 1023]
    labels[1, 1024] = labels[1, 1023] % 31 + 1
    assert labels[0, 1023] == labels[0, 1024] and labels[1, 1023] != labels[1, 1024] and not (labels == W).any()
    both("classic", 0, x, labels, ll, tl)
    both("classic", 0, x, labels, ll, tl, tf=64)


# ---- 4: formats and inputs ----

@pytest.mark.parametrize("kind", KINDS)
def test_formats_and_inputs(kind):
    x, labels, ll, tl = make(**LL.FMT, seed=7, wild=((5, 1023), (0,)))
    B, T, V = x.shape
    xt = dev(x)
    base, _ = both(kind, 0, xt, labels, ll, tl)
    for dt in (torch.bfloat16, torch.float16):
        got, _ = both(kind, 0, xt.to(dt), labels, ll, tl)
        assert got[1].dtype == dt
    # time-major: read in place, the gradient comes back in the same layout
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)
    assert xtm.stride() == (V, B * V, 1)
    got, _ = both(kind, 0, xtm, labels, ll, tl)
    assert got[1].stride() == xtm.stride() and same(got, base)
    # an unaligned V: the element-wise accesses
    x31, lab31, _, _ = make(2, 1100, 31, 1026, (1026, 700), (1100, 1000), seed=22, wild=((5, 1023), (0,)))
    both(kind, 0, x31, lab31, ll, tl)
    # a blank other than 0
    xb, labb, _, _ = make(**LL.FMT, seed=9, blank=31, wild=((1023,), ()))
    both(kind, 0, xb, labb, ll, tl, blank=31)
    # with respect to log-probabilities that are not normalised
    lp = WLT.logprobs32(x) - np.float32(0.25)
    both(kind, 1, lp, labels, ll, tl, weight=-0.25, d_loss=np.asarray([0.5, -2.0], np.float32))


# ---- 5: one block ----

@pytest.mark.parametrize("shape", [(2, 1300, 32, 1024), (2, 200, 32, 129)], ids=["U1024", "U129"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_block(kind, shape):
    """K = 1 (R = 1: one time block in flight): the bits of the existing long call, and of the one-wavefront call as far as the
    existing long call has them."""
    B, T, V, U = shape
    x, labels, ll, tl = make(B, T, V, U, (U, U - U // 4), (T, T - 40), seed=6, random_wild=0.1)
    got, want = both(kind, 0, x, labels, ll, tl)
    assert same(got, run(kind, 0, x, labels, ll, tl, tf=64))
    loss1, grad1 = WLT.run(kind, 0, x, labels, ll, tl)
    assert OW.same_bits(got[0], loss1) and OW.same_bits(got[1], grad1), "the one-wavefront call's bits (DESIGN.md section 5.20)"


# ---- 6: the raw C call with an exact-size workspace ----

@pytest.mark.parametrize("kind", KINDS)
def test_raw_call_exact_workspace_and_guards(kind):
    x, labels, ll, tl = make(3, 2200, 32, 2060, (2060, 1025, 900), (2200, 1024, 1200), seed=13, wild=((0, 1024, 2050), (), (899,)))
    B, T, V = x.shape  # (utterance 1: more labels than frames, its zeros are written, not left over)
    U, tf, guard = 2060, 64, 64
    xt, lt, llt, tlt = dev(x), dev(labels), dev(ll), dev(tl)
    d = dev(np.asarray([1.5, np.nan, -2.0], np.float32))
    n = ws_bytes(kind, xt, U, tf)
    from tf_seq2seq_losses_amd import _lib
    assert n < _lib.long_wildcard_loss_workspace_bytes(kind_id(kind), B, T, V, U, tf, True) // 4
    want = run(kind, 0, x, labels, ll, tl, d_loss=d, weight=-0.25, tf=tf, checkpoint=False)
    outs = []
    for pattern in (0x00, 0xFF, None):
        ws = OW.workspace(n + 512, pattern or 0xA5)
        if pattern is None:  # the leftovers of a different call: other logits, weight and lengths in the same workspace
            lo, go = torch.empty(B, device=DEV), torch.empty((B, T, V), device=DEV)
            raw_call(kind, 0, xt.flip(0).contiguous(), lt, llt.flip(0).contiguous(), tlt, 0, 0.0, U, tf, None, lo, go, ws.data_ptr() + 256, n)
        p = pattern or 0xA5
        lbuf = OW.filled((B + 2 * guard,), torch.float32, p, DEV)
        gbuf = OW.filled((B * T * V + 2 * guard,), torch.float32, p, DEV)
        loss, grad = lbuf[guard:guard + B], gbuf[guard:guard + B * T * V].view(B, T, V)
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, tf, d, loss, grad, ws.data_ptr() + 256, n)
        torch.cuda.synchronize()
        for buf in (lbuf, gbuf):
            keep = OW.keeps_prefill(buf, p)
            assert bool(keep[:guard].all()) and bool(keep[-guard:].all()), pattern
        keep = OW.keeps_prefill(ws, pattern or 0xA5)
        assert bool(keep[:256].all()) and bool(keep[-256:].all()), pattern
        outs.append((loss, grad))
    assert same(outs[0], outs[1]) and same(outs[0], outs[2]) and same(outs[0], want)
    assert float(outs[0][0][1]) == np.inf and torch.all(outs[0][1][1] == 0) and torch.isfinite(outs[0][1]).all()


# ---- 7: capture ----

@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_and_replay_with_fresh_logits(kind):
    x, labels, ll, tl = make(2, 1300, 32, 2050, (1290, 900), (1300, 1200), seed=15, wild=((0, 1024), (899,)))
    B, T, V = x.shape
    U, tf = 2050, 64
    rng = np.random.default_rng(16)
    fresh = [x] + [rng.standard_normal(x.shape).astype(np.float32) for _ in range(2)]
    xt, lt, llt, tlt = dev(x).clone(), dev(labels), dev(ll), dev(tl)
    d = dev(np.asarray([1.5, -2.0], np.float32))
    n = ws_bytes(kind, xt, U, tf)
    ws = OW.byte_fill(n, 0x5A, DEV)
    loss = OW.filled((B,), torch.float32, 0x5A, DEV)
    grad = OW.filled((B, T, V), torch.float32, 0x5A, DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):  # one stream: no parallel branches
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, tf, d, loss, grad, ws.data_ptr(), n)
    for xi in fresh[1:]:
        xt.copy_(dev(xi))
        loss.fill_(7.0)
        grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(kind, 0, xi, labels, ll, tl, d_loss=d, weight=-0.25, tf=tf)
        assert same((loss, grad), eager)
        assert same(eager, run(kind, 0, xi, labels, ll, tl, d_loss=d, weight=-0.25, tf=tf, checkpoint=False))


# ---- 8: the public surface ----

@pytest.mark.parametrize("kind", KINDS)
def test_public_surface(kind):
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops
    x, labels, ll, tl = make(**LL.FMT, seed=7, wild=((5, 1023), (0,)))
    B, T, V = x.shape
    fn = ctc.classic_ctc_long_loss if kind == "classic" else ctc.simplified_ctc_long_loss
    lt, llt, tlt = dev(labels), dev(ll), dev(tl)
    d = torch.tensor([0.75, -1.5], device=DEV)
    res = {}
    for ck in (False, True):
        xt = dev(x).requires_grad_(True)
        loss = fn(lt, xt, llt, tlt, 0, frames_per_tile=64, max_label_length=1026, checkpoint=ck)
        assert loss.requires_grad
        (g,) = torch.autograd.grad(loss, xt, d)
        torch.cuda.synchronize()
        res[ck] = (loss.detach(), g)
    assert same(res[True], res[False]) and bool((res[True][1] != 0).any())
    # each flag asks for its own workspace size, under its own key
    k = kind_id(kind)
    sizes = {key[0]: n for key, n in ops._WS_BYTES.items() if key[1:] == (k, B, T, V, 1026, 64, True)}
    assert sizes == {"long_wildcard_loss_grad": _lib.long_wildcard_loss_workspace_bytes(k, B, T, V, 1026, 64, True),
                     "long_wildcard_loss_grad_ckpt": _lib.long_wildcard_loss_ckpt_workspace_bytes(k, B, T, V, 1026, 64, True)}, sizes
    assert sizes["long_wildcard_loss_grad_ckpt"] < sizes["long_wildcard_loss_grad"] // 4
    # log-probabilities, the lattice by class
    cls = None if kind == "classic" else ctc.SimplifiedCtcLossData
    grads = []
    for ck in (False, True):
        lp = dev(WLT.logprobs32(x)).requires_grad_(True)
        loss = ctc.ctc_long_loss_from_logproba(lt, lp, llt, tlt, 0, cls, wildcard_log_weight=-0.5, checkpoint=ck)
        loss.sum().backward()
        grads.append((loss.detach(), lp.grad))
    assert same(*grads)
    # forward only is the same call either way; a second derivative raises; keyword-only
    assert OW.same_bits(fn(lt, dev(x), llt, tlt, 0, checkpoint=True), fn(lt, dev(x), llt, tlt, 0))
    xt = dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(fn(lt, xt, llt, tlt, 0, checkpoint=True).sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
    with pytest.raises(TypeError):
        fn(lt, dev(x), llt, tlt, 0, 0.0, None, None, True)
