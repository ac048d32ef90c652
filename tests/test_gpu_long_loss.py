"""Long-form CTC loss and gradient on the GPU (ctc_amd_long_wildcard_loss_grad, csrc/ctc_loss_long.hip: the lattice of
ctc_amd_wildcard_loss_grad tiled over label blocks of 1024 positions x time blocks) against the float64 oracle
tests/tools/wildcard_loss_oracle.py, which has no limit on U and which tests/test_wildcard_loss_oracle.py pins without a GPU.

Bars: those of tests/test_gpu_wildcard_loss.py, through its compare():
  loss      |loss - oracle| <= 1e-4 + 1e-6 * |loss|
  gradient  |grad - oracle| <= 1e-4 * max(1, |d_loss[b]|) per element, plus 2^-8 * |oracle| for a 16-bit gradient
  row sums  |sum_k grad[t, k]| <= the same 1e-4 bar, for logits (16-bit gradients: V roundings of 2^-9 relative are added)
Every figure is printed before it is asserted (pytest -s shows them).  The oracle is computed once per input and left unchanged.
V = 32 unless a case says otherwise; every shape has at least one position in a second label block unless it is about one block."""
import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_wildcard_loss as WLT
from tests.tools import wildcard_loss_oracle as WL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = WL.WILDCARD
KINDS = WL.KINDS
dev, compare, oracle, kind_id = WLT.dev, WLT.compare, WLT.oracle, WLT.kind_id


def make(B, T, V, U, ll, tl, seed, wild=None, blank=0, scale=1.0, random_wild=0.0):
    """x[B, T, V] ~ N(0, scale^2), labels[B, U] without the blank, the given lengths; wild: per utterance the positions of its
    wildcards; random_wild: the share of further positions that become one."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    toks = np.asarray([k for k in range(V) if k != blank])
    labels = toks[rng.integers(0, len(toks), (B, U))].astype(np.int32)
    if random_wild:
        labels[rng.random((B, U)) < random_wild] = W
    for b, pos in enumerate(wild or ()):
        for i in pos:
            labels[b, i] = W
    return x, labels, np.asarray(ll, np.int32), np.asarray(tl, np.int32)


def run(kind, wrt, x, labels, ll, tl, blank=0, d_loss=None, weight=0.0, want_grad=True, grad_dtype=None, U=None, tf=0):
    """ops.long_wildcard_loss_grad on device copies; x may be a tensor in any format.  Returns (loss, grad) as device tensors."""
    from tf_seq2seq_losses_amd import ops
    loss, grad = ops.long_wildcard_loss_grad(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank,
                                             None if d_loss is None else dev(d_loss, torch.float32), U, grad_dtype, weight, want_grad, tf)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (len(ll),)
    return loss, grad


def ws_bytes(kind, x, U, tf=0, want_grad=True):
    from tf_seq2seq_losses_amd import _lib
    B, T, V = x.shape
    return _lib.long_wildcard_loss_workspace_bytes(kind_id(kind), B, T, V, U, tf, want_grad)


def raw_call(kind, wrt, x, labels, ll, tl, blank, weight, U, tf, d_loss, loss, grad, ws_ptr, ws_n):
    """The C entry point with every buffer under the caller's control; x and grad are [B, T, V] views with any strides."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V = x.shape
    rc = lib.ctc_amd_long_wildcard_loss_grad(
        kind_id(kind), wrt, x.data_ptr(), ops._DTYPES[x.dtype], x.stride(0), x.stride(1), labels.data_ptr(), labels.shape[1],
        ll.data_ptr(), tl.data_ptr(), blank, weight, B, T, V, U, tf, None if d_loss is None else d_loss.data_ptr(), loss.data_ptr(),
        None if grad is None else grad.data_ptr(), ops._DTYPES[(x if grad is None else grad).dtype],
        T * V if grad is None else grad.stride(0), V if grad is None else grad.stride(1), ws_ptr, ws_n,
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_long_wildcard_loss_grad")


def same(a, b):
    return OW.same_bits(a[0], b[0]) and OW.same_bits(a[1].contiguous(), b[1].contiguous())


# ---- 1: a second label block ----

CASE1 = dict(B=2, T=1300, V=32, U=1025, ll=(1025, 900), tl=(1300, 1200))


def case1(seed=1, **kw):
    return make(**dict(CASE1, **kw), seed=seed)


@pytest.mark.parametrize("kind", KINDS)
def test_second_label_block(kind):
    x, labels, ll, tl = case1()
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long1", kind))
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl)
    assert grad.dtype == torch.float32 and grad.is_contiguous()
    compare(f"long {kind} U=1025 (one position in block 1)", loss, grad, *ref)
    assert torch.all(grad[1, 1200:] == 0), "zeros beyond T_b"
    loss0, none = run(kind, 0, x, labels, ll, tl, want_grad=False)
    assert none is None and OW.same_bits(loss0, loss), "grad = NULL: the bits of the forward of the gradient call"


# ---- 2: three blocks, skipped tiles ----

@pytest.mark.parametrize("tf", [128, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_three_blocks_and_skipped_tiles(kind, tf):
    x, labels, ll, tl = make(2, 2600, 32, 2100, (2100, 1500), (2600, 2300), seed=2, random_wild=0.05)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long2", kind))
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl, tf=tf)
    compare(f"long {kind} U=2100 T=2600 tf={tf}", loss, grad, *ref)
    assert torch.all(grad[1, 2300:] == 0)


# ---- 3: the block boundary ----

@pytest.mark.parametrize("weight", [-0.5, 0.0])
@pytest.mark.parametrize("kind", KINDS)
def test_wildcards_at_the_block_boundary(kind, weight):
    """A wildcard at position 1023, at 1024, at both; as first and as last label.  U = 1030, label lengths 1025 .. 1030."""
    x, labels, ll, tl = make(4, 1300, 32, 1030, (1025, 1027, 1030, 1028), (1300, 1250, 1300, 1290), seed=3,
                             wild=((1023,), (1024,), (1023, 1024), (0, 1023, 1024, 1027)))
    ref = oracle(kind, 0, x, labels, ll, tl, weight=weight, key=("long3", kind, weight))
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl, weight=weight)
    compare(f"long {kind} boundary wildcards w={weight}", loss, grad, *ref)


def test_repeated_label_across_the_block_boundary():
    """Classic lattice, no wildcard: label[1023] == label[1024] forbids the skip into the second block, != allows it."""
    x, labels, ll, tl = make(2, 1300, 32, 1026, (1026, 1025), (1300, 1300), seed=4)
    labels[0, 1024] = labels[0, 1023]
    labels[1, 1024] = labels[1, 1023] % 31 + 1
    assert labels[0, 1023] == labels[0, 1024] and labels[1, 1023] != labels[1, 1024] and not (labels == W).any()
    ref = oracle("classic", 0, x, labels, ll, tl, key=("long3-repeat",))
    loss, grad = run("classic", 0, x, labels, ll, tl)
    compare("long classic label[1023] ==/!= label[1024]", loss, grad, *ref)
    # had the skip been allowed the loss of utterance 0 would be that of the lattice with the repeat treated as distinct: the
    # oracle tells the two apart by far more than the bar
    other = labels.copy()
    other[0, 1024] = labels[0, 1023] % 31 + 1
    assert abs(oracle("classic", 0, x, other, ll, tl, key=("long3-repeat-other",))[0][0] - ref[0][0]) > 1e-2


# ---- 4: invariance, bit for bit ----

@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_for_every_tile_height_and_batch(kind):
    x, labels, ll, tl = case1()
    base = run(kind, 0, x, labels, ll, tl, tf=128)
    assert same(base, run(kind, 0, x, labels, ll, tl, tf=0))
    for tf in (4, 64, 1300):
        assert same(base, run(kind, 0, x, labels, ll, tl, tf=tf)), tf
    # an utterance alone against the same utterance inside a batch of three
    x3, lab3, ll3, tl3 = case1(B=3, ll=(700, 1025, 900), tl=(1100, 1300, 1200), seed=5)
    x3[1:], lab3[1:] = x, labels
    three = run(kind, 0, x3, lab3, ll3, tl3)
    for b in (0, 1):
        alone = run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1])
        assert same(alone, (base[0][b:b + 1], base[1][b:b + 1])) and same(alone, (three[0][b + 1:b + 2], three[1][b + 1:b + 2])), b


# ---- 5: one block: the existing call ----

@pytest.mark.parametrize("shape", [(2, 1300, 32, 1024), (2, 200, 32, 129)], ids=["U1024", "U129"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_block_against_the_one_wavefront_call(kind, shape):
    B, T, V, U = shape
    x, labels, ll, tl = make(B, T, V, U, (U, U - U // 4), (T, T - 40), seed=6, random_wild=0.1)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long5", kind, shape))
    loss, grad = run(kind, 0, x, labels, ll, tl)
    compare(f"long {kind} {shape}", loss, grad, *ref)
    loss1, grad1 = WLT.run(kind, 0, x, labels, ll, tl)
    compare(f"one-wavefront {kind} {shape}", loss1, grad1, *ref)
    lerr = (loss - loss1).abs().cpu().numpy()
    gerr = float((grad - grad1).abs().max())
    print(f"LONG-LOSS {kind} {shape}: worst |loss - one-wavefront| {lerr.max():.3e}, worst |grad - one-wavefront| {gerr:.3e}, "
          f"loss bits equal: {OW.same_bits(loss, loss1)}, gradient bits equal: {OW.same_bits(grad, grad1)}")
    assert np.all(lerr <= WLT.loss_tol(ref[0])) and gerr <= 1e-4


# ---- 6: formats ----

FMT = dict(B=2, T=1100, V=32, U=1026, ll=(1026, 700), tl=(1100, 1000))


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    x, labels, ll, tl = make(**FMT, seed=7, wild=((5, 1023), (0,)))
    B, T, V = x.shape
    xt = dev(x)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long6", kind))
    base = run(kind, 0, xt, labels, ll, tl)
    compare(f"long {kind} formats float32", *base, *ref)
    for dt in (torch.bfloat16, torch.float16):  # the oracle reads what the kernel reads
        xh = xt.to(dt)
        refh = oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl, key=("long6", kind, str(dt)))
        loss, grad = run(kind, 0, xh, labels, ll, tl)
        assert grad.dtype == dt
        compare(f"long {kind} {dt}", loss, grad, *refh, sixteen=True)
    # time-major: read in place, the gradient comes back in the same layout, the same bits
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)
    assert xtm.stride() == (V, B * V, 1)
    got = run(kind, 0, xtm, labels, ll, tl)
    assert got[1].stride() == xtm.stride() and same(got, base)
    # an offset base pointer: the element-wise accesses give identical bits
    flat = torch.zeros(B * T * V + 1, dtype=torch.float32, device=DEV)
    xo = flat[1:].view(B, T, V)
    xo.copy_(xt)
    assert xo.data_ptr() % 16 == 4
    assert same(run(kind, 0, xo, labels, ll, tl), base)
    # strides beyond V: the same bits, and what no row owns keeps its prefill
    for pad in (3, 4):
        st, sb = V + pad, (V + pad) * T + 8
        _, xv, _ = OW.strided_storage(xt, sb, st, pattern=0x7F)
        gstore, gv, owned = OW.strided_storage(torch.zeros((B, T, V), device=DEV), sb, st, pattern=0xA5)
        gv.copy_(OW.filled((B, T, V), torch.float32, 0xA5, DEV))
        loss = OW.filled((B,), torch.float32, 0xA5, DEV)
        n = ws_bytes(kind, xt, 1026)
        ws = OW.byte_fill(n, 0xA5, DEV)
        raw_call(kind, 0, xv, dev(labels), dev(ll), dev(tl), 0, 0.0, 1026, 0, None, loss, gv, ws.data_ptr(), n)
        torch.cuda.synchronize()
        assert bool(OW.keeps_prefill(gstore, 0xA5)[~owned].all()), "elements between V and the stride are untouched"
        assert same((loss, gv), base), pad


@pytest.mark.parametrize("kind", KINDS)
def test_log_probabilities_and_the_last_token_as_blank(kind):
    x, labels, ll, tl = make(**FMT, seed=8, wild=((5, 1024), (699,)))
    lp = WLT.logprobs32(x) - np.float32(0.25)  # not normalised: e_w carries the rows' log-sum-exp
    ref = oracle(kind, 1, lp, labels, ll, tl, weight=-0.25, key=("long6-lp", kind))
    loss, grad = run(kind, 1, lp, labels, ll, tl, weight=-0.25)
    compare(f"long {kind} log-probabilities", loss, grad, *ref, wrt=1)
    x, labels, ll, tl = make(**FMT, seed=9, blank=31, wild=((1023,), ()))
    ref = oracle(kind, 0, x, labels, ll, tl, blank=31, key=("long6-blank", kind))
    loss, grad = run(kind, 0, x, labels, ll, tl, blank=31)
    compare(f"long {kind} blank=V-1", loss, grad, *ref)


# ---- 7: column passes ----

@pytest.mark.parametrize("kind", KINDS)
def test_a_vocabulary_of_more_than_one_column_pass(kind):
    x, labels, ll, tl = make(1, 1100, 1030, 1025, (1025,), (1100,), seed=10, wild=((7,),))
    labels[0, 1], labels[0, 3], labels[0, 1024], labels[0, 1020] = 1029, 1029, 1024, 1027  # the second pass, from both blocks
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long7", kind))
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 0, x, labels, ll, tl)
    compare(f"long {kind} V=1030", loss, grad, *ref)


# ---- 8: sharp logits ----

@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits(kind):
    x, labels, ll, tl = case1(seed=11, scale=4.0)
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long8", kind))
    loss, grad = run(kind, 0, x, labels, ll, tl)
    compare(f"long {kind} N(0, 4^2) logits", loss, grad, *ref)


# ---- 9: edges ----

@pytest.mark.parametrize("kind", KINDS)
def test_edges(kind):
    V, U, T = 32, 1040, 1200
    ll = (0, 5, 1040, 1041, 1040, 1040, 1040, 0)
    tl = (900, 0, T, T, T, T, 1039, 0)
    x, labels, ll, tl = make(8, T, V, U, ll, tl, seed=12, wild=((), (), (), (), (), (0, 1023, 1024, 1039), (), ()))
    labels[2, 1030] = 0   # a label equal to the blank, in the second label block
    labels[4, 1025] = -3  # not a label and not the wildcard
    d = (np.random.default_rng(2).standard_normal(8) * 3).astype(np.float32)
    d[[1, 2, 3, 4, 6]] = np.nan  # the infeasible ones: not interpreted
    ref = oracle(kind, 0, x, labels, ll, tl, d_loss=d, key=("long9", kind))
    assert np.array_equal(np.isfinite(ref[0]), [True, False, False, False, False, True, False, True]) and ref[0][7] == 0.0
    loss, grad = run(kind, 0, x, labels, ll, tl, d_loss=d, tf=64)
    compare(f"long {kind} edges, random d_loss, NaN for the infeasible", loss, grad, *ref, d_loss=d)
    for b in (1, 2, 3, 4, 6):
        assert float(loss[b]) == np.inf and torch.all(grad[b] == 0), b
    assert float(loss[7]) == 0.0 and torch.all(grad[7] == 0)  # no frames, no labels
    assert torch.all(grad[0, 900:] == 0) and torch.isfinite(grad).all()
    want = -WLT.logprobs32(x[0, :900]).astype(np.float64)[:, 0].sum()  # label_length 0: the all-blank path
    print(f"LONG-LOSS {kind} L = 0: loss {float(loss[0]):.6f}, -sum lp[t, blank] {want:.6f}")
    assert abs(float(loss[0]) - want) <= WLT.loss_tol(want)
    loss0, _ = run(kind, 0, x, labels, ll, tl, want_grad=False, tf=64)
    assert OW.same_bits(loss0, loss)
    # the feasible long one alone: the others change nothing in it
    alone = run(kind, 0, x[5:6], labels[5:6], ll[5:6], tl[5:6], d_loss=d[5:6], tf=64)
    assert same(alone, (loss[5:6], grad[5:6]))


def test_empty_shapes():
    import tf_seq2seq_losses_amd as ctc
    i32 = dict(dtype=torch.int32, device=DEV)
    z = ctc.classic_ctc_long_loss(torch.zeros((0, 2), **i32), torch.zeros((0, 4, 3), device=DEV), torch.zeros(0, **i32), torch.zeros(0, **i32))
    assert z.shape == (0,)
    x = torch.zeros((2, 0, 3), device=DEV, requires_grad=True)
    z = ctc.simplified_ctc_long_loss(torch.tensor([[W, 2], [1, 2]], **i32), x, torch.tensor([2, 0], **i32), torch.zeros(2, **i32))
    z[1].backward()
    torch.cuda.synchronize()
    assert z.detach().cpu().tolist() == [np.inf, 0.0] and x.grad.shape == (2, 0, 3)


# ---- 10: prefill and graph replay ----

@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_whatever_the_buffers_held_and_under_graph_capture(kind):
    x, labels, ll, tl = make(3, 1300, 32, 1025, (1025, 1025, 900), (1300, 1024, 1200), seed=13, wild=((0, 1024), (), (899,)))
    B, T, V = x.shape  # (utterance 1: more labels than frames, its zeros are written, not left over)
    xt, lt, llt, tlt = dev(x), dev(labels), dev(ll), dev(tl)
    d = dev(np.asarray([1.5, np.nan, -2.0], np.float32))
    n = ws_bytes(kind, xt, 1025, 64)
    outs = []
    for pattern in (0x00, 0xFF):
        ws = OW.byte_fill(n, pattern, DEV)
        loss = OW.filled((B,), torch.float32, pattern, DEV)
        grad = OW.filled((B, T, V), torch.float32, pattern, DEV)
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, 1025, 64, d, loss, grad, ws.data_ptr(), n)
        torch.cuda.synchronize()
        outs.append((loss, grad))
    assert same(outs[0], outs[1])
    assert float(outs[0][0][1]) == np.inf and torch.all(outs[0][1][1] == 0) and torch.isfinite(outs[0][1]).all()
    assert same(outs[0], run(kind, 0, x, labels, ll, tl, d_loss=d, weight=-0.25))
    # capture on one stream (no parallel branches), replay twice
    ws = OW.byte_fill(n, 0x5A, DEV)
    loss = OW.filled((B,), torch.float32, 0x5A, DEV)
    grad = OW.filled((B, T, V), torch.float32, 0x5A, DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, 1025, 64, d, loss, grad, ws.data_ptr(), n)
    for _ in range(2):
        loss.fill_(7.0)
        grad.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same((loss, grad), outs[0])


# ---- 11: ownership ----

def guarded_call(kind, inp, pattern, d_loss, tf=64, guard=64):
    """The call on guarded, prefilled outputs and a guarded workspace: nothing around them is written."""
    B, T, V, U = inp.shape
    n = ws_bytes(kind, inp.x, U, tf)
    ws = OW.workspace(n + 512, pattern)
    lbuf = OW.filled((B + 2 * guard,), torch.float32, pattern, DEV)
    gbuf = OW.filled((B * T * V + 2 * guard,), torch.float32, pattern, DEV)
    loss, grad = lbuf[guard:guard + B], gbuf[guard:guard + B * T * V].view(B, T, V)
    raw_call(kind, 0, inp.x, inp.labels, inp.ll, inp.tl, 0, 0.0, U, tf, d_loss, loss, grad, ws.data_ptr() + 256, n)
    torch.cuda.synchronize()
    for buf in (lbuf, gbuf):
        keep = OW.keeps_prefill(buf, pattern)
        assert bool(keep[:guard].all()) and bool(keep[-guard:].all())
    keep = OW.keeps_prefill(ws, pattern)
    assert bool(keep[:256].all()) and bool(keep[-256:].all())
    return {"loss": loss, "grad": grad}


@pytest.mark.parametrize("kind", KINDS)
def test_ownership(kind):
    x, labels, ll, tl = make(2, 1200, 32, 1030, (1030, 300), (1200, 500), seed=14, wild=((0, 1023, 1024, 1029), (0, 150)))
    clean = OW.make_inputs(kind_id(kind), x, labels, ll, tl)
    d = dev(np.asarray([0.5, -1.25], np.float32))
    a = guarded_call(kind, clean, 0xA5, d)
    assert bool(torch.isfinite(a["loss"]).all()) and bool((a["grad"][1, 500:] == 0).all())
    assert not bool(OW.keeps_prefill(a["grad"], 0xA5).any()) and not bool(OW.keeps_prefill(a["loss"], 0xA5).any())  # every element is written
    # what the utterances do not own may hold anything: padding frames, label tails, the outputs and the workspace on entry
    xt = torch.from_numpy(x).to(DEV)
    for pattern, value in ((0x00, float("nan")), (0xFF, 3.0e38)):
        dirty = clean.replace(x=OW.poison_padding(xt, tl, value), labels=OW.poison_labels(clean.labels, ll, OW.label_poison_cycle(32, 0)))
        b = guarded_call(kind, dirty, pattern, d)
        diff = OW.total_diff(a, b)
        assert not any(diff.values()), (pattern, diff)


# ---- 12: the public surface ----

@pytest.mark.parametrize("kind", KINDS)
def test_public_surface(kind):
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = make(**FMT, seed=7, wild=((5, 1023), (0,)))
    ref = oracle(kind, 0, x, labels, ll, tl, key=("long6", kind))
    fn = ctc.classic_ctc_long_loss if kind == "classic" else ctc.simplified_ctc_long_loss
    lt, llt, tlt = dev(labels), dev(ll), dev(tl)
    loss = fn(lt, dev(x), llt, tlt, 0)
    assert not loss.requires_grad and loss.dtype == torch.float32
    compare(f"long {kind} public, forward only", loss, None, *ref)
    xt = dev(x).requires_grad_(True)
    loss = fn(lt, xt, llt, tlt, 0, frames_per_tile=64, max_label_length=1026)
    assert loss.requires_grad
    d = torch.tensor([0.75, -1.5], device=DEV)
    loss.backward(d)
    torch.cuda.synchronize()
    want = run(kind, 0, x, labels, ll, tl, d_loss=d)
    assert same((loss.detach(), xt.grad), want), "backward is the ops-level gradient, bit for bit"
    # log-probabilities, the lattice by class (classic by default)
    lp = dev(WLT.logprobs32(x)).requires_grad_(True)
    cls = None if kind == "classic" else ctc.SimplifiedCtcLossData
    loss = ctc.ctc_long_loss_from_logproba(lt, lp, llt, tlt, 0, cls, wildcard_log_weight=-0.5)
    loss.sum().backward()
    assert same((loss.detach(), lp.grad), run(kind, 1, lp.detach(), labels, ll, tl, weight=-0.5))
    # bfloat16: the gradient in the logits' dtype
    xh = dev(x).to(torch.bfloat16).requires_grad_(True)
    fn(lt, xh, llt, tlt).sum().backward()
    assert xh.grad.dtype == torch.bfloat16 and xh.grad.shape == xh.shape
    # a second derivative raises
    xt = dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(fn(lt, xt, llt, tlt, 0).sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
    # keyword-only, and what is refused
    with pytest.raises(TypeError):
        fn(lt, dev(x), llt, tlt, 0, 0.0)
    with pytest.raises(TypeError):
        ctc.ctc_long_loss_from_logproba(lt, dev(x), llt, tlt, 0, None, 0.0)
    for bad in (6, -4, 1):
        with pytest.raises(Exception, match="frames_per_tile"):
            fn(lt, dev(x), llt, tlt, 0, frames_per_tile=bad)
    with pytest.raises(ValueError):
        fn(lt, dev(x), llt, tlt, 0, wildcard_log_weight=0.1)
    # check_labels keeps rejecting the wildcard
    with pytest.raises(Exception):
        ctc.check_labels(lt, llt, 32, 0)
