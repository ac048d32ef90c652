"""Label posteriors on the GPU (ctc_amd_label_posterior, the MODE 3 sweep of csrc/ctc_wild_loss.hip) against the float64 oracle
tests/tools/label_posterior_oracle.py, which tests/test_label_posterior_oracle.py pins without a GPU.

Bars, from the project:
  label_posterior, blank_posterior   |gpu - oracle| <= 1e-4 per element: the bar of a posterior-valued element (the gradient's)
  row sums                           |sum_i label_posterior + blank_posterior - 1| <= 1e-4
  loss                               the bits of ops.wildcard_loss_grad forward-only on the same inputs
  duration, expected_frame           within 2 float32 ulps of a float64 host reduction of the RETURNED label_posterior (they are
                                     defined as that reduction, rounded once); against the oracle's own values T_b * 1e-4, the
                                     per-element bar summed over the frames, for both
Inputs are those of tests/test_gpu_wildcard_loss.py: wildcards at both ends, inside and adjacent, repeated labels, ragged lengths.
The oracle reads the float32 value of every element the kernel reads.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests.test_gpu_wildcard_loss import dev, kind_id, logprobs32, make_inputs
from tests.tools import label_posterior_oracle as LP
from tests.tools import wildcard_loss_oracle as WL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = LP.WILDCARD
KINDS = ("classic", "simplified")
# the smallest shapes on both sides of every NL boundary, and a U that is no multiple of 4 below its padded width
GRID = [(4, 12, 5, 3), (2, 88, 8, 64), (2, 90, 7, 70), (2, 169, 8, 129), (2, 649, 8, 513), (2, 1288, 8, 1024)]
SMALL = (2, 90, 7, 70)
NAMES = ("loss", "label_posterior", "blank_posterior", "duration", "expected_frame")


def run(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, U=None, want_stats=True):
    """ops.label_posterior on device copies; x may be a tensor in any format.  Returns the five device tensors."""
    from tf_seq2seq_losses_amd import ops
    out = ops.label_posterior(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank, labels.shape[1] if U is None else U,
                              weight, want_stats)
    torch.cuda.synchronize()
    B, T = len(ll), x.shape[1]
    Uo = out[1].shape[2]
    assert all(o.dtype == torch.float32 and o.is_contiguous() for o in out if o is not None)
    assert tuple(out[0].shape) == (B,) and tuple(out[1].shape) == (B, T, Uo) and tuple(out[2].shape) == (B, T)
    if want_stats:
        assert tuple(out[3].shape) == (B, Uo) == tuple(out[4].shape)
    return out


def wild_loss(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, U=None):
    from tf_seq2seq_losses_amd import ops
    return ops.wildcard_loss_grad(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank, None,
                                  labels.shape[1] if U is None else U, None, weight, False)[0]


_ORACLE_INPUTS = {}


@functools.lru_cache(maxsize=None)
def _oracle_cached(kind, wrt, key, blank, weight):
    x, labels, ll, tl = _ORACLE_INPUTS[key]
    return LP.label_posterior(kind, wrt, labels, x, ll, tl, blank, weight)


def oracle(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, key=None):
    """The float64 reference, computed once per `key` and left unchanged."""
    if key is None:
        return LP.label_posterior(kind, wrt, labels, x, ll, tl, blank, weight)
    _ORACLE_INPUTS.setdefault(key, (x, labels, ll, tl))
    return _oracle_cached(kind, wrt, key, blank, weight)


def ulps(got, want):
    """|got - want| in units of the float32 spacing at `want` (float64 arrays; 0 where both are equal)."""
    sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.abs(got - want) / sp


def host_reduction(post, tl):
    """duration and expected_frame as the header defines them: float64 sums over t < T_b of the returned float32 matrix."""
    B, T, U = post.shape
    p = post.astype(np.float64) * (np.arange(T)[None, :, None] < np.asarray(tl).clip(0, T)[:, None, None])
    d = p.sum(axis=1)
    m = (p * np.arange(T, dtype=np.float64)[None, :, None]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return d, np.where(d > 0.0, m / d, -1.0)


def compare(what, out, ref, labels, ll, tl, wild_bits=None):
    """Prints every figure, then asserts the bars of the module docstring and the padding rules.  Returns the worst errors."""
    loss, post, blk, dur, exf = (o.cpu().numpy().astype(np.float64) for o in out)
    rloss, rpost, rblk, rdur, rexf = ref
    B, T, U = post.shape
    fin = np.isfinite(rloss)
    assert np.array_equal(np.isfinite(loss), fin) and np.all(loss[~fin] == np.inf), (what, loss, rloss)
    assert not np.isnan(post).any() and not np.isnan(blk).any() and not np.isnan(dur).any() and not np.isnan(exf).any(), what
    Tb = np.where(fin, np.asarray(tl).clip(0, T), 0)
    Lb = np.where(fin, np.asarray(ll).clip(0, None), 0)
    live = np.arange(T)[None, :] < Tb[:, None]
    perr, berr = np.abs(post - rpost).max(initial=0.0), np.abs(blk - rblk).max(initial=0.0)
    rows = post.sum(axis=2) + blk
    rerr = np.abs(rows[live] - 1.0).max(initial=0.0)
    hd, he = host_reduction(out[1].cpu().numpy(), Tb)
    du, eu = ulps(dur, hd).max(initial=0.0), ulps(exf, he).max(initial=0.0)
    sbar = np.maximum(Tb, 1)[:, None] * 1e-4
    derr, eerr = np.abs(dur - rdur), np.abs(exf - rexf)
    print(f"LABEL-POSTERIOR {what}: worst |gpu - oracle| label {perr:.3e} blank {berr:.3e}, worst |row sum - 1| {rerr:.3e}, "
          f"duration {du:.2f} ulp / expected_frame {eu:.2f} ulp from the host reduction, |gpu - oracle| duration {derr.max(initial=0.0):.3e} "
          f"expected_frame {eerr.max(initial=0.0):.3e} (bar {sbar.min():.1e}), smallest duration {np.min(np.where(np.arange(U)[None, :] < Lb[:, None], dur, np.inf)):.6f}")
    assert perr <= 1e-4 and berr <= 1e-4, (what, perr, berr)
    assert rerr <= 1e-4, (what, rerr)
    assert du <= 2.0 and eu <= 2.0, (what, du, eu)
    assert np.all(derr <= sbar) and np.all(eerr <= sbar), (what, derr.max(), eerr.max())
    # every element is written: zeros beyond T_b and L and for the infeasible, -1 in expected_frame there
    dead = np.arange(U)[None, :] >= Lb[:, None]
    assert not rows[~live].any() and not post[~live].any(), what
    assert not post[np.broadcast_to(dead[:, None, :], post.shape)].any() and not dur[dead].any() and np.all(exf[dead] == -1.0), what
    assert np.all(dur[~dead] >= 1.0 - 1e-4 * np.broadcast_to(np.maximum(Tb, 1)[:, None], dur.shape)[~dead]), "every position holds a frame"
    if wild_bits is not None:
        assert OW.same_bits(out[0], wild_bits), (what, "the loss is the wildcard loss's, bit for bit")
    return perr, berr, rerr, du, eu, derr.max(initial=0.0), eerr.max(initial=0.0)


# ---- the grid ----

@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_grid_logits(kind, shape):
    B, T, V, U = shape
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=U)
    assert (labels == W).any()
    ref = oracle(kind, 0, x, labels, ll, tl, key=("grid", kind, shape))
    assert np.isfinite(ref[0]).all(), "ragged and feasible"
    out = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} {shape} logits", out, ref, labels, ll, tl, wild_bits=wild_loss(kind, 0, x, labels, ll, tl))
    if kind == "simplified":  # an ordinary label is entered exactly once
        for b in range(B):
            d = out[3][b, :ll[b]].cpu().numpy()[labels[b, :ll[b]] != W]
            assert np.abs(d - 1.0).max(initial=0.0) <= 1e-4 * tl[b]


@pytest.mark.parametrize("kind", KINDS)
def test_log_probabilities(kind):
    x, labels, ll, tl = make_inputs(kind, *SMALL, seed=101)
    lp = logprobs32(x) - np.float32(0.25)  # not normalised: e_w carries the rows' log-sum-exp
    out = run(kind, 1, lp, labels, ll, tl)
    compare(f"{kind} log-probabilities", out, oracle(kind, 1, lp, labels, ll, tl), labels, ll, tl,
            wild_bits=wild_loss(kind, 1, lp, labels, ll, tl))


@pytest.mark.parametrize("kind", KINDS)
def test_wildcard_weight(kind):
    x, labels, ll, tl = make_inputs(kind, *SMALL, seed=102)
    ref, ref0 = oracle(kind, 0, x, labels, ll, tl, weight=-0.5), oracle(kind, 0, x, labels, ll, tl)
    assert np.abs(ref[1] - ref0[1]).max() > 1e-2, "the penalty is felt"
    out = run(kind, 0, x, labels, ll, tl, weight=-0.5)
    compare(f"{kind} w=-0.5", out, ref, labels, ll, tl, wild_bits=wild_loss(kind, 0, x, labels, ll, tl, weight=-0.5))


@pytest.mark.parametrize("kind", KINDS)
def test_last_token_as_blank(kind):
    B, T, V, U = SMALL
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=103, blank=V - 1)
    out = run(kind, 0, x, labels, ll, tl, blank=V - 1)
    compare(f"{kind} blank=V-1", out, oracle(kind, 0, x, labels, ll, tl, blank=V - 1), labels, ll, tl,
            wild_bits=wild_loss(kind, 0, x, labels, ll, tl, blank=V - 1))


@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits(kind):
    x, labels, ll, tl = make_inputs(kind, *SMALL, seed=104, scale=4.0)
    out = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} N(0, 4^2) logits", out, oracle(kind, 0, x, labels, ll, tl), labels, ll, tl,
            wild_bits=wild_loss(kind, 0, x, labels, ll, tl))


@pytest.mark.parametrize("kind", KINDS)
def test_a_vocabulary_of_more_than_one_producer_pass(kind):
    B, T, V, U = 2, 20, 1500, 6
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=105)
    labels[0, 1], labels[0, 3], labels[1, 1] = 1499, 1499, 1024
    ref = oracle(kind, 0, x, labels, ll, tl)
    assert np.isfinite(ref[0]).all()
    compare(f"{kind} V=1500", run(kind, 0, x, labels, ll, tl), ref, labels, ll, tl, wild_bits=wild_loss(kind, 0, x, labels, ll, tl))


# ---- formats ----

def same_outputs(a, b):
    return all(OW.same_bits(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    """16-bit logits convert exactly to the float32 the sweeps work in, and both access paths read the same elements in the same
    order: every format gives the bits of the contiguous float32 call on the same values."""
    B, T, V, U = 3, 90, 260, 20
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=106)
    xt = dev(x)
    out_c = run(kind, 0, xt, labels, ll, tl)
    compare(f"{kind} float32", out_c, oracle(kind, 0, x, labels, ll, tl), labels, ll, tl)
    for dt in (torch.bfloat16, torch.float16):
        xh = xt.to(dt)
        out32 = run(kind, 0, xh.float(), labels, ll, tl)
        assert same_outputs(run(kind, 0, xh, labels, ll, tl), out32), dt
        compare(f"{kind} {dt}", out32, oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl), labels, ll, tl)
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)  # time-major, read in place
    assert xtm.stride() == (V, B * V, 1)
    assert same_outputs(run(kind, 0, xtm, labels, ll, tl), out_c)
    for pad in (3, 4):  # row strides beyond V: element-wise and vector accesses
        _, xv, _ = OW.strided_storage(xt, (V + pad) * T + 8, V + pad, pattern=0x7F)
        assert same_outputs(run(kind, 0, xv, labels, ll, tl), out_c), pad
        _, xb, _ = OW.strided_storage(xt.to(torch.bfloat16), (V + pad) * T + 8, V + pad, pattern=0x7F)
        assert same_outputs(run(kind, 0, xb, labels, ll, tl), run(kind, 0, xt.to(torch.bfloat16), labels, ll, tl)), pad


# ---- against the rest of the library ----

@pytest.mark.parametrize("kind", KINDS)
def test_without_a_wildcard_the_scatter_by_token_is_softmax_minus_the_gradient_of_the_plain_loss(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = SMALL
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=107, wild=False)
    assert not (labels == W).any()
    xt = dev(x).requires_grad_(True)
    fn = ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss
    plain = fn(dev(labels), xt, dev(ll), dev(tl), 0)
    (gplain,) = torch.autograd.grad(plain.sum(), xt)
    loss, post, blk, dur, exf = run(kind, 0, x, labels, ll, tl)
    idx = dev(np.where(np.arange(U)[None, :] < ll[:, None], labels, 0)).long()[:, None, :].expand(B, T, U)
    gamma = torch.zeros((B, T, V), device=DEV).scatter_add_(2, idx, post)  # (positions from L on hold zeros)
    gamma[:, :, 0] += blk
    live = (torch.arange(T, device=DEV)[None, :] < dev(tl)[:, None]).float()[:, :, None]
    want = (torch.softmax(xt.detach(), dim=2) - gplain) * live
    err = float((gamma - want).abs().max())
    print(f"LABEL-POSTERIOR {kind} no wildcard: worst |scatter - (softmax - grad of the plain loss)| {err:.3e}, "
          f"worst |loss - plain| {float((loss - plain.detach()).abs().max()):.3e}")
    assert err <= 2e-4  # two results of 1e-4 each
    assert same_outputs(run(kind, 0, x, labels, ll, tl, weight=-2.5), (loss, post, blk, dur, exf)), "nothing reads the weight"


@pytest.mark.parametrize("kind", KINDS)
def test_the_wildcard_share_of_every_frame_is_the_loss_oracles_gamma(kind):
    """Gamma_t of ctc_amd_wildcard_loss_grad = the sum of label_posterior over the wildcard positions, against the float64 Gamma of
    tests/tools/wildcard_loss_oracle.py (another state layout, another file): itself a posterior-valued element, bar 1e-4."""
    B, T, V, U = SMALL
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=108)
    post = run(kind, 0, x, labels, ll, tl)[1].cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(B):
        L, Tb = int(ll[b]), int(tl[b])
        _, _, Gamma = WL.posteriors_one(kind, labels[b, :L], x[b, :Tb], 0, 0, 0.0)
        got = post[b, :Tb, :L][:, labels[b, :L] == W].sum(axis=1)
        assert Gamma.max() > 0.1
        worst = max(worst, float(np.abs(got - Gamma).max()))
    print(f"LABEL-POSTERIOR {kind}: worst |sum over wildcard positions - Gamma_t of the loss oracle| {worst:.3e}")
    assert worst <= 1e-4


# ---- edges ----

@pytest.mark.parametrize("kind", KINDS)
def test_edges(kind):
    """Every degenerate utterance gives its documented outputs, and the other utterances keep the bits of a run without it."""
    B, T, V, U = 3, 24, 6, 5
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=109)
    out_c = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} edges: clean", out_c, oracle(kind, 0, x, labels, ll, tl), labels, ll, tl)

    def variant(name, want, **change):
        xx, lab, l2, t2 = x.copy(), labels.copy(), ll.copy(), tl.copy()
        for k, v in change.items():
            {"x": xx, "labels": lab, "ll": l2, "tl": t2}[k][v[0]] = v[1]
        out = run(kind, 0, xx, lab, l2, t2)
        compare(f"{kind} edge {name}", out, oracle(kind, 0, xx, lab, l2, t2), lab, l2, t2, wild_bits=wild_loss(kind, 0, xx, lab, l2, t2))
        if want is not None:
            assert float(out[0][1]) == want, (name, float(out[0][1]))
        if want == np.inf:
            assert not out[1][1].any() and not out[2][1].any() and not out[3][1].any() and bool((out[4][1] == -1).all()), name
        for b in (0, 2):
            assert all(OW.same_bits(o[b], c[b]) for o, c in zip(out, out_c)), (name, b)
        return out

    variant("T_b = 0, a transcript", np.inf, tl=(1, 0))
    out = variant("T_b = 0, no transcript", 0.0, tl=(1, 0), ll=(1, 0))
    assert not out[1][1].any() and not out[2][1].any() and bool((out[4][1] == -1).all())
    out = variant("L = 0", None, ll=(1, 0))
    assert bool((out[2][1, :tl[1]] == 1).all()) and not out[2][1, tl[1]:].any(), "no label: every frame is blank, exactly"
    variant("negative label_length", None, ll=(1, -3))
    variant("too few frames", np.inf, tl=(1, int(ll[1]) - 1))
    variant("a label equal to the blank", np.inf, labels=((1, 1), 0))
    variant("a label >= V", np.inf, labels=((1, 0), V))
    variant("a label of -3", np.inf, labels=((1, 1), -3))
    variant("label_length > U", np.inf, ll=(1, U + 1))
    variant("a row of -inf", np.inf, x=((1, 0), -np.inf))


@pytest.mark.parametrize("kind", KINDS)
def test_no_frames_at_all_and_no_label_positions_at_all(kind):
    """T == 0: the alpha sweep and the statistics alone; U == 0: no label_posterior element and no statistics launch."""
    lab = np.asarray([[1, W, 2], [W, 1, 1]], np.int32)
    out = run(kind, 0, np.zeros((2, 0, 5), np.float32), lab, np.asarray([0, 2], np.int32), np.asarray([0, 0], np.int32))
    assert out[0].tolist() == [0.0, np.inf] and tuple(out[1].shape) == (2, 0, 3) and not out[3].any() and bool((out[4] == -1).all())
    x = np.random.default_rng(0).standard_normal((2, 6, 5)).astype(np.float32)
    out = run(kind, 0, x, lab, np.asarray([0, 2], np.int32), np.asarray([6, 4], np.int32), U=0)
    assert tuple(out[1].shape) == (2, 6, 0) and tuple(out[3].shape) == (2, 0)
    assert np.isfinite(float(out[0][0])) and float(out[0][1]) == np.inf
    assert bool((out[2][0] == 1).all()) and not out[2][1].any()


# ---- determinism ----

def raw_call(kind, wrt, x, labels, ll, tl, blank, weight, U, out, ws):
    """The C entry point with every buffer under the caller's control; out = (loss, label_posterior, blank_posterior, duration or
    None, expected_frame or None)."""
    from tf_seq2seq_losses_amd import _lib, ops
    B, T, V = x.shape
    rc = _lib.load().ctc_amd_label_posterior(
        kind_id(kind), wrt, x.data_ptr(), ops._DTYPES[x.dtype], x.stride(0), x.stride(1), labels.data_ptr(), labels.shape[1],
        ll.data_ptr(), tl.data_ptr(), blank, weight, B, T, V, U, *(None if o is None else o.data_ptr() for o in out),
        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_label_posterior")


def buffers(B, T, U, pattern, stats=True):
    shapes = ((B,), (B, T, U), (B, T)) + (((B, U), (B, U)) if stats else ())
    return tuple(OW.filled(s, torch.float32, pattern, DEV) for s in shapes) + (() if stats else (None, None))


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_whatever_the_buffers_held_without_statistics_and_under_graph_capture(kind):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = 3, 90, 7, 70
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=110)
    tl[1] = int(ll[1]) - 1  # one infeasible utterance: its zeros are written, not left over
    xt, lt, llt, tlt = dev(x), dev(labels), dev(ll), dev(tl)
    n = _lib.label_posterior_workspace_bytes(kind_id(kind), B, T, V, U)
    outs = []
    for pattern in (0x00, 0xFF, 0xFF):  # (the third: a second run)
        out = buffers(B, T, U, pattern)
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, out, OW.byte_fill(n, pattern, DEV))
        torch.cuda.synchronize()
        outs.append(out)
    assert same_outputs(outs[0], outs[1]) and same_outputs(outs[1], outs[2])
    assert float(outs[0][0][1]) == np.inf and not outs[0][1][1].any() and all(bool(torch.isfinite(o).all()) for o in outs[0][1:])
    compare(f"{kind} raw call", outs[0], oracle(kind, 0, x, labels, ll, tl, weight=-0.25), labels, ll, tl)
    # duration / expected_frame NULL: no statistics launch, the same bits elsewhere
    out = buffers(B, T, U, 0xFF, stats=False)
    raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, out, OW.byte_fill(n, 0xFF, DEV))
    torch.cuda.synchronize()
    assert same_outputs(out[:3], outs[0][:3])
    # capture on one stream, replay twice
    ws = OW.byte_fill(n, 0x5A, DEV)
    out = buffers(B, T, U, 0x5A)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, out, ws)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same_outputs(out, outs[0])


# ---- the public surface ----

@pytest.mark.parametrize("kind", KINDS)
def test_public_surface(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 3, 40, 6, 10
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=111)
    ref = oracle(kind, 0, x, labels, ll, tl, weight=-0.3)
    fn = ctc.classic_ctc_label_posterior if kind == "classic" else ctc.simplified_ctc_label_posterior
    xt = dev(x).requires_grad_(True)
    res = fn(dev(labels), xt, dev(ll), dev(tl), 0, wildcard_log_weight=-0.3)
    torch.cuda.synchronize()
    assert isinstance(res, ctc.CtcLabelPosterior) and res._fields == NAMES
    assert all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 and t.device == xt.device for t in res)
    assert tuple(res.label_posterior.shape) == (B, T, U) and tuple(res.expected_frame.shape) == (B, U)
    compare(f"{kind} public", res, ref, labels, ll, tl)
    # max_label_length bounds U; a longer transcript becomes infeasible
    cut = int(ll.min())
    res2 = fn(dev(labels), dev(x), dev(ll), dev(tl), 0, wildcard_log_weight=-0.3, max_label_length=cut)
    assert tuple(res2.label_posterior.shape) == (B, T, cut) and tuple(res2.duration.shape) == (B, cut)
    for b in range(B):
        if ll[b] > cut:
            assert float(res2.loss[b]) == np.inf and not res2.label_posterior[b].any()
        else:
            assert OW.same_bits(res2.loss[b], res.loss[b]) and OW.same_bits(res2.label_posterior[b], res.label_posterior[b, :, :cut])
    # log-probabilities, the lattice by class (classic by default)
    lp = logprobs32(x)
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    res = ctc.ctc_label_posterior_from_logproba(dev(labels), dev(lp), dev(ll), dev(tl), 0, cls if kind != "classic" else None)
    compare(f"{kind} public from_logproba", res, oracle(kind, 1, lp, labels, ll, tl), labels, ll, tl)
    # bfloat16 logits are read in place
    xh = dev(x).to(torch.bfloat16)
    res = fn(dev(labels), xh, dev(ll), dev(tl))
    compare(f"{kind} public bfloat16", res, oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl), labels, ll, tl)
    with pytest.raises(ValueError):
        fn(dev(labels), dev(x), dev(ll), dev(tl), 0, wildcard_log_weight=0.1)
    # check_labels keeps rejecting the wildcard
    assert (labels == W).any()
    with pytest.raises(ValueError):
        ctc.check_labels(dev(labels), dev(ll), V, 0)
