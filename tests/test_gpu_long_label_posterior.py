"""Long-form label posteriors on the GPU (ctc_amd_long_label_posterior, the posterior stage of csrc/ctc_loss_long.hip; DESIGN.md
section 5.22) against the float64 oracle tests/tools/label_posterior_oracle.py (vectorised over U, a loop over T; pinned without a GPU
by tests/test_label_posterior_oracle.py), against the existing calls, and against its own definition.

Bars, those of section 5.17 (tests/test_gpu_label_posterior.py):
  label_posterior, blank_posterior, peak_posterior   |gpu - oracle| <= 1e-4 per element; |row sum - 1| <= 1e-4
  duration, expected_frame                           |gpu - oracle| <= T_b * 1e-4 (the per-element bar summed over the frames)
  peak_frame                                         equal to the oracle's wherever the oracle's two largest posteriors of the
                                                     position differ by more than 2e-4 (twice the per-element bar: nearer than that
                                                     the order of the two is not determined); the positions left out are counted
                                                     and must stay below 5 %
Bits, never a tolerance: duration, expected_frame, peak_posterior and peak_frame against a host reduction of the returned dense
matrix (float64 np.add.accumulate over the reversed frames, one rounding); dense=False, frames_per_tile and the batch composition
against the plain call; loss against ctc_amd_long_wildcard_loss_grad; loss and label_posterior against ctc_amd_label_posterior for
U <= 1024 (blank_posterior is summed in another float32 order there: 1e-4; duration / expected_frame in another float64 order: 2 ulp).
Every figure is printed before it is asserted (pytest -s shows them).  V = 8, B = 2 unless a case says otherwise."""
import functools

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_label_posterior as LPT
from tests import test_gpu_long_loss as LL
from tests import test_gpu_wildcard_loss as WLT
from tests.tools import label_posterior_oracle as LP

pytestmark = pytest.mark.gpu

DEV = LL.DEV
W = LL.W
KINDS = LL.KINDS
dev, kind_id, make = LL.dev, LL.kind_id, LL.make
NAMES = ("loss", "label_posterior", "blank_posterior", "duration", "expected_frame", "peak_posterior", "peak_frame")


def run(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, U=None, tf=0, dense=True):
    """ops.long_label_posterior on device copies; x may be a tensor in any format.  The seven outputs as device tensors."""
    from tf_seq2seq_losses_amd import ops
    out = ops.long_label_posterior(kind_id(kind), wrt, dev(labels), dev(x), dev(ll), dev(tl), blank, labels.shape[1] if U is None else U,
                                   weight, tf, dense)
    torch.cuda.synchronize()
    B, T = len(ll), x.shape[1]
    Uo = out[3].shape[1]
    assert all(o.dtype == torch.float32 and o.is_contiguous() for o in out[:6] if o is not None) and out[6].dtype == torch.int32
    assert tuple(out[0].shape) == (B,) and tuple(out[2].shape) == (B, T) and all(tuple(o.shape) == (B, Uo) for o in out[3:])
    assert (out[1] is None) == (not dense) and (out[1] is None or tuple(out[1].shape) == (B, T, Uo))
    return out


def same(a, b, what=""):
    """Every output the same bits (a dense matrix that one side left out is not compared)."""
    for name, p, q in zip(NAMES, a, b):
        if p is None or q is None:
            continue
        assert OW.same_bits(p.contiguous(), q.contiguous()), (what, name, OW.count_diff(p.contiguous(), q.contiguous()))
    return True


def host_stats(post, ok_pos):
    """The per-position outputs as the header defines them, from the returned float32 matrix post[B, T, U]: float64 sums in
    descending frame order (np.add.accumulate over the reversed frames), one rounding; the peak and the lowest frame that attains
    it.  ok_pos[B, U]: the position belongs to a feasible utterance and lies below its label length."""
    B, T, U = post.shape
    p = post.astype(np.float64)[:, ::-1, :]
    t = np.arange(T, dtype=np.float64)[::-1][None, :, None]
    zero = np.zeros((B, U))
    d = np.add.accumulate(p, axis=1)[:, -1, :] if T else zero
    m = np.add.accumulate(t * p, axis=1)[:, -1, :] if T else zero
    with np.errstate(divide="ignore", invalid="ignore"):
        dur = np.where(ok_pos, d, 0.0).astype(np.float32)
        exf = np.where(ok_pos & (d > 0.0), m / d, -1.0).astype(np.float32)
    peak = np.where(ok_pos, post.max(axis=1, initial=0.0), 0.0).astype(np.float32)
    pfr = np.where(ok_pos, post.argmax(axis=1) if T else -1, -1).astype(np.int32)
    return dur, exf, peak, pfr


def check_definition(what, out, ll, tl):
    """duration, expected_frame, peak_posterior, peak_frame are a host reduction of the returned matrix, bit for bit."""
    loss, post = out[0].cpu().numpy(), out[1].cpu().numpy()
    B, T, U = post.shape
    ok = np.isfinite(loss)[:, None] & (np.arange(U)[None, :] < np.asarray(ll)[:, None])
    ok &= (np.asarray(tl).clip(0, T) > 0)[:, None]
    for name, got, want in zip(NAMES[3:], out[3:], host_stats(post, ok)):
        g = got.cpu().numpy()
        n = int((g.view(np.int32) != want.view(np.int32)).sum())
        print(f"LONG-LABEL-POSTERIOR {what}: {name} differs from the host reduction in {n} of {g.size} elements")
        assert n == 0, (what, name, n)


_ORACLE_INPUTS = {}


@functools.lru_cache(maxsize=None)
def _oracle_cached(kind, wrt, key, blank, weight):
    x, labels, ll, tl = _ORACLE_INPUTS[key]
    return LP.label_posterior(kind, wrt, labels, x, ll, tl, blank, weight)


def oracle(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, key=None):
    """The float64 reference, computed once per `key` and left unchanged."""
    _ORACLE_INPUTS.setdefault(key, (x, labels, ll, tl))
    return _oracle_cached(kind, wrt, key, blank, weight)


def compare(what, out, ref, ll, tl):
    """Prints every figure, then asserts the bars of the module docstring and the padding rules.  Returns the worst figures."""
    loss, post, blk, dur, exf, peak = (o.cpu().numpy().astype(np.float64) for o in out[:6])
    pfr = out[6].cpu().numpy()
    rloss, rpost, rblk, rdur, rexf = ref
    B, T, U = post.shape
    fin = np.isfinite(rloss)
    assert np.array_equal(np.isfinite(loss), fin) and np.all(loss[~fin] == np.inf), (what, loss, rloss)
    assert not any(np.isnan(a).any() for a in (post, blk, dur, exf, peak)), what
    Tb = np.where(fin, np.asarray(tl).clip(0, T), 0)
    Lb = np.where(fin, np.asarray(ll).clip(0, None), 0)
    live = np.arange(T)[None, :] < Tb[:, None]
    dead = np.arange(U)[None, :] >= Lb[:, None]
    perr, berr = np.abs(post - rpost).max(initial=0.0), np.abs(blk - rblk).max(initial=0.0)
    lerr = np.abs(loss[fin] - rloss[fin]).max(initial=0.0)
    rerr = np.abs((post.sum(axis=2) + blk)[live] - 1.0).max(initial=0.0)
    sbar = np.maximum(Tb, 1)[:, None] * 1e-4
    derr, eerr = np.abs(dur - rdur), np.abs(exf - rexf)
    kerr = np.abs(peak - rpost.max(axis=1, initial=0.0)).max(initial=0.0)
    # peak_frame where the oracle's two largest values of the position are more than 2e-4 apart
    top2 = np.partition(rpost, T - 2, axis=1)[:, -2:, :] if T >= 2 else np.zeros((B, 2, U))
    clear = ~dead & ((top2[:, 1, :] - top2[:, 0, :]) > 2e-4)
    left_out = int((~dead & ~clear).sum())
    share = left_out / max(int((~dead).sum()), 1)
    wrong = int((pfr[clear] != rpost.argmax(axis=1)[clear]).sum())
    print(f"LONG-LABEL-POSTERIOR {what}: worst |gpu - oracle| loss {lerr:.3e} label {perr:.3e} blank {berr:.3e} peak {kerr:.3e}, "
          f"worst |row sum - 1| {rerr:.3e}, duration {derr.max(initial=0.0):.3e} expected_frame {eerr.max(initial=0.0):.3e} "
          f"(bar {sbar.min():.1e}); peak_frame compared at {int(clear.sum())} positions, {left_out} left out ({100 * share:.2f} %), {wrong} differ")
    assert perr <= 1e-4 and berr <= 1e-4 and kerr <= 1e-4, (what, perr, berr, kerr)
    assert rerr <= 1e-4, (what, rerr)
    assert np.all(derr <= sbar) and np.all(eerr <= sbar), (what, derr.max(), eerr.max())
    assert share < 0.05, (what, "too many positions without a clear peak: choose other seeds", share)
    assert wrong == 0, (what, wrong)
    # every element is written: zeros beyond T_b and L and for the infeasible, -1 in expected_frame and peak_frame there
    assert not post[~live].any() and not blk[~live].any(), what
    assert not post[np.broadcast_to(dead[:, None, :], post.shape)].any(), what
    assert not dur[dead].any() and not peak[dead].any() and np.all(exf[dead] == -1.0) and np.all(pfr[dead] == -1), what
    return perr, berr, rerr, derr.max(initial=0.0), eerr.max(initial=0.0), kerr, share


def long_loss(kind, wrt, x, labels, ll, tl, blank=0, weight=0.0, U=None, tf=0):
    return LL.run(kind, wrt, x, labels, ll, tl, blank=blank, weight=weight, want_grad=False, U=labels.shape[1] if U is None else U, tf=tf)[0]


# ---- 1: the second and the third label block against the oracle; the definition; dense=False; the tiling; the batch ----

SHAPES = {"T1300_U1030": dict(T=1300, U=1030, ll=(1030, 800), tl=(1300, 1150), seed=31),
          "T2600_U2100": dict(T=2600, U=2100, ll=(2100, 1500), tl=(2600, 2300), seed=32)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_definition_tiling_and_batch(kind, shape):
    s = SHAPES[shape]
    x, labels, ll, tl = make(2, s["T"], 8, s["U"], s["ll"], s["tl"], seed=s["seed"], random_wild=0.05)
    assert (labels == W).any()
    ref = oracle(kind, 0, x, labels, ll, tl, key=(shape, kind))
    assert np.isfinite(ref[0]).all()
    out = run(kind, 0, x, labels, ll, tl)
    compare(f"{kind} {shape}", out, ref, ll, tl)
    check_definition(f"{kind} {shape}", out, ll, tl)
    assert OW.same_bits(out[0], long_loss(kind, 0, x, labels, ll, tl)), "the loss is ctc_amd_long_wildcard_loss_grad's"
    # dense=False: the same bits in every other output
    same(run(kind, 0, x, labels, ll, tl, dense=False), out, "dense=False")
    # frames_per_tile changes no bit (1300: J = 1 or 2; 4: the ring wraps hundreds of times), nor does the batch
    for tf in (128, 64, 4, 1300):
        same(run(kind, 0, x, labels, ll, tl, tf=tf), out, f"tf={tf}")
        same(run(kind, 0, x, labels, ll, tl, tf=tf, dense=False), out, f"tf={tf} dense=False")
    alone = run(kind, 0, x[1:], labels[1:], ll[1:], tl[1:])
    same(alone, tuple(o[1:] for o in out), "utterance 1 alone")


# ---- 2: one label block: the bits of ctc_amd_label_posterior ----

@pytest.mark.parametrize("shape", [(1300, 1024), (200, 129)], ids=["T1300_U1024", "T200_U129"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_block_against_the_existing_call(kind, shape):
    T, U = shape
    x, labels, ll, tl = make(2, T, 8, U, (U, U - U // 4), (T, T - 40), seed=33, random_wild=0.1)
    out = run(kind, 0, x, labels, ll, tl)
    old = LPT.run(kind, 0, x, labels, ll, tl)
    assert np.isfinite(out[0].cpu().numpy()).all()
    assert OW.same_bits(out[0], old[0]) and OW.same_bits(out[1], old[1]), (OW.count_diff(out[0], old[0]), OW.count_diff(out[1], old[1]))
    berr = float((out[2] - old[2]).abs().max())
    du = LPT.ulps(out[3].cpu().numpy().astype(np.float64), old[3].cpu().numpy().astype(np.float64)).max()
    eu = LPT.ulps(out[4].cpu().numpy().astype(np.float64), old[4].cpu().numpy().astype(np.float64)).max()
    print(f"LONG-LABEL-POSTERIOR {kind} {shape} against ctc_amd_label_posterior: loss and label_posterior the same bits, "
          f"blank_posterior within {berr:.3e}, duration {du:.2f} ulp, expected_frame {eu:.2f} ulp")
    assert berr <= 1e-4 and du <= 2.0 and eu <= 2.0
    check_definition(f"{kind} {shape}", out, ll, tl)
    same(run(kind, 0, x, labels, ll, tl, tf=64, dense=False), out, "tf=64 dense=False")


# ---- 3: against the gradient of the long-form loss ----

@pytest.mark.parametrize("kind", KINDS)
def test_posteriors_scattered_by_token_are_softmax_minus_gradient(kind):
    """Without wildcards: sum over the positions of a token of label_posterior, and blank_posterior in the blank's column, equal
    softmax - d loss / d logits of *_long_loss(checkpoint=True).  Bar 2e-4, section 5.17's for this check."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 2, 1300, 8, 1030
    x, labels, ll, tl = make(B, T, V, U, (1030, 800), (1300, 1150), seed=34)
    assert not (labels == W).any()
    fn = ctc.classic_ctc_long_loss if kind == "classic" else ctc.simplified_ctc_long_loss
    xt = dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(fn(dev(labels), xt, dev(ll), dev(tl), 0, checkpoint=True).sum(), xt)
    out = run(kind, 0, x, labels, ll, tl)
    occ = torch.zeros((B, T, V), device=DEV)
    idx = dev(labels).long()[:, None, :].expand(B, T, U)
    occ.scatter_add_(2, idx, out[1] * (torch.arange(U, device=DEV)[None, None, :] < dev(ll).long()[:, None, None]))
    occ[:, :, 0] += out[2]
    live = (torch.arange(T, device=DEV)[None, :] < dev(tl).long()[:, None])[:, :, None]
    want = (torch.softmax(dev(x), dim=2) - g) * live
    err = float((occ - want).abs().max())
    print(f"LONG-LABEL-POSTERIOR {kind}: worst |scattered posteriors - (softmax - gradient)| {err:.3e}")
    assert err <= 2e-4


# ---- 4: edges ----

@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch(kind):
    """Beside a two-block utterance: more labels than frames, no labels, no frames, neither, a short one, more labels than U."""
    U, T = 1100, 1300
    ll = (1100, 900, 0, 5, 0, 40, 1101)
    tl = (1300, 800, 300, 0, 0, 1300, 1300)
    x, labels, ll, tl = make(7, T, 8, U, ll, tl, seed=35, random_wild=0.03)
    out = run(kind, 0, x, labels, ll, tl, tf=64)
    loss = out[0].cpu().numpy()
    assert np.array_equal(np.isfinite(loss), [True, False, True, False, True, True, False]), loss
    assert loss[4] == 0.0
    for b in (1, 3, 6):  # +inf, zeros, -1
        assert loss[b] == np.inf and not out[1][b].any() and not out[2][b].any() and not out[3][b].any() and not out[5][b].any()
        assert bool((out[4][b] == -1).all()) and bool((out[6][b] == -1).all())
    assert bool((out[2][2, :300] == 1).all()) and not out[2][2, 300:].any() and not out[1][2].any(), "no labels: the all-blank path"
    assert bool((out[4][2] == -1).all()) and bool((out[6][4] == -1).all()) and not out[3][4].any()
    assert not out[1][0, :, 1100:].any() and not out[1][5, :, 40:].any() and bool((out[6][5, 40:] == -1).all())
    ref = oracle(kind, 0, x[[0, 5]], labels[[0, 5]], ll[[0, 5]], tl[[0, 5]], key=("ragged", kind))
    compare(f"{kind} ragged", tuple(o[[0, 5]] for o in out), ref, ll[[0, 5]], tl[[0, 5]])
    check_definition(f"{kind} ragged", out, ll, tl)
    same(run(kind, 0, x, labels, ll, tl, tf=128, dense=False), out, "tf=128 dense=False")
    same(run(kind, 0, x[:1], labels[:1], ll[:1], tl[:1]), tuple(o[:1] for o in out), "utterance 0 alone")


@pytest.mark.parametrize("kind", KINDS)
def test_block_boundary_blank_and_log_probabilities(kind):
    """A wildcard and a repeated label on either side of position 1024; the last token as blank; log-probabilities."""
    x, labels, ll, tl = make(2, 1300, 8, 1030, (1030, 1028), (1300, 1290), seed=36, blank=7, wild=((1023,), (1024, 1027)))
    labels[0, 1025] = labels[0, 1026]
    labels[1, 1023] = labels[1, 1022]
    assert not (labels == 7).any()
    for wrt, xin, weight in ((0, x, -0.5), (1, WLT.logprobs32(x) - np.float32(0.25), -0.25)):
        ref = oracle(kind, wrt, xin, labels, ll, tl, blank=7, weight=weight, key=("boundary", kind, wrt))
        out = run(kind, wrt, xin, labels, ll, tl, blank=7, weight=weight)
        compare(f"{kind} boundary wrt={wrt}", out, ref, ll, tl)
        check_definition(f"{kind} boundary wrt={wrt}", out, ll, tl)
        assert OW.same_bits(out[0], long_loss(kind, wrt, xin, labels, ll, tl, blank=7, weight=weight))


@pytest.mark.parametrize("kind", KINDS)
def test_formats_give_the_bits_of_the_float32_call(kind):
    x, labels, ll, tl = make(2, 1300, 8, 1026, (1026, 700), (1300, 1000), seed=37, wild=((5, 1023), (0,)))
    B, T, V = x.shape
    assert np.isfinite(run(kind, 0, x, labels, ll, tl)[0].cpu().numpy()).all()
    for dt in (torch.bfloat16, torch.float16):
        x16 = dev(x).to(dt)
        same(run(kind, 0, x16, labels, ll, tl), run(kind, 0, x16.float(), labels, ll, tl), str(dt))
    xt = dev(x)
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)
    assert xtm.stride() == (V, B * V, 1)
    same(run(kind, 0, xtm, labels, ll, tl), run(kind, 0, xt, labels, ll, tl), "time-major")


def raw_call(kind, wrt, x, labels, ll, tl, blank, weight, U, tf, loss, post, blk, dur, exf, peak, pfr, ws_ptr, ws_n):
    """The C entry point with every buffer under the caller's control (None: NULL)."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V = x.shape
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.ctc_amd_long_label_posterior(
        kind_id(kind), wrt, x.data_ptr(), ops._DTYPES[x.dtype], x.stride(0), x.stride(1), labels.data_ptr(), labels.shape[1],
        ll.data_ptr(), tl.data_ptr(), blank, weight, B, T, V, U, tf, p(loss), p(post), p(blk), p(dur), p(exf), p(peak), p(pfr),
        ws_ptr, ws_n, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ctc_amd_long_label_posterior")


def ws_bytes(kind, x, U, tf=0):
    from tf_seq2seq_losses_amd import _lib
    B, T, V = x.shape
    return _lib.long_label_posterior_workspace_bytes(kind_id(kind), B, T, V, U, tf)


@pytest.mark.parametrize("kind", KINDS)
def test_element_wise_stores_exact_workspace_and_guards(kind):
    """U = 1030 is a multiple of 4 and U = 1027 is not; a dense pointer 4 bytes off a 16-byte boundary takes the element-wise path
    too: the bits of the aligned call.  An exact-size workspace and outputs prefilled 0x00 / 0xFF between guard bands: every element
    is written, the guards are not; a second run gives the same bits.  Utterance 1 is infeasible."""
    guard = 64
    for U, off in ((1027, 0), (1030, 1), (1030, 0)):
        x, labels, ll, tl = make(3, 1300, 8, U, (U, 1030, 700), (1300, 1029, 900), seed=38, wild=((0, 1024), (), (699,)))
        B, T, V = x.shape
        xt, lt, llt, tlt = dev(x), dev(labels), dev(ll), dev(tl)
        want = run(kind, 0, x, labels, ll, tl, weight=-0.25, tf=64)
        n = ws_bytes(kind, xt, U, 64)
        outs = []
        for pattern in (0x00, 0xFF, 0xFF):
            ws = OW.workspace(n + 512, pattern)
            sizes = (B, B * T * U, B * T, B * U, B * U, B * U, B * U)
            bufs = [OW.filled((s + 2 * guard + 4,), torch.int32 if i == 6 else torch.float32, pattern, DEV) for i, s in enumerate(sizes)]
            views = [b[guard + (off if i == 1 else 0):][:s] for i, (b, s) in enumerate(zip(bufs, sizes))]
            assert views[1].data_ptr() % 16 == 4 * off
            raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, 64, *views, ws.data_ptr() + 256, n)
            torch.cuda.synchronize()
            for i, (b, s) in enumerate(zip(bufs, sizes)):
                keep = OW.keeps_prefill(b, pattern)
                lo = guard + (off if i == 1 else 0)
                assert bool(keep[:lo].all()) and bool(keep[lo + s:].all()), (NAMES[i], pattern)
            keep = OW.keeps_prefill(ws, pattern)
            assert bool(keep[:256].all()) and bool(keep[-256:].all()), pattern
            outs.append((views[0], views[1].view(B, T, U), views[2].view(B, T), *(v.view(B, U) for v in views[3:])))
        for o in outs:
            same(o, want, f"U={U} offset {off}")
        assert float(want[0][1]) == np.inf and not want[1][1].any() and bool((want[6][1] == -1).all())
        # without the dense matrix, and without either pair: the others keep their bits
        ws = OW.workspace(n, 0xFF)
        o = [OW.filled(v.shape, v.dtype, 0xFF, DEV) for v in outs[0]]
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, 64, o[0], None, o[2], None, None, o[5], o[6], ws.data_ptr(), n)
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, 64, o[0], None, o[2], o[3], o[4], None, None, ws.data_ptr(), n)
        torch.cuda.synchronize()
        same((o[0], None, *o[2:]), want, "NULL outputs")


def test_empty_shapes():
    """B = 0, T = 0, U = 0."""
    from tf_seq2seq_losses_amd import ops
    for kind in KINDS:
        x, labels, ll, tl = make(2, 0, 8, 5, (0, 3), (0, 0), seed=39)
        out = run(kind, 0, x, labels, ll, tl)
        assert out[0].tolist() == [0.0, float("inf")] and tuple(out[1].shape) == (2, 0, 5)
        assert not out[3].any() and not out[5].any() and bool((out[4] == -1).all()) and bool((out[6] == -1).all())
        x, labels, ll, tl = make(2, 40, 8, 5, (0, 0), (40, 17), seed=39)
        out = run(kind, 0, x, labels[:, :0], ll, tl)
        assert tuple(out[1].shape) == (2, 40, 0) and tuple(out[3].shape) == (2, 0) == tuple(out[6].shape)
        assert bool((out[2][0] == 1).all()) and bool((out[2][1, :17] == 1).all()) and not out[2][1, 17:].any()
        assert OW.same_bits(out[0], long_loss(kind, 0, x, labels[:, :0], ll, tl))
        out = ops.long_label_posterior(kind_id(kind), 0, dev(labels[:0]), dev(x[:0]), dev(ll[:0]), dev(tl[:0]), 0)
        assert tuple(out[0].shape) == (0,) and tuple(out[1].shape) == (0, 40, 5) and tuple(out[6].shape) == (0, 5)


# ---- 5: capture ----

@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_and_replay_with_fresh_logits(kind):
    x, labels, ll, tl = make(2, 1300, 8, 1030, (1030, 800), (1300, 1200), seed=40, wild=((0, 1024), (799,)))
    B, T, V = x.shape
    U, tf = 1030, 64
    rng = np.random.default_rng(41)
    fresh = [rng.standard_normal(x.shape).astype(np.float32) for _ in range(2)]
    xt, lt, llt, tlt = dev(x).clone(), dev(labels), dev(ll), dev(tl)
    n = ws_bytes(kind, xt, U, tf)
    ws = OW.byte_fill(n, 0x5A, DEV)
    shapes = ((B,), (B, T, U), (B, T), (B, U), (B, U), (B, U), (B, U))
    outs = [OW.filled(s, torch.int32 if i == 6 else torch.float32, 0x5A, DEV) for i, s in enumerate(shapes)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):  # one stream: no parallel branches
        raw_call(kind, 0, xt, lt, llt, tlt, 0, -0.25, U, tf, *outs, ws.data_ptr(), n)
    for xi in fresh:
        xt.copy_(dev(xi))
        for o in outs:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        same(tuple(outs), run(kind, 0, xi, labels, ll, tl, weight=-0.25, tf=tf), "replay")


# ---- 6: the public surface ----

@pytest.mark.parametrize("kind", KINDS)
def test_public_surface(kind):
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = make(2, 1300, 8, 1026, (1026, 700), (1300, 1000), seed=37, wild=((5, 1023), (0,)))
    fn = ctc.classic_ctc_long_label_posterior if kind == "classic" else ctc.simplified_ctc_long_label_posterior
    lt, llt, tlt = dev(labels), dev(ll), dev(tl)
    want = run(kind, 0, x, labels, ll, tl, weight=-0.5, tf=64)
    res = fn(lt, dev(x).requires_grad_(True), llt, tlt, 0, wildcard_log_weight=-0.5, frames_per_tile=64, max_label_length=1026)
    assert isinstance(res, ctc.CtcLongLabelPosterior) and res._fields == NAMES
    assert all(not t.requires_grad and t.grad_fn is None and t.device == DEV for t in res)
    assert res.peak_frame.dtype == torch.int32 and all(t.dtype == torch.float32 for t in res[:6])
    same(tuple(res), want, "public")
    lean = fn(lt, dev(x), llt, tlt, 0, wildcard_log_weight=-0.5, dense=False)
    assert lean.label_posterior is None
    same(tuple(lean), want, "dense=False")
    # log-probabilities, the lattice by class
    cls = None if kind == "classic" else ctc.SimplifiedCtcLossData
    lp = WLT.logprobs32(x)
    res = ctc.ctc_long_label_posterior_from_logproba(lt, dev(lp), llt, tlt, 0, cls, wildcard_log_weight=-0.5)
    same(tuple(res), run(kind, 1, lp, labels, ll, tl, weight=-0.5), "log-probabilities")
    with pytest.raises(TypeError):
        fn(lt, dev(x), llt, tlt, 0, 0.0)
    with pytest.raises(ValueError):
        fn(lt, dev(x), llt, tlt, 0, wildcard_log_weight=0.5)
