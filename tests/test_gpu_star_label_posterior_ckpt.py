"""Star label posteriors from block checkpoints on the GPU (ctc_amd_star_label_posterior_ckpt) against the float64 oracle
tests/tools/star_exclusion_oracle.label_posterior.  Bars: those of tests/test_gpu_star_exclusion.py::check for the posteriors (element
and row sum 1e-4, loss 1e-4 + 1e-6 |loss| and the bits of the forward-only per-frame call) and those of
tests/test_gpu_label_posterior.py::compare for duration / expected_frame (2 ulp from the host reduction of the returned matrix,
T_b * 1e-4 from the oracle).  F = 32 / 16 / 8 frames per block at U <= 64 / 128 / 256."""
import ctypes
import pathlib

import numpy as np
import pytest
import torch

import tf_seq2seq_losses_amd as ctc
from tf_seq2seq_losses_amd import _lib, ops
from tests import test_gpu_label_posterior as P
from tests.test_gpu_star_loss_ckpt import DEV, EDGES, FLAGS, LATTICES, PATTERNS, Q, W, WEIGHT, cyclic, dev, logits, same, stars
from tests.tools import star_exclusion_oracle as SO

pytestmark = pytest.mark.gpu
NAME = "ctc_amd_star_label_posterior_ckpt"


def check(kind, wrt, x, labels, ll, tl, flags, blank=0, U=None, xdev=None):
    """Against the oracle on the values in x (xdev: as the device holds them).  Returns the five outputs and who is feasible."""
    kw = dict(optional_wildcards=flags[0], exclude_next_label=flags[1])
    a = (ops.KINDS[kind], wrt, dev(labels), dev(x) if xdev is None else xdev, dev(ll), dev(tl), blank)
    out = ops.star_label_posterior(*a, U, WEIGHT, **kw)
    loss0 = ops.wildcard_loss_grad(*a, None, U, None, WEIGHT, False, **kw)[0]
    torch.cuda.synchronize()
    ref = SO.label_posterior(kind, wrt, labels, x, ll, tl, blank, WEIGHT, U, optional=flags[0], exclude=flags[1])
    loss, post, blk, dur, exf = (o.cpu().numpy().astype(np.float64) for o in out)
    fin = np.isfinite(ref[0])
    assert same([loss0], [out[0]]) and np.array_equal(np.isfinite(loss), fin) and np.all(loss[~fin] == np.inf)
    assert np.all(np.abs(loss[fin] - ref[0][fin]) <= 1e-4 + 1e-6 * np.abs(ref[0][fin]))
    assert np.abs(post - ref[1]).max(initial=0.0) <= 1e-4 and np.abs(blk - ref[2]).max(initial=0.0) <= 1e-4
    Tb = np.where(fin, np.asarray(tl).clip(0, x.shape[1]), 0)
    live = np.arange(x.shape[1])[None, :] < Tb[:, None]
    rows = post.sum(axis=2) + blk
    assert np.abs(rows[live] - 1.0).max(initial=0.0) <= 1e-4 and not rows[~live].any() and not post[~live].any()
    hd, he = P.host_reduction(out[1].cpu().numpy(), Tb)
    assert P.ulps(dur, hd).max(initial=0.0) <= 2.0 and P.ulps(exf, he).max(initial=0.0) <= 2.0
    bar = np.maximum(Tb, 1)[:, None] * 1e-4
    assert np.all(np.abs(dur - ref[3]) <= bar) and np.all(np.abs(exf - ref[4]) <= bar)
    return out, fin


@pytest.mark.parametrize("U,F,T,i", EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_block_edges_and_pipeline_fill_and_drain(kind, wrt, flags, U, F, T, i):
    """1 to 4 blocks, T_b = (T, 0, max(T - 2, 1)), V = 6; the five star patterns (cut to the frames there are) in all three tiers."""
    rng = np.random.default_rng(100 * U + T)
    x = logits(rng, 3, T, 6, wrt)
    tl = np.asarray([T, 0, max(T - 2, 1)], np.int32)
    labels = rng.integers(1, 6, (3, max(U, 6))).astype(np.int32)
    ll = np.zeros(3, np.int32)
    for b in range(3):
        pat = PATTERNS[(i + 2 * b) % 5][:min(U, max(int(tl[b]), 1))]
        labels[b, :len(pat)] = pat
        ll[b] = len(pat)
    check(kind, wrt, x, stars(labels, flags[0]), ll, tl, flags, U=U)


@pytest.mark.parametrize("NL,U", [(1, 43), (2, 85), (4, 169)])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_lane_and_register_boundaries(kind, wrt, flags, NL, U):
    """An excluding star on a lane's last position, an optional star on a lane's last and first position; the second utterance ends
    on an optional star."""
    B, V, T = 2, 8, U + 5
    labels = cyclic(B, U, V, [5 * NL - 1, 13 * NL + NL // 2], [9 * NL - 1, 17 * NL, U - 2], flags[0])
    assert check(kind, wrt, logits(np.random.default_rng(U), B, T, V, wrt), labels, np.asarray([U, U - 1], np.int32),
                 np.asarray([T, T - 3], np.int32), flags)[1].all()


@pytest.mark.parametrize("U", [64, 65, 129, 256])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_full_tiers(kind, wrt, flags, U):
    """T a few frames above the fewest that fit; the second utterance a frame short: +inf, every posterior zero, expected_frame -1."""
    B, V = 3, 8
    labels = cyclic(B, U, V, slice(3, None, 8), slice(7, None, 16), flags[0])
    need = int((labels[0] != Q).sum())  # (every mandatory position takes a frame; no blank is forced between unequal labels)
    tl = np.asarray([need + 3, need - 1, need + 2], np.int32)
    out, fin = check(kind, wrt, logits(np.random.default_rng(U), B, need + 3, V, wrt), labels, np.full(B, U, np.int32), tl, flags)
    assert list(fin) == [True, False, True] and float(out[0][1]) == np.inf
    assert not out[1][1].any() and not out[2][1].any() and not out[3][1].any() and bool((out[4][1] == -1).all())


def raw(kind, wrt, x, labels, ll, tl, flags, U, pattern, stats=True):
    """The C entry point into outputs and a workspace prefilled with the byte `pattern`; duration = NULL without `stats`."""
    B, T, V = x.shape
    n = _lib.label_posterior_ckpt_workspace_bytes(ops.KINDS[kind], B, T, V, U)
    out = [torch.full(s, pattern, dtype=torch.uint8, device=DEV) for s in ((B * 4,), (B * T * U * 4,), (B * T * 4,), (B * U * 4,), (B * U * 4,))]
    ws = torch.full((n,), pattern, dtype=torch.uint8, device=DEV)
    ptr = [o.data_ptr() for o in out[:3]] + [o.data_ptr() if stats else None for o in out[3:]]
    rc = _lib.load().ctc_amd_star_label_posterior_ckpt(
        ops.KINDS[kind], wrt, x.data_ptr(), 0, T * V, V, labels.data_ptr(), labels.shape[1], ll.data_ptr(), tl.data_ptr(), 0, int(flags[0]),
        int(flags[1]), WEIGHT, B, T, V, U, *ptr, ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, NAME)
    torch.cuda.synchronize()
    return [o.view(torch.float32) for o in (out if stats else out[:3])]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_geometry_and_determinism(kind, wrt, flags):
    """U no multiple of 4 in a wider label tensor with hostile tails; buffers of 0x00 / 0xFF give the same bits; without statistics."""
    B, T, V, U = 3, 90, 7, 70
    labels = cyclic(B, U, V, slice(4, None, 9), slice(8, None, 9), flags[0])
    wide = np.concatenate([labels, np.asarray([[-7, 10 ** 9, V, Q, W]] * B, np.int32)], axis=1)
    x, ll, tl = logits(np.random.default_rng(9), B, T, V, wrt), np.asarray([U, 12, 50], np.int32), np.asarray([T, 30, 35], np.int32)
    a = (kind, wrt, dev(x), dev(wide), dev(ll), dev(tl), flags, U)
    o0, o1 = raw(*a, 0x00), raw(*a, 0xFF)
    want, fin = check(kind, wrt, x, labels, ll, tl, flags)
    assert list(fin) == [True, True, False]  # (the third needs more frames than it has: its zeros are written, not left over)
    assert same(o0, o1) and same([o.reshape(-1) for o in want], [o.reshape(-1) for o in o1]) and same(raw(*a, 0xFF, stats=False), o0[:3])


@pytest.mark.parametrize("V,blank,dt", [(5, 0, None), (5, 2, None), (5, 4, None), (1030, 0, None), (1030, 1029, None),
                                        (260, 0, torch.bfloat16), (260, 0, torch.float16)], ids=str)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_vocabulary_and_blank(kind, wrt, flags, V, blank, dt):
    """The blank first, in the middle and last; the excluded token and an ordinary label above column 1024; 16-bit logits."""
    hi = [k for k in range(V - 1, 0, -1) if k != blank][:3]
    lo = [k for k in range(1, V) if k != blank][:2]
    labels = stars([[W, hi[0], lo[0], Q, hi[1], hi[2]], [hi[1], Q, hi[0], W, hi[0], lo[1]]], flags[0])
    xdev = dev(logits(np.random.default_rng(V + blank), 2, 40, V, wrt, scale=3.0))
    xdev = xdev if dt is None else xdev.to(dt)
    assert check(kind, wrt, xdev.float().cpu().numpy(), labels, np.asarray([6, 6], np.int32), np.asarray([40, 31], np.int32), flags,
                 blank=blank, xdev=xdev)[1].all()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("kind,wrt", LATTICES)
def test_routing(kind, wrt, flags):
    """No -3 and no excluding star: label_posterior(checkpoint=True)'s bits.  U = 257: the per-frame call's.  The public functions."""
    k, kw = ops.KINDS[kind], dict(optional_wildcards=flags[0], exclude_next_label=flags[1])
    B, T, V, U = 3, 150, 8, 129
    labels = cyclic(B, U, V)
    labels[0, 100:] = W  # (followed by stars alone)
    a = (k, wrt, dev(labels), dev(logits(np.random.default_rng(3), B, T, V, wrt)), dev(np.asarray([U, 60, 40], np.int32)),
         dev(np.asarray([T, T - 9, 70], np.int32)), 0, None, WEIGHT)
    assert same(ops.star_label_posterior(*a, **kw), ops.label_posterior(*a, checkpoint=True))
    B, T, U = 2, 300, 257
    labels = cyclic(B, U, V, slice(3, None, 8), slice(7, None, 16), flags[0])
    a = (dev(labels), dev(logits(np.random.default_rng(4), B, T, V, wrt)), dev(np.asarray([U, 200], np.int32)), dev(np.asarray([T, T - 5], np.int32)), 0)
    got = ops.star_label_posterior(k, wrt, *a, None, WEIGHT, **kw)
    assert torch.isfinite(got[0]).all() and same(got, ops.label_posterior(k, wrt, *a, None, WEIGHT, **kw))
    cls = [ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData] if wrt else []
    fn = ctc.ctc_star_label_posterior_from_logproba if wrt else getattr(ctc, f"{kind}_ctc_star_label_posterior")
    a = (a[0][:, :40].contiguous(), a[1][:, :60], torch.tensor([40, 25], dtype=torch.int32, device=DEV), a[3] - 245, 0)
    pub = fn(*a, *cls, wildcard_log_weight=WEIGHT, **kw)
    assert isinstance(pub, ctc.CtcLabelPosterior) and same(pub, ops.star_label_posterior(k, wrt, *a, None, WEIGHT, **kw))


def test_the_entry_point_is_declared_exported_and_bound():
    """ctc_amd_star_label_posterior's signature with `int exclude_next_label` right behind `int optional_wildcards`."""
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "ctc_amd.h").read_text()
    res, args = _lib.SIGNATURES["ctc_amd_star_label_posterior"]
    assert f"int {NAME}(int kind, int wrt," in header and hasattr(_lib.load(), NAME)
    assert _lib.SIGNATURES[NAME] == (res, args[:12] + [ctypes.c_int] + args[12:]) and args[11] is ctypes.c_int
