"""Label posteriors from block checkpoints on the GPU (ctc_amd_label_posterior_ckpt, wild_ckpt_post_kernel of
csrc/ctc_wild_loss_ckpt.hip) against the float64 oracle, with the helpers and the bars of tests/test_gpu_label_posterior.py as they
stand; the loss has the bits of the forward-only wildcard loss.  F = 32 / 16 / 8 frames per block at U <= 64 / 128 / 256."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_label_posterior as P
from tests.test_gpu_wildcard_loss import needed_frames
from tests.test_gpu_wildcard_loss_ckpt import EDGES, PATTERNS

pytestmark = pytest.mark.gpu
W, KINDS, dev = P.W, P.KINDS, P.dev


def run_ck(*a, **kw):  # P.run with checkpoint=True
    from tf_seq2seq_losses_amd import ops
    with mock.patch.object(ops, "label_posterior", functools.partial(ops.label_posterior, checkpoint=True)):
        return P.run(*a, **kw)


def raw_ck(*a):  # P.raw_call on ctc_amd_label_posterior_ckpt
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    with mock.patch.object(lib, "ctc_amd_label_posterior", lib.ctc_amd_label_posterior_ckpt):
        P.raw_call(*a)


def check(what, kind, wrt, x, labels, ll, tl, **kw):  # against the oracle of the float32 values of x, the loss bits included
    xr = x.float().cpu().numpy() if isinstance(x, torch.Tensor) else x
    ref = P.oracle(kind, wrt, xr, labels[:, :kw.get("U", labels.shape[1])], ll, tl, **{k: v for k, v in kw.items() if k != "U"})
    out = run_ck(kind, wrt, x, labels, ll, tl, **kw)
    P.compare(what, out, ref, labels, ll, tl, wild_bits=P.wild_loss(kind, wrt, x, labels, ll, tl, **kw))
    return out


@pytest.mark.parametrize("U,F,T,i", EDGES, ids=lambda v: str(v))
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_block_edges_and_pipeline_fill_and_drain(kind, wrt, U, F, T, i):
    """1 to 4 blocks, T_b = (T, 0, max(T - 2, 1)); short transcripts (cut to the frames there are) in the widths of all three tiers."""
    rng = np.random.default_rng(100 * U + T)
    x = rng.standard_normal((3, T, 6)).astype(np.float32)
    if wrt:
        x = P.logprobs32(x) - np.float32(0.25)
    tl = np.asarray([T, 0, max(T - 2, 1)], np.int32)
    labels = rng.integers(1, 6, (3, max(U, 6))).astype(np.int32)
    ll = np.zeros(3, np.int32)
    for b in range(3):
        pat = PATTERNS[(i + 2 * b) % 5][:min(U, max(int(tl[b]), 1))]
        labels[b, :len(pat)] = pat
        ll[b] = len(pat)
    check(f"ckpt {kind} wrt={wrt} U={U} T={T}", kind, wrt, x, labels, ll, tl, U=U)


@pytest.mark.parametrize("U", [64, 65, 129, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_full_tiers(kind, U):
    x, labels, ll, tl = P.make_inputs(kind, 3, 2 * U + 4, 8, U, seed=U)
    ll[:] = U
    need = [needed_frames(kind, labels[b]) for b in range(3)]
    tl[:] = [need[0] + 3, need[1] - 1, need[2] + 2]  # the second a frame short
    out = check(f"ckpt {kind} full U={U}", kind, 0, x, labels, ll, tl)
    assert float(out[0][1]) == np.inf and not out[1][1].any() and bool((out[4][1] == -1).all())


@pytest.mark.parametrize("kind", KINDS)
def test_writer_geometry_and_determinism(kind):
    """U no multiple of 4, a wider labels tensor with hostile tails; buffers of 0x00 / 0xFF, no statistics, two replays of a graph."""
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = 3, 90, 7, 70
    x, labels, ll, tl = P.make_inputs(kind, B, T, V, U, seed=110)
    tl[1] = int(ll[1]) - 1  # one infeasible utterance: its zeros are written, not left over
    wide = np.concatenate([labels, np.asarray([[-7, 10 ** 9, V, 0, W]] * B, np.int32)], axis=1)
    args = (kind, 0, dev(x), dev(wide), dev(ll), dev(tl), 0, -0.25, U)
    n = _lib.label_posterior_ckpt_workspace_bytes(P.kind_id(kind), B, T, V, U)
    outs = []
    for pattern in (0x00, 0xFF):
        outs.append(P.buffers(B, T, U, pattern))
        raw_ck(*args, outs[-1], OW.byte_fill(n, pattern, P.DEV))
        torch.cuda.synchronize()
    assert P.same_outputs(outs[0], outs[1])
    P.compare(f"ckpt {kind} raw call", outs[1], P.oracle(kind, 0, x, labels, ll, tl, weight=-0.25), labels, ll, tl)
    out = P.buffers(B, T, U, 0xFF, stats=False)
    raw_ck(*args, out, OW.byte_fill(n, 0xFF, P.DEV))
    torch.cuda.synchronize()
    assert P.same_outputs(out[:3], outs[0][:3])
    ws, out = OW.byte_fill(n, 0x5A, P.DEV), P.buffers(B, T, U, 0x5A)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        raw_ck(*args, out, ws)
    for _ in range(2):
        for o in out:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert P.same_outputs(out, outs[0])


@pytest.mark.parametrize("V,blank", [(5, 0), (5, 2), (5, 4), (1030, 0), (1030, 1029)])
@pytest.mark.parametrize("kind", KINDS)
def test_vocabulary_and_blank(kind, V, blank):
    x, labels, ll, tl = P.make_inputs(kind, 2, 40, V, 6, seed=30 + blank, blank=blank)
    if V > 1024:
        labels[0, 1], labels[1, 1] = 1025, 1025  # a token of the second pass of 1024 columns
        tl[:] = 40
    check(f"ckpt {kind} V={V} blank={blank}", kind, 0, x, labels, ll, tl, blank=blank)


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    B, T, V, U = 3, 40, 260, 20
    x, labels, ll, tl = P.make_inputs(kind, B, T, V, U, seed=106)
    xt = dev(x)
    out_c = check(f"ckpt {kind} float32", kind, 0, x, labels, ll, tl)
    for dt in (torch.bfloat16, torch.float16):
        check(f"ckpt {kind} {dt}", kind, 0, xt.to(dt), labels, ll, tl)
    xtm = xt.transpose(0, 1).contiguous().transpose(0, 1)  # time-major, read in place
    flat = torch.zeros(B * T * V + 1, dtype=torch.float32, device=P.DEV)
    xo = flat[1:].view(B, T, V)  # an unaligned base pointer
    xo.copy_(xt)
    assert xtm.stride() == (V, B * V, 1) and xo.data_ptr() % 16 == 4
    for xv in (xtm, xo):
        assert P.same_outputs(run_ck(kind, 0, xv, labels, ll, tl), out_c)


@pytest.mark.parametrize("kind", KINDS)
def test_wildcard_weight_on_log_probabilities(kind):
    x, labels, ll, tl = P.make_inputs(kind, 4, 70, 7, 20, seed=7)
    check(f"ckpt {kind} w=-0.5 wrt=1", kind, 1, P.logprobs32(x), labels, ll, tl, weight=-0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_above_256_labels_it_is_the_per_frame_call(kind):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = 2, 329, 8, 257
    x, labels, ll, tl = P.make_inputs(kind, B, T, V, U, seed=U)
    assert P.same_outputs(run_ck(kind, 0, x, labels, ll, tl), P.run(kind, 0, x, labels, ll, tl))
    k = P.kind_id(kind)
    assert _lib.label_posterior_ckpt_workspace_bytes(k, B, T, V, U) == _lib.label_posterior_workspace_bytes(k, B, T, V, U)
    assert 3 * _lib.label_posterior_ckpt_workspace_bytes(k, B, T, V, 256) < _lib.label_posterior_workspace_bytes(k, B, T, V, 256)


@pytest.mark.parametrize("kind", KINDS)
def test_public_route(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 3, 40, 6, 10
    x, labels, ll, tl = P.make_inputs(kind, B, T, V, U, seed=70)
    a = (dev(labels), dev(x), dev(ll), dev(tl), 0)
    fn = ctc.classic_ctc_label_posterior if kind == "classic" else ctc.simplified_ctc_label_posterior
    assert P.same_outputs(fn(*a, checkpoint=True), run_ck(kind, 0, x, labels, ll, tl))
    cls, lp = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData, P.logprobs32(x)
    assert P.same_outputs(ctc.ctc_label_posterior_from_logproba(a[0], dev(lp), *a[2:], cls, checkpoint=True), run_ck(kind, 1, lp, labels, ll, tl))
    window = torch.tensor([0, T - 1], dtype=torch.int32, device=P.DEV).expand(B, U, 2).contiguous()
    for other in (dict(frame_window=window), dict(optional_wildcards=True), dict(exclude_next_label=True)):  # owed: today's path
        assert P.same_outputs(fn(*a, checkpoint=True, **other), fn(*a, **other)), other
