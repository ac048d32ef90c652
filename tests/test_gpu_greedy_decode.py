"""Greedy CTC decoding on the GPU (ctc_amd_greedy_decode, csrc/ctc_decode.hip) against the float64 oracle
tests/tools/greedy_oracle.py.

Exact: tokens, labels, label_length, frames and every padding value.  The tie rule (the lowest token index at the row maximum)
is specified, so this holds for bfloat16 / float16 too, where ties at the maximum are common.
Tolerances (derived, not measured):
  score        |score - oracle| <= 1e-4 + 1e-6 * |score| (the alignment tests' score_tol): every lp is a float32 (rounding at
               most 6e-8 * |lp|, and all terms have one sign, so at most 6e-8 * |score| in the sum), the float32 row statistics
               behind the log-sum-exps take the rest of the relative term; the sum itself is float64.
  label_score  the same form on its own magnitude.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KIND_ID = {"classic": 0, "simplified": 1}


def score_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def data_cls(kind):
    import tf_seq2seq_losses_amd as ctc
    return ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData


def run(kind, wrt, x, tl, blank=0):
    """x: a NumPy array or a device tensor (taken as it stands).  Returns the six results as NumPy arrays."""
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=DEV)
    tlt = torch.from_numpy(np.asarray(tl, np.int32)).to(DEV)
    if wrt:
        out = ctc.ctc_greedy_decode_from_logproba(xt, tlt, blank, data_cls(kind))
    else:
        out = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(xt, tlt, blank)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcDecoding)
    B, T = xt.shape[0], xt.shape[1]
    assert out.score.shape == (B,) and out.label_length.shape == (B,)
    assert out.tokens.shape == out.labels.shape == out.frames.shape == out.label_score.shape == (B, T)
    assert out.score.dtype == torch.float32 and out.label_score.dtype == torch.float32
    assert all(t.dtype == torch.int32 for t in (out.tokens, out.labels, out.label_length, out.frames))
    assert not out.score.requires_grad
    return tuple(t.cpu().numpy() for t in out)


def check(got, want, what):
    """got: the six arrays of the GPU; want: GO.Decoding.  Integers and padding exactly, the two sums within score_tol."""
    score, tokens, labels, length, frames, label_score = got
    assert np.array_equal(tokens, want.tokens), (what, "tokens", np.argwhere(tokens != want.tokens)[:5])
    assert np.array_equal(length, want.label_length), (what, "label_length", length, want.label_length)
    assert np.array_equal(labels, want.labels), (what, "labels", np.argwhere(labels != want.labels)[:5])
    assert np.array_equal(frames, want.frames), (what, "frames", np.argwhere(frames != want.frames)[:5])
    pad = np.arange(tokens.shape[1])[None, :] >= want.label_length[:, None]
    assert np.all(np.isneginf(label_score[pad])), (what, "label_score padding")
    fin = np.isfinite(want.score)
    assert np.array_equal(score[~fin], want.score[~fin].astype(np.float32)), (what, score, want.score)
    err = np.abs(score[fin] - want.score[fin])
    lfin = ~pad & np.isfinite(want.label_score)
    assert np.array_equal(label_score[~pad & ~lfin], want.label_score[~pad & ~lfin].astype(np.float32)), (what, "non-finite label_score")
    lerr = np.abs(label_score[lfin] - want.label_score[lfin])
    print(f"DECODE-MEASURE {what}: worst |score - oracle| {err.max() if err.size else 0.0:.3e} "
          f"(bound {score_tol(np.abs(want.score[fin]).max() if err.size else 0.0):.3e} at the largest |score|), worst |label_score - oracle| "
          f"{lerr.max() if lerr.size else 0.0:.3e} (bound {score_tol(np.abs(want.label_score[lfin]).max() if lerr.size else 0.0):.3e}), "
          f"labels per utterance {want.label_length.min()}..{want.label_length.max()}", flush=True)
    assert np.all(err <= score_tol(want.score[fin])), (what, score, want.score)
    assert np.all(lerr <= score_tol(want.label_score[lfin])), (what, "label_score", lerr.max())


def ragged_lengths(B, T, rng):
    """logit_length in [0, T]; utterance 0 is full, utterance 1 empty, the last one T - 1 (where there are that many)."""
    tl = rng.integers(0, T + 1, B).astype(np.int32)
    tl[0] = T
    if B > 1:
        tl[1] = 0
    if B > 2:
        tl[-1] = max(T - 1, 0)
    return tl


@functools.lru_cache(maxsize=None)
def inputs(B, T, V, wrt):
    """Shared by the cases of one shape, never modified: (x float32 as the kernel reads it, logit_length)."""
    rng = np.random.default_rng(100000 * wrt + 1000 * T + V + B)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if V >= 8:
        x[..., : V // 8] += 2.0  # a few favoured tokens: repeats and blanks (token 0) do occur on the argmax path
    if wrt:
        x = VO.log_softmax64(x).astype(np.float32)
    x.setflags(write=False)
    return x, ragged_lengths(B, T, rng)


@functools.lru_cache(maxsize=None)
def reference(kind, B, T, V, wrt, blank):
    x, tl = inputs(B, T, V, wrt)
    return GO.decode(kind, x, tl, blank, wrt)


# T across the collapse stage's 64-frame steps, V across the 256-element steps of a row (and odd: the element-wise path), B * T
# not a multiple of the 16 rows of a workgroup; V = 20000 lies beyond every other entry point's vocabulary limit; (67, 1000, 6): six
# tokens, so runs of repeats cross the collapse stage's 64-frame steps and its 256-frame load batches in nearly every utterance
SHAPES = [(5, 1, 3), (3, 63, 64), (3, 64, 255), (3, 65, 256), (4, 130, 260), (2, 300, 1000), (2, 40, 8192), (2, 20, 20000),
          (7, 129, 33), (32, 1000, 256), (67, 1000, 6)]


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V", SHAPES, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}" for s in SHAPES])
def test_decoding_against_the_oracle(B, T, V, kind, wrt):
    x, tl = inputs(B, T, V, wrt)
    check(run(kind, wrt, x, tl), reference(kind, B, T, V, wrt, 0), f"{kind} wrt={wrt} B={B} T={T} V={V}")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_no_frames_at_all(kind):
    got = run(kind, 0, np.zeros((3, 0, 5), np.float32), [0, 0, 0])
    assert got[0].tolist() == [0.0, 0.0, 0.0] and got[3].tolist() == [0, 0, 0]
    assert got[1].shape == got[2].shape == got[4].shape == got[5].shape == (3, 0)


def test_empty_batch():
    import tf_seq2seq_losses_amd as ctc
    z = ctc.classic_ctc_greedy_decode(torch.zeros((0, 4, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert z.score.shape == (0,) and z.tokens.shape == (0, 4) and z.labels.shape == (0, 4) and z.label_length.shape == (0,)


def test_cpu_tensors_are_refused():
    import tf_seq2seq_losses_amd as ctc
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc.classic_ctc_greedy_decode(torch.zeros((1, 4, 3)), torch.tensor([4]))


def test_a_nonzero_blank_and_a_length_beyond_T():
    B, T, V, blank = 4, 70, 12, 5
    x, _ = inputs(B, T, V, 0)
    tl = np.asarray([T + 9, -3, 64, 1], np.int32)  # clamped to [0, T]
    for kind in VO.KINDS:
        check(run(kind, 0, x, tl, blank), GO.decode(kind, x, tl, blank, 0), f"{kind} blank={blank}, lengths {tl.tolist()}")


# ---- designed paths: logits 5 on the path, 0 elsewhere; the collapse stage's 64-frame steps ----
def designed_paths():
    V, blank = 6, 0
    def path(Tb, spans):
        p = np.full(Tb, blank, np.int32)
        for a, b, k in spans:
            p[a:b] = k
        return p
    paths = [
        path(130, [(60, 68, 2)]),                        # a run crossing t = 63 / 64
        path(128, [(60, 63, 3), (64, 67, 3)]),           # the same token on both sides, a blank at 63
        path(128, [(61, 64, 3), (65, 68, 3)]),           # ... a blank at 64
        path(65, [(63, 64, 4), (64, 65, 4)]),            # the run is exactly frames 63 and 64
        path(65, [(63, 64, 4), (64, 65, 5)]),            # two different tokens at 63 and 64
        path(65, [(0, 1, 1), (64, 65, 4)]),              # a non-blank at t = 0 and at T_b - 1
        path(64, [(0, 1, 2), (63, 64, 2)]),              # T_b = 64
        path(128, [(0, 1, 5), (127, 128, 5)]),           # T_b = 128
        path(130, []),                                   # all blank
        path(129, [(t, t + 1, 1 + t % 2) for t in range(129)]),  # no blank at all: T_b labels on either lattice
        path(130, [(0, 130, 3)]),                        # one run over three steps
        path(1, [(0, 1, 1)]),
    ]
    T = 130
    x = np.zeros((len(paths), T, V), np.float32)
    tl = np.asarray([len(p) for p in paths], np.int32)
    for b, p in enumerate(paths):
        x[b, np.arange(len(p)), p] = 5.0
        x[b, len(p):, 1 + b % 5] = 9.0                   # beyond the length: must not be looked at
    return x, tl, paths, blank


@pytest.mark.parametrize("kind", VO.KINDS)
def test_designed_paths_across_the_64_frame_steps(kind):
    x, tl, paths, blank = designed_paths()
    got = run(kind, 0, x, tl, blank)
    for b, p in enumerate(paths):  # the planted path is the argmax path, and its collapse is known in closed form
        assert np.array_equal(got[1][b, :len(p)], p), b
        assert got[2][b, :got[3][b]].tolist() == VO.reduces_to(kind, p, blank), b
    check(got, GO.decode(kind, x, tl, blank, 0), f"{kind} designed paths")
    assert got[3][8] == 0 and got[3][9] == 129
    assert got[3][10] == (1 if kind == "classic" else 130)
    assert got[3][1] == (2 if kind == "classic" else 6) and got[4][1, :2].tolist() == ([60, 64] if kind == "classic" else [60, 61])


@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("Tb", [64, 65, 128])
def test_constant_rows(kind, Tb):
    """Every element of every row the same: token 0 throughout (ties to the lowest index).  With blank = 0 nothing is decoded;
    with blank = V - 1 token 0 is one label on the classic lattice and T_b labels on the simplified one."""
    B, T, V = 3, 128, 7
    x = np.full((B, T, V), 0.25, np.float32)
    tl = np.asarray([Tb, Tb - 1, 0], np.int32)
    got = run(kind, 0, x, tl, 0)
    check(got, GO.decode(kind, x, tl, 0, 0), f"{kind} constant rows, blank=0, T_b={Tb}")
    assert got[3].tolist() == [0, 0, 0] and np.all(got[1][0, :Tb] == 0)
    assert np.all(np.abs(got[0] - tl * np.log(1.0 / V)) <= score_tol(tl * np.log(1.0 / V)))
    got = run(kind, 0, x, tl, V - 1)
    check(got, GO.decode(kind, x, tl, V - 1, 0), f"{kind} constant rows, blank={V - 1}, T_b={Tb}")
    assert got[3].tolist() == ([1, 1, 0] if kind == "classic" else [Tb, Tb - 1, 0])
    assert np.all(got[2][0, :got[3][0]] == 0)


# ---- producer formats ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_producer_formats_read_in_place(kind):
    """bfloat16, float16, time-major views, padded rows, a base pointer off by one element and an odd V give what the contiguous
    float32 copy of the same values gives: the conversions are exact and every access path hands a lane the same elements in the
    same order."""
    B, T, V = 5, 70, 64
    x, tl = inputs(B, T, V, 0)
    xt = torch.tensor(x, device=DEV)
    off = torch.zeros(B * T * V + 1, device=DEV)
    off[1:].copy_(xt.reshape(-1))
    xo, _ = inputs(B, T, 37, 0)
    xot = torch.tensor(xo, device=DEV)
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16)),
                      ("time-major float32", xt.transpose(0, 1).contiguous().transpose(0, 1)),
                      ("time-major bfloat16", xt.to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1)),
                      ("padded rows", torch.zeros((B, T, V + 4), device=DEV).copy_(torch.nn.functional.pad(xt, (0, 4)))[:, :, :V]),
                      ("padded rows, odd stride", torch.zeros((B, T, V + 3), device=DEV).copy_(torch.nn.functional.pad(xt, (0, 3)))[:, :, :V]),
                      ("base pointer off by one element", off[1:].view(B, T, V)),
                      ("odd V, bfloat16", xot.to(torch.bfloat16)),
                      ("odd V, time-major float16", xot.to(torch.float16).transpose(0, 1).contiguous().transpose(0, 1))):
        if name.startswith("base pointer"):
            assert xin.data_ptr() % 16 == 4 and xin.is_contiguous()
        else:
            assert not (xin.dtype == torch.float32 and xin.is_contiguous())
        x32 = xin.float().contiguous().clone()
        assert x32.data_ptr() % 16 == 0 and x32.is_contiguous()
        got = run(kind, 0, xin, tl)
        ref = run(kind, 0, x32, tl)
        for g, r, part in zip(got, ref, ("score", "tokens", "labels", "label_length", "frames", "label_score")):
            assert g.tobytes() == r.tobytes(), (name, part)
        check(got, GO.decode(kind, x32.cpu().numpy(), tl, 0, 0), f"{kind} {name}")


# ---- a frame of log-probabilities that is all -inf ----
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("wrt", [0, 1])
def test_a_row_of_minus_infinity(kind, wrt):
    """score -inf for that utterance, token 0 at that frame (the lowest index), everything else as without it."""
    B, T, V = 3, 70, 16
    x0, tl = inputs(B, T, V, wrt)
    tl = np.asarray([T, T, 40], np.int32)
    x = x0.copy()
    x[1, 64, :] = -np.inf
    x[1, 3, 5] = -np.inf  # one -inf element in an ordinary row: no trouble
    got, base = run(kind, wrt, x, tl), run(kind, wrt, x0, tl)
    want = GO.decode(kind, x, tl, 0, wrt)
    assert got[0][1] == -np.inf and got[1][1, 64] == 0 and want.score[1] == -np.inf
    check(got, want, f"{kind} wrt={wrt} a row of -inf")
    for b in (0, 2):  # nothing else is disturbed
        for g, r in zip(got, base):
            assert g[b].tobytes() == r[b].tobytes(), b


# ---- cross-checks between features ----
CROSS = [(6, 300, 64), (3, 1000, 256), (2, 200, 8192)]


@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V", CROSS, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}" for s in CROSS])
def test_alignment_and_loss_of_the_decoded_labels(B, T, V, kind):
    """The frame-wise argmax path is the optimum over ALL paths, so the best path that gives the decoded labels is that path (or
    one of equal value): the alignment's score equals the decoding's, its tokens reduce to the same labels, and the loss of the
    decoded labels -- the sum over every path that gives them -- is at least the one path's probability.
    Blank-biased logits (+3 on the blank column) so that labels are shorter than frames."""
    import tf_seq2seq_losses_amd as ctc
    x, tl = inputs(B, T, V, 0)
    x = x.copy()
    x[..., 0] += 3.0
    tl = np.maximum(tl, 1).astype(np.int32)
    xt, tlt = torch.from_numpy(x).to(DEV), torch.from_numpy(tl).to(DEV)
    dec = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(xt, tlt, 0)
    n = dec.label_length.cpu().numpy()
    assert n.max() <= 1024 and n.max() < tl.max(), n
    align = (ctc.classic_ctc_alignment if kind == "classic" else ctc.simplified_ctc_alignment)(dec.labels, xt, dec.label_length, tlt, 0)
    loss = (ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss)(dec.labels, xt, dec.label_length, tlt, 0)
    torch.cuda.synchronize()
    score, a_score, loss = dec.score.cpu().numpy(), align.score.cpu().numpy(), loss.cpu().numpy()
    labels, a_tokens = dec.labels.cpu().numpy(), align.tokens.cpu().numpy()
    tol = 2 * score_tol(score)
    print(f"DECODE-MEASURE {kind} B={B} T={T} V={V}: labels {n.tolist()}, alignment score - decode score {(a_score - score).tolist()}, "
          f"-loss - score {(-loss - score).tolist()}, bound {tol.tolist()}", flush=True)
    assert np.all(np.isfinite(score)) and np.all(np.isfinite(a_score)) and np.all(np.isfinite(loss))
    assert np.all(np.abs(a_score - score) <= tol), (a_score, score)
    for b in range(B):
        assert VO.reduces_to(kind, a_tokens[b, :tl[b]], 0) == labels[b, :n[b]].tolist(), b
    assert np.all(-loss >= score - tol), (loss, score)


# ---- graph capture ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_greedy_decode_in_a_hip_graph(kind):
    """Two launches on one stream, a single serial branch: captured once and replayed on new logits in the same buffers."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = 6, 90, 64
    k = KIND_ID[kind]
    x = torch.zeros((B, T, V), device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    score = torch.zeros(B, device=DEV)
    tokens, labels, frames = (torch.zeros((B, T), dtype=torch.int32, device=DEV) for _ in range(3))
    length = torch.zeros(B, dtype=torch.int32, device=DEV)
    label_score = torch.zeros((B, T), device=DEV)
    ws = torch.zeros(max(_lib.greedy_decode_workspace_bytes(B, T), 1), dtype=torch.uint8, device=DEV)
    outs = (score, tokens, labels, length, frames, label_score)

    def call():
        rc = lib.ctc_amd_greedy_decode(k, _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, tl.data_ptr(), 0, B, T, V,
                                       score.data_ptr(), tokens.data_ptr(), labels.data_ptr(), length.data_ptr(), frames.data_ptr(),
                                       label_score.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(seed):
        rng = np.random.default_rng(seed)
        h = (rng.standard_normal((B, T, V)).astype(np.float32), ragged_lengths(B, T, rng))
        x.copy_(torch.from_numpy(h[0])); tl.copy_(torch.from_numpy(h[1]))
        return h

    fill(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (2, 3):
        h = fill(seed)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = tuple(o.cpu().numpy() for o in outs)
        for o in outs:
            o.zero_()
        call()
        torch.cuda.synchronize()
        for a, o in zip(got, outs):
            assert a.tobytes() == o.cpu().numpy().tobytes()
        check(got, GO.decode(kind, h[0], h[1], 0, 0), f"{kind} graph replay seed {seed}")
