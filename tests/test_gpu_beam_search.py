"""Prefix beam search on the GPU (ctc_amd_beam_search, csrc/ctc_beam.hip) against the float64 oracle tests/tools/beam_oracle.py.

Exact: labels, label_length, the order of the hypotheses and every padding value -- under the asserted condition that the oracle's
margin (the smallest gap in ln mass at any pruning decision and between neighbours of the returned list) is at least 1e-9 for every
utterance.  Derivation: about 300 frames x at most K + 2 <= 34 float64 operations into one mass per frame x 2^-53 ~ 1e-12 of
relative difference between two float64 evaluations of the same definition; 1e-9 leaves three orders.  The seeds below were chosen
with the oracle (their margins are 1e-6 or more); no case is skipped.
Tolerance (derived, not measured): |score - oracle| <= 1e-4 + 1e-6 * |score|, the bound of tests/test_gpu_alignment.py and
tests/test_gpu_greedy_decode.py: the float32 row log-sum-exps behind the score and its own float32 rounding.
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ctc_oracle as O
from tests import _ownership as OW
from tests.tools import beam_oracle as BO
from tests.tools.viterbi_oracle import KINDS, log_softmax64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KIND_ID = {"classic": 0, "simplified": 1}
MIN_MARGIN = 1e-9


def score_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def data_cls(kind):
    import tf_seq2seq_losses_amd as ctc
    return ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData


def run(kind, wrt, x, tl, blank, W, K, nbest):
    """x: a NumPy array or a device tensor (taken as it stands).  Returns (score, labels, label_length) as NumPy arrays."""
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=DEV)
    tlt = torch.from_numpy(np.asarray(tl, np.int32)).to(DEV)
    kw = dict(beam_width=W, top_k=K, nbest=nbest)
    if wrt:
        out = ctc.ctc_beam_search_from_logproba(xt, tlt, blank, data_cls(kind), **kw)
    else:
        out = (ctc.classic_ctc_beam_search if kind == "classic" else ctc.simplified_ctc_beam_search)(xt, tlt, blank, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcBeamDecoding)
    B, T = xt.shape[0], xt.shape[1]
    assert out.score.shape == (B, nbest) and out.labels.shape == (B, nbest, T) and out.label_length.shape == (B, nbest)
    assert out.score.dtype == torch.float32 and out.labels.dtype == torch.int32 and out.label_length.dtype == torch.int32
    assert not out.score.requires_grad
    return tuple(t.cpu().numpy() for t in out)


def check(got, want, what):
    """got: the three arrays of the GPU; want: BO.search's four.  Margin first, then integers and padding exactly, scores within
    score_tol, -inf where the oracle has no hypothesis."""
    score, labels, length = got
    wscore, wlabels, wlength, margin = want
    print(f"BEAM-MEASURE {what}: oracle margin per utterance {margin.tolist()}", flush=True)
    assert np.all(margin >= MIN_MARGIN), (what, "the inputs do not separate the hypotheses; choose another seed", margin)
    assert np.array_equal(length, wlength), (what, "label_length", np.argwhere(length != wlength)[:5])
    assert np.array_equal(labels, wlabels), (what, "labels", np.argwhere(labels != wlabels)[:5])
    fin = np.isfinite(wscore)
    assert np.all(np.isneginf(score[~fin])), (what, "missing hypotheses", score[~fin])
    err = np.abs(score[fin] - wscore[fin])
    print(f"BEAM-MEASURE {what}: worst |score - oracle| {err.max() if err.size else 0.0:.3e} (bound "
          f"{score_tol(np.abs(wscore[fin]).max() if err.size else 0.0):.3e} at the largest |score|), labels per hypothesis "
          f"{wlength.min()}..{wlength.max()}, hypotheses per utterance {fin.sum(axis=1).tolist()}", flush=True)
    assert np.all(err <= score_tol(wscore[fin])), (what, err.max())


def lengths_for(B, T, rng):
    """Ragged; T, 0 and 1 are there as far as B allows (two utterances: T and a ragged one; SHORT_LENGTHS then has 0 and 1)."""
    tl = rng.integers(T // 2, T + 1, B).astype(np.int32)
    tl[0] = T
    if B > 2:
        tl[1], tl[2] = 0, 1
    return tl


SHORT_LENGTHS = (0, 1)  # the second run of the shapes with two utterances


@functools.lru_cache(maxsize=None)
def inputs(B, T, V, seed, blank=0):
    """Blank-biased N(0, 2^2) logits and ragged lengths; read-only, shared by the tests of one shape."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    x[..., blank] += 3.0
    x.setflags(write=False)
    return x, lengths_for(B, T, rng)


@functools.lru_cache(maxsize=None)
def reference(kind, B, T, V, W, K, nbest, seed, blank=0, wrt=0):
    x, tl = inputs(B, T, V, seed, blank)
    if wrt:
        x = log_softmax64(x).astype(np.float32)
    return BO.search(kind, x, tl, blank, wrt, W, K, nbest)


# ---- exhaustive: nothing is pruned, every labelling of non-zero probability comes back ----
@pytest.mark.parametrize("blank", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_exhaustive_small_case(kind, blank):
    B, T, V, W, K, nbest = 6, 5, 3, 64, 2, 64
    x = (2.0 * np.random.default_rng(7 + blank).standard_normal((B, T, V))).astype(np.float32)
    tl = np.arange(B, dtype=np.int32)  # 0 .. 5
    got = run(kind, 0, x, tl, blank, W, K, nbest)
    want = BO.search(kind, x, tl, blank, 0, W, K, nbest)
    check(got, want, f"exhaustive {kind} blank={blank}")
    score, labels, length = got
    assert np.isfinite(score[0]).sum() == 1 and score[0, 0] == 0.0 and length[0, 0] == 0  # no frames: the empty prefix alone
    # every score is -loss of its labelling (float64 loss oracle): the beam holds every path
    for b in range(1, B):
        n = int(np.isfinite(score[b]).sum())
        assert n == int(np.isfinite(want[0][b]).sum()) and n >= 2 * b
        lab = np.where(labels[b, :n] < 0, (blank + 1) % V, labels[b, :n])
        loss = np.asarray(O.ctc_loss(kind, lab, np.broadcast_to(x[b], (n, T, V)), length[b, :n], np.full(n, tl[b], np.int32), blank).loss)
        err = np.abs(score[b, :n] + loss)
        print(f"BEAM-MEASURE exhaustive {kind} blank={blank} T_b={tl[b]}: {n} labellings, worst |score + loss| {err.max():.3e}", flush=True)
        assert np.all(err <= score_tol(loss)), (b, err.max())
        assert abs(np.exp(score[b, :n].astype(np.float64)).sum() - 1.0) < 1e-4  # the labellings partition the paths


# ---- against the beam oracle ----
# (B, T, V, W, K, nbest)
ORACLE_SHAPES = [(4, 40, 6, 4, 5, 4), (3, 150, 64, 8, 8, 8), (2, 300, 256, 16, 8, 4), (2, 120, 1000, 64, 16, 16),
                 (2, 70, 8192, 5, 32, 5), (2, 130, 260, 64, 3, 1)]
SEED = 1  # every case below has an oracle margin of 1e-6 or more with it


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("short", [False, True], ids=["ragged", "short"])
@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=["B%d-T%d-V%d-W%d-K%d-n%d" % s for s in ORACLE_SHAPES])
def test_search_against_the_oracle(shape, short, kind):
    """Every shape sees the lengths T, 0 and 1: in one batch where it has three utterances or more, in a second run with the
    lengths (0, 1) where it has two."""
    B, T, V, W, K, nbest = shape
    seed = SEED
    x, tl = inputs(B, T, V, seed)
    if short:
        if B > 2:
            assert {0, 1, T} <= set(tl.tolist())
            return  # (nothing to add: the one run has them)
        tl = np.asarray(SHORT_LENGTHS, np.int32)
    xin = x
    if shape == (2, 130, 260, 64, 3, 1):
        # a batch stride of T * V + 2 elements: the rows of utterance 1 start 8 bytes off a 16-byte boundary
        _, xin, _ = OW.strided_storage(torch.tensor(x, device=DEV), T * V + 2, V)
        assert xin.stride() == (T * V + 2, V, 1) and (xin[1].data_ptr() - xin[0].data_ptr()) % 16 == 8
    want = BO.search(kind, x, tl, 0, 0, W, K, nbest) if short else reference(kind, B, T, V, W, K, nbest, seed)
    check(run(kind, 0, xin, tl, 0, W, K, nbest), want, f"{kind} {shape} seed {seed} lengths {tl.tolist()}")


@pytest.mark.parametrize("kind", KINDS)
def test_a_blank_in_the_middle_and_lengths_beyond_T(kind):
    B, T, V, W, K, nbest, blank = 4, 70, 12, 8, 4, 8, 5
    seed = SEED
    x, _ = inputs(B, T, V, seed, blank)
    tl = np.asarray([T + 9, -3, 64, 1], np.int32)  # clamped to [0, T]
    check(run(kind, 0, x, tl, blank, W, K, nbest), BO.search(kind, x, tl, blank, 0, W, K, nbest), f"{kind} blank={blank}")


def test_empty_batch_no_frames_and_cpu_tensors():
    import tf_seq2seq_losses_amd as ctc
    z = ctc.classic_ctc_beam_search(torch.zeros((0, 4, 3), device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), nbest=2)
    assert z.score.shape == (0, 2) and z.labels.shape == (0, 2, 4) and z.label_length.shape == (0, 2)
    score, labels, length = run("simplified", 0, np.zeros((3, 0, 5), np.float32), [0, 0, 0], 0, 4, 4, 2)
    assert score.tolist() == [[0.0, -np.inf]] * 3 and length.tolist() == [[0, 0]] * 3 and labels.shape == (3, 2, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc.classic_ctc_beam_search(torch.zeros((1, 4, 3)), torch.tensor([4]))
    with pytest.raises(ValueError, match="beam_width"):
        ctc.classic_ctc_beam_search(torch.zeros((1, 4, 3), device=DEV), torch.tensor([4]), beam_width=65)
    with pytest.raises(ValueError, match="nbest"):
        ctc.classic_ctc_beam_search(torch.zeros((1, 4, 3), device=DEV), torch.tensor([4]), beam_width=4, nbest=5)


# ---- producer formats ----
@pytest.mark.parametrize("kind", KINDS)
def test_producer_formats_read_in_place(kind):
    """bfloat16, float16, time-major views and padded rows give the bits the contiguous float32 copy of the same values gives
    (the conversions are exact, the cut's tie rule is specified -- 16-bit rows are full of ties -- and every access path hands a
    lane the same elements)."""
    B, T, V, W, K, nbest = 4, 70, 64, 8, 8, 8
    x, tl = inputs(B, T, V, 11)
    xt = torch.tensor(x, device=DEV)
    xo, _ = inputs(B, T, 37, 11)
    xot = torch.tensor(xo, device=DEV)
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16)),
                      ("time-major float32", xt.transpose(0, 1).contiguous().transpose(0, 1)),
                      ("time-major bfloat16", xt.to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1)),
                      ("padded rows", torch.zeros((B, T, V + 4), device=DEV).copy_(torch.nn.functional.pad(xt, (0, 4)))[:, :, :V]),
                      ("padded rows, odd stride", torch.zeros((B, T, V + 3), device=DEV).copy_(torch.nn.functional.pad(xt, (0, 3)))[:, :, :V]),
                      ("odd V, bfloat16", xot.to(torch.bfloat16)),
                      ("odd V, time-major float16", xot.to(torch.float16).transpose(0, 1).contiguous().transpose(0, 1))):
        assert not (xin.dtype == torch.float32 and xin.is_contiguous())
        x32 = xin.float().contiguous().clone()
        got = run(kind, 0, xin, tl, 0, W, K, nbest)
        ref = run(kind, 0, x32, tl, 0, W, K, nbest)
        for g, r, part in zip(got, ref, ("score", "labels", "label_length")):
            assert g.tobytes() == r.tobytes(), (name, part)


@pytest.mark.parametrize("kind", KINDS)
def test_log_probabilities_give_the_hypotheses_of_their_logits(kind):
    """lp = log_softmax(x) rounded to float32 is another input (its ranking may differ from x's in the last bits), so it has its
    own oracle run; where both margins hold the hypotheses are those of the logits."""
    shape = (3, 150, 64, 8, 8, 8)
    B, T, V, W, K, nbest = shape
    seed = SEED
    x, tl = inputs(B, T, V, seed)
    lp = log_softmax64(x).astype(np.float32)
    got = run(kind, 1, lp, tl, 0, W, K, nbest)
    check(got, reference(kind, B, T, V, W, K, nbest, seed, 0, 1), f"{kind} log-probabilities {shape}")
    from_logits = run(kind, 0, x, tl, 0, W, K, nbest)
    assert np.array_equal(got[1], from_logits[1]) and np.array_equal(got[2], from_logits[2])
    fin = np.isfinite(got[0])
    assert np.array_equal(fin, np.isfinite(from_logits[0]))
    diff = np.abs(got[0][fin] - from_logits[0][fin])
    print(f"BEAM-MEASURE {kind} log-probabilities against logits: worst |score difference| {diff.max():.3e}", flush=True)
    assert np.all(diff <= score_tol(got[0][fin]))


# ---- between features ----
@pytest.mark.parametrize("kind", KINDS)
def test_scores_are_lower_bounds_of_the_loss_and_beat_greedy(kind):
    import tf_seq2seq_losses_amd as ctc
    B, T, V = 3, 200, 64
    x, _ = inputs(B, T, V, SEED)
    tl = np.asarray([T, T - 37, 90], np.int32)
    xt, tlt = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(tl).to(DEV)
    search = ctc.classic_ctc_beam_search if kind == "classic" else ctc.simplified_ctc_beam_search
    loss_fn = ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss
    nb = search(xt, tlt, 0, beam_width=16, top_k=8, nbest=8)
    score = nb.score.cpu().numpy()
    assert np.all(np.isfinite(score)) and np.all(np.diff(score, axis=1) <= 0), score
    labels, length = nb.labels.cpu().numpy(), nb.label_length.cpu().numpy()
    for b in range(B):
        seqs = {tuple(labels[b, n, :length[b, n]]) for n in range(8)}
        assert len(seqs) == 8, (b, "hypotheses are not pairwise distinct")
    for n in range(8):  # the N-best outputs go straight back into the loss
        loss = loss_fn(nb.labels[:, n], xt, nb.label_length[:, n], tlt, 0).cpu().numpy()
        print(f"BEAM-MEASURE {kind} n={n}: -loss - score {(-loss - score[:, n]).tolist()}", flush=True)
        assert np.all(score[:, n] <= -loss + score_tol(loss)), (n, score[:, n], loss)
    # the widest search the interface takes: W = 64 and the cut at its limit (top_k <= 32, so K = V - 1 = 63 cannot be asked for;
    # the argmax token of every frame is inside any cut)
    wide = search(xt, tlt, 0, beam_width=64, top_k=32, nbest=1)
    greedy = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(xt, tlt, 0)
    top = loss_fn(wide.labels[:, 0], xt, wide.label_length[:, 0], tlt, 0).cpu().numpy()
    base = loss_fn(greedy.labels, xt, greedy.label_length, tlt, 0).cpu().numpy()
    print(f"BEAM-MEASURE {kind}: -loss of the top hypothesis {(-top).tolist()}, of the greedy decoding {(-base).tolist()}", flush=True)
    assert np.all(-top >= -base - score_tol(base)), (top, base)


# ---- contract ----
def raw_call(kind, x, tl, blank, W, K, nbest, ws_pattern, fill=0xA5, ws=None):
    """The C ABI with every buffer under the test's control."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = x.shape
    if ws is None:
        ws = OW.workspace(_lib.beam_search_workspace_bytes(B, T, V, W, K), ws_pattern)
    score = OW.filled((B, nbest), torch.float32, fill, DEV)
    labels = OW.filled((B, nbest, T), torch.int32, fill, DEV)
    length = OW.filled((B, nbest), torch.int32, fill, DEV)
    tlt = torch.from_numpy(np.asarray(tl, np.int32)).to(DEV)
    rc = lib.ctc_amd_beam_search(KIND_ID[kind], 0, x.data_ptr(), OW._dt(x), x.stride(0), x.stride(1), tlt.data_ptr(), blank, B, T, V,
                                 W, K, nbest, score.data_ptr(), labels.data_ptr(), length.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    return {"score": score, "labels": labels, "label_length": length}, ws


@pytest.mark.parametrize("kind", KINDS)
def test_unowned_memory_changes_no_bit(kind):
    """Padding frames full of NaN / +-inf, a workspace left by another call (or full of 0xFF / 0xA5 bytes) and the outputs' contents
    on entry change no bit of any output."""
    B, T, V, W, K, nbest = 4, 90, 64, 8, 8, 8
    x, _ = inputs(B, T, V, 5)
    tl = np.asarray([T, 0, 1, 57], np.int32)
    xt = torch.tensor(x, device=DEV)
    clean, ws = raw_call(kind, xt, tl, 0, W, K, nbest, 0x00, fill=0x00)
    for value in OW.poison_values(torch.float32):
        other, _ = raw_call(kind, OW.poison_padding(xt, tl, value), tl, 0, W, K, nbest, 0x00)
        assert OW.total_diff(clean, other) == {"score": 0, "labels": 0, "label_length": 0}, value
    for pattern in (0xFF, 0xA5):
        other, _ = raw_call(kind, xt, tl, 0, W, K, nbest, pattern, fill=pattern)
        assert OW.total_diff(clean, other) == {"score": 0, "labels": 0, "label_length": 0}, pattern
    # the workspace another call left: a longer batch of other logits, the other lattice
    x2, _ = inputs(B, T, V, 6)
    _, ws2 = raw_call(KINDS[1 - KINDS.index(kind)], torch.tensor(x2, device=DEV), [T] * B, 0, W, K, nbest, 0x00)
    other, _ = raw_call(kind, xt, tl, 0, W, K, nbest, 0x00, ws=ws2)
    assert OW.total_diff(clean, other) == {"score": 0, "labels": 0, "label_length": 0}


@pytest.mark.parametrize("kind", KINDS)
def test_missing_hypotheses_and_a_frame_of_minus_infinity(kind):
    B, T, V, W, K, nbest = 4, 12, 5, 8, 4, 8
    x = np.array(inputs(B, T, V, 9)[0])
    x[1, 7, :] = -np.inf          # kills the beam of utterance 1
    x[2, :, 1:] = -np.inf         # utterance 2: only the blank is possible, one hypothesis (the empty one) survives
    x[3, 3, 2] = -np.inf          # one -inf element: no trouble
    tl = np.asarray([0, T, T, 2], np.int32)
    got = run(kind, 0, x, tl, 0, W, K, nbest)
    want = BO.search(kind, x, tl, 0, 0, W, K, nbest)
    check(got, want, f"{kind} missing hypotheses")
    score, labels, length = got
    assert score[0].tolist() == [0.0] + [-np.inf] * 7 and np.all(labels[0] == -1) and np.all(length[0] == 0)
    assert np.all(np.isneginf(score[1])) and np.all(labels[1] == -1) and np.all(length[1] == 0)
    assert np.isfinite(score[2]).tolist() == [True] + [False] * 7 and abs(score[2, 0]) <= 1e-6 and np.all(labels[2] == -1)
    alive = np.isfinite(score[3])
    assert 2 <= alive.sum() <= 8 and np.all(labels[3][~alive] == -1) and np.all(length[3][~alive] == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_a_vocabulary_of_the_blank_alone(kind):
    """V = 1: the effective cut is 0, the empty prefix is the one hypothesis, and its probability is 1 (logits) or exp(sum x)."""
    x = np.asarray([[[0.5], [-2.0], [1.25]], [[0.0], [0.0], [0.0]]], np.float32)
    tl = np.asarray([3, 2], np.int32)
    for wrt, want0 in ((0, 0.0), (1, -0.25)):
        score, labels, length = run(kind, wrt, x, tl, 0, 4, 3, 2)
        assert abs(score[0, 0] - want0) <= 1e-6 and score[1, 0] == 0.0 and np.all(np.isneginf(score[:, 1]))
        assert np.all(labels == -1) and np.all(length == 0)


# ---- graph capture ----
@pytest.mark.parametrize("kind", KINDS)
def test_beam_search_in_a_hip_graph(kind):
    """Two launches on one stream, a single serial branch: captured once and replayed on new logits in the same buffers."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, W, K, nbest = 4, 90, 64, 8, 8, 4
    x = torch.zeros((B, T, V), device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    score = torch.zeros((B, nbest), device=DEV)
    labels = torch.zeros((B, nbest, T), dtype=torch.int32, device=DEV)
    length = torch.zeros((B, nbest), dtype=torch.int32, device=DEV)
    ws = torch.zeros(_lib.beam_search_workspace_bytes(B, T, V, W, K), dtype=torch.uint8, device=DEV)
    outs = (score, labels, length)

    def call():
        rc = lib.ctc_amd_beam_search(KIND_ID[kind], _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, tl.data_ptr(), 0, B, T, V, W, K, nbest,
                                     score.data_ptr(), labels.data_ptr(), length.data_ptr(), ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(seed):
        h = inputs(B, T, V, seed)
        x.copy_(torch.from_numpy(np.array(h[0]))); tl.copy_(torch.from_numpy(h[1]))
        return h

    fill(21)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (22, 23):
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
        check(got, BO.search(kind, h[0], h[1], 0, 0, W, K, nbest), f"{kind} graph replay seed {seed}")
