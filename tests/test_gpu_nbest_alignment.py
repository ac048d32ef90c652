"""N-best forced alignment on the GPU (ctc_amd_nbest_best_path, csrc/ctc_nbest_align.hip) against the float64
oracle tests/tools/viterbi_oracle.py, one hypothesis at a time.  The checks are those of tests/test_gpu_alignment.py, restated:
paths are never compared element-wise with the oracle's (ties may be broken differently); what is compared is validity (exact),
the value of the returned path against the oracle's optimum, and the score.

Tolerances (derived in tests/test_gpu_alignment.py, the project's, not new numbers):
  optimality  oracle optimum - value of the returned path <= 1e-6 absolute, both in float64.  The kernel's choice is exact in
              float64; reordering a T-term float64 sum costs about T * 2^-53 * |score| (5e-10 at T = 1000).
  score       |score - oracle| <= 1e-4 + 1e-6 * |score|: the project's absolute bar, plus a relative term for the float32
              rounding of the output (6e-8) and the float32 row statistics behind the log-sum-exps.
Every figure is printed before it is asserted (pytest -s shows them).

Blocks: the sweep runs in blocks of 16, 8, 4, 2, 1 frames and the back-trace in blocks of 64, 64, 32, 16, 8 frames for 1, 2, 4, 8, 16
label positions per lane.  Every T below crosses at least two blocks of both; the first shape, T = 40 in tests/test_gpu_alignment.py,
has T = 130 here for that reason (its walk block is 64 frames)."""
import math

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OPT_TOL = 1e-6
KIND_ID = {"classic": 0, "simplified": 1}
NAMES = ("score", "tokens", "label_index", "first_frame", "last_frame")


def score_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def needed_frames(kind, label):
    label = list(label)
    return len(label) + (sum(a == b for a, b in zip(label, label[1:])) if kind == "classic" else 0)


def make_inputs(kind, B, T, V, U, N, seed, scale=1.0, blank=0):
    """Ragged, feasible, per hypothesis: label_length in [U/2, U] (hypothesis (0, 0): U), logit_length from what the utterance's
    longest hypothesis needs up to T (utterance 0: T)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    labels = rng.integers(0, V - 1, (B, N, U)).astype(np.int32)
    labels += labels >= blank
    ll = rng.integers(U // 2, U + 1, (B, N)).astype(np.int32)
    ll[0, 0] = U
    tl = np.zeros(B, np.int32)
    for b in range(B):
        need = max(needed_frames(kind, labels[b, n, :ll[b, n]]) for n in range(N))
        assert need <= T
        tl[b] = rng.integers(max(need, T // 2), T + 1)
    tl[0] = T
    return x, labels, ll, tl


def data_cls(kind):
    import tf_seq2seq_losses_amd as ctc
    return ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData


def run(kind, wrt, x, labels, ll, tl, blank=0, U=None, mask=None):
    """The public functions.  x: a NumPy array or a device tensor (taken as it stands).  Returns the five outputs as NumPy arrays."""
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    labels, ll = np.asarray(labels, np.int32), np.asarray(ll, np.int32)
    args = (torch.from_numpy(labels).to(DEV), xt, torch.from_numpy(ll).to(DEV), torch.from_numpy(np.asarray(tl, np.int32)).to(DEV), blank)
    U = labels.shape[2] if U is None else U
    kw = dict(max_label_length=U, hypothesis_mask=None if mask is None else torch.from_numpy(np.asarray(mask)).to(DEV))
    if wrt:
        out = ctc.ctc_nbest_alignment_from_logproba(*args, data_cls(kind), **kw)
    else:
        out = (ctc.classic_ctc_nbest_alignment if kind == "classic" else ctc.simplified_ctc_nbest_alignment)(*args, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcNbestAlignment) and out._fields == NAMES
    B, N, T = labels.shape[0], labels.shape[1], xt.shape[1]
    assert out.score.shape == (B, N) and out.tokens.shape == out.label_index.shape == (B, N, T)
    assert out.first_frame.shape == out.last_frame.shape == (B, N, min(U, labels.shape[2]))
    assert out.score.dtype == torch.float32 and all(t.dtype == torch.int32 for t in out[1:])
    assert not any(t.requires_grad for t in out)
    return tuple(t.cpu().numpy() for t in out)


def same(a, b):
    return all(OW.same_bits(torch.from_numpy(np.ascontiguousarray(p)), torch.from_numpy(np.ascontiguousarray(q))) for p, q in zip(a, b))


def pick(got, n):
    """The outputs of list position(s) n of every utterance."""
    return tuple(a[:, n] for a in got)


def check_valid(kind, tokens, index, label, Tb, blank):
    """Exact: the path gives the label, label_index agrees with tokens and labels, -1 beyond the length."""
    label = [int(k) for k in label]
    assert np.all(tokens[Tb:] == -1) and np.all(index[Tb:] == -1)
    tok, idx = tokens[:Tb], index[:Tb]
    assert VO.reduces_to(kind, tok, blank) == label
    assert np.all(idx[tok == blank] == -1)
    nb = np.nonzero(tok != blank)[0]
    if not label:
        assert len(nb) == 0
        return
    seq = idx[nb]
    assert seq[0] == 0 and seq[-1] == len(label) - 1
    step = np.diff(seq)
    assert np.all((step == 0) | (step == 1))
    assert np.all(np.asarray(label)[seq] == tok[nb])
    if kind == "simplified":
        assert np.all(step == 1)  # every non-blank frame emits exactly one label
    else:
        assert np.all(np.diff(nb)[step == 0] == 1)  # the same label again only as an unbroken repeat


def frames_from_index(index, U):
    """first_frame / last_frame [.., U] recomputed on the host from label_index [.., T]: -1 where no frame has that index."""
    lead = index.shape[:-1]
    flat = index.reshape(-1, index.shape[-1])
    first = np.full((flat.shape[0], U), -1, np.int32)
    last = np.full((flat.shape[0], U), -1, np.int32)
    for r in range(flat.shape[0]):
        for t, i in enumerate(flat[r]):
            if i >= 0:
                if first[r, i] < 0:
                    first[r, i] = t
                last[r, i] = t
    return first.reshape(*lead, U), last.reshape(*lead, U)


def check_frames(kind, got, ll):
    """first_frame / last_frame are exactly what label_index says; -1 from label_length on and for an infeasible hypothesis."""
    score, _, index, first, last = got
    U = first.shape[-1]
    want_first, want_last = frames_from_index(index, U)
    assert np.array_equal(first, want_first) and np.array_equal(last, want_last)
    live = np.isfinite(score)[..., None] & (np.arange(U) < np.maximum(np.asarray(ll), 0)[..., None])
    assert np.all(first[~live] == -1) and np.all(last[~live] == -1)
    assert np.all(first[live] >= 0) and np.all(last[live] >= first[live])
    if kind == "simplified":
        assert np.array_equal(first, last)


def check_against_oracle(kind, wrt, x, labels, ll, tl, got, blank=0, what="", mask=None):
    """x: the float32 values the kernel read.  Every hypothesis against the oracle on labels[:, n]; returns (worst gap, worst error)."""
    score, tokens, index = got[:3]
    B, T = x.shape[0], x.shape[1]
    N = labels.shape[1]
    worst_gap, worst_err, bound = 0.0, 0.0, 1e-4
    for n in range(N):
        o_score, o_paths = VO.best_path(kind, labels[:, n], x, ll[:, n], tl, blank, wrt)
        for b in range(B):
            Tb = min(max(int(tl[b]), 0), T)
            if o_paths[b] is None or (mask is not None and not mask[b, n]):
                assert score[b, n] == -np.inf, (what, b, n, score[b, n])
                assert np.all(tokens[b, n] == -1) and np.all(index[b, n] == -1), (what, b, n)
                continue
            assert np.isfinite(score[b, n]), (what, b, n, score[b, n], o_score[b])
            check_valid(kind, tokens[b, n], index[b, n], labels[b, n, :max(int(ll[b, n]), 0)], Tb, blank)
            gap = o_score[b] - VO.path_score(x[b, :Tb], tokens[b, n, :Tb], wrt)
            err = abs(float(score[b, n]) - o_score[b])
            worst_gap, worst_err, bound = max(worst_gap, abs(gap)), max(worst_err, err), max(bound, float(score_tol(o_score[b])))
            assert -OPT_TOL <= gap <= OPT_TOL, (what, b, n, gap)
            assert err <= score_tol(o_score[b]), (what, b, n, score[b, n], o_score[b])
    print(f"NBEST-ALIGN-MEASURE {what}: worst optimality gap {worst_gap:.3e} (cap {OPT_TOL:.0e}), worst |score - oracle| {worst_err:.3e} "
          f"(bound {bound:.3e} at the largest |score|)", flush=True)
    if len(got) == 5:
        check_frames(kind, got, ll)
    return worst_gap, worst_err


def logprobs32(x):
    return VO.log_softmax64(x).astype(np.float32)


# (B, T, V, U, N): every boundary of the label positions per lane (U = 64 NL) and of the group of eight; see the header for T = 130
SHAPES = [(3, 130, 3, 1, 1), (2, 150, 256, 64, 8), (2, 160, 3, 65, 9), (2, 300, 1000, 128, 3), (2, 300, 256, 129, 8), (1, 600, 8192, 256, 2),
          (1, 600, 256, 257, 9), (1, 1100, 1000, 512, 2), (1, 1100, 3, 513, 8), (1, 2100, 256, 1024, 2)]
SHAPE_IDS = [f"B{s[0]}-T{s[1]}-V{s[2]}-U{s[3]}-N{s[4]}" for s in SHAPES]


# ---- 1. against the oracle (and 2.: every call's first_frame / last_frame against its own label_index) ----
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U,N", SHAPES, ids=SHAPE_IDS)
def test_against_the_oracle(B, T, V, U, N, kind, wrt):
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=1000 * U + V + wrt)
    if wrt:
        x = logprobs32(x)
    got = run(kind, wrt, x, labels, ll, tl)
    check_against_oracle(kind, wrt, x, labels, ll, tl, got, what=f"{kind} wrt={wrt} B={B} T={T} V={V} U={U} N={N}")


# ---- 2. first_frame and last_frame ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_first_and_last_frame(kind):
    """Recomputed on the host from the returned label_index they match exactly; padding is -1.  Few tokens, so that the classic
    path has long runs, repeats with a blank between them and runs that cross the edges of the 64-frame walk blocks."""
    B, T, V, U, N = 3, 200, 4, 20, 9
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=23)
    ll[1, 2], ll[2, 0], ll[2, 1] = 0, 1, -3
    x[:, :, 0] -= 1.0  # blanks are dear: labels stretch over many frames
    got = run(kind, 0, x, labels, ll, tl)
    check_against_oracle(kind, 0, x, labels, ll, tl, got, what=f"{kind} frames")  # (calls check_frames)
    score, tokens, index, first, last = got
    assert np.all(first[1, 2] == -1) and np.all(last[2, 1] == -1) and first[2, 0, 0] >= 0 and np.all(first[2, 0, 1:] == -1)
    runs = (last - first)[first >= 0]
    print(f"NBEST-ALIGN-MEASURE {kind} frames: longest run {int(runs.max()) + 1} frames, {int((runs > 0).sum())} of {runs.size} labels "
          f"on more than one frame", flush=True)
    if kind == "classic":
        assert runs.max() > 0
    # NULL first_frame / last_frame / label_index: the other outputs keep their bits
    for drop in (("first_frame",), ("last_frame",), ("label_index", "first_frame", "last_frame")):
        r = raw_call(kind, 0, torch.from_numpy(x).to(DEV), labels, ll, tl, 0, U, drop=drop)
        for name, a in zip(NAMES, got):
            if name not in drop:
                assert OW.same_bits(r[name].cpu(), torch.from_numpy(a)), (drop, name)


# ---- 3. agreement with the existing call ----
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U,N", SHAPES[1:5], ids=SHAPE_IDS[1:5])
def test_agreement_with_the_alignment_call(B, T, V, U, N, kind):
    """tokens[:, n] and label_index[:, n] equal those of classic_ctc_alignment / simplified_ctc_alignment on labels[:, n], element
    for element.  A mismatch is excused only by a genuine tie (the two paths' raw-logit sums, math.fsum in float64, exactly equal),
    and on continuous random float32 values the number of excused hypotheses must be 0."""
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=77 + U)
    got = run(kind, 0, x, labels, ll, tl)
    fn = ctc.classic_ctc_alignment if kind == "classic" else ctc.simplified_ctc_alignment
    xt, tlt = torch.from_numpy(x).to(DEV), torch.from_numpy(tl).to(DEV)
    excused, worst = 0, 0.0
    for n in range(N):
        ref = fn(torch.from_numpy(labels[:, n].copy()).to(DEV), xt, torch.from_numpy(ll[:, n].copy()).to(DEV), tlt, 0, max_label_length=U)
        r_score, r_tok, r_idx = (a.cpu().numpy() for a in ref)
        for b in range(B):
            if not (np.array_equal(got[1][b, n], r_tok[b]) and np.array_equal(got[2][b, n], r_idx[b])):
                Tb = int(tl[b])
                mine = math.fsum(float(x[b, t, got[1][b, n, t]]) for t in range(Tb))
                theirs = math.fsum(float(x[b, t, r_tok[b, t]]) for t in range(Tb))
                assert mine == theirs, (kind, b, n, mine, theirs)
                excused += 1
        err = np.abs(got[0][:, n].astype(np.float64) - r_score)
        worst = max(worst, float((err / score_tol(r_score)).max()))
        assert np.all(err <= score_tol(r_score)), (kind, n, got[0][:, n], r_score)
    print(f"NBEST-ALIGN-MEASURE {kind} B={B} T={T} V={V} U={U} N={N} against the one-hypothesis call: {excused} hypotheses excused by a "
          f"tie (cap 0), worst score difference / bound {worst:.3e}", flush=True)
    assert excused == 0


# ---- 4. isolation, bit for bit ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_isolation(kind):
    rng = np.random.default_rng(5)
    B, T, V, N, U = 2, 150, 8, 9, 12
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=31, scale=1.5)
    base = run(kind, 0, x, labels, ll, tl)
    check_against_oracle(kind, 0, x, labels, ll, tl, base, what=f"isolation {kind}")
    for n in range(N):  # alone
        assert same(run(kind, 0, x, labels[:, n:n + 1], ll[:, n:n + 1], tl), pick(base, slice(n, n + 1))), n
    for s in range(1, N):  # every hypothesis at every position
        got = run(kind, 0, x, np.roll(labels, s, axis=1), np.roll(ll, s, axis=1), tl)
        assert same(got, tuple(np.roll(a, s, axis=1) for a in base)), s
    perm = rng.permutation(N)
    assert same(run(kind, 0, x, labels[:, perm], ll[:, perm], tl), pick(base, perm))
    # the five malformed neighbours of tests/test_gpu_nbest_loss.py: their own result is the contract's, the others keep their bits
    empty = run(kind, 0, x, labels[:, :1], np.zeros((B, 1), np.int32), tl)
    k = 3
    others = [n for n in range(N) if n != k]
    for name, tok, length in (("blank", 0, None), ("minus one", -1, None), ("V", V, None), ("too long", None, U + 1), ("negative", None, -2)):
        lab2, ll2 = labels.copy(), ll.copy()
        if tok is not None:
            lab2[:, k, 0] = tok
        if length is not None:
            ll2[:, k] = length
        got = run(kind, 0, x, lab2, ll2, tl)
        assert same(pick(got, others), pick(base, others)), name
        if name == "negative":
            assert same(pick(got, slice(k, k + 1)), empty) and np.all(np.isfinite(got[0][:, k])), name
        else:
            assert np.all(got[0][:, k] == -np.inf), (name, got[0][:, k])
            assert all(np.all(a[:, k] == -1) for a in got[1:]), name


# ---- 5. formats ----
def format_views(xt):
    B, T, V = xt.shape
    yield "bfloat16", xt.to(torch.bfloat16)
    yield "float16", xt.to(torch.float16)
    yield "time-major float32", xt.transpose(0, 1).contiguous().transpose(0, 1)
    yield "time-major bfloat16", xt.to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1)
    yield "padded rows, odd stride (element-wise)", OW.strided_storage(xt, T * (V + 3) + 5, V + 3, 0xFF)[1]
    if V % 4 == 0:
        yield "padded rows, stride V + 4 (vector)", OW.strided_storage(xt, T * (V + 4), V + 4, 0xFF)[1]
    yield "padded rows float16", OW.strided_storage(xt.to(torch.float16), T * (V + 3) + 5, V + 3, 0xFF)[1]


@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U,N,blank,scale", [(2, 150, 256, 64, 8, 0, 1.0), (2, 150, 37, 50, 5, 17, 4.0)], ids=["V256", "V37-blank17-sharp"])
def test_formats(kind, B, T, V, U, N, blank, scale):
    """bfloat16, float16, time-major and padded-row inputs give what float32 of the same (rounded) values gives: the conversions
    are exact, so the chains see the same numbers -- the same paths bit for bit -- and the score agrees within its tolerance."""
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=9, scale=scale, blank=blank)
    xt = torch.from_numpy(x).to(DEV)
    for name, xin in format_views(xt):
        assert not (xin.dtype == torch.float32 and xin.is_contiguous()), name
        x32 = xin.float().contiguous()
        got = run(kind, 0, xin, labels, ll, tl, blank)
        ref = run(kind, 0, x32, labels, ll, tl, blank)
        assert same(got[1:], ref[1:]), name
        assert np.all(np.abs(got[0] - ref[0]) <= score_tol(ref[0])), (name, got[0], ref[0])
        print(f"NBEST-ALIGN-MEASURE {kind} {name}: score bits {'equal' if same(got[:1], ref[:1]) else 'differ'}", flush=True)
        if name in ("bfloat16", "padded rows, odd stride (element-wise)"):
            check_against_oracle(kind, 0, x32.cpu().numpy(), labels, ll, tl, got, blank, what=f"{kind} V={V} {name}")
    check_against_oracle(kind, 0, x, labels, ll, tl, run(kind, 0, xt, labels, ll, tl, blank), blank, what=f"{kind} V={V} float32")


# ---- 6. edges ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_edges(kind):
    B, T, V, N, U = 4, 70, 12, 5, 6
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=13)
    tl[1] = 0                                   # no frames: score 0 for an empty hypothesis, -inf otherwise
    ll[1, 0], ll[1, 1] = 0, -1
    ll[0, 1], ll[0, 2] = 0, -5                  # the all-blank path
    tl[2] = 5                                   # too few frames by one
    labels[2, 0, :6] = [3, 3, 4, 5, 6, 7] if kind == "classic" else [3, 4, 5, 6, 7, 8]
    ll[2, 0] = 5 if kind == "classic" else 6    # classic: five labels, one repeat: six frames; simplified: six labels
    labels[2, 1, :5], ll[2, 1] = [3, 4, 5, 6, 7], 5  # ... and beside it one that just fits
    ll[2, 2:] = 2
    x[3, 9, :] = -np.inf                        # a frame that is -inf everywhere
    tl[0] = T + 1000                            # clamps to T
    got = run(kind, 0, x, labels, ll, tl)
    check_against_oracle(kind, 0, x, labels, ll, tl, got, what=f"{kind} edges")
    score, tokens, index, first, last = got
    assert np.array_equal(np.isfinite(score[1]), [True, True, False, False, False]) and score[1, 0] == 0.0 and score[1, 1] == 0.0
    assert np.all(tokens[0, 1] == 0) and np.all(index[0, 1] == -1) and np.all(tokens[0, 2] == 0) and np.all(first[0, 1:3] == -1)
    assert score[2, 0] == -np.inf and np.isfinite(score[2, 1]) and np.array_equal(first[2, 1, :5], np.arange(5))
    assert np.all(score[3] == -np.inf) and all(np.all(a[3] == -1) for a in got[1:])
    # label_length > U: a static bound below some lengths
    cut = run(kind, 0, x, labels, ll, tl, U=4)
    for b in range(B):
        for n in range(N):
            if ll[b, n] > 4:
                assert cut[0][b, n] == -np.inf and all(np.all(a[b, n] == -1) for a in cut[1:])
            else:
                assert cut[0][b, n].tobytes() == score[b, n].tobytes() and np.array_equal(cut[1][b, n], tokens[b, n])
                assert np.array_equal(cut[2][b, n], index[b, n]) and np.array_equal(cut[3][b, n], first[b, n, :4])
    # empty shapes
    import tf_seq2seq_losses_amd as ctc
    z = ctc.classic_ctc_nbest_alignment(torch.zeros((0, 3, 2), dtype=torch.int32, device=DEV), torch.zeros((0, 4, 3), device=DEV),
                                        torch.zeros((0, 3), dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert z.score.shape == (0, 3) and z.tokens.shape == (0, 3, 4) and z.first_frame.shape == (0, 3, 2)
    z = ctc.simplified_ctc_nbest_alignment(torch.ones((2, 2, 2), dtype=torch.int32, device=DEV), torch.zeros((2, 0, 3), device=DEV),
                                           torch.tensor([[2, 0], [0, 1]], dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert z.tokens.shape == (2, 2, 0) and z.score.cpu().tolist() == [[-np.inf, 0.0], [0.0, -np.inf]] and bool((z.first_frame == -1).all())


@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_beam_decoding_goes_in_as_it_stands(kind):
    """The -1 padding of a real beam search output fed straight in with hypothesis_mask = isfinite(score): masked entries come out
    infeasible and every live hypothesis passes the oracle checks."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, NB = 3, 80, 6, 8
    rng = np.random.default_rng(41)
    x = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([T, 1, 47], np.int32)  # one frame and two candidate tokens: three hypotheses at the most, five are missing
    xt, tlt = torch.from_numpy(x).to(DEV), torch.from_numpy(tl).to(DEV)
    beam = ctc.classic_ctc_beam_search if kind == "classic" else ctc.simplified_ctc_beam_search
    dec = beam(xt, tlt, 0, beam_width=NB, top_k=2, nbest=NB)
    mask = torch.isfinite(dec.score)
    fn = ctc.classic_ctc_nbest_alignment if kind == "classic" else ctc.simplified_ctc_nbest_alignment
    out = fn(dec.labels, xt, dec.label_length, tlt, 0, hypothesis_mask=mask)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in out)
    labels, ll, m = dec.labels.cpu().numpy(), dec.label_length.cpu().numpy(), mask.cpu().numpy()
    assert labels.shape == (B, NB, T) and not m.all() and m[:, 0].all() and (labels == -1).any()
    assert np.all(got[0][~m] == -np.inf) and all(np.all(a[~m] == -1) for a in got[1:])
    safe = np.where(labels < 0, 1, labels)  # (the oracle slices by label_length and never reads the padding; -1 would still be refused)
    check_against_oracle(kind, 0, x, safe, ll, tl, got[:3], what=f"{kind} beam decoding", mask=m)
    want_first, want_last = frames_from_index(got[2], got[3].shape[-1])
    assert np.array_equal(got[3], want_first) and np.array_equal(got[4], want_last)


# ---- 7. ownership and garbage ----
GUARD = 64


def raw_call(kind, wrt, xt, labels, ll, tl, blank, U, fill=0xA5, ws_pattern=0xFF, drop=()):
    """The C ABI with every buffer under the test's control: outputs inside guard bands, all prefilled with the byte `fill`, the
    workspace with `ws_pattern`.  Returns {name: tensor} of the outputs (None for those in `drop`, passed as NULL)."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.asarray(labels, np.int32)).to(DEV)
    llt = torch.from_numpy(np.asarray(ll, np.int32)).to(DEV)
    tlt = torch.from_numpy(np.asarray(tl, np.int32)).to(DEV)
    B, T, V = xt.shape
    N, W = lab.shape[1], lab.shape[2]
    sizes = dict(score=B * N, tokens=B * N * T, label_index=B * N * T, first_frame=B * N * U, last_frame=B * N * U)
    bufs = {k: OW.filled((n + 2 * GUARD,), torch.float32 if k == "score" else torch.int32, fill, DEV) for k, n in sizes.items()}
    ws = OW.byte_fill(_lib.nbest_best_path_workspace_bytes(KIND_ID[kind], B, T, V, U, N), ws_pattern, DEV)
    ptr = {k: None if k in drop else bufs[k][GUARD:].data_ptr() for k in sizes}
    rc = lib.ctc_amd_nbest_best_path(KIND_ID[kind], wrt, xt.data_ptr(), {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[xt.dtype],
                                     xt.stride(0), xt.stride(1), lab.data_ptr(), W, llt.data_ptr(), tlt.data_ptr(), blank, B, T, V, U, N,
                                     ptr["score"], ptr["tokens"], ptr["label_index"], ptr["first_frame"], ptr["last_frame"],
                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    out = {}
    shapes = dict(score=(B, N), tokens=(B, N, T), label_index=(B, N, T), first_frame=(B, N, U), last_frame=(B, N, U))
    for k, n in sizes.items():
        assert bool(OW.keeps_prefill(bufs[k][:GUARD], fill).all()) and bool(OW.keeps_prefill(bufs[k][GUARD + n:], fill).all()), ("guards", k)
        if k in drop:
            assert bool(OW.keeps_prefill(bufs[k], fill).all()), k
            out[k] = None
        else:
            out[k] = bufs[k][GUARD:GUARD + n].clone().view(shapes[k])
    return out


def same_outputs(a, b):
    return all(OW.same_bits(a[k], b[k]) for k in NAMES)


@pytest.mark.parametrize("kind", VO.KINDS)
def test_unowned_memory_changes_no_bit(kind):
    B, T, V, U, N = 3, 150, 8, 12, 9
    x, labels, ll, tl = make_inputs(kind, B, T, V, U + 1, N, seed=19)
    W = U + 1
    ll = np.minimum(ll, U).astype(np.int32)
    ll[1, 1], ll[2, 2], tl[1] = 0, -2, 77
    xt, lab = torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV)
    clean = raw_call(kind, 0, xt, lab, ll, tl, 0, U, fill=0x00, ws_pattern=0x00)
    check_against_oracle(kind, 0, x, labels, ll, tl, tuple(clean[k].cpu().numpy() for k in NAMES), what=f"ownership {kind}")
    for value in OW.poison_values(torch.float32):  # frames beyond logit_length
        assert same_outputs(raw_call(kind, 0, OW.poison_padding(xt, tl, value), lab, ll, tl, 0, U), clean), value
    poisoned = OW.poison_labels(lab.view(B * N, W), ll.reshape(-1), OW.label_poison_cycle(V, 0)).view(B, N, W)
    assert same_outputs(raw_call(kind, 0, xt, poisoned, ll, tl, 0, U), clean), "label tails"
    for sb, st in ((T * (V + 3) + 5, V + 3), (V + 4, B * (V + 4))):  # padded rows; time-major with padded rows
        storage, view, owned = OW.strided_storage(xt, sb, st)
        for value in OW.poison_values(torch.float32):  # between V and the row stride
            gaps = OW.poison_gaps(storage, owned, value).as_strided((B, T, V), (sb, st, 1))
            assert same_outputs(raw_call(kind, 0, gaps, lab, ll, tl, 0, U), clean), (sb, st, value)
    for pattern in OW.BYTE_PATTERNS:  # the outputs' contents on entry and every workspace prefill (0xFF among them)
        assert same_outputs(raw_call(kind, 0, xt, lab, ll, tl, 0, U, fill=pattern, ws_pattern=pattern), clean), pattern
    # everything at once
    nan = float("nan")
    storage, view, owned = OW.strided_storage(OW.poison_padding(xt, tl, nan), T * (V + 3) + 5, V + 3)
    gaps = OW.poison_gaps(storage, owned, nan).as_strided((B, T, V), (T * (V + 3) + 5, V + 3, 1))
    assert same_outputs(raw_call(kind, 0, gaps, poisoned, ll, tl, 0, U, fill=0xA5, ws_pattern=0xFF), clean), "all at once"


# ---- 8. graph capture ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_in_a_hip_graph(kind):
    """One launch on one stream: captured once and replayed twice on changed inputs in the same buffers, the bits of the eager call."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U, N = 3, 90, 64, 20, 5
    x = torch.zeros((B, T, V), device=DEV)
    labels = torch.ones((B, N, U), dtype=torch.int32, device=DEV)
    ll = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    outs = [torch.zeros((B, N), device=DEV)] + [torch.zeros((B, N, d), dtype=torch.int32, device=DEV) for d in (T, T, U, U)]
    ws = torch.zeros(max(_lib.nbest_best_path_workspace_bytes(KIND_ID[kind], B, T, V, U, N), 1), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_nbest_best_path(KIND_ID[kind], _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), U, ll.data_ptr(),
                                         tl.data_ptr(), 0, B, T, V, U, N, *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(seed):
        h = make_inputs(kind, B, T, V, U, N, seed)
        for dst, src in zip((x, labels, ll, tl), h):
            dst.copy_(torch.from_numpy(src))
        return h

    def read():
        res = tuple(o.cpu().numpy().copy() for o in outs)
        for o in outs:
            o.zero_()
        return res

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
        read()
        g.replay()
        torch.cuda.synchronize()
        got = read()
        call()
        torch.cuda.synchronize()
        assert same(got, read()), seed
        check_against_oracle(kind, 0, *h, got, what=f"{kind} graph replay seed {seed}")


# ---- 9. determinism ----
@pytest.mark.parametrize("kind", VO.KINDS)
def test_two_runs_are_bit_identical(kind):
    B, T, V, U, N = 2, 300, 1000, 128, 8
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, N, seed=17)
    a = run(kind, 0, x, labels, ll, tl)
    b = run(kind, 0, x, labels, ll, tl)
    assert same(a, b) and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    # quarter steps: plenty of exact ties between paths; the choice among them is the same every run
    xq = np.round(x * 4) / 4
    a = run(kind, 0, xq, labels, ll, tl)
    b = run(kind, 0, xq, labels, ll, tl)
    assert same(a, b)
    check_against_oracle(kind, 0, xq, labels, ll, tl, a, what=f"{kind} tied logits")
