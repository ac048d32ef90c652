"""The wildcard and long-form alignment kernels along the axes their own modules hold at one point: the vocabulary (more than one
round of the V-wide row pass, whole and partial last groups, the documented limit of 16384), the blank index, and rows whose
maximum is attained by several columns.  ctc_amd_wildcard_best_path (plain instantiation, csrc/ctc_align_wild.hip),
ctc_amd_long_wildcard_best_path (csrc/ctc_align_long_wild.hip), ctc_amd_long_best_path and ctc_amd_long_label_posterior are compared
with the float64 oracles tests/tools/wildcard_oracle.py, viterbi_oracle.py, greedy_oracle.py and label_posterior_oracle.py.  Inputs,
runners, acceptors and bars are those of tests/test_gpu_wildcard_alignment.py, test_gpu_long_alignment.py,
test_gpu_long_wildcard_alignment.py, test_gpu_long_label_posterior.py and tests/_ownership.py (imported, not copied).  Every input
is drawn once per process and kept read-only.  Every case runs on both lattices.

The row pass gives lane l the columns 4l .. 4l + 3 of round 0, the same + 256 in round 1, and so on: column c sits in lane
(c mod 256) // 4 and round c // 256.

Host conditions, asserted before the GPU call:
  A1, B1, C  no label inside label_length is the blank; the forced wildcards are where the case says (B1, C: positions 1023 and
             1024); C: the oracle finds every utterance feasible
  A2, B3     the layouts take the access path they are meant to take (the kernel's own test, restated on the host)
  A3, B2     on the float32 image of what the kernel reads: every frame's maximum is strictly above x[t, blank]; every planted
             frame has at least two columns equal to its maximum; the other frames have exactly one, at a column >= 256; the
             planted frames' lowest columns fall in at least 4 lanes and 2 rounds
  A4         the oracle's score is finite for every utterance; some frame has every column 1024 .. 1029 at -inf and some frame
             has all of round 0 but the blank and the labels at -inf
A3 and B2 use blank = 2: with the blank at 0 the planted set {0, 256} would make the blank a row maximum, which the first
condition forbids; 2 is in no planted set.  An eighth set, {40, 1000}, is planted beside the seven because at V = 1028 the seven
lowest columns (255, 8, 3, 1026, 1, 259, 0) fall in three lanes only.

Bars: those of the imported modules, none changed.  Optimality gap 1e-6; score, label_score and sum(label_score) + blanks
1e-4 + 1e-6 |.|; posteriors 1e-4 per element, duration and expected frame 1e-4 T_b; everything called "bits" is exact.

Worst figures measured on an MI355X, both lattices (bar):
  A1  float32, four shapes       optimality gap 0 (1e-6), |score - oracle| 1.1e-5, |label_score - float64| 7.6e-6,
                                 |sum(label_score) + blanks - score| 2.2e-5 (1e-4 + 1e-6 |.|)
  A1  16-bit and time-major      gap 0, score 1.4e-5, label_score 1.9e-6, sum 8.1e-6; against float32 on the rounded values: 0
                                 elements of the path and the per-label frames differ, |score - that call's| 0
  A2  five layouts               0 elements differ from the contiguous call in any output
  A3  ties, 16 cases             0 frames off label 0, 0 tokens differ from the lowest index (32 tied frames a case) and from
                                 greedy decoding, |score - float64| 8.8e-6
  A4  rows 52 % -inf             gap 0, score 2.4e-6, label_score 0, sum 1.4e-6
  B1  four cases                 gap 0, score 4.8e-4 (9.3e-3 at the largest |score|), label_score 6.1e-5, sum 4.8e-4; 39 .. 86 frames
                                 an utterance outside any label, each reported as the blank; frames_per_tile 4 against the
                                 default: 0 elements differ, |score - default| 0, |score - oracle| 3.2e-4
  B2  ties, 32 cases             0 tokens differ, |score - float64| 2.7e-5, 0 elements differ from the short-form call, score included
  B3  five layouts               0 elements differ
  C   long alignment             gap 3.6e-12, |score - oracle| 4.5e-4 (8.7e-3)
  C   long label posteriors      label 3.4e-6, blank 3.0e-6, peak 3.4e-6, row sum 3.4e-6 (1e-4 each), duration 4.6e-4, expected
                                 frame 6.3e-5 (1.15e-1 = 1e-4 T_b), peak_frame 0 of 1829 compared differ, 1 left out; the four
                                 per-position outputs are the host reduction's bits and loss has the bits of *_long_loss
No case exceeded a bar and no defect was found.

With value-only mistakes planted in two scratch builds (no index changed, nothing able to fault), each run once on an MI355X with
this module and the three existing alignment modules (tests/test_gpu_wildcard_alignment.py, test_gpu_long_alignment.py,
test_gpu_long_wildcard_alignment.py; 216 cases), these failed:
  build X, 58 cases, none in the existing modules
    1  the long wildcard row pass stops after its first round (c += V)        B1 (all 16), B2 (all 32)
    3  the short wildcard element-wise path drops column k + 1 of a partial   A1 at V = 1030 on logits (2; the column is the
       group from round 1 on (k + 1 < V - (k >= 256))                         blank and only the log-sum-exp misses it), A3 at
                                                                              V = 1030 (all 8; a frame's only maximum is there)
  build Y, 70 cases, 2 of them in the existing modules
    2  both files: among tied columns from 64 on the highest wins             A3 (all 16), B2 (all 32), test_a1_producer_formats
                                                                              (all 4) and the existing short-form module's
                                                                              test_producer_formats_read_in_place (both): rounding
                                                                              to 16 bits makes equal maxima at V = 260 and 1028
    4  the long wildcard back-trace reports blank & 1023 on blank frames      B1 (all 16)
Broader forms of 2 and 4 (offering lane * 4; token 0) fail the existing modules at once, and the pad test k + 3 < V never decides
at V = 1030, so these narrower ones were planted.  A4, B3 and C failed under none of them: A4 has
no maximum in the dropped column, B3 compares the mutated kernel with itself, and C runs other units."""
import functools

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_long_alignment as GL
from tests import test_gpu_long_label_posterior as LPL
from tests import test_gpu_long_wildcard_alignment as LW
from tests import test_gpu_wildcard_alignment as WA
from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO
from tests.tools import wildcard_oracle as WO

pytestmark = pytest.mark.gpu

DEV = WA.DEV
W = WA.W
KINDS = VO.KINDS
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
POISON = 0xFF  # a NaN in every element type


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def no_blank_in_labels(labels, ll, blank):
    for b in range(len(ll)):
        assert not np.any(labels[b, :ll[b]] == blank), b


def lane_of(c):
    return (c % 256) // 4


def round_of(c):
    return c // 256


def takes_vector_path(x):
    """The kernels' own test: 16 bytes of float32 or 8 bytes of 16-bit elements per access need aligned rows."""
    return ((x.shape[2] | x.stride(0) | x.stride(1)) & 3) == 0 and x.data_ptr() % (16 if x.dtype == torch.float32 else 8) == 0


def layouts(xt):
    """name -> (a [B, T, V] view of the same values, whether it takes the vector path).  V must be a multiple of 4.  The gaps
    between V and a row stride hold NaN."""
    B, T, V = xt.shape
    assert V % 4 == 0 and xt.dtype == torch.float32 and xt.is_contiguous()
    out = {"contiguous": (xt, True)}
    off = torch.zeros(xt.numel() + 1, device=xt.device)[1:].view(xt.shape).copy_(xt)
    out["base 4 bytes off"] = (off, False)
    storage, view, _ = OW.strided_storage(xt, T * (V + 4), V + 4, POISON)
    out[f"row stride {V + 4}"] = (view, True)
    shifted = OW.filled((storage.numel() + 1,), xt.dtype, POISON, xt.device)
    shifted[1:].copy_(storage)
    out[f"row stride {V + 4}, base 4 bytes off"] = (shifted[1:].as_strided(view.shape, view.stride()), False)
    out[f"row stride {V + 3}"] = (OW.strided_storage(xt, T * (V + 3), V + 3, POISON)[1], False)
    for name, (v, vec) in out.items():
        assert takes_vector_path(v) == vec, name
        assert torch.equal(v, xt), name
    return out


def count_diff(a, b, names):
    """{name: elements whose bits differ} between two tuples of NumPy outputs in the order of LW.NAMES."""
    res = {}
    for name in names:
        k = LW.NAMES.index(name)
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, name
        res[name] = int((a[k].view(np.int32) != b[k].view(np.int32)).sum())
    return res


# ---- A1: the short-form wildcard alignment beyond one round of the row pass ----

A1_SHAPES = [(2, 40, 1028, 12, 1027),    # the vector path, five rounds, the blank in the last column
             (2, 40, 1030, 12, 1029),    # element-wise, the last group: two columns and two pads
             (2, 88, 2052, 64, 1024),
             (1, 24, 16384, 8, 16383)]   # 64 full rounds: the documented limit of V


@functools.lru_cache(maxsize=None)
def a1_input(kind, shape, wrt):
    B, T, V, U, blank = shape
    x, labels, ll, tl = WA.make_inputs(kind, B, T, V, U, seed=7000 + V + U, blank=blank)
    if wrt:
        x = WA.logprobs32(x)
    return frozen(x, labels, ll, tl)


def a1_host(shape, labels, ll):
    B, T, V, U, blank = shape
    no_blank_in_labels(labels, ll, blank)
    assert labels[0, 0] == W and labels[0, U - 1] == W and ll[0] == U


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", A1_SHAPES, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}-U{s[3]}-blank{s[4]}" for s in A1_SHAPES])
def test_a1_short_form_against_the_oracle(shape, kind, wrt):
    x, labels, ll, tl = a1_input(kind, shape, wrt)
    a1_host(shape, labels, ll)
    got = WA.run(kind, wrt, x, labels, ll, tl, shape[4])
    o_score = WA.check(kind, wrt, x, labels, ll, tl, got, shape[4], what=f"A1 {kind} wrt={wrt} {shape}")
    assert np.all(np.isfinite(o_score)), o_score


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_a1_producer_formats(kind, wrt):
    """bfloat16, float16 and time-major storage at V = 1028: the path of float32 on the converted values, bit for bit, and the
    bars against the oracle on the float32 image of what the kernel read."""
    shape = A1_SHAPES[0]
    x, labels, ll, tl = a1_input(kind, shape, wrt)
    a1_host(shape, labels, ll)
    blank = shape[4]
    xt = WA.dev(x)
    tm = xt.transpose(0, 1).contiguous().transpose(0, 1)
    tm16 = xt.to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1)
    assert tm.stride() == (shape[2], shape[0] * shape[2], 1)
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16)), ("time-major float32", tm),
                      ("time-major bfloat16", tm16)):
        x32 = xin.float().contiguous()
        got = WA.run(kind, wrt, xin, labels, ll, tl, blank)
        ref = WA.run(kind, wrt, x32, labels, ll, tl, blank)
        diff = count_diff(got, ref, LW.NAMES[1:5])
        print(f"AXES A1 {kind} wrt={wrt} {name}: elements that differ from float32 on the same values {diff}, "
              f"|score - that call's| {np.abs(got[0] - ref[0]).max():.3e}", flush=True)
        assert not any(diff.values()), (name, diff)
        assert np.all(np.abs(got[0] - ref[0]) <= 2 * WA.score_tol(ref[0])), (name, got[0], ref[0])
        WA.check(kind, wrt, x32.cpu().numpy(), labels, ll, tl, got, blank, what=f"A1 {kind} wrt={wrt} {name}")


# ---- A2: vector and element-wise rows, five rounds ----

@pytest.mark.parametrize("kind", KINDS)
def test_a2_vector_and_element_wise_rows_agree(kind):
    shape = A1_SHAPES[0]
    x, labels, ll, tl = a1_input(kind, shape, 0)
    a1_host(shape, labels, ll)
    views = layouts(WA.dev(x))
    assert sum(vec for _, vec in views.values()) >= 2 and sum(not vec for _, vec in views.values()) >= 3
    ref = WA.run(kind, 0, views["contiguous"][0], labels, ll, tl, shape[4])
    for name, (v, vec) in views.items():
        diff = count_diff(WA.run(kind, 0, v, labels, ll, tl, shape[4]), ref, LW.NAMES)
        print(f"AXES A2 {kind} {name} ({'vector' if vec else 'element-wise'}): elements that differ from the contiguous call {diff}",
              flush=True)
        assert not any(diff.values()), (name, diff)


# ---- A3 / B2: rows whose maximum several columns attain ----

TIE_BLANK = 2
TIE_WIDTH = 1100  # B2: the width of the label tensor, two label blocks


def tie_sets(V):
    return [(255, 260),        # the lowest index in the highest lane, against round 1 of lane 1
            (8, 300),          # round 0 against round 1
            (3, 4),            # neighbouring lanes
            (V - 2, V - 1),    # the partial last group (V = 1030), the last two of a whole one (V = 1028)
            (1, V - 1),
            (259, 515, 771),   # one lane, three rounds, offset by 3
            (0, 256),          # one lane, two rounds, offset by 0
            (40, 1000)]        # a fourth lane for the lowest column at V = 1028


def tie_frames(T, b):
    """Per column set two frames of utterance b: 7 apart from either end, so that they fall on every frame slot of a producer."""
    return [(1 + 7 * i + b, T - 2 - 7 * i - b) for i in range(8)]


@functools.lru_cache(maxsize=None)
def tie_logits(T, V):
    """N(0, 1) logits with (row maximum + 1), rounded to bfloat16, on the planted columns of the planted frames and on one column
    >= 256 of every other frame: the edges of the rounds and of the last group first (V - 1, V - 2, 256, 1023, 1024, V - 3), then
    random ones.  Returns (x[2, T, V], {(b, t): columns})."""
    rng = np.random.default_rng(9000 + T + V)
    x = rng.standard_normal((2, T, V)).astype(np.float32)
    top = torch.from_numpy(x.max(axis=-1) + 1.0).to(torch.bfloat16).float().numpy()
    plan = {}
    for b in range(2):
        for cols, frames in zip(tie_sets(V), tie_frames(T, b)):
            for t in frames:
                assert (b, t) not in plan and 0 <= t < T
                plan[(b, t)] = cols
        edges = [V - 1, V - 2, 256, 1023, 1024, V - 3]
        for t in range(T):
            cols = plan.get((b, t)) or ((edges.pop(0),) if edges else (int(rng.integers(256, V)),))
            x[b, t, list(cols)] = top[b, t]
    return frozen(x)[0], plan


@functools.lru_cache(maxsize=None)
def tie_case(T, V, dtype, wrt):
    """(the CPU tensor the kernel reads, its float32 image, the plan) with the host conditions asserted."""
    x, plan = tie_logits(T, V)
    if wrt:
        x = WA.logprobs32(x)
    xt = torch.tensor(x).to(DTYPES[dtype])  # (a copy: the shared logits stay read-only)
    x32 = xt.float().numpy()
    top = x32.max(axis=-1)
    assert TIE_BLANK not in {c for cols in plan.values() for c in cols}
    assert np.all(top > x32[:, :, TIE_BLANK])
    lowest = set()
    for b in range(2):
        for t in range(T):
            at = np.nonzero(x32[b, t] == top[b, t])[0]
            if (b, t) in plan:
                assert len(at) >= 2 and tuple(at) == plan[(b, t)], (b, t, at)
                lowest.add(int(at[0]))
            else:
                assert len(at) == 1 and at[0] >= 256, (b, t, at)
    assert len({lane_of(c) for c in lowest}) >= 4 and len({round_of(c) for c in lowest}) >= 2, sorted(lowest)
    assert len(plan) == 2 * 2 * len(tie_sets(V))  # every set on two frames of either utterance
    return xt, frozen(x32)[0], plan


def greedy_tokens(kind, wrt, xt, tl, blank):
    import tf_seq2seq_losses_amd as ctc
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        dec = ctc.ctc_greedy_decode_from_logproba(xt, WA.dev(tl), blank, cls)
    else:
        dec = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(xt, WA.dev(tl), blank)
    torch.cuda.synchronize()
    return dec.tokens.cpu().numpy()


def check_ties(what, kind, wrt, got, xt_dev, x32, tl, plan):
    """label_index is 0 on every frame, the tokens are the lowest column at the maximum and those of greedy decoding, the score is
    the float64 sum of max - lse."""
    score, tokens, index, first, last, label_score = got
    B, T = x32.shape[:2]
    want = np.stack([WO.argmax_tokens(x32[b]) for b in range(B)])
    ref = GO.decode(kind, x32, tl, TIE_BLANK, wrt)
    assert np.array_equal(ref.tokens, want)
    dec = greedy_tokens(kind, wrt, xt_dev, tl, TIE_BLANK)
    lp = np.asarray(x32, np.float64) if wrt else VO.log_softmax64(x32)
    value = np.take_along_axis(lp, want[:, :, None], 2)[:, :, 0].sum(axis=1)
    planted = np.zeros((B, T), bool)
    for b, t in plan:
        planted[b, t] = True
    err = np.abs(score - value)
    print(f"AXES {what}: frames off label 0: {int((index != 0).sum())}; tokens that differ from the lowest index: "
          f"{int((tokens != want)[planted].sum())} of {int(planted.sum())} tied frames, {int((tokens != want)[~planted].sum())} of the "
          f"others; from greedy decoding: {int((tokens != dec).sum())}; |score - float64| {err.max():.3e} "
          f"(bound {WA.score_tol(value).min():.3e})", flush=True)
    assert np.all(index == 0)
    assert np.array_equal(tokens, want)
    assert tokens.dtype == dec.dtype and tokens.tobytes() == dec.tobytes()
    assert np.all(err <= WA.score_tol(value)), (score, value)
    assert np.all(first[:, 0] == 0) and np.all(last[:, 0] == T - 1)
    assert np.all(np.abs(label_score[:, 0] - value) <= WA.score_tol(value))


TIE_PARAMS = [pytest.param(V, dtype, wrt, id=f"V{V}-{dtype}-wrt{wrt}") for V in (1030, 1028) for dtype in ("float32", "bfloat16")
              for wrt in (0, 1)]


@pytest.mark.parametrize("V,dtype,wrt", TIE_PARAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_a3_tied_row_maxima_short_form(kind, V, dtype, wrt):
    T = 64
    xt, x32, plan = tie_case(T, V, dtype, wrt)
    labels, ll, tl = np.full((2, 1), W, np.int32), np.ones(2, np.int32), np.full(2, T, np.int32)
    xd = xt.to(DEV)
    got = WA.run(kind, wrt, xd, labels, ll, tl, TIE_BLANK)
    check_ties(f"A3 {kind} V={V} {dtype} wrt={wrt}", kind, wrt, got, xd, x32, tl, plan)


@pytest.mark.parametrize("V,dtype,wrt", TIE_PARAMS)
@pytest.mark.parametrize("T", [64, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_b2_tied_row_maxima_long_form(kind, T, V, dtype, wrt):
    """... and every output has the bits of the short-form call (one label block: the same recursion, the same row pass; the frames'
    log-sum-exps are added in float64 in another order, which one rounding to float32 hides)."""
    xt, x32, plan = tie_case(T, V, dtype, wrt)
    labels, ll, tl = np.full((2, TIE_WIDTH), 5, np.int32), np.ones(2, np.int32), np.full(2, T, np.int32)
    labels[:, 0] = W
    xd = xt.to(DEV)
    got = LW.run(kind, wrt, xd, labels, ll, tl, TIE_BLANK, max_label_length=TIE_WIDTH)
    assert got[3].shape == (2, TIE_WIDTH)
    check_ties(f"B2 {kind} T={T} V={V} {dtype} wrt={wrt}", kind, wrt, got, xd, x32, tl, plan)
    short = WA.run(kind, wrt, xd, labels[:, :1].copy(), ll, tl, TIE_BLANK)
    diff = count_diff(got[:3] + tuple(np.ascontiguousarray(a[:, :1]) for a in got[3:]), short, LW.NAMES)
    print(f"AXES B2 {kind} T={T} V={V} {dtype} wrt={wrt}: elements that differ from the short-form call {diff}", flush=True)
    assert not any(diff.values()), diff
    assert np.all(got[3][:, 1:] == -1) and np.all(got[4][:, 1:] == -1) and np.all(got[5][:, 1:] == -np.inf)


# ---- A4: rows that are partly -inf, as log-probabilities ----

A4_SHAPE = (2, 40, 1030, 12, 0)


@functools.lru_cache(maxsize=None)
def a4_input(kind):
    B, T, V, U, blank = A4_SHAPE
    x, labels, ll, tl = WA.make_inputs(kind, B, T, V, U, seed=7400, blank=blank)
    x = WA.logprobs32(x)
    rng = np.random.default_rng(7401)
    for b in range(B):
        free = np.ones(V, bool)
        free[blank] = False
        free[[k for k in labels[b, :ll[b]] if k >= 0]] = False
        for t in range(T):
            gone = free & (rng.random(V) < 0.5)
            if t % 5 == 1:
                gone[1024:] = free[1024:]   # the whole last round, a partial group included
            if t % 5 == 3:
                gone[:256] = free[:256]     # all of round 0: every lane but the blank's and the labels' starts at -inf
            x[b, t, gone] = -np.inf
    return frozen(x, labels, ll, tl)


@pytest.mark.parametrize("kind", KINDS)
def test_a4_rows_that_are_partly_minus_infinity(kind):
    B, T, V, U, blank = A4_SHAPE
    x, labels, ll, tl = a4_input(kind)
    no_blank_in_labels(labels, ll, blank)
    used = {int(k) for b in range(B) for k in labels[b, :ll[b]] if k >= 0} | {blank}
    assert not any(k >= 1024 for k in used) and np.any(np.all(np.isneginf(x[:, :, 1024:]), axis=2))
    r0 = [k for k in range(256) if k not in used]
    assert len(r0) >= 240 and np.any(np.all(np.isneginf(x[:, :, r0]), axis=2))
    share = np.isneginf(x).mean()
    assert 0.45 < share < 0.65, share
    o_score = WO.best_path(kind, labels, x, ll, tl, blank, 1)[0]
    assert np.all(np.isfinite(o_score)), o_score
    got = WA.run(kind, 1, x, labels, ll, tl, blank)
    WA.check(kind, 1, x, labels, ll, tl, got, blank, what=f"A4 {kind} {100 * share:.0f} % -inf")


# ---- B1: the long-form wildcard alignment beyond one round of the row pass ----

B1_CASES = {
    "V1030": dict(shape=(2, 1300, 1030, 1030, 1029), ll=(1030, 900), tl=(1300, 1200), wild=((0, 1023, 1024, 1029), (450, 899)), seed=71),
    "V1028": dict(shape=(1, 1100, 1028, 1026, 1027), ll=(1026,), tl=(1100,), wild=((0, 1023, 1024, 1025),), seed=72),
    "V4100": dict(shape=(1, 1100, 4100, 1026, 2048), ll=(1026,), tl=(1100,), wild=((0, 1023, 1024, 1025),), seed=73),  # 17 rounds, the last partial
}
B1_PARAMS = [("V1030", "float32"), ("V1028", "float32"), ("V1028", "bfloat16"), ("V4100", "float32")]


@functools.lru_cache(maxsize=None)
def b1_input(name, wrt):
    c = B1_CASES[name]
    B, T, V, U, blank = c["shape"]
    x, labels, ll, tl = LW.wild_input(B, T, V, U, c["ll"], c["tl"], c["seed"], c["wild"], blank)
    if wrt:
        x = WA.logprobs32(x)
    return frozen(x, labels, ll, tl)


def b1_host(name, labels, ll):
    blank = B1_CASES[name]["shape"][4]
    no_blank_in_labels(labels, ll, blank)
    assert labels[0, 1023] == W and labels[0, 1024] == W and ll[0] > 1025


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,dtype", B1_PARAMS, ids=[f"{n}-{d}" for n, d in B1_PARAMS])
def test_b1_long_form_against_the_oracle(name, dtype, kind, wrt):
    x, labels, ll, tl = b1_input(name, wrt)
    b1_host(name, labels, ll)
    blank = B1_CASES[name]["shape"][4]
    xin = WA.dev(x).to(DTYPES[dtype])
    x32 = x if dtype == "float32" else xin.float().cpu().numpy()
    got = LW.run(kind, wrt, xin, labels, ll, tl, blank)
    o_score = WA.check(kind, wrt, x32, labels, ll, tl, got, blank, what=f"B1 long {kind} wrt={wrt} {name} {dtype}")
    assert np.all(np.isfinite(o_score)), o_score
    blanks = [int((got[2][b, :tl[b]] < 0).sum()) for b in range(len(tl))]  # (check_admissible: every one of them reports `blank`)
    print(f"AXES B1 long {kind} wrt={wrt} {name} {dtype}: frames outside any label, reported as token {blank}: {blanks}", flush=True)
    assert min(blanks) > 0
    if name == "V1030":  # frames_per_tile 4: label blocks 1+ read m_t of hundreds of earlier launches
        small = LW.run(kind, wrt, xin, labels, ll, tl, blank, tf=4)
        diff = count_diff(got, small, LW.INVARIANT)
        print(f"AXES B1 long {kind} wrt={wrt} {name} frames_per_tile=4: elements that differ from the default {diff}, "
              f"|score - default| {np.abs(small[0] - got[0]).max():.3e}, |score - oracle| {np.abs(small[0] - o_score).max():.3e}", flush=True)
        assert not any(diff.values()), diff
        assert np.all(np.abs(small[0] - got[0]) <= WA.score_tol(got[0])) and np.all(np.abs(small[0] - o_score) <= WA.score_tol(o_score))


# ---- B3: vector and element-wise rows through the long entry point ----

@pytest.mark.parametrize("kind", KINDS)
def test_b3_vector_and_element_wise_rows_agree_long_form(kind):
    x, labels, ll, tl = b1_input("V1028", 0)
    b1_host("V1028", labels, ll)
    blank = B1_CASES["V1028"]["shape"][4]
    views = layouts(WA.dev(x))
    ref = LW.run(kind, 0, views["contiguous"][0], labels, ll, tl, blank)
    for name, (v, vec) in views.items():
        diff = count_diff(LW.run(kind, 0, v, labels, ll, tl, blank), ref, LW.NAMES)
        print(f"AXES B3 long {kind} {name} ({'vector' if vec else 'element-wise'}): elements that differ from the contiguous call {diff}",
              flush=True)
        assert not any(diff.values()), (name, diff)


# ---- C: the plain long-form alignment and the long-form label posteriors ----

C_ALIGN = {"V1030-float32": dict(shape=(2, 1300, 1030, 1030, 1029), ll=(1030, 900), tl=(1300, 1200), seed=81, dtype="float32"),
           "V1028-bfloat16": dict(shape=(1, 1100, 1028, 1026, 1027), ll=(1026,), tl=(1100,), seed=82, dtype="bfloat16")}


@functools.lru_cache(maxsize=None)
def c_align_input(name):
    """(the CPU tensor the kernel reads, its float32 image, labels, ll, tl)."""
    c = C_ALIGN[name]
    B, T, V, U, blank = c["shape"]
    x, labels, ll, tl = GL.random_input(B, T, V, U, c["ll"], c["tl"], c["seed"], blank)
    xt = torch.from_numpy(x).to(DTYPES[c["dtype"]])
    return (xt,) + frozen(xt.float().numpy(), labels, ll, tl)


@functools.lru_cache(maxsize=None)
def c_align_oracle(name, kind):
    _, x32, labels, ll, tl = c_align_input(name)
    return VO.best_path(kind, labels, x32, ll, tl, C_ALIGN[name]["shape"][4])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(C_ALIGN))
def test_c_long_alignment(name, kind):
    xt, x32, labels, ll, tl = c_align_input(name)
    blank = C_ALIGN[name]["shape"][4]
    no_blank_in_labels(labels, ll, blank)
    oracle = c_align_oracle(name, kind)
    assert np.all(np.isfinite(oracle[0])), oracle[0]
    got = GL.run(kind, 0, xt.to(DEV), labels, ll, tl, blank)
    gap, err = GL.check(kind, 0, x32, labels, ll, tl, oracle, got, blank, what=f"C {kind} {name}")
    print(f"AXES C long alignment {kind} {name}: worst optimality gap {gap:.3e}, worst |score - oracle| {err:.3e}", flush=True)


C_POST = dict(shape=(2, 1300, 1030, 1030, 1029), ll=(1030, 800), tl=(1300, 1150), wild=((1023, 1024), (5,)), seed=83)


@functools.lru_cache(maxsize=None)
def c_post_input():
    B, T, V, U, blank = C_POST["shape"]
    return frozen(*LPL.make(B, T, V, U, C_POST["ll"], C_POST["tl"], seed=C_POST["seed"], blank=blank, wild=C_POST["wild"]))


@pytest.mark.parametrize("kind", KINDS)
def test_c_long_label_posterior(kind):
    x, labels, ll, tl = c_post_input()
    blank = C_POST["shape"][4]
    no_blank_in_labels(labels, ll, blank)
    assert labels[0, 1023] == W and labels[0, 1024] == W
    ref = LPL.oracle(kind, 0, x, labels, ll, tl, blank=blank, key=("axes C", kind))
    assert np.isfinite(ref[0]).all(), ref[0]
    out = LPL.run(kind, 0, x, labels, ll, tl, blank=blank)
    LPL.compare(f"AXES C {kind} V=1030 blank={blank}", out, ref, ll, tl)
    LPL.check_definition(f"AXES C {kind} V=1030", out, ll, tl)
    loss = LPL.long_loss(kind, 0, x, labels, ll, tl, blank=blank)
    print(f"AXES C long label posterior {kind}: losses whose bits differ from the long-form loss: {OW.count_diff(out[0], loss)}", flush=True)
    assert OW.same_bits(out[0], loss)
