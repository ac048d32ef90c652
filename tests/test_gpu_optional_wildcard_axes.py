"""The optional-wildcard kernels along the axes that tests/test_gpu_optional_wildcard.py and tests/test_gpu_long_optional_wildcard.py
hold at one point: the vocabulary and the blank index, d_loss, the width of the label tensor with hostile tails, and ownership
(poisoned padding frames, row strides).  Every `OPT = true` instantiation (short and long form; loss, gradient, label posteriors,
alignment) is compared with tests/tools/optional_wildcard_oracle.py, which tests/test_optional_wildcard_oracle.py pins at a blank
of V - 1 and with a weighted gradient.  Inputs, runners, bit comparison and checks are those two modules' own and those of
tests/_ownership.py (imported, not copied).  Every input is drawn once per process and kept, read-only, with its oracle result;
before any GPU call the host asserts that no label inside label_length is the blank and that the oracle's loss is finite exactly
for the utterances meant to be feasible.

Bars: those of the two modules.  Loss and score 1e-4 + 1e-6 |.|; gradient, posterior and blank posterior 1e-4 per element; duration
and expected frame as `check` of either module has them; a bfloat16 gradient 1e-4 + 2^-8 (short form, its test_formats), a 16-bit
gradient 1e-4 + 2^-8 |oracle| (long form, its test_formats_strides_and_blank); a weighted gradient 1e-4 max(1, |d_loss[b]|).  Zero
rows, widths and ownership: bits.

Worst errors measured on an MI355X, both lattices (bar):
  a. short form, blank 17 / 66       loss 1.9e-5 (1e-4 + 1e-6 |loss|), gradient 8.9e-7, posterior 8.2e-7, blank 3.4e-7 (1e-4 each),
                                     duration 1.6e-5 against the oracle (1e-4 T), expected frame 1.2e-5 against the oracle
  a. V = 1028 / 1030, float32        loss 1.6e-5, gradient 3.4e-7, posterior 4.2e-7, blank 2.5e-7, duration 2.5e-6, expected frame 1.8e-6
  a. V = 1028, bfloat16              gradient 1.9e-3 (4.0e-3), loss 6.7e-6, posterior 2.3e-7, blank 3.1e-7
  a. alignment, every case           optimality gap 0 (1e-6), |score - oracle| 2.7e-5, |label_score - float64| 3.8e-6 (1e-4 + 1e-6 |.|)
  b. long form, blank 17             loss 8.9e-5 (5e-3), gradient 1.5e-6, posterior 1.5e-6, blank 1.4e-6 (1e-4 each), duration 1.1e-5
                                     (1e-4 max(1, oracle)), expected frame 6.2e-5 (1e-4 max(1, oracle) / min(1, duration))
  b. long form, V = 1028             loss 2.6e-4 (7e-3), gradient 9.8e-7, blank 4.1e-7, duration 4.6e-6, expected frame 6.2e-5
  c. d_loss 2.5 / -1.5, short form   gradient 6.8e-7 / 4.7e-7 (2.5e-4 / 1.5e-4)
  c. the same, long form             gradient 2.9e-6 / 2.8e-6; float16 9.8e-4 / 4.9e-4 (2.5e-4 / 1.5e-4 plus 2^-8 |oracle|)
  c. d_loss 0, NaN, +inf             +0 in every element; the loss has the bits of the call without d_loss
Every bit comparison of c., d. and e. held exactly.  Before the fix in the OPT row stages that came with this module, the row with
d_loss = 0 held 0 * g, that is -0 wherever g is negative.

With one-line mistakes planted in a scratch build (each in an OPT = true path), these tests failed and the two existing modules
did not:
  the short-form row stage adds the blank's share only in the first column pass    test_two_column_passes_short_form (all six)
  the long-form row stage drops the bins of the second column pass                 test_two_column_passes_long_form (both)
  the short-form row stage writes infeasible rows as d_loss * 0                    test_d_loss_short_form (both)
  the short-form adjacent-pair test reads position L (i + 1 <= L)                  test_label_width_and_hostile_tails_short_form (both)
The four were planted together in one build: each reaches only the inputs of the tests named beside it (V > 1024 in the short or
the long form, a non-finite d_loss on an infeasible row, -3 at position L beside an owned -3), and those twelve cases were the
only failures; all 132 cases of the two existing modules passed on that build."""
import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_long_optional_wildcard as TL
from tests import test_gpu_optional_wildcard as TS
from tests.tools import optional_wildcard_oracle as OO

pytestmark = pytest.mark.gpu
KINDS = OO.KINDS
W, Q = OO.WILDCARD, OO.OPTIONAL
WEIGHT = TS.WEIGHT
DEV = TS.DEV
SHORT = [((2, 88, 37, 64), 17), ((2, 169, 67, 129), 66)]  # ((B, T, V, U), blank): V odd, no multiple of 4; V beyond a wavefront, NL = 4
TWO_PASS = [((2, 40, 1028, 12), 1027, torch.float32), ((2, 40, 1028, 12), 1027, torch.bfloat16), ((2, 40, 1030, 12), 1029, torch.float32)]
LONG_MAIN = (2, 1400, 37, 1030, 17)  # B, T, V, U, blank
D_LOSS = np.array([2.5, 0.0, -1.5, np.nan, np.inf], np.float32)  # rows 3 and 4 are infeasible
FEASIBLE = np.array([True, True, True, False, False])
PAD = 7
FILL = 0xA5

_INPUTS, _REFS = {}, {}


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def logp(x):
    return torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()


def short_ref(key, kind, wrt, x64, labels, ll, tl, blank, d_loss=None):
    """The oracle's (loss, grad, label_posterior, blank_posterior, duration, expected_frame), once per key."""
    if key not in _REFS:
        ref = OO.loss_and_grad(kind, wrt, labels, x64, ll, tl, blank, WEIGHT, d_loss) + OO.label_posterior(kind, wrt, labels, x64, ll, tl, blank, WEIGHT)[1:]
        _REFS[key] = frozen(*ref)
    return _REFS[key]


def host_checks(labels, ll, blank, ref_loss, feasible=None):
    """What must hold before a GPU call."""
    for b in range(len(ll)):
        assert not np.any(labels[b, :ll[b]] == blank), b
    want = np.ones(len(ll), bool) if feasible is None else np.asarray(feasible)
    assert np.array_equal(np.isfinite(ref_loss), want) and np.all(ref_loss[~want] == np.inf), ref_loss


def report(what, **errs):
    print(f"AXES {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items()), flush=True)


def short_errors(ref, got):
    loss, grad, post, blk, dur, exf = ref
    fin = np.isfinite(loss)
    sure = dur > 1e-3
    return dict(loss=np.abs(got["loss"].numpy()[fin] - loss[fin]).max(initial=0.0),
                grad=np.abs(got["grad"].float().numpy() - grad).max(initial=0.0),
                posterior=np.abs(got["p_label_posterior"].numpy() - post).max(initial=0.0),
                blank=np.abs(got["p_blank_posterior"].numpy() - blk).max(initial=0.0),
                duration=np.abs(got["p_duration"].numpy() - dur).max(initial=0.0),
                expected_frame=np.abs(got["p_expected_frame"].numpy() - exf)[sure].max(initial=0.0))


def long_errors(ref, got):
    fin = np.isfinite(ref["loss"])
    out = dict(loss=np.abs(got["loss"].numpy()[fin] - ref["loss"][fin]).max(initial=0.0),
               grad=np.abs(got["grad"].float().numpy() - ref["grad"]).max(initial=0.0))
    if "p_blank_posterior" in got:
        sure = ref["dur"] > 1e-3
        out.update(blank=np.abs(got["p_blank_posterior"].numpy() - ref["blk"]).max(initial=0.0),
                   duration=np.abs(got["p_duration"].numpy() - ref["dur"]).max(initial=0.0),
                   expected_frame=np.abs(got["p_expected_frame"].numpy() - ref["exf"])[sure].max(initial=0.0))
    if "p_label_posterior" in got:
        out["posterior"] = np.abs(got["p_label_posterior"].numpy() - ref["post"]).max(initial=0.0)
    return out


def check_blank_frames(got, tl, blank, what):
    """Frames the alignment reports as blank carry the token `blank`, and there are such frames."""
    tokens, index = got["tokens"].numpy(), got["label_index"].numpy()
    n = 0
    for b in range(len(tl)):
        free = index[b, :tl[b]] < 0
        n += int(free.sum())
        assert np.all(tokens[b, :tl[b]][free] == blank), (what, b)
    assert n > 0, what


def zero_bits(t):
    """Every element is +0, bit for bit."""
    return not bool(OW.bits(t.contiguous()).any())


# ---- a. vocabulary and blank, the short form ----

def short_input(kind, case, wrt):
    """The input of SHORT[case] on a lattice, as tests/test_gpu_optional_wildcard.py draws it: utterance 0 ends in an optional
    wildcard, utterance 1 in an ordinary label and has fewer frames than T."""
    key = ("short", kind, case, wrt)
    if key not in _INPUTS:
        (B, T, V, U), blank = SHORT[case]
        for seed in range(5000 + 10 * U + wrt, 6000 + 10 * U, 2):  # the first draw that is all of this
            x, labels, ll, tl = TS.draw(kind, B, T, V, U, seed=seed, blank=blank)
            if labels[1, ll[1] - 1] >= 0 and ll[1] < U and tl[1] < T and any(np.any(labels[b, :ll[b]] == 0) for b in range(B)):
                break
        assert any(np.any(labels[b, :ll[b]] == 0) for b in range(B))  # the column a blank of 0 would have taken is a label's
        assert ll[0] == U and labels[0, U - 1] == Q and labels[1, ll[1] - 1] >= 0 and ll[1] < U and tl[1] < T
        if wrt:
            x = logp(x)
        _INPUTS[key] = frozen(x, labels, ll, tl)
    return _INPUTS[key]


def check_short(kind, wrt, x, labels, ll, tl, blank, key, what, grad_tol=1e-4):
    """Loss, gradient, label posteriors and alignment of one input against the oracle.  x: numpy float32, or a CPU tensor of a 16-bit
    type (the oracle then reads the values the kernel reads)."""
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x)
    x64, x32 = xt.double().numpy(), xt.float().numpy()
    ref = short_ref(key, kind, wrt, x64, labels, ll, tl, blank)
    host_checks(labels, ll, blank, ref[0])
    xd = xt.to(DEV)
    got = TS.run_all(kind, wrt, xd, labels, ll, tl, blank=blank)
    report(what, **short_errors(ref, got))
    TS.check(kind, wrt, x64, labels, ll, tl, got, what, blank=blank, grad_tol=grad_tol, ref=ref)
    al = TS.run_align(kind, wrt, xd, labels, ll, tl, blank=blank)
    o_score = TS.check_align(kind, wrt, x32, labels, ll, tl, al, what + " alignment", blank=blank)
    assert np.all(np.isfinite(o_score))
    check_blank_frames(al, tl, blank, what)
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(SHORT)), ids=lambda c: "x".join(map(str, SHORT[c][0])) + f"-blank{SHORT[c][1]}")
def test_vocabulary_and_blank_short_form(kind, case):
    shape, blank = SHORT[case]
    for wrt in (0, 1):
        x, labels, ll, tl = short_input(kind, case, wrt)
        check_short(kind, wrt, x, labels, ll, tl, blank, ("short", kind, case, wrt), f"a. {kind} {shape} blank={blank} wrt={wrt}")


def two_pass_input(kind, V, blank):
    """U = 12, V beyond one column pass of the row stage.  Utterance 0: label tokens on both sides of column 1024, a mandatory
    wildcard and four optional ones."""
    key = ("two pass", kind, V)
    if key not in _INPUTS:
        x, labels, ll, tl = TS.draw(kind, 2, 40, V, 12, seed=5200 + V, blank=blank)
        labels[0, 1:4] = [3, 1025, W]
        labels[0, 5] = 1026
        labels[1, 1] = 1024
        # utterance 1 has no wildcard, every frame and three frames that are sure of the blank: the best path has blank frames
        # (a wildcard's emission is the frame's maximum, so beside wildcards a path need not hold any)
        wild = np.nonzero(labels[1] < 0)[0]
        labels[1, wild] = 2 + wild
        tl[1] = 40
        x[1, :3, blank] += 10.0
        lab0 = labels[0, :ll[0]]
        assert ll[0] == 12 and ll[1] >= 6 and np.any((lab0 >= 0) & (lab0 < 1024)) and np.any(lab0 >= 1024)
        assert np.sum(lab0 == W) >= 1 and np.sum(lab0 == Q) >= 2 and not np.any((lab0[1:] == Q) & (lab0[:-1] == Q))
        _INPUTS[key] = frozen(x, labels, ll, tl)
    return _INPUTS[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(TWO_PASS)), ids=lambda c: f"V{TWO_PASS[c][0][2]}-{str(TWO_PASS[c][2]).split('.')[1]}")
def test_two_column_passes_short_form(kind, case):
    """V = 1028: the float32 vector path and, as bfloat16, the 16-bit vector stores; V = 1030: the element-wise path.  The blank is
    the last column of the second pass."""
    (B, T, V, U), blank, dtype = TWO_PASS[case]
    x, labels, ll, tl = two_pass_input(kind, V, blank)
    xt = torch.from_numpy(x).to(dtype)
    grad_tol = 1e-4 if dtype == torch.float32 else 1e-4 + 2.0 ** -8
    got = check_short(kind, 0, xt, labels, ll, tl, blank, ("two pass", kind, V, dtype), f"a. {kind} V={V} blank={blank} {dtype}", grad_tol)
    assert got["grad"].dtype == dtype


# ---- b. vocabulary and blank, the long form ----

def long_input(where):
    """T = 1400, V = 37, U = 1030, blank 17.  Utterance 0 has full length and every frame, ends in an ordinary label and holds -3 at
    1023, or at 1022 and 1024 (`where`); utterance 1 has label_length 1024, exactly one label block, with -3 at 1023, and 1333 frames."""
    key = ("long", where)
    if key not in _INPUTS:
        B, T, V, U, blank = LONG_MAIN
        x, labels, ll, tl = TL.draw(B, T, U, seed=5100, ll=[U, 1024], tl=[T, 1333], V=V, blank=blank)
        labels[0, U - 1] = 5
        TL.put(labels, 0, [1023] if where == "1023" else [1022, 1024], V=V, blank=blank)
        TL.put(labels, 1, [1023], V=V, blank=blank)
        assert labels[0, U - 1] >= 0 and labels[1, 1023] == Q and np.any(labels == 0)
        _INPUTS[key] = frozen(x, labels, ll, tl)
    return _INPUTS[key]


def long_ref(kind, where):
    x, labels, ll, tl = long_input(where)
    ref = TL.oracle(f"axes long {where}", kind, 0, x.astype(np.float64), labels, ll, tl, blank=LONG_MAIN[4])
    host_checks(labels, ll, LONG_MAIN[4], ref["loss"])
    return ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["1023", "1022+1024"])
def test_vocabulary_and_blank_long_form(kind, where):
    blank = LONG_MAIN[4]
    x, labels, ll, tl = long_input(where)
    ref = long_ref(kind, where)
    got = TL.run(kind, 0, x, labels, ll, tl, blank=blank)
    report(f"b. {kind} long blank={blank} -3 at {where}", **long_errors(ref, got))
    TL.check(ref, got, tl, f"{kind} long blank={blank} -3 at {where}")
    ck = TL.run(kind, 0, x, labels, ll, tl, blank=blank, checkpoint=True, post=False)
    TL.same_bits(ck, got, ["loss", "grad"])


def wide_input(kind):
    """T = 1100 (classic: 1200), V = 1028, U = 1026, blank 1027: two column passes of the long-form row stage, the blank in the last
    column of the second; token 0 and a token >= 1024 in both label blocks."""
    key = ("wide", kind)
    if key not in _INPUTS:
        T, V, U, blank = (1200 if kind == "classic" else 1100), 1028, 1026, 1027
        x, labels, ll, tl = TL.draw(1, T, U, seed=5150, V=V, blank=blank)
        labels[0, 10:12] = [0, 1025]
        labels[0, 1024:1026] = [0, 1026]
        _INPUTS[key] = frozen(x, labels, ll, tl) + (blank,)
    return _INPUTS[key]


@pytest.mark.parametrize("kind", KINDS)
def test_two_column_passes_long_form(kind):
    x, labels, ll, tl, blank = wide_input(kind)
    for lo, hi in ((0, 1024), (1024, 1026)):
        assert np.any(labels[0, lo:hi] == 0) and np.any(labels[0, lo:hi] >= 1024)
    ref = TL.oracle("axes wide", kind, 0, x.astype(np.float64), labels, ll, tl, blank=blank)
    host_checks(labels, ll, blank, ref["loss"])
    got = TL.run(kind, 0, x, labels, ll, tl, blank=blank, dense=False)
    assert "p_label_posterior" not in got and "p_duration" in got
    report(f"b. {kind} long V=1028 blank={blank}", **long_errors(ref, got))
    TL.check(ref, got, tl, f"{kind} long V=1028 blank={blank}")


# ---- c. d_loss ----

def weighted_ref(key, kind, x64, labels, ll, tl):
    """(loss, gradient weighted by D_LOSS) of the oracle, once per key; the host checks of the batch of five."""
    if key not in _REFS:
        _REFS[key] = frozen(*OO.loss_and_grad(kind, 0, labels, x64, ll, tl, 0, WEIGHT, D_LOSS))
        lab4 = labels[4, :ll[4]]  # one frame short: with one more it is feasible
        assert np.isfinite(OO.posteriors_one(kind, lab4, x64[4, :tl[4] + 1], 0, 0, WEIGHT)[0])
    loss, grad = _REFS[key]
    host_checks(labels, ll, 0, loss, FEASIBLE)
    assert not np.isnan(grad).any() and not grad[3].any() and not grad[4].any() and not grad[1].any()
    lab3 = labels[3, :ll[3]]
    assert np.any((lab3[1:] == Q) & (lab3[:-1] == Q)) and tl[3] >= TS.need_frames(kind, lab3)
    return loss, grad


def check_weighted(ref, got, plain, what, rel=0.0):
    """`got` with D_LOSS against the oracle's weighted gradient; `plain`: the same call without d_loss."""
    o_loss, o_grad = ref
    loss, grad = got["loss"].numpy(), got["grad"].float().numpy().astype(np.float64)
    assert np.array_equal(np.isfinite(loss), FEASIBLE) and np.all(loss[~FEASIBLE] == np.inf), (what, loss)
    TS.same_bits(got, plain, ["loss"])  # the loss is unaffected by d_loss
    worst = {}
    for b in range(5):
        if not FEASIBLE[b] or D_LOSS[b] == 0.0:
            assert zero_bits(got["grad"][b]), (what, b)  # +0 in every element
            continue
        e = np.abs(grad[b] - o_grad[b])
        worst[f"d_loss={D_LOSS[b]}"] = e.max()
        assert np.all(e <= 1e-4 * max(1.0, abs(float(D_LOSS[b]))) + rel * np.abs(o_grad[b])), (what, b, e.max())
        assert grad[b].any() and abs(loss[b] - o_loss[b]) <= TS.tol(o_loss[b]), (what, b)
    report(what, **worst)


def d_loss_short_input(kind):
    key = ("d_loss short", kind)
    if key not in _INPUTS:
        x, labels, ll, tl = TS.draw(kind, 5, 89, 8, 65, seed=5300)
        i = int(ll[3]) // 2
        labels[3, i] = labels[3, i + 1] = Q
        tl[3] = 89
        tl[4] = TS.need_frames(kind, labels[4, :ll[4]]) - 1
        _INPUTS[key] = frozen(x, labels, ll, tl)
    return _INPUTS[key]


@pytest.mark.parametrize("kind", KINDS)
def test_d_loss_short_form(kind):
    x, labels, ll, tl = d_loss_short_input(kind)
    ref = weighted_ref(("d_loss short", kind), kind, x.astype(np.float64), labels, ll, tl)
    got = TS.run_all(kind, 0, x, labels, ll, tl, d_loss=D_LOSS)
    plain = TS.run_all(kind, 0, x, labels, ll, tl)
    check_weighted(ref, got, plain, f"c. {kind} short d_loss")
    raw = TS._raw_calls(kind, x, labels, ll, tl, 0xFF, d_loss=D_LOSS)  # the C entry point with the d_loss pointer: the same bits
    TS.same_bits(got, raw, ["loss", "grad"])


def d_loss_long_input(kind):
    """B = 5, T = 1300, U = 1030: the adjacent pair of utterance 3 straddles the label-block boundary (1023, 1024)."""
    key = ("d_loss long", kind)
    if key not in _INPUTS:
        x, labels, ll, tl = TL.draw(5, 1300, 1030, seed=5400)
        labels[3, 1023] = labels[3, 1024] = Q
        labels[3, 1022] = labels[3, 1025] = 2
        tl[4] = TS.need_frames(kind, labels[4]) - 1
        _INPUTS[key] = frozen(x, labels, ll, tl)
    return _INPUTS[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_d_loss_long_form(kind, dtype):
    """float16: the weighted value passes through the 16-bit store."""
    x, labels, ll, tl = d_loss_long_input(kind)
    xt = torch.from_numpy(x).to(dtype)
    ref = weighted_ref(("d_loss long", kind, dtype), kind, xt.double().numpy(), labels, ll, tl)
    xd = xt.to(DEV)
    got = TL.run(kind, 0, xd, labels, ll, tl, d_loss=D_LOSS, post=False)
    assert got["grad"].dtype == dtype
    TL.same_bits(TL.run(kind, 0, xd, labels, ll, tl, d_loss=D_LOSS, checkpoint=True, post=False), got)
    plain = TL.run(kind, 0, xd, labels, ll, tl, post=False)
    check_weighted(ref, got, plain, f"c. {kind} long d_loss {dtype}", rel=0.0 if dtype == torch.float32 else 2.0 ** -8)


# ---- d. the width of the label tensor and hostile tails ----

def widened(labels, ll, V, blank, hostile):
    """labels in a tensor PAD positions wider.  hostile: every position from label_length[b] on, inside the original width too,
    holds -3 first, then the blank, -2, -1, V + 5, INT32_MIN, INT32_MAX, repeating; otherwise the new columns hold a token."""
    B, U = labels.shape
    out = np.full((B, U + PAD), 1 if blank != 1 else 2, np.int32)
    out[:, :U] = labels
    if hostile:
        cycle = [blank, W, -1, V + 5, OW.INT32_MIN, OW.INT32_MAX]
        for b in range(B):
            L = int(ll[b])
            out[b, L] = Q
            out[b, L + 1:] = [cycle[j % len(cycle)] for j in range(U + PAD - L - 1)]
            assert np.array_equal(out[b, :L], labels[b, :L])
    return out


# what include/ctc_amd.h says of label positions from label_length on, as check_align and check of the two modules assert it
BEYOND = {"p_label_posterior": 0.0, "p_duration": 0.0, "p_expected_frame": -1.0, "p_peak_posterior": 0.0, "p_peak_frame": -1,
          "a_first_frame": -1, "a_last_frame": -1, "a_label_score": -np.inf}


def check_widths(call, labels, ll, V, blank, what):
    """call(labels, max_label_length) -> dict of outputs.  The hostile tensor gives the bits of the clean one of the same width at
    every bound; at the true maximum those are the bits of the labels as drawn; positions from label_length on hold BEYOND."""
    U = labels.shape[1]
    clean, bad = widened(labels, ll, V, blank, False), widened(labels, ll, V, blank, True)
    assert int(max(ll)) == U
    drawn = call(labels, None)
    assert np.isfinite(drawn["loss"].numpy()).all(), what
    for bound in (None, U, U + PAD):
        got = call(bad, bound)
        TS.same_bits(call(clean, bound), got)
        if bound == U:
            TS.same_bits(drawn, got)
        for k, fill in BEYOND.items():
            if k in got:
                assert got[k].shape[-1] == (U + PAD if bound == U + PAD else U) or bound is None, (what, bound, k)
                for b in range(len(ll)):
                    assert torch.all(got[k][b][..., int(ll[b]):] == fill), (what, bound, k, b)


@pytest.mark.parametrize("kind", KINDS)
def test_label_width_and_hostile_tails_short_form(kind):
    (B, T, V, U), blank = SHORT[0]
    x, labels, ll, tl = short_input(kind, 0, 0)
    host_checks(labels, ll, blank, short_ref(("short", kind, 0, 0), kind, 0, x.astype(np.float64), labels, ll, tl, blank)[0])

    def call(lab, bound):
        kw = {} if bound is None else {"max_label_length": bound}
        out = TS.run_all(kind, 0, x, lab, ll, tl, blank=blank, **kw)
        out.update({"a_" + k: v for k, v in TS.run_align(kind, 0, x, lab, ll, tl, blank=blank, **kw).items()})
        return out

    check_widths(call, labels, ll, V, blank, f"{kind} short widths")


@pytest.mark.parametrize("kind", KINDS)
def test_label_width_and_hostile_tails_long_form(kind):
    B, T, V, U, blank = LONG_MAIN
    x, labels, ll, tl = long_input("1023")
    long_ref(kind, "1023")
    assert ll[1] == 1024 and labels[1, 1023] == Q  # the first unowned position opens the second label block, beside an owned -3

    def call(lab, bound):
        kw = {} if bound is None else {"max_label_length": bound}
        out = TL.run(kind, 0, x, lab, ll, tl, blank=blank, **kw)
        ck = TL.run(kind, 0, x, lab, ll, tl, blank=blank, checkpoint=True, post=False, **kw)
        TL.same_bits(ck, out, ["loss", "grad"])
        return out

    check_widths(call, labels, ll, V, blank, f"{kind} long widths")


# ---- e. ownership: padding frames and strides ----

def layouts(xd):
    """Dense xd[B, T, V] (device) batch-major and time-major with a row stride of V + 3, NaN between V and the stride:
    (name, view, mask of the buffer's owned elements)."""
    B, T, V = xd.shape
    S = V + 3
    for name, sb, st in (("batch-major", T * S, S), ("time-major", S, B * S)):
        storage, _, owned = OW.strided_storage(xd, sb, st)
        storage = OW.poison_gaps(storage, owned, float("nan"))
        yield name, storage.as_strided((B, T, V), (sb, st, 1)), owned.cpu()


def check_ownership(entry, x, tl, dtype, what):
    """entry(view) -> dict of CPU outputs with grad (a view with the strides of the logits) and its whole buffer(s) *grad_storage."""
    B, T, V = x.shape
    xd = torch.from_numpy(x).to(DEV).to(dtype)
    pad = OW.padding_mask(tl, T)
    assert pad.any()
    for name, view, owned in layouts(xd):
        clean = entry(view)
        assert np.isfinite(clean["loss"].numpy()).all(), (what, name)
        for k, v in clean.items():
            if k.endswith("grad_storage"):
                assert OW.keeps_prefill(v, FILL)[~owned].all() and (~owned).any(), (what, name, k)  # the gaps are untouched
            elif k.endswith("grad"):
                assert zero_bits(v[pad]) and v[~pad].any(), (what, name, k)  # exactly zero at the padding frames
        for value in OW.poison_values(dtype):
            (_, pview, _), = [l for l in layouts(OW.poison_padding(xd, tl, value)) if l[0] == name]
            assert not OW.same_bits(pview, view)
            TS.same_bits(clean, entry(pview))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_ownership_short_form(kind, dtype):
    (B, T, V, U), blank = SHORT[0]
    x, labels, ll, tl = short_input(kind, 0, 0)
    host_checks(labels, ll, blank, short_ref(("short", kind, 0, 0), kind, 0, x.astype(np.float64), labels, ll, tl, blank)[0])

    def entry(view):
        out = TS._raw_calls(kind, view, labels, ll, tl, FILL, blank=blank, like_x=True)
        out.update({"a_" + k: v for k, v in TS.run_align(kind, 0, view, labels, ll, tl, blank=blank).items()})
        return out

    check_ownership(entry, x, tl, dtype, f"{kind} short ownership {dtype}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_ownership_long_form(kind, dtype):
    B, T, V, U, blank = LONG_MAIN
    x, labels, ll, tl = long_input("1023")
    long_ref(kind, "1023")
    check_ownership(lambda view: TL._raw_calls(kind, view, labels, ll, tl, FILL, blank=blank, like_x=True), x, tl, dtype,
                    f"{kind} long ownership {dtype}")
