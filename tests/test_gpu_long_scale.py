"""The long-form kernels (csrc/ctc_loss_long.hip, ctc_align_long.hip, ctc_align_long_wild.hip) at the sizes they were built for:
workspace regions whose device-side byte offsets pass 2^31 and 2^32, tile grids with more label blocks than time blocks, 16384
frames, and the format combinations at two label blocks that tests/test_gpu_long_loss.py leaves out.

References and bars are the siblings', through their own functions and unchanged: tests/test_gpu_wildcard_loss.compare (loss
1e-4 + 1e-6 |loss|, gradient 1e-4 per element, row sums), tests/test_gpu_long_alignment.check (Viterbi oracle) and
tests/test_gpu_wildcard_alignment.check (wildcard oracle).  No tolerance is defined here.  Where two runs of the same recursion are
compared, they are compared by bits.  Every figure is printed before it is asserted (pytest -s shows them), with the wall time of
the GPU calls and of the float64 oracle.

A and B need about 5 GB of free device memory each and skip, naming both numbers, on a device that reports less."""
import contextlib
import time

import numpy as np
import pytest
import torch

from tests import _ownership as OW
from tests import test_gpu_alignment as GA
from tests import test_gpu_long_alignment as GL
from tests import test_gpu_long_loss as LL
from tests import test_gpu_long_wildcard_alignment as GLW
from tests import test_gpu_wildcard_alignment as WA
from tests import test_gpu_wildcard_loss as WLT
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = LL.W
KINDS = LL.KINDS
UB = 1024
make, run, ws_bytes, same = LL.make, LL.run, LL.ws_bytes, LL.same
compare, oracle, kind_id, loss_tol = WLT.compare, WLT.oracle, WLT.kind_id, WLT.loss_tol
FLOOR = 2 ** 32 + 2 ** 24  # what the workspace of B - 1 utterances must reach: utterance B - 1's large region lies past 2^32


class Clock:
    """Wall time of the blocks it wraps, by name (the GPU calls synchronise before they return)."""

    def __init__(self):
        self.t = {}

    @contextlib.contextmanager
    def __call__(self, name):
        t0 = time.perf_counter()
        yield
        self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0

    def __str__(self):
        return ", ".join(f"{k} {v:.2f} s" for k, v in self.t.items())


@pytest.fixture(autouse=True)
def release_device_memory():
    """The gigabytes of A and B go back to the device after each test: the alignment calls keep their workspace per stream."""
    yield
    from tf_seq2seq_losses_amd import ops
    ops._WS_CACHE.clear()
    torch.cuda.empty_cache()


def need_free(need, what):
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{what}: needs {need} bytes of free device memory, the device reports {free}")


def smallest_batch(size_of, also=lambda B: True):
    B = 2
    while size_of(B - 1) < FLOOR or not also(B):
        B += 1
    return B


def heavy_places(B, first, per):
    """b = 0, the first b whose region [first + b * per, first + (b + 1) * per) ends past 2^31, and b = B - 1."""
    cross = next(b for b in range(B) if first + (b + 1) * per > 2 ** 31)
    assert 0 < cross < B - 1 and first + cross * per < 2 ** 31
    return [0, cross, B - 1]


def fillers_of(B, heavy, ll, tl):
    """Every utterance that is not heavy, in place: the first with no label, the second infeasible, the third with no frame."""
    f = [b for b in range(B) if b not in heavy]
    ll[f[0]] = 0
    ll[f[1]], tl[f[1]] = 21, 20
    tl[f[2]] = 0
    return f


def beyond_frames_is_zero(grad, tl):
    T = grad.shape[1]
    mask = torch.arange(T, device=grad.device)[None, :] >= WLT.dev(tl)[:, None].long()
    return bool((grad[mask] == 0).all())


# ---- A: saved rows past 2^32 bytes ----

A_T, A_V, A_U = 4400, 32, 4100
A_FORCED = (1023, 1024, 4095, 4096)


def rows_per_utterance(kind, T, U):
    K = (U + UB - 1) // UB
    return 8 * K * T * ((2 if kind == "classic" else 1) * UB + 2)


@pytest.mark.parametrize("kind", KINDS)
def test_saved_rows_beyond_4_gib(kind):
    """B is the smallest batch whose first B - 1 utterances fill 2^32 + 2^24 bytes of workspace: every saved row of utterance B - 1
    is written and read at a byte offset >= 2^32, and those of one utterance in the middle straddle 2^31.  Three distinct heavy
    utterances (L = 4100, T_b = 4400, 3 % wildcards, among them positions 1023 / 1024 and 4095 / 4096) sit at b = 0, at the 2^31
    crossing and at b = B - 1; everything else is a short random filler.  Each heavy utterance must have the bits it has when run
    alone with B = 1, where every offset is small.  Only utterance B - 1 (alone) and the fillers are compared with the float64
    oracle: one heavy oracle call costs 1.5 to 6 s of CPU, so the other two heavy utterances get none -- their check is the bits."""
    from tf_seq2seq_losses_amd import _lib
    clock = Clock()
    T, V, U = A_T, A_V, A_U
    B = smallest_batch(lambda n: _lib.long_wildcard_loss_workspace_bytes(kind_id(kind), n, T, V, U, 0, True))
    n_ws = _lib.long_wildcard_loss_workspace_bytes(kind_id(kind), B, T, V, U, 0, True)
    per = rows_per_utterance(kind, T, U)
    off_rows = n_ws - ((B * per + 255) & ~255)  # the saved rows are the workspace's last region
    heavy = heavy_places(B, off_rows, per)
    top = B - 1
    print(f"LONG-SCALE A {kind}: B = {B}, workspace {n_ws} bytes, saved rows from byte {off_rows}, {per} per utterance; heavy at "
          f"b = {heavy}; rows of b = {heavy[1]} from byte {off_rows + heavy[1] * per}; rows of b = {top} from byte {off_rows + top * per}")
    assert B == (13 if kind == "classic" else 25) and B <= 32 and n_ws < 6e9
    assert off_rows + top * per >= 2 ** 32
    need_free(n_ws + 3 * B * T * V * 4 + 2 ** 28, f"saved rows beyond 4 GiB ({kind})")

    rng = np.random.default_rng(7001)
    x, labels, ll, tl = make(B, T, V, U, rng.integers(0, 41, B), rng.integers(0, 161, B), seed=7000, random_wild=0.1)
    for n, b in enumerate(heavy):
        xb, lb, _, _ = make(1, T, V, U, (U,), (T,), seed=7010 + n, wild=(A_FORCED,), random_wild=0.03)
        x[b], labels[b], ll[b], tl[b] = xb[0], lb[0], U, T
        assert WLT.needed_frames(kind, labels[b]) <= T, "feasible on the classic lattice too"
    assert not np.array_equal(labels[heavy[0]], labels[heavy[1]]) and not np.array_equal(x[heavy[1]], x[top])
    fill = fillers_of(B, heavy, ll, tl)

    with clock("batch"):
        loss, grad = run(kind, 0, x, labels, ll, tl)
    with clock("forward only"):
        loss0, none = run(kind, 0, x, labels, ll, tl, want_grad=False)
    alone = {}
    with clock("alone"):
        for b in heavy:
            alone[b] = run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1])
    with clock("oracle, one heavy utterance"):
        ref = oracle(kind, 0, x[top:top + 1], labels[top:top + 1], ll[top:top + 1], tl[top:top + 1], key=("scale-A", kind))
    with clock("oracle, fillers"):
        ref_f = oracle(kind, 0, x[fill], labels[fill], ll[fill], tl[fill], key=("scale-A-fill", kind))
    print(f"LONG-SCALE A {kind}: {clock}")
    for b in heavy:
        d = float((grad[b] - alone[b][1][0]).abs().max())
        print(f"LONG-SCALE A {kind} b = {b}: loss in the batch {float(loss[b]):.4f}, alone {float(alone[b][0][0]):.4f}, "
              f"worst |gradient in the batch - alone| {d:.3e}")
    for b in heavy:
        assert same((loss[b:b + 1], grad[b:b + 1]), alone[b]), f"utterance {b}: the bits of the run alone"
    assert np.isfinite(ref[0]).all()
    compare(f"long-scale A {kind} b = {top} alone", *alone[top], *ref)
    assert not np.isfinite(ref_f[0][1]) and np.isfinite(ref_f[0]).sum() >= len(fill) // 2
    idx = torch.as_tensor(fill, device=DEV)
    compare(f"long-scale A {kind} fillers", loss[idx], grad[idx], *ref_f)
    assert bool(torch.isfinite(grad).all()) and beyond_frames_is_zero(grad, tl)
    assert none is None and OW.same_bits(loss0, loss), "grad = NULL: the bits of the forward of the gradient call"


# ---- B: back-pointers past 2^32 bytes ----

B_T, B_V, B_U = 4400, 8, 4100


def distinct_neighbours(label, V, rng, repeats=()):
    """Neighbouring labels made to differ (blank = 0), then label[i] = label[i - 1] at the given positions."""
    for i in range(1, len(label)):
        if label[i] == label[i - 1]:
            label[i] = label[i] % (V - 1) + 1
    for i in repeats:
        label[i] = label[i - 1]
    return label


def alignment_batch(B, heavy, wild):
    """x[B, T, 8]; heavy utterances of 4100 labels over 4400 frames with 40 repeated neighbours (1024 and 4096 among them), wild:
    3 % wildcards, positions 1023 / 1024 and 4095 / 4096 among them; fillers of up to 40 labels and 160 frames."""
    T, V, U = B_T, B_V, B_U
    rng = np.random.default_rng(7101)
    x, labels, ll, tl = make(B, T, V, U, rng.integers(0, 41, B), rng.integers(0, 161, B), seed=7100, random_wild=0.1 if wild else 0.0)
    for n, b in enumerate(heavy):
        xb, lb, _, _ = make(1, T, V, U, (U,), (T,), seed=7110 + n)
        r = np.random.default_rng(7120 + n)
        lab = distinct_neighbours(lb[0], V, r, repeats=[1024, 4096] + list(r.choice(np.arange(2, U, 2), 38, replace=False)))
        if wild:
            lab[r.random(U) < 0.03] = W
            lab[list(A_FORCED)] = W
        x[b], labels[b], ll[b], tl[b] = xb[0], lab, U, T
        assert WLT.needed_frames("classic", lab) <= T
    return x, labels, ll, tl, fillers_of(B, heavy, ll, tl)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("call", ["plain", "wildcard"])
def test_back_pointers_beyond_4_gib(call, kind):
    """The construction of A for the two alignment calls: the back-pointers, B * K * T * 512 bytes, are the first region of the
    workspace, so with more than 2^23 / (K * T) utterances those of utterance B - 1 start past 2^32 and every other region (columns,
    rows, LSE partials, label_index, the wildcard call's per-frame statistics) lies past 2^32 as a whole.  Heavy utterances at
    b = 0, at the 2^31 crossing and at b = B - 1: every output in the batch has the bits of the run alone; the top one, alone,
    and the fillers pass the sibling's oracle check; and on each heavy utterance score <= -loss + loss_tol(loss) with the
    forward-only long-form loss of the same labels (wildcard weight 0: the loss sums what the best path takes the maximum of)."""
    from tf_seq2seq_losses_amd import _lib
    clock = Clock()
    T, V, U = B_T, B_V, B_U
    K = (U + UB - 1) // UB
    wild = call == "wildcard"
    size_of = _lib.long_wildcard_best_path_workspace_bytes if wild else _lib.long_best_path_workspace_bytes
    per = K * T * 512
    B = smallest_batch(lambda n: size_of(kind_id(kind), n, T, V, U, 0), also=lambda n: (n - 1) * per >= 2 ** 32)
    n_ws = size_of(kind_id(kind), B, T, V, U, 0)
    heavy = heavy_places(B, 0, per)
    top = B - 1
    print(f"LONG-SCALE B {call} {kind}: B = {B} (B * K * T = {B * K * T} > 2^23), workspace {n_ws} bytes, logits {B * T * V * 4} bytes; heavy "
          f"at b = {heavy}; back-pointers of b = {heavy[1]} from byte {heavy[1] * per}, of b = {top} from byte {top * per}")
    assert B * K * T > 2 ** 23 and top * per >= 2 ** 32 and B <= 400 and n_ws + B * T * V * 4 < 6e9
    need_free(n_ws + 2 * B * T * V * 4 + 6 * B * max(T, U) * 4 + 2 ** 28, f"back-pointers beyond 4 GiB ({call}, {kind})")

    x, labels, ll, tl, fill = alignment_batch(B, heavy, wild)
    go = GLW.run if wild else GL.run
    xt = WA.dev(x)
    with clock("batch"):
        got = go(kind, 0, xt, labels, ll, tl, max_label_length=U)
    alone, losses = {}, {}
    with clock("alone"):
        for b in heavy:
            alone[b] = go(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], max_label_length=U)
    with clock("forward-only loss"):
        for b in heavy:
            losses[b] = float(run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], want_grad=False)[0][0])
    for b in heavy:
        print(f"LONG-SCALE B {call} {kind} b = {b}: score in the batch {got[0][b]:.4f}, alone {alone[b][0][0]:.4f}, -loss {-losses[b]:.4f} "
              f"(+ {loss_tol(losses[b]):.3e})")
    for b in heavy:
        for name, a, c in zip(GLW.NAMES, got, alone[b]):
            assert a[b:b + 1].shape == c.shape and a[b:b + 1].tobytes() == c.tobytes(), (b, name)
        assert np.isfinite(losses[b]) and got[0][b] <= -losses[b] + loss_tol(losses[b]), (b, got[0][b], losses[b])
    s = slice(top, top + 1)
    got_f = tuple(a[fill] for a in got)
    with clock("oracle checks"):
        if wild:
            WA.check(kind, 0, x[s], labels[s], ll[s], tl[s], alone[top], what=f"long-scale B {kind} b = {top} alone")
            o_score = WA.check(kind, 0, x[fill], labels[fill], ll[fill], tl[fill], got_f, what=f"long-scale B {kind} fillers")
        else:
            GL.check(kind, 0, x[s], labels[s], ll[s], tl[s], VO.best_path(kind, labels[s], x[s], ll[s], tl[s]), alone[top],
                     what=f"long-scale B {kind} b = {top} alone")
            o_score, o_paths = VO.best_path(kind, labels[fill], x[fill], ll[fill], tl[fill])
            GL.check(kind, 0, x[fill], labels[fill], ll[fill], tl[fill], (o_score, o_paths), got_f, what=f"long-scale B {kind} fillers")
    assert not np.isfinite(o_score[1]) and np.isfinite(o_score).sum() >= len(fill) // 2
    print(f"LONG-SCALE B {call} {kind}: {clock}")


# ---- C: more label blocks than time blocks, ragged tiles ----

C_SHAPE = dict(B=3, T=3305, V=32, U=3100, ll=(3100, 2049, 1024), tl=(3305, 3304, 1653))
C_TF = (1652, 128, 100)


@pytest.mark.parametrize("kind", KINDS)
def test_deep_ragged_grid(kind):
    """K = 4 label blocks.  frames_per_tile = 1652 gives J = 3 time blocks, K > J > 1: the last tile of utterance 0 has exactly one
    frame, tile (1, 0) straddles frame 1024 and tile (3, 1) frame 3072 (a block's first reachable frame inside a tile at j > 0),
    tiles (2, 0) and (3, 0) are skipped, utterance 1 ends with its second tile and utterance 2 one frame into it.  The loss and
    gradient against the oracle, the same bits at 128 and at 100 frames per tile (100: a multiple of 4 that does not divide 1024,
    J = 34), the forward-only loss with the same bits at each.  Both alignment calls on the same logits and lengths -- the plain
    call on the labels before 5 % of them became wildcards: label_index, tokens and the per-label outputs with the same bits at
    the three tile heights, score within the siblings' bar (the order of its LSE sum depends on the tiling), and at 1652 frames
    per tile against the oracle."""
    clock = Clock()
    x, labels, ll, tl = make(**C_SHAPE, seed=7200, random_wild=0.05)
    _, plain, _, _ = make(**C_SHAPE, seed=7200)
    assert np.array_equal(plain[labels != W], labels[labels != W]) and (labels == W).any() and not (plain == W).any()
    for b in range(3):
        assert WLT.needed_frames(kind, labels[b, :ll[b]]) <= tl[b] and GA.needed_frames(kind, plain[b, :ll[b]]) <= tl[b]
    with clock("oracle, loss"):
        ref = oracle(kind, 0, x, labels, ll, tl, key=("scale-C", kind))
    assert np.isfinite(ref[0]).all()
    xt = WLT.dev(x)
    with clock("loss"):
        base = run(kind, 0, xt, labels, ll, tl, tf=C_TF[0])
        others = {tf: run(kind, 0, xt, labels, ll, tl, tf=tf) for tf in C_TF[1:]}
        forward = {tf: run(kind, 0, xt, labels, ll, tl, tf=tf, want_grad=False)[0] for tf in C_TF}
    compare(f"long-scale C {kind} tf = {C_TF[0]} (K x J = 4 x 3)", *base, *ref)
    for tf in C_TF[1:]:
        d = float((others[tf][1] - base[1]).abs().max())
        print(f"LONG-SCALE C {kind}: tf = {tf} against tf = {C_TF[0]}: worst |gradient difference| {d:.3e}, losses equal: "
              f"{OW.same_bits(others[tf][0], base[0])}")
    for tf in C_TF[1:]:
        assert same(base, others[tf]), tf
    for tf in C_TF:
        assert OW.same_bits(forward[tf], base[0]), tf
    assert beyond_frames_is_zero(base[1], tl)
    with clock("alignments"):
        pl = {tf: GL.run(kind, 0, xt, plain, ll, tl, tf=tf) for tf in C_TF}
        wd = {tf: GLW.run(kind, 0, xt, labels, ll, tl, tf=tf) for tf in C_TF}
    for tf in C_TF[1:]:
        print(f"LONG-SCALE C {kind}: tf = {tf} against tf = {C_TF[0]}: |score difference| plain "
              f"{np.abs(pl[tf][0] - pl[C_TF[0]][0]).max():.3e}, wildcard {np.abs(wd[tf][0] - wd[C_TF[0]][0]).max():.3e}")
    for tf in C_TF[1:]:
        for k in range(1, 5):
            assert pl[tf][k].tobytes() == pl[C_TF[0]][k].tobytes(), (tf, GLW.NAMES[k])
        GLW.same_bits(wd[C_TF[0]], wd[tf], GLW.INVARIANT)
        assert np.all(np.abs(pl[tf][0] - pl[C_TF[0]][0]) <= GA.score_tol(pl[C_TF[0]][0])), tf
        assert np.all(np.abs(wd[tf][0] - wd[C_TF[0]][0]) <= WA.score_tol(wd[C_TF[0]][0])), tf
    with clock("oracle checks, alignments"):
        GL.check(kind, 0, x, plain, ll, tl, VO.best_path(kind, plain, x, ll, tl), pl[C_TF[0]], what=f"long-scale C {kind} plain")
        WA.check(kind, 0, x, labels, ll, tl, wd[C_TF[0]], what=f"long-scale C {kind} wildcard")
    print(f"LONG-SCALE C {kind}: {clock}")


# ---- D: 16384 frames ----

@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("kind", KINDS)
def test_error_over_16384_frames(kind, scale):
    """The chain keeps its state in float64 and takes every log-sum-exp increment through float32 exp2 and log2, once per position
    and frame: the error this adds up to over T = 16384 (U = 1025: two label blocks, 5 % wildcards) under the project's bars, for
    N(0, 1) and N(0, 4^2) logits.  The figures are those of profiles/long_loss_time.md, "accuracy over T"."""
    clock = Clock()
    T, U = 16384, 1025
    x, labels, ll, tl = make(1, T, 32, U, (U,), (T,), seed=7300 + int(scale), scale=scale, random_wild=0.05)
    with clock("oracle"):
        ref = oracle(kind, 0, x, labels, ll, tl, key=("scale-D", kind, scale))
    assert np.isfinite(ref[0]).all()
    with clock("loss and gradient"):
        loss, grad = run(kind, 0, x, labels, ll, tl)
    lerr = abs(float(loss[0]) - ref[0][0])
    gerr = float(np.abs(grad.cpu().numpy().astype(np.float64) - ref[1]).max())
    print(f"LONG-SCALE D {kind} N(0, {scale:g}^2) T = {T} U = {U}: loss {ref[0][0]:.3f}, |loss - oracle| {lerr:.3e}, error / bar "
          f"{lerr / loss_tol(ref[0][0]):.4f}; worst |gradient - oracle| {gerr:.3e}, error / bar {gerr / 1e-4:.4f}; {clock}")
    compare(f"long-scale D {kind} N(0, {scale:g}^2) T = {T}", loss, grad, *ref)


# ---- E: formats at two label blocks ----

FMT = LL.FMT


@pytest.mark.parametrize("kind", KINDS)
def test_bfloat16_log_probabilities(kind):
    x, labels, ll, tl = make(**FMT, seed=7400, wild=((5, 1023, 1024), (699,)))
    lp = WLT.dev(WLT.logprobs32(x) - np.float32(0.25)).to(torch.bfloat16)  # not normalised: e_w carries the rows' log-sum-exp
    ref = oracle(kind, 1, lp.float().cpu().numpy(), labels, ll, tl, weight=-0.25, key=("scale-E-lp", kind))  # what the kernel reads
    assert np.isfinite(ref[0]).all()
    loss, grad = run(kind, 1, lp, labels, ll, tl, weight=-0.25, tf=64)
    assert grad.dtype == torch.bfloat16
    compare(f"long-scale E {kind} bfloat16 log-probabilities tf = 64 w = -0.25", loss, grad, *ref, wrt=1, sixteen=True)


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_dtype_differs_from_the_logits(kind):
    x, labels, ll, tl = make(**FMT, seed=7401, wild=((5, 1023), (0,)))
    ref = oracle(kind, 0, x, labels, ll, tl, key=("scale-E-g16", kind))
    loss, grad = run(kind, 0, x, labels, ll, tl, grad_dtype=torch.bfloat16)
    assert grad.dtype == torch.bfloat16 and tuple(grad.shape) == x.shape
    compare(f"long-scale E {kind} float32 logits, bfloat16 gradient", loss, grad, *ref, sixteen=True)
    xh = WLT.dev(x).to(torch.bfloat16)
    refh = oracle(kind, 0, xh.float().cpu().numpy(), labels, ll, tl, key=("scale-E-g32", kind))  # the rounded logits
    loss, grad = run(kind, 0, xh, labels, ll, tl, grad_dtype=torch.float32)
    assert grad.dtype == torch.float32
    compare(f"long-scale E {kind} bfloat16 logits, float32 gradient", loss, grad, *refh)


@pytest.mark.parametrize("kind", KINDS)
def test_two_column_passes_on_the_vector_path(kind):
    """V = 1028: aligned rows of a multiple of 4 elements, so the row stage takes the vector path, and 4 columns beyond its first
    pass of 1024.  Tokens 1025 and 1026 stand in both label blocks; the blank is 1027, the last column of the second pass."""
    V, U, blank = 1028, 1026, 1027
    x, labels, ll, tl = make(1, 1100, V, U, (U,), (1100,), seed=7402, blank=blank, wild=((7,),))
    labels[0, [1, 3, 1020]] = 1025, 1026, 1025
    labels[0, [1024, 1025]] = 1026, 1025
    assert x.shape[2] % 4 == 0 and blank not in labels
    ref = oracle(kind, 0, x, labels, ll, tl, blank=blank, key=("scale-E-v1028", kind))
    assert np.isfinite(ref[0]).all()
    xt = WLT.dev(x)
    assert xt.data_ptr() % 16 == 0 and xt.stride() == (1100 * V, V, 1)
    loss, grad = run(kind, 0, xt, labels, ll, tl, blank=blank)
    compare(f"long-scale E {kind} V = 1028 blank = 1027", loss, grad, *ref)
