"""Best-path (Viterbi) forced alignment on the GPU (ctc_amd_best_path, csrc/ctc_align.hip) against the float64 oracle
tests/tools/viterbi_oracle.py.  Paths are never compared element-wise with the oracle's (ties may be broken differently);
what is compared is validity (exact), the value of the returned path against the oracle's optimum, and the score.

Tolerances (derived, not measured):
  optimality  oracle optimum - value of the returned path <= 1e-6 absolute, both in float64.  The kernel's choice is exact in
              float64; reordering a T-term float64 sum costs about T * 2^-53 * |score| (5e-10 at T = 1000): a cap with three
              orders of margin.
  score       |score - oracle| <= 1e-4 + 1e-6 * |score|: the project's absolute bar, plus a relative term for the float32
              rounding of the output (6e-8) and the float32 row statistics behind the log-sum-exps.
Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OPT_TOL = 1e-6


def score_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def needed_frames(kind, label):
    label = list(label)
    return len(label) + (sum(a == b for a, b in zip(label, label[1:])) if kind == "classic" else 0)


def make_inputs(kind, B, T, V, U, seed, scale=1.0):
    """Ragged, feasible: label_length in [U/2, U] (utterance 0: U), logit_length from what the label needs up to T (utterance 0: T)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    ll = rng.integers(U // 2, U + 1, B).astype(np.int32)
    ll[0] = U
    tl = np.zeros(B, np.int32)
    for b in range(B):
        need = needed_frames(kind, labels[b, :ll[b]])
        assert need <= T
        tl[b] = rng.integers(max(need, T // 2), T + 1)
    tl[0] = T
    return x, labels, ll, tl


def run(kind, wrt, x, labels, ll, tl, blank=0, **kw):
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    args = (torch.from_numpy(labels).to(DEV), xt, torch.from_numpy(ll).to(DEV), torch.from_numpy(tl).to(DEV), blank)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        out = ctc.ctc_alignment_from_logproba(*args, cls)
    else:
        out = (ctc.classic_ctc_alignment if kind == "classic" else ctc.simplified_ctc_alignment)(*args, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcAlignment)
    assert out.score.dtype == torch.float32 and out.tokens.dtype == torch.int32 and out.label_index.dtype == torch.int32
    assert not out.score.requires_grad
    return out.score.cpu().numpy(), out.tokens.cpu().numpy(), out.label_index.cpu().numpy()


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


def check_against_oracle(kind, wrt, x, labels, ll, tl, got, blank=0, what=""):
    """x: the float32 values the kernel read.  Returns (worst optimality gap, worst score error)."""
    score, tokens, index = got
    o_score, o_paths = VO.best_path(kind, labels, x, ll, tl, blank, wrt)
    B, T = x.shape[0], x.shape[1]
    worst_gap, worst_err = 0.0, 0.0
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        if o_paths[b] is None:
            assert score[b] == -np.inf, (what, b, score[b])
            assert np.all(tokens[b] == -1) and np.all(index[b] == -1), (what, b)
            continue
        assert np.isfinite(score[b]), (what, b, score[b], o_score[b])
        check_valid(kind, tokens[b], index[b], labels[b, :ll[b]], Tb, blank)
        gap = o_score[b] - VO.path_score(x[b, :Tb], tokens[b, :Tb], wrt)
        err = abs(float(score[b]) - o_score[b])
        worst_gap, worst_err = max(worst_gap, abs(gap)), max(worst_err, err)
        assert -OPT_TOL <= gap <= OPT_TOL, (what, b, gap)
        assert err <= score_tol(o_score[b]), (what, b, score[b], o_score[b])
    print(f"ALIGN-MEASURE {what}: worst optimality gap {worst_gap:.3e} (cap {OPT_TOL:.0e}), worst |score - oracle| {worst_err:.3e} "
          f"(bound {score_tol(np.min(o_score[np.isfinite(o_score)])):.3e} at the largest |score|)", flush=True)
    return worst_gap, worst_err


def logprobs32(x):
    return VO.log_softmax64(x).astype(np.float32)


# every boundary of the label positions per lane (U = 64 NL), vocabularies 3 .. 8192
SHAPES = [(5, 40, 3, 1), (4, 150, 256, 64), (4, 160, 3, 65), (3, 300, 1000, 128), (3, 300, 256, 129), (2, 600, 8192, 256),
          (3, 600, 256, 257), (2, 1100, 1000, 512), (2, 1100, 3, 513), (2, 2100, 256, 1024)]


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U", SHAPES, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}-U{s[3]}" for s in SHAPES])
def test_alignment_against_the_oracle(B, T, V, U, kind, wrt):
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=1000 * U + V + wrt)
    if wrt:
        x = logprobs32(x)
    got = run(kind, wrt, x, labels, ll, tl)
    check_against_oracle(kind, wrt, x, labels, ll, tl, got, what=f"{kind} wrt={wrt} B={B} T={T} V={V} U={U}")


def test_north_star_shape():
    B, T, V, U = 256, 1000, 256, 128
    x, labels, ll, tl = make_inputs("classic", B, T, V, U, seed=7)
    got = run("classic", 0, x, labels, ll, tl)
    check_against_oracle("classic", 0, x, labels, ll, tl, got, what=f"classic wrt=0 B={B} T={T} V={V} U={U} (north star)")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_sharp_logits_and_a_nonzero_blank(kind):
    """N(0, 4^2) logits, blank in the middle of the vocabulary, odd V (element-wise row accesses)."""
    B, T, V, U = 4, 200, 37, 50
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=11, scale=4.0)
    blank = 17
    labels[labels == blank] = 18
    for b in range(B):  # (the replacement may have made a repeat: keep every utterance feasible)
        tl[b] = max(tl[b], needed_frames(kind, labels[b, :ll[b]]))
    got = run(kind, 0, x, labels, ll, tl, blank)
    check_against_oracle(kind, 0, x, labels, ll, tl, got, blank, what=f"{kind} sharp, blank=17, V=37")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_score_is_at_most_minus_the_loss_of_this_library(kind):
    """One path is at most the sum over all of them.  tol = the score's bar + the loss's (1e-4 * max(1, |loss|), tests/test_gpu_graph.py)."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 8, 300, 256, 100
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=3)
    score, _, _ = run(kind, 0, x, labels, ll, tl)
    fn = ctc.classic_ctc_loss if kind == "classic" else ctc.simplified_ctc_loss
    loss = fn(torch.from_numpy(labels).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(ll).to(DEV),
              torch.from_numpy(tl).to(DEV), 0).cpu().numpy()
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(score))
    tol = score_tol(score) + 1e-4 * np.maximum(1.0, np.abs(loss))
    print(f"ALIGN-MEASURE {kind}: score + loss = {score + loss}", flush=True)
    assert np.all(score <= -loss + tol), (score, loss)


def planted_path(kind, label, Tb, rng, blank=0):
    """A random path of Tb frames that gives `label`."""
    label = list(label)
    frames = [[k] for k in label]
    if kind == "classic":
        gaps = [[] for _ in range(len(label) + 1)]
        for i in range(1, len(label)):
            if label[i] == label[i - 1]:
                gaps[i].append(blank)
    else:
        gaps = [[] for _ in range(len(label) + 1)]
    used = len(label) + sum(len(g) for g in gaps)
    assert used <= Tb
    for _ in range(Tb - used):
        if kind == "classic" and label and rng.random() < 0.5:
            frames[rng.integers(len(label))].append(None)  # one more frame of the same label
        else:
            gaps[rng.integers(len(gaps))].append(blank)
    path, index = [], []
    for i in range(len(label) + 1):
        path += gaps[i]; index += [-1] * len(gaps[i])
        if i < len(label):
            path += [label[i]] * len(frames[i]); index += [i] * len(frames[i])
    return np.asarray(path, np.int32), np.asarray(index, np.int32)


@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U", [(6, 120, 50, 30), (3, 400, 256, 150)])
def test_planted_path_is_recovered(kind, B, T, V, U):
    """N(0,1) logits plus 30 on a planted path: that path is the unique optimum (any other loses 30 minus a difference of two
    N(0,1) draws in at least one frame), so tokens and label_index must equal it."""
    rng = np.random.default_rng(5)
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=21)
    want_tok = np.full((B, T), -1, np.int32)
    want_idx = np.full((B, T), -1, np.int32)
    for b in range(B):
        pth, idx = planted_path(kind, labels[b, :ll[b]], int(tl[b]), rng)
        assert VO.reduces_to(kind, pth, 0) == list(labels[b, :ll[b]])
        want_tok[b, :tl[b]], want_idx[b, :tl[b]] = pth, idx
        x[b, np.arange(tl[b]), pth] += 30.0
    score, tokens, index = run(kind, 0, x, labels, ll, tl)
    assert np.array_equal(tokens, want_tok)
    assert np.array_equal(index, want_idx)
    for b in range(B):
        assert abs(score[b] - VO.path_score(x[b, :tl[b]], want_tok[b, :tl[b]], 0)) <= score_tol(score[b])


@pytest.mark.parametrize("kind", VO.KINDS)
def test_producer_formats_read_in_place(kind):
    """bfloat16, float16 and time-major views give what float32 of the same (rounded) values gives: the conversions are exact,
    so the chain sees the same numbers -- the same path bit for bit -- and the score agrees within its tolerance."""
    B, T, V, U = 5, 180, 64, 40
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=9)
    xt = torch.from_numpy(x).to(DEV)
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16)),
                      ("time-major float32", xt.transpose(0, 1).contiguous().transpose(0, 1)),
                      ("time-major bfloat16", xt.to(torch.bfloat16).transpose(0, 1).contiguous().transpose(0, 1)),
                      ("padded rows", torch.zeros((B, T, V + 3), device=DEV).copy_(torch.nn.functional.pad(xt, (0, 3)))[:, :, :V])):
        assert not (xin.dtype == torch.float32 and xin.is_contiguous())
        x32 = xin.float().contiguous()
        got = run(kind, 0, xin, labels, ll, tl)
        ref = run(kind, 0, x32, labels, ll, tl)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), name
        assert np.all(np.abs(got[0] - ref[0]) <= 2 * score_tol(ref[0])), (name, got[0], ref[0])
        check_against_oracle(kind, 0, x32.cpu().numpy(), labels, ll, tl, got, what=f"{kind} {name}")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_infeasible_utterances(kind):
    """-inf and -1 everywhere exactly where the oracle says so: a label equal to the blank, a label outside [0, V), too few
    frames, label_length beyond the label tensor's bound; beside them feasible ones, an empty label and an empty utterance."""
    from tf_seq2seq_losses_amd import _lib, ops
    B, T, V, U = 8, 30, 12, 6
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=13)
    labels[0, 2] = 0                       # the blank inside the label
    labels[1, 0] = V                       # outside the vocabulary
    labels[2, 1] = -3
    ll[3], tl[3] = 6, 5                    # too few frames
    ll[4] = 0                              # empty label: the all-blank path
    tl[5] = 0                              # no frames, non-empty label
    ll[6], tl[6] = 0, 0                    # no frames, empty label: score 0
    got = run(kind, 0, x, labels, ll, tl)
    check_against_oracle(kind, 0, x, labels, ll, tl, got, what=f"{kind} infeasible mix")
    score, tokens, index = got
    assert np.array_equal(np.isfinite(score), [False, False, False, False, True, False, True, True])
    assert score[6] == 0.0
    assert np.all(tokens[4, :tl[4]] == 0) and np.all(index[4] == -1)
    # label_length > U: a static bound below the label's length
    p = ops.Prepared(torch.from_numpy(labels).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(ll).to(DEV),
                     torch.from_numpy(tl).to(DEV), 0, U=4)
    s2, t2, i2 = (a.cpu().numpy() for a in ops.best_path(ops.KINDS[kind], _lib.WRT_LOGITS, p))
    for b in range(B):
        if ll[b] > 4:
            assert s2[b] == -np.inf and np.all(t2[b] == -1) and np.all(i2[b] == -1)
        else:
            assert s2[b] == score[b] and np.array_equal(t2[b], tokens[b]) and np.array_equal(i2[b], index[b])


def test_empty_shapes():
    import tf_seq2seq_losses_amd as ctc
    z = ctc.classic_ctc_alignment(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((0, 4, 3), device=DEV),
                                  torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert z.score.shape == (0,) and z.tokens.shape == (0, 4) and z.label_index.shape == (0, 4)
    z = ctc.simplified_ctc_alignment(torch.tensor([[1, 2], [1, 2]], dtype=torch.int32, device=DEV), torch.zeros((2, 0, 3), device=DEV),
                                     torch.tensor([2, 0], dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert z.tokens.shape == (2, 0) and z.score.cpu().tolist() == [-np.inf, 0.0]


def test_cpu_tensors_are_refused():
    import tf_seq2seq_losses_amd as ctc
    with pytest.raises(RuntimeError):
        ctc.classic_ctc_alignment(torch.ones((1, 2), dtype=torch.int32), torch.zeros((1, 4, 3)), torch.tensor([2]), torch.tensor([4]))


@pytest.mark.parametrize("kind", VO.KINDS)
def test_two_runs_are_bit_identical(kind):
    B, T, V, U = 16, 400, 128, 90
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=17)
    x = np.round(x * 4) / 4  # quarter steps: plenty of exact ties between paths
    a = run(kind, 0, x, labels, ll, tl)
    b = run(kind, 0, x, labels, ll, tl)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    check_against_oracle(kind, 0, x, labels, ll, tl, a, what=f"{kind} tied logits")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_best_path_in_a_hip_graph(kind):
    """One launch, a single serial branch: captured once and replayed on new data it reproduces the eager call."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V, U = 6, 90, 64, 20
    k = ops.KINDS[kind]
    x = torch.zeros((B, T, V), device=DEV)
    labels = torch.zeros((B, U), dtype=torch.int32, device=DEV)
    ll = torch.zeros(B, dtype=torch.int32, device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    score = torch.zeros(B, device=DEV)
    tokens = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    index = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    ws = torch.zeros(max(_lib.best_path_workspace_bytes(k, B, T, V, U), 1), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_best_path(k, _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), U, ll.data_ptr(),
                                   tl.data_ptr(), 0, B, T, V, U, score.data_ptr(), tokens.data_ptr(), index.data_ptr(),
                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(seed):
        h = make_inputs(kind, B, T, V, U, seed)
        for dst, src in zip((x, labels, ll, tl), h):
            dst.copy_(torch.from_numpy(src))
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
        score.zero_(); tokens.zero_(); index.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = (score.cpu().numpy(), tokens.cpu().numpy(), index.cpu().numpy())
        score.zero_(); tokens.zero_(); index.zero_()
        call()
        torch.cuda.synchronize()
        assert got[0].tobytes() == score.cpu().numpy().tobytes()
        assert np.array_equal(got[1], tokens.cpu().numpy()) and np.array_equal(got[2], index.cpu().numpy())
        check_against_oracle(kind, 0, *h, got, what=f"{kind} graph replay seed {seed}")
