"""Forced alignment with wildcard labels on the GPU (ctc_amd_wildcard_best_path, csrc/ctc_align_wild.hip) against the float64
oracle tests/tools/wildcard_oracle.py.  Ties are unspecified, so paths are never compared with the oracle's: the returned
(tokens, label_index) must be admissible by the acceptor below, its float64 value must meet the optimality bar and `score` must
match the oracle's optimum.

Tolerances: those of tests/test_gpu_alignment.py, derived there.
  optimality  oracle optimum - float64 value of the returned path <= 1e-6 absolute
  score       |score - oracle| <= 1e-4 + 1e-6 * |score|; the same bar for every label_score against the float64 sum over its frames
              and for sum(label_score) + the blank frames' lp against score (U float32 roundings of 6e-8 relative each stay below
              the relative term).
Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO
from tests.tools import wildcard_oracle as WO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OPT_TOL = 1e-6
W = WO.WILDCARD


def score_tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def nl_for(U):
    nl = 1
    while 64 * nl < U:
        nl *= 2
    return nl


def needed_frames(kind, label):
    label = list(label)
    return len(label) + (sum(a == b and a != W for a, b in zip(label, label[1:])) if kind == "classic" else 0)


def make_inputs(kind, B, T, V, U, seed, blank=0, wild=True, scale=1.0):
    """Ragged and feasible.  label_length in [U/2, U] (utterance 0: U), logit_length from what the label needs up to T (utterance
    0: T).  Wildcards: about one position in five; in every even utterance also position 0, the last position, both sides of lane
    boundaries (positions k * NL - 1 and k * NL) and an adjacent pair in the middle."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    toks = np.asarray([k for k in range(V) if k != blank])
    labels = toks[rng.integers(0, len(toks), (B, U))].astype(np.int32)
    ll = rng.integers(U // 2, U + 1, B).astype(np.int32)
    ll[0] = U
    NL = nl_for(U)
    for b in range(B):
        L = int(ll[b])
        if not wild or L == 0:
            continue
        labels[b, :L][rng.random(L) < 0.2] = W
        if b % 2 == 0:
            forced = [0, L - 1, L // 2, L // 2 + 1] + [k * NL + d for k in (1, 2, 31, 63) for d in (-1, 0)]
            for i in forced:
                if 0 <= i < L:
                    labels[b, i] = W
    tl = np.zeros(B, np.int32)
    for b in range(B):
        need = needed_frames(kind, labels[b, :ll[b]])
        assert need <= T, (need, T)
        tl[b] = rng.integers(need, T + 1)
    tl[0] = T
    return x, labels, ll, tl


def logprobs32(x):
    return VO.log_softmax64(x).astype(np.float32)


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(kind, wrt, x, labels, ll, tl, blank=0, **kw):
    import tf_seq2seq_losses_amd as ctc
    args = (dev(labels), dev(x), dev(ll), dev(tl), blank)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        out = ctc.ctc_wildcard_alignment_from_logproba(*args, cls, **kw)
    else:
        out = (ctc.classic_ctc_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_wildcard_alignment)(*args, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcWildcardAlignment)
    assert out.score.dtype == torch.float32 and out.label_score.dtype == torch.float32
    assert all(t.dtype == torch.int32 for t in (out.tokens, out.label_index, out.first_frame, out.last_frame))
    assert not out.score.requires_grad
    return tuple(t.cpu().numpy() for t in out)


def check_admissible(kind, tokens, index, label, arg, Tb, blank):
    """Exact: is (tokens, label_index) a path the definition admits for `label`?  arg: the frame-wise argmax tokens a_t."""
    label = [int(k) for k in label]
    L = len(label)
    assert np.all(tokens[Tb:] == -1) and np.all(index[Tb:] == -1)
    tok, idx = tokens[:Tb], index[:Tb]
    assert np.all(tok[idx < 0] == blank)            # outside any label: blanks only
    assert np.all((idx >= -1) & (idx < L))
    seq = idx[idx >= 0]
    assert np.all(np.diff(seq) >= 0)                # labels in order
    first, last = np.full(L, -1), np.full(L, -1)
    for i, k in enumerate(label):
        fr = np.nonzero(idx == i)[0]
        assert len(fr) >= 1, i                       # every position takes a frame, a wildcard included
        assert np.all(np.diff(fr) == 1), i           # ... and its frames are contiguous
        first[i], last[i] = fr[0], fr[-1]
        if k == W:
            assert np.array_equal(tok[fr], arg[fr]), i  # a wildcard reports the frame's best token
        else:
            assert np.all(tok[fr] == k), i
            if kind == "simplified":
                assert len(fr) == 1, i
        if kind == "classic" and i > 0 and k != W and label[i - 1] == k:
            assert first[i] > last[i - 1] + 1, i     # a repeated label needs a blank in between
        if kind == "simplified" and i > 0 and label[i - 1] == W:
            assert first[i] == last[i - 1] + 1, i    # a wildcard owns every frame until the next label's
    if kind == "simplified" and L and label[-1] == W:
        assert last[-1] == Tb - 1                   # ... or until the end
    return first, last


def check(kind, wrt, x, labels, ll, tl, got, blank=0, what="", U=None):
    """x: the float32 values the kernel read.  Everything the module docstring lists, per utterance, and the per-label outputs."""
    score, tokens, index, first_frame, last_frame, label_score = got
    o_score, o_paths, _ = WO.best_path(kind, labels if U is None else labels[:, :U], x, ll, tl, blank, wrt)
    B, T = x.shape[0], x.shape[1]
    worst = dict(gap=0.0, err=0.0, lab=0.0, total=0.0)
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        if o_paths[b] is None:
            assert score[b] == -np.inf, (what, b, score[b])
            assert np.all(tokens[b] == -1) and np.all(index[b] == -1), (what, b)
            assert np.all(first_frame[b] == -1) and np.all(last_frame[b] == -1) and np.all(label_score[b] == -np.inf), (what, b)
            continue
        L = max(int(ll[b]), 0)
        assert np.isfinite(score[b]), (what, b, score[b], o_score[b])
        arg = WO.argmax_tokens(x[b, :Tb])
        first, last = check_admissible(kind, tokens[b], index[b], labels[b, :L], arg, Tb, blank)
        lp = np.asarray(x[b, :Tb], np.float64) if wrt else VO.log_softmax64(x[b, :Tb])
        plp = lp[np.arange(Tb), tokens[b, :Tb]]
        value = float(sum(plp))  # time order
        gap = o_score[b] - value
        err = abs(float(score[b]) - o_score[b])
        worst["gap"], worst["err"] = max(worst["gap"], abs(gap)), max(worst["err"], err)
        assert -OPT_TOL <= gap <= OPT_TOL, (what, b, gap)
        assert err <= score_tol(o_score[b]), (what, b, score[b], o_score[b])
        # per-label outputs
        assert np.array_equal(first_frame[b, :L], first) and np.array_equal(last_frame[b, :L], last), (what, b)
        assert np.all(first_frame[b, L:] == -1) and np.all(last_frame[b, L:] == -1) and np.all(label_score[b, L:] == -np.inf), (what, b)
        total = float(sum(plp[index[b, :Tb] < 0]))
        for i in range(L):
            want = float(sum(plp[first[i]:last[i] + 1]))
            worst["lab"] = max(worst["lab"], abs(label_score[b, i] - want))
            assert abs(label_score[b, i] - want) <= score_tol(want), (what, b, i, label_score[b, i], want)
            total += float(label_score[b, i])
        worst["total"] = max(worst["total"], abs(total - float(score[b])))
        assert abs(total - float(score[b])) <= score_tol(score[b]), (what, b, total, score[b])
    fin = o_score[np.isfinite(o_score)]
    print(f"WILD-MEASURE {what}: optimality gap {worst['gap']:.3e} (cap {OPT_TOL:.0e}), |score - oracle| {worst['err']:.3e}, "
          f"|label_score - float64| {worst['lab']:.3e}, |sum(label_score) + blanks - score| {worst['total']:.3e} "
          f"(bound {score_tol(np.min(fin)) if len(fin) else 0.0:.3e} at the largest |score|)", flush=True)
    return o_score


GRID = [(4, 12, 5, 3), (3, 40, 6, 10)] + [(2, U + U // 4 + 8, 8, U) for U in (64, 65, 129, 257, 513, 1024)]


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
@pytest.mark.parametrize("B,T,V,U", GRID, ids=[f"B{s[0]}-T{s[1]}-V{s[2]}-U{s[3]}" for s in GRID])
def test_against_the_oracle(B, T, V, U, kind, wrt):
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=1000 * U + V + wrt)
    assert np.any(labels[0, :U] == W) and labels[0, 0] == W and labels[0, U - 1] == W
    if wrt:
        x = logprobs32(x)
    got = run(kind, wrt, x, labels, ll, tl)
    o_score = check(kind, wrt, x, labels, ll, tl, got, what=f"{kind} wrt={wrt} B={B} T={T} V={V} U={U}")
    assert np.all(np.isfinite(o_score)), o_score  # T was chosen so that every utterance is feasible


@pytest.mark.parametrize("kind", VO.KINDS)
def test_without_a_wildcard_it_is_the_plain_alignment(kind):
    import tf_seq2seq_losses_amd as ctc
    for B, T, V, U in ((5, 90, 11, 30), (2, 400, 8, 257)):
        x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=31, wild=False)
        got = run(kind, 0, x, labels, ll, tl)
        ref = (ctc.classic_ctc_alignment if kind == "classic" else ctc.simplified_ctc_alignment)(dev(labels), dev(x), dev(ll), dev(tl), 0)
        assert np.array_equal(got[1], ref.tokens.cpu().numpy()) and np.array_equal(got[2], ref.label_index.cpu().numpy())
        s = ref.score.cpu().numpy()
        print(f"WILD-MEASURE {kind} no wildcard U={U}: |score - plain alignment| {np.abs(got[0] - s).max():.3e}", flush=True)
        assert np.all(np.abs(got[0] - s) <= 2 * score_tol(s))
        check(kind, 0, x, labels, ll, tl, got, what=f"{kind} no wildcard U={U}")


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_lone_wildcard_is_the_greedy_decoding(kind, wrt):
    import tf_seq2seq_losses_amd as ctc
    B, T, V = 5, 130, 37
    rng = np.random.default_rng(41)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if wrt:
        x = logprobs32(x)
    tl = np.asarray([T, 1, 64, 65, 99], np.int32)
    labels, ll = np.full((B, 1), W, np.int32), np.ones(B, np.int32)
    got = run(kind, wrt, x, labels, ll, tl, 3)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        dec = ctc.ctc_greedy_decode_from_logproba(dev(x), dev(tl), 3, cls)
    else:
        dec = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(dev(x), dev(tl), 3)
    assert np.array_equal(got[1], dec.tokens.cpu().numpy())
    s = dec.score.cpu().numpy()
    assert np.all(np.abs(got[0] - s) <= score_tol(s)), (got[0], s)
    ref = GO.decode(kind, x, tl, 3, wrt)
    assert np.array_equal(got[1], ref.tokens) and np.all(np.abs(got[0] - ref.score) <= score_tol(ref.score))
    check(kind, wrt, x, labels, ll, tl, got, 3, what=f"{kind} wrt={wrt} lone wildcard")


def planted(frames, V, T):
    """One-hot-like logits: 10 on the planted token of every frame, 0 elsewhere."""
    x = np.zeros((1, T, V), np.float32)
    x[0, np.arange(len(frames)), frames] = 10.0
    return x


@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_planted_region_is_found(kind):
    """`a b [junk] c d` with labels `a b * c d`: the wildcard takes exactly the junk and the known labels keep their planted frames;
    without the wildcard the junk is squeezed into blanks and neighbours and the per-frame score drops.  The labels beside a
    wildcard have one frame each and the junk begins and ends with tokens of its own, so the optimum is unique."""
    import tf_seq2seq_losses_amd as ctc
    V, a, b, c, d, e, f, g = 9, 1, 2, 3, 4, 5, 6, 7
    junk = [e, f, 0, e, g, 0, f]
    # in the middle
    frames = [0, a, 0, b] + junk + [c, 0, d, 0]
    T = len(frames)
    x = planted(frames, V, T)
    labels, ll, tl = np.asarray([[a, b, W, c, d]], np.int32), np.asarray([5], np.int32), np.asarray([T], np.int32)
    score, tokens, index, first, last, ls = run(kind, 0, x, labels, ll, tl)
    assert np.array_equal(tokens[0], frames)
    assert (first[0, 2], last[0, 2]) == (4, 4 + len(junk) - 1)
    assert first[0].tolist() == [1, 3, 4, 11, 13] and last[0].tolist() == [1, 3, 10, 11, 13]
    assert np.array_equal(index[0], [-1, 0, -1, 1] + [2] * len(junk) + [3, -1, 4, -1])
    check(kind, 0, x, labels, ll, tl, (score, tokens, index, first, last, ls), what=f"{kind} planted, middle")
    if kind == "classic":
        plain = ctc.classic_ctc_alignment(dev(np.asarray([[a, b, c, d]], np.int32)), dev(x), dev(np.asarray([4], np.int32)), dev(tl), 0)
        ps = float(plain.score.cpu()[0])
        print(f"WILD-MEASURE planted: per-frame score {score[0] / T:.4f} with the wildcard, {ps / T:.4f} without", flush=True)
        assert ps / T < score[0] / T - 1.0  # (at least three junk frames lose 10 each)
    # first and last
    j1, j2 = [e, 0, f, g], [g, 0, 0, e]
    frames = j1 + [a, 0, b, c, 0, d] + j2
    T = len(frames)
    x = planted(frames, V, T)
    labels, ll, tl = np.asarray([[W, a, b, c, d, W]], np.int32), np.asarray([6], np.int32), np.asarray([T], np.int32)
    got = run(kind, 0, x, labels, ll, tl)
    assert np.array_equal(got[1][0], frames)
    assert got[3][0].tolist() == [0, 4, 6, 7, 9, 10] and got[4][0].tolist() == [3, 4, 6, 7, 9, 13]
    check(kind, 0, x, labels, ll, tl, got, what=f"{kind} planted, both ends")


def test_against_the_caller_side_route():
    """Classic, log-probabilities: the existing alignment on [lp, max(lp)] with the wildcard mapped to token V scores the same
    (no adjacent wildcards here: as ordinary labels two of them would need a blank in between)."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, U = 4, 120, 12, 40
    x, labels, ll, tl = make_inputs("classic", B, T, V, U, seed=51)
    for bb in range(B):
        for i in range(1, U):
            if labels[bb, i] == W and labels[bb, i - 1] == W:
                labels[bb, i] = 1 + (i % (V - 1))
        tl[bb] = max(tl[bb], needed_frames("classic", labels[bb, :ll[bb]]))
    lp = logprobs32(x)
    got = run("classic", 1, lp, labels, ll, tl)
    lpt = dev(lp)
    ext = torch.cat([lpt, lpt.max(-1, keepdim=True).values], -1)
    mapped = np.where(labels == W, V, labels).astype(np.int32)
    ref = ctc.ctc_alignment_from_logproba(dev(mapped), ext, dev(ll), dev(tl), 0, ctc.ClassicCtcLossData)
    s = ref.score.cpu().numpy()
    print(f"WILD-MEASURE caller-side route: |score - route| {np.abs(got[0] - s).max():.3e}", flush=True)
    assert np.all(np.isfinite(s)) and np.all(np.abs(got[0] - s) <= 2 * score_tol(s)), (got[0], s)
    assert np.array_equal(got[2], ref.label_index.cpu().numpy())  # (random inputs: no ties)
    check("classic", 1, lp, labels, ll, tl, got, what="classic caller-side route")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_producer_formats_read_in_place(kind):
    """bfloat16, float16, time-major storage and an unaligned base with V = 260 (the element-wise access path) give the path of
    float32 on the converted values bit for bit: the conversions are exact, so the chain sees the same numbers."""
    B, T, V, U = 3, 90, 260, 20
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=9)
    xt = dev(x)
    x_tm = xt.transpose(0, 1).contiguous()
    x_tm16 = xt.to(torch.bfloat16).transpose(0, 1).contiguous()
    offset = torch.zeros(B * T * V + 1, device=DEV)[1:].view(B, T, V).copy_(xt)
    assert offset.data_ptr() % 16 == 4
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16)),
                      ("time-major float32", x_tm.transpose(0, 1)), ("time-major bfloat16", x_tm16.transpose(0, 1)),
                      ("offset base", offset)):
        x32 = xin.float().contiguous()
        got = run(kind, 0, xin, labels, ll, tl)
        ref = run(kind, 0, x32, labels, ll, tl)
        for k in (1, 2, 3, 4):
            assert np.array_equal(got[k], ref[k]), (name, k)
        assert np.all(np.abs(got[0] - ref[0]) <= 2 * score_tol(ref[0])), (name, got[0], ref[0])
        check(kind, 0, x32.cpu().numpy(), labels, ll, tl, got, what=f"{kind} {name}")


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("blank", [1, 8])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_nonzero_blank(kind, blank, wrt):
    """The blank in the first non-zero and in the last column; wildcards at the first and last label position."""
    B, T, V, U = 4, 70, 9, 25
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=61 + blank, blank=blank, scale=3.0)
    if wrt:
        x = logprobs32(x)
    got = run(kind, wrt, x, labels, ll, tl, blank)
    check(kind, wrt, x, labels, ll, tl, got, blank, what=f"{kind} wrt={wrt} blank={blank}")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_infeasible_utterances(kind):
    """-inf and -1 everywhere exactly where the oracle says so, and the feasible neighbours are what they are on their own."""
    from tf_seq2seq_losses_amd import _lib, ops
    B, T, V, U = 9, 30, 12, 6
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=13)
    labels[0, :6], ll[0], tl[0] = [W, 1, W, 2, W, W], 6, 5   # fewer frames than positions: a wildcard needs a frame of its own
    labels[1, 2], ll[1] = 0, 6                               # the blank inside the label
    labels[2, 1], ll[2] = -1, 6
    labels[3, 0], ll[3] = -3, 6
    labels[4, 3], ll[4] = V, 6
    x[5, 7, :], tl[5] = -np.inf, T                           # a row that is -inf throughout
    ll[6] = 0                                                # empty label: the all-blank path
    tl[7] = 0                                                # no frames, non-empty label
    got = run(kind, 0, x, labels, ll, tl)
    check(kind, 0, x, labels, ll, tl, got, what=f"{kind} infeasible mix")
    assert np.array_equal(np.isfinite(got[0]), [False] * 6 + [True, False, True])
    assert np.all(got[1][6, :tl[6]] == 0) and np.all(got[2][6] == -1)
    alone = run(kind, 0, x[8:], labels[8:], ll[8:], tl[8:])
    for k in range(6):
        assert np.array_equal(got[k][8:], alone[k]), k
    got1 = run(kind, 1, x, labels, ll, tl)                   # the -inf row as a log-probability
    assert np.array_equal(np.isfinite(got1[0]), [False] * 6 + [True, False, True])
    # label_length > U: a static bound below the label's length
    p = ops.Prepared(dev(labels), dev(x), dev(ll), dev(tl), 0, U=4)
    out = tuple(a.cpu().numpy() for a in ops.wildcard_best_path(ops.KINDS[kind], _lib.WRT_LOGITS, p))
    assert out[3].shape == (B, 4)
    for b in range(B):
        if ll[b] > 4:
            assert out[0][b] == -np.inf and np.all(out[1][b] == -1) and np.all(out[2][b] == -1)
            assert np.all(out[3][b] == -1) and np.all(out[4][b] == -1) and np.all(out[5][b] == -np.inf)
        else:
            assert out[0][b] == got[0][b] and np.array_equal(out[1][b], got[1][b]) and np.array_equal(out[3][b], got[3][b, :4])


def test_empty_shapes():
    import tf_seq2seq_losses_amd as ctc
    i32 = dict(dtype=torch.int32, device=DEV)
    z = ctc.classic_ctc_wildcard_alignment(torch.zeros((0, 2), **i32), torch.zeros((0, 4, 3), device=DEV), torch.zeros(0, **i32),
                                           torch.zeros(0, **i32))
    assert z.score.shape == (0,) and z.tokens.shape == (0, 4) and z.label_index.shape == (0, 4)
    assert z.first_frame.shape == z.last_frame.shape == z.label_score.shape == (0, 2)
    z = ctc.simplified_ctc_wildcard_alignment(torch.tensor([[W, 2], [1, 2]], **i32), torch.zeros((2, 0, 3), device=DEV),
                                              torch.tensor([2, 0], **i32), torch.zeros(2, **i32))
    torch.cuda.synchronize()
    assert z.tokens.shape == (2, 0) and z.score.cpu().tolist() == [-np.inf, 0.0]
    assert np.all(z.first_frame.cpu().numpy() == -1) and np.all(z.last_frame.cpu().numpy() == -1)
    assert np.all(z.label_score.cpu().numpy() == -np.inf)


def test_cpu_tensors_are_refused():
    import tf_seq2seq_losses_amd as ctc
    with pytest.raises(RuntimeError):
        ctc.classic_ctc_wildcard_alignment(torch.tensor([[W, 2]], dtype=torch.int32), torch.zeros((1, 4, 3)), torch.tensor([2]),
                                           torch.tensor([4]))


def test_check_labels_keeps_rejecting_the_wildcard():
    import tf_seq2seq_losses_amd as ctc
    with pytest.raises(ValueError):
        ctc.check_labels(torch.tensor([[1, W]], dtype=torch.int32, device=DEV), torch.tensor([2], device=DEV), 5, 0)


@pytest.mark.parametrize("kind", VO.KINDS)
def test_two_runs_are_bit_identical(kind):
    B, T, V, U = 8, 200, 16, 90
    x, labels, ll, tl = make_inputs(kind, B, T, V, U, seed=17)
    x = np.round(x * 4) / 4  # quarter steps: plenty of exact ties between paths
    a = run(kind, 0, x, labels, ll, tl)
    b = run(kind, 0, x, labels, ll, tl)
    for k in range(6):
        assert a[k].tobytes() == b[k].tobytes(), k
    check(kind, 0, x, labels, ll, tl, a, what=f"{kind} tied logits")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_in_a_hip_graph(kind):
    """One launch on a single stream: captured once and replayed on new data it reproduces the eager call."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V, U = 4, 90, 16, 20
    k = ops.KINDS[kind]
    x = torch.zeros((B, T, V), device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    labels, ll, tl = torch.zeros((B, U), **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
    outs = [torch.zeros(B, device=DEV), torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.zeros((B, U), **i32),
            torch.zeros((B, U), **i32), torch.zeros((B, U), device=DEV)]
    ws = torch.zeros(max(_lib.wildcard_best_path_workspace_bytes(k, B, T, V, U), 1), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_wildcard_best_path(k, _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), U, ll.data_ptr(),
                                            tl.data_ptr(), 0, B, T, V, U, *(o.data_ptr() for o in outs),
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
    h = fill(2)
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
    check(kind, 0, *h, got, what=f"{kind} graph replay")
