"""Long-form forced alignment with optional wildcards and the exclusion of the next label on the GPU
(ctc_amd_long_optional_wildcard_best_path / ctc_amd_long_star_best_path, csrc/ctc_align_long_star.hip).
The reference is the float64 oracle tests/tools/star_exclusion_oracle.py::best_path.

Bars, the project's: the returned (tokens, label_index) is admissible (`admissible`, exact); oracle optimum - float64 value of the
returned path <= OPT_TOL = 1e-6; |score - oracle| <= 1e-4 + 1e-6 |score|; the same bar for every label_score against the float64 sum
over its frames and for sum(label_score) + the blank frames against score.  Paths are compared with the oracle's only where a planted
optimum is unique, and bit for bit where two runs of the same recursion are compared.  Classic label blocks hold 512 positions,
simplified ones 1024."""
import functools

import numpy as np
import pytest
import torch

from tests.tools import star_exclusion_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, Q = SO.WILDCARD, SO.OPTIONAL
OPT_TOL = 1e-6
NAMES = ("score", "tokens", "label_index", "first_frame", "last_frame", "label_score")
MODES = [(True, False), (False, True), (True, True)]  # (optional_wildcards, exclude_next_label)


def tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(kind, wrt, x, labels, ll, tl, mode, blank=0, tf=64, long=True, **kw):
    import tf_seq2seq_losses_amd as ctc
    stem = "long_wildcard_alignment" if long else "wildcard_alignment"
    args = (dev(labels), dev(x), dev(ll), dev(tl), blank)
    kw.update(dict(frames_per_tile=tf) if long else {})
    if mode is not None:
        kw.update(optional_wildcards=mode[0], exclude_next_label=mode[1])
    if wrt:
        out = getattr(ctc, f"ctc_{stem}_from_logproba")(*args, ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData, **kw)
    else:
        out = getattr(ctc, f"{kind}_ctc_{stem}")(*args, **kw)
    torch.cuda.synchronize()
    assert not out.score.requires_grad and out.label_score.dtype == torch.float32
    return tuple(t.cpu().numpy() for t in out)


def same_bits(a, b, names=NAMES[1:]):
    for name in names:
        k = NAMES.index(name)
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), name


def admissible(kind, lab, tokens, index, wild, y, opt, blank):
    """A path of the lattice: label_index monotone with steps of 1, or 2 over an optional wildcard, from the first position to the last
    (or their neighbour past an optional one); every position's frames contiguous, one frame per ordinary position on the simplified
    lattice; tokens as the positions prescribe; a blank between equal neighbours on the classic one."""
    L, on = len(lab), np.nonzero(index >= 0)[0]
    seq = index[on]
    pos = seq[np.concatenate([[True], seq[1:] != seq[:-1]])] if len(seq) else seq
    assert np.all(np.diff(pos) >= 1) and np.all((np.diff(pos) == 1) | ((np.diff(pos) == 2) & opt[pos[1:] - 1]))
    if len(pos) == 0:
        assert L == 0 or (L == 1 and opt[0])
    else:
        assert (pos[0] == 0 or (pos[0] == 1 and opt[0])) and (pos[-1] == L - 1 or (pos[-1] == L - 2 and opt[L - 1]))
    assert np.all(tokens[index < 0] == blank)
    w = wild[seq]
    assert np.array_equal(tokens[on][~w], lab[seq][~w]) and np.all(tokens[on][w] != y[seq][w]) and np.all(tokens[on][w] >= 0)
    for a, c in zip(pos[:-1], pos[1:]):
        fa, fc = on[seq == a], on[seq == c]
        assert fa[-1] - fa[0] + 1 == len(fa) and (kind == "classic" or wild[a] or len(fa) == 1)
        if kind == "classic" and not wild[a] and not wild[c] and lab[a] == lab[c]:
            assert fc[0] > fa[-1] + 1


def check(kind, wrt, x, labels, ll, tl, got, mode, blank=0, what=""):
    ref_score, rest = SO.best_path(kind, labels, x, ll, tl, blank, wrt, optional=mode[0], exclude=mode[1])
    score, tokens, index, first, last, ls = got
    for b, r in enumerate(rest):
        Tb, L = int(tl[b]), int(ll[b])
        if r is None:
            assert score[b] == -np.inf and np.all(tokens[b] == -1) and np.all(index[b] == -1), (what, b)
            assert np.all(first[b] == -1) and np.all(last[b] == -1) and np.all(ls[b] == -np.inf), (what, b)
            continue
        lab = labels[b, :L].astype(np.int64)
        wild, y = SO.excluded_tokens([int(k) for k in lab], x.shape[2], blank, mode[0], mode[1])
        opt = (lab == Q) & mode[0]
        admissible(kind, lab, tokens[b, :Tb], index[b, :Tb], np.asarray(wild, bool), np.asarray(y), opt, blank)
        lp = SO.log_probs(x[b, :Tb], wrt)[np.arange(Tb), tokens[b, :Tb]]
        gap = ref_score[b] - lp.sum()
        sums = np.array([lp[index[b, :Tb] == i].sum() for i in range(L)])
        e_score, e_ls = abs(score[b] - ref_score[b]), np.abs(ls[b, :L] - sums).max() if L else 0.0
        e_sum = abs(ls[b, :L].astype(np.float64).sum() + lp[index[b, :Tb] < 0].sum() - score[b])
        print(f"{what} b={b}: gap {gap:.3g} score {e_score:.3g} label_score {e_ls:.3g} sum rule {e_sum:.3g}")
        assert gap <= OPT_TOL and e_score <= tol(ref_score[b]) and e_ls <= tol(ref_score[b]) and e_sum <= tol(ref_score[b]), (what, b)
        assert np.all(tokens[b, Tb:] == -1) and np.all(index[b, Tb:] == -1) and np.all(first[b, L:] == -1) and np.all(ls[b, L:] == -np.inf)
        for i in range(L):
            t = np.nonzero(index[b, :Tb] == i)[0]
            assert (first[b, i], last[b, i]) == ((t[0], t[-1]) if len(t) else (-1, -1)) and (len(t) or ls[b, i] == 0.0), (what, b, i)


def base_labels(B, U):
    return np.tile(1 + np.arange(U) % 6, (B, 1)).astype(np.int32)  # neighbours, and neighbours' neighbours, differ


def logits(seed, B, T, V):
    return (np.random.default_rng(seed).standard_normal((B, T, V)) * 2.0).astype(np.float32)


# ---- 1: stars of both kinds on both sides of both block boundaries ----

@functools.lru_cache(maxsize=None)
def boundaries(optional):
    """Utterance 1 has exactly as many frames as ordinary positions: its two optional stars are skipped across position 512 and 1024.
    The stars at 511 and 1023 sit on a block's last position and exclude the label that opens the next block."""
    labels, o = base_labels(3, 1100), Q if optional else W
    for b, stars in enumerate(({510: o, 512: W, 1022: o, 1023: W}, {511: o, 1023: o, 1024: W}, {510: W, 511: W, 512: o})):
        for i, v in stars.items():
            labels[b, i] = v
    ll, tl = np.array([1100, 1030, 513], np.int32), np.array([1400, 1028 if optional else 1030, 700], np.int32)
    return logits(31, 3, 1400, 8), labels, ll, tl


@functools.lru_cache(maxsize=None)
def boundaries_run(kind, mode, tf=64):
    return run(kind, 0, *boundaries(mode[0]), mode, tf=tf)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", SO.KINDS)
def test_boundaries(kind, mode):
    got = boundaries_run(kind, mode)
    check(kind, 0, *boundaries(mode[0]), got, mode, what=f"boundaries {kind} {mode}")
    if mode[0]:
        assert got[3][1, 511] == -1 and got[3][1, 1023] == -1 and got[5][1, 511] == 0.0  # skipped for want of frames


# ---- 2: a planted, unique optimum through every label block ----

def planted(optional):
    """(x, labels, ll, tl) on log-probability input: every ordinary label has one frame, the stars at 511 and 1500 a run of foreign
    tokens, those at 0, 1023 and 2099 no frame (not optional: one foreign frame), and the star at 1024 one frame whose row maximum is
    the label behind it."""
    T, V, U, far = 2700, 32, 2100, 31
    lab = (1 + np.arange(U) % 30).astype(np.int32)
    seq = []
    for i in range(U):
        if i in (0, 1023, 2099):
            lab[i] = Q if optional else W
            seq += [] if optional else [far]
        elif i in (511, 1500):
            lab[i] = Q if optional else W
            seq += [far, far, 0, far, 0, 0, far] * 20
        elif i == 1024:
            lab[i], star = W, len(seq)
            seq += [lab[1025]]
        else:
            seq += [lab[i]]
    x = np.full((1, T, V), -5.0, np.float32)
    x[0, np.arange(len(seq)), seq] = 0.0
    x[0, star, far] = -1.0
    return x, lab[None], np.array([U], np.int32), np.array([len(seq)], np.int32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", SO.KINDS)
def test_planted_optimum_exact_path(kind, mode):
    x, labels, ll, tl = planted(mode[0])
    got = run(kind, 1, x, labels, ll, tl, mode)
    _, (r,) = SO.best_path(kind, labels, x, ll, tl, 0, 1, optional=mode[0], exclude=mode[1])
    Tb = int(tl[0])
    for k, ref in ((1, r[0]), (2, r[1])):
        assert np.array_equal(got[k][0, :Tb], ref), NAMES[k]
    assert np.array_equal(got[3][0], r[2]) and np.array_equal(got[4][0], r[3])
    assert (got[1][0, int(r[2][1024])] == 31) == mode[1]  # the excluded row maximum is not the token reported


# ---- 3: end states and degenerate utterances ----

@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("kind", SO.KINDS)
def test_end_states_and_degenerate_utterances(kind, exclude):
    U, T = 1029, 1040
    labels = base_labels(10, U)
    ll = np.array([1025, 1025, 1026, 1026, 513, 513, 1, 1029, 1029, 1029], np.int32)
    tl = np.array([1025, 1024, 1026, 1025, 600, 512, 0, 1040, 600, 500], np.int32)  # an optional last star used / skipped, in turn
    for b in range(7):
        labels[b, ll[b] - 1] = Q
    labels[7, 1023] = labels[7, 1024] = Q  # adjacent: infeasible
    labels[8:, 0::2] = Q                   # star temporal classification: 514 labels between 515 stars
    x = logits(33, 10, T, 8)
    got = run(kind, 0, x, labels, ll, tl, (True, exclude))
    check(kind, 0, x, labels, ll, tl, got, (True, exclude), what=f"ends {kind} exclude={exclude}")
    assert np.array_equal(np.isfinite(got[0]), [1, 1, 1, 1, 1, 1, 1, 0, 1, 0]) and got[0][6] == 0.0
    assert got[3][1, 1024] == -1 and got[3][3, 1025] == -1 and got[3][5, 512] == -1 and got[3][6, 0] == -1 and got[5][6, 0] == 0.0


# ---- 4: invariance and equalities, bit for bit ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", SO.KINDS)
def test_tiles_and_batch_composition(kind, mode):
    x, labels, ll, tl = boundaries(mode[0])
    ref = boundaries_run(kind, mode)
    for tf in (4, 128):
        same_bits(ref, boundaries_run(kind, mode, tf))
    alone = run(kind, 0, x[1:2], labels[1:2], ll[1:2], tl[1:2], mode, max_label_length=labels.shape[1])
    same_bits(tuple(a[1:2] for a in ref), alone)


@pytest.mark.parametrize("kind", SO.KINDS)
def test_equal_to_the_existing_calls(kind):
    x, labels, ll, tl = boundaries(False)
    plain = np.where(labels < 0, 7, labels).astype(np.int32)
    plain[:, 600] = W  # (a wildcard behind which another one stands excludes nothing)
    plain[:, 601] = W
    for mode in MODES:
        same_bits(run(kind, 0, x, plain, ll, tl, mode), run(kind, 0, x, plain, ll, tl, None))
    ub = 512 if kind == "classic" else 1024  # one label block: the short-form call with the same keywords
    x, labels = logits(34, 2, 1300, 8), base_labels(2, ub)
    labels[:, [0, 7, 8, 200, ub - 1]] = [Q, W, Q, W, Q]
    ll, tl = np.array([ub, ub - 3], np.int32), np.array([1300, ub - 4], np.int32)
    for mode in MODES:
        same_bits(run(kind, 0, x, labels, ll, tl, mode), run(kind, 0, x, labels, ll, tl, mode, long=False))


@pytest.mark.parametrize("kind", SO.KINDS)
def test_exact_workspace_prefill_and_graph(kind):
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib
    lib, k = _lib.load(), SO.KINDS.index(kind)
    x, labels, ll, tl = boundaries(True)
    B, T, V = x.shape
    U = labels.shape[1]
    t = [dev(a) for a in (x, labels, ll, tl)]
    n = _lib.long_star_best_path_workspace_bytes(k, B, T, V, U, 64, True)
    for fill in (0x00, 0xFF):
        buf = lambda shape, dtype: torch.full((int(np.prod(shape)) * 4,), fill, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)
        out = [buf((B,), torch.float32), buf((B, T), torch.int32), buf((B, T), torch.int32), buf((B, U), torch.int32),
               buf((B, U), torch.int32), buf((B, U), torch.float32)]
        w = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
        rc = lib.ctc_amd_long_star_best_path(k, 0, t[0].data_ptr(), 0, T * V, V, t[1].data_ptr(), U, t[2].data_ptr(), t[3].data_ptr(), 0, 1,
                                             B, T, V, U, 64, *(v.data_ptr() for v in out), w.data_ptr(), n, None)
        assert rc == 0, lib.ctc_amd_last_error()
        torch.cuda.synchronize()
        same_bits(boundaries_run(kind, (True, True)), tuple(v.cpu().numpy() for v in out), NAMES)
    fn = ctc.classic_ctc_long_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_long_wildcard_alignment
    work = lambda: fn(t[1], t[0], t[2], t[3], 0, frames_per_tile=64, max_label_length=U, optional_wildcards=True, exclude_next_label=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a = work()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    same_bits(boundaries_run(kind, (True, True)), tuple(v.cpu().numpy() for v in a), NAMES)


# ---- 5: formats and axes, one case each ----

@pytest.mark.parametrize("case", ["bfloat16", "time_major", "blank_last", "wide"])
@pytest.mark.parametrize("kind", SO.KINDS)
def test_formats_and_axes(kind, case):
    B, T, U, V, blank = 2, 1200, 1030, (1030 if case == "wide" else 8), (7 if case == "blank_last" else 0)
    labels = base_labels(B, U) - (1 if blank else 0)
    labels[:, [5, 511, 1023, 1029]] = [W, Q, W, Q]
    ll, tl = np.array([1030, 700], np.int32), np.array([1200, 1100], np.int32)
    x = logits(35, B, T, V)
    if case == "wide":  # the second round of the row pass; in round one the best token is the one the star at 5 and 1023 excludes
        x[:, :, int(labels[0, 6])] += 6.0
        x[:, :, 700] += 5.0
    xd = dev(x)
    if case == "bfloat16":
        xd = xd.bfloat16()
        x = xd.float().cpu().numpy()
    elif case == "time_major":
        xd = dev(np.ascontiguousarray(x.transpose(1, 0, 2))).transpose(0, 1)
    got = run(kind, 0, xd, labels, ll, tl, (True, True), blank=blank)
    check(kind, 0, x, labels, ll, tl, got, (True, True), blank=blank, what=f"{case} {kind}")


def test_frame_window_with_either_keyword_is_refused():
    x, labels, ll, tl = boundaries(True)
    fw = np.zeros((3, 1100, 2), np.int32)
    for mode in MODES:
        with pytest.raises(ValueError):
            run("classic", 0, x, labels, ll, tl, mode, frame_window=fw)
