"""Long-form forced alignment on the GPU (ctc_amd_long_best_path, csrc/ctc_align_long.hip): transcripts beyond 1024 labels, the
lattice tiled over label blocks of 1024 positions x time blocks of frames_per_tile frames.  The reference is the float64 oracle
tests/tools/viterbi_oracle.py, computed once per input and shared.

Bounds: the project's own, from tests/test_gpu_alignment.py (derived there): the returned path reduces to the labels (exact); oracle
optimum - float64 value of the returned path <= 1e-6; |score - oracle| <= 1e-4 + 1e-6 |score|.  Paths are compared by value, except
where a planted optimum is unique (tokens element for element) and where two runs of the same recursion are compared (bits).
Every figure is printed before it is asserted (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from tests import _ownership as OWN
from tests import test_gpu_alignment as GA
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
UB = 1024        # label positions per label block
TF_MIN = 4       # CTC_AMD_LONG_FRAMES_MULTIPLE: the smallest legal frames_per_tile


def run(kind, wrt, x, labels, ll, tl, blank=0, tf=None, **kw):
    """(score, tokens, label_index, first_frame, last_frame) as NumPy arrays."""
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    args = (torch.from_numpy(labels).to(DEV), xt, torch.from_numpy(ll).to(DEV), torch.from_numpy(tl).to(DEV), blank)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        out = ctc.ctc_long_alignment_from_logproba(*args, cls, frames_per_tile=tf, **kw)
    else:
        out = (ctc.classic_ctc_long_alignment if kind == "classic" else ctc.simplified_ctc_long_alignment)(*args, frames_per_tile=tf, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcLongAlignment)
    assert out.score.dtype == torch.float32 and not out.score.requires_grad
    assert all(t.dtype == torch.int32 for t in out[1:])
    return tuple(t.cpu().numpy() for t in out)


def check_frames(index, first, last, ll, feasible):
    """first_frame / last_frame against label_index: the first and last frame that shows i, -1 from label_length on."""
    B, U = first.shape
    for b in range(B):
        L = min(max(int(ll[b]), 0), U) if feasible[b] else 0
        assert np.all(first[b, L:] == -1) and np.all(last[b, L:] == -1), b
        if L == 0:
            continue
        t = np.nonzero(index[b] >= 0)[0]
        i = index[b, t]
        want_first, want_last = np.full(L, -1), np.full(L, -1)
        want_first[i[::-1]] = t[::-1]
        want_last[i] = t
        assert np.array_equal(first[b, :L], want_first) and np.array_equal(last[b, :L], want_last), b
        assert np.all(want_first >= 0) and np.all(want_first <= want_last)


def check(kind, wrt, x, labels, ll, tl, oracle, got, blank=0, what=""):
    """The three bounds against a precomputed oracle (score[B], paths), and the per-label frames."""
    score, tokens, index, first, last = got
    o_score, o_paths = oracle
    B, T = x.shape[0], x.shape[1]
    worst_gap, worst_err = 0.0, 0.0
    for b in range(B):
        Tb = min(max(int(tl[b]), 0), T)
        if o_paths[b] is None:
            assert score[b] == -np.inf, (what, b, score[b])
            assert np.all(tokens[b] == -1) and np.all(index[b] == -1), (what, b)
            continue
        assert np.isfinite(score[b]), (what, b, score[b], o_score[b])
        GA.check_valid(kind, tokens[b], index[b], labels[b, :max(int(ll[b]), 0)], Tb, blank)
        gap = o_score[b] - VO.path_score(x[b, :Tb], tokens[b, :Tb], wrt)
        err = abs(float(score[b]) - o_score[b])
        worst_gap, worst_err = max(worst_gap, abs(gap)), max(worst_err, err)
        print(f"LONG-ALIGN-MEASURE {what} b={b}: optimality gap {gap:.3e} (cap {GA.OPT_TOL:.0e}), |score - oracle| {err:.3e} "
              f"(bound {GA.score_tol(o_score[b]):.3e})", flush=True)
        assert -GA.OPT_TOL <= gap <= GA.OPT_TOL, (what, b, gap)
        assert err <= GA.score_tol(o_score[b]), (what, b, score[b], o_score[b])
    check_frames(index, first, last, ll, [q is not None for q in o_paths])
    return worst_gap, worst_err


def random_input(B, T, V, U, ll, tl, seed, blank=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tokens = np.array([k for k in range(V) if k != blank])
    labels = tokens[rng.integers(0, len(tokens), (B, U))].astype(np.int32)
    return x, labels, np.asarray(ll, np.int32), np.asarray(tl, np.int32)


# ---- 1: one position in the second label block, default tiles (fails without the feature: the functions do not exist) ----

@functools.lru_cache(maxsize=None)
def case1():
    return random_input(2, 1300, 32, 1025, (1025, 900), (1300, 1200), seed=11)


@functools.lru_cache(maxsize=None)
def case1_oracle(kind):
    x, labels, ll, tl = case1()
    return VO.best_path(kind, labels, x, ll, tl)


@pytest.mark.parametrize("kind", VO.KINDS)
def test_1025_labels_default_tiles(kind):
    x, labels, ll, tl = case1()
    got = run(kind, 0, x, labels, ll, tl)
    check(kind, 0, x, labels, ll, tl, case1_oracle(kind), got, what=f"{kind} U=1025")


# ---- 2: three label blocks, many time blocks, blocks wholly beyond logit_length and beyond label_length ----

@functools.lru_cache(maxsize=None)
def case2():
    return random_input(2, 2600, 32, 2100, (2100, 1500), (2600, 2300), seed=12)


@functools.lru_cache(maxsize=None)
def case2_oracle(kind):
    x, labels, ll, tl = case2()
    return VO.best_path(kind, labels, x, ll, tl)


@functools.lru_cache(maxsize=None)
def case2_run(kind, tf):
    x, labels, ll, tl = case2()
    return run(kind, 0, x, labels, ll, tl, tf=tf)


@pytest.mark.parametrize("tf", [TF_MIN, 256])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_three_label_blocks(kind, tf):
    x, labels, ll, tl = case2()
    check(kind, 0, x, labels, ll, tl, case2_oracle(kind), case2_run(kind, tf), what=f"{kind} U=2100 tf={tf}")


# ---- 3: planted paths on log-probability input: the optimum is known exactly ----

PLANT_T, PLANT_V, PLANT_U, PLANT_TF = 1300, 32, 1100, 64


def _planted_cases(kind):
    """(labels[U], path[Tb]) per utterance: crossings of the boundary 1023 -> 1024 on the first and on the last frame of a time
    block, equal labels (a blank in between: the closed state on the classic lattice), different labels straight across, different
    labels through a blank; T_b exactly what the labels need; T_b one short of that."""
    base = (1 + np.arange(PLANT_U) % 30).astype(np.int32)  # neighbours differ
    out = []
    for tc in (17 * PLANT_TF, 18 * PLANT_TF - 1):  # label 1024 is emitted on frame tc
        for equal, through_blank in ((True, True), (False, False), (False, True)):
            lab = base.copy()
            if equal:
                lab[UB] = lab[UB - 1]
            L = UB + 6
            path = np.zeros(PLANT_T, np.int64)  # blank = 0
            off = tc - UB - (1 if through_blank else 0)
            path[off + np.arange(UB)] = lab[:UB]
            path[tc + np.arange(L - UB)] = lab[UB:L]
            out.append((lab, L, path))
    lab = base.copy()
    out.append((lab, PLANT_U, lab[:PLANT_U].astype(np.int64)))        # T_b = L: the diagonal of the tile grid
    out.append((lab, PLANT_U, None))                                  # T_b = L - 1: infeasible
    return out


@pytest.mark.parametrize("kind", VO.KINDS)
def test_planted_paths_across_the_block_boundary(kind):
    cases = _planted_cases(kind)
    B = len(cases)
    x = np.full((B, PLANT_T, PLANT_V), -5.0, np.float32)
    labels = np.stack([c[0] for c in cases])
    ll = np.array([c[1] for c in cases], np.int32)
    tl = np.array([PLANT_U - 1 if c[2] is None else len(c[2]) for c in cases], np.int32)
    for b, (_, L, path) in enumerate(cases):
        if path is not None:
            assert VO.reduces_to(kind, path, 0) == [int(k) for k in labels[b, :L]]
            x[b, np.arange(len(path)), path] = 0.0
    score, tokens, index, first, last = run(kind, 1, x, labels, ll, tl, tf=PLANT_TF)
    for b, (_, L, path) in enumerate(cases):
        if path is None:
            assert score[b] == -np.inf and np.all(tokens[b] == -1) and np.all(index[b] == -1), b
            continue
        Tb = len(path)
        print(f"LONG-ALIGN-MEASURE planted {kind} b={b}: score {score[b]} (0 exactly), "
              f"{int((tokens[b, :Tb] != path).sum())} frames off the planted path", flush=True)
        assert score[b] == 0.0, (b, score[b])
        assert np.array_equal(tokens[b, :Tb], path) and np.all(tokens[b, Tb:] == -1), b
        GA.check_valid(kind, tokens[b], index[b], labels[b, :L], Tb, 0)
    check_frames(index, first, last, ll, [c[2] is not None for c in cases])


# ---- 4: one label block gives the path of the existing call ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_one_label_block_equals_the_whole_utterance_kernel(kind):
    x, labels, ll, tl = random_input(2, 1500, 32, 700, (700, 450), (1500, 1100), seed=14)
    s0, t0, i0 = GA.run(kind, 0, x, labels, ll, tl)
    s1, t1, i1, first, last = run(kind, 0, x, labels, ll, tl, tf=32)
    assert np.array_equal(t0, t1) and np.array_equal(i0, i1)
    assert np.all(np.abs(s0 - s1) <= GA.score_tol(s0)), (s0, s1)
    check_frames(i1, first, last, ll, [True, True])


# ---- 5: the path depends on nothing but the input ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_path_is_invariant(kind):
    x, labels, ll, tl = case2()
    ref = case2_run(kind, 256)
    for tf in (TF_MIN, None):  # (None: the default)
        got = case2_run(kind, tf)
        assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2]), tf
        assert np.all(np.abs(ref[0] - got[0]) <= GA.score_tol(ref[0])), tf  # (the order of the LSE sum differs)
    again = run(kind, 0, x, labels, ll, tl, tf=256)
    for a, b in zip(ref, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))  # two runs: the same bits, score included
    alone = run(kind, 0, x[:1], labels[:1], ll[:1], tl[:1], tf=256)
    for a, b in zip(ref, alone):
        assert np.array_equal(a[:1].view(np.int32), b.view(np.int32))


# ---- 6: formats ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_bfloat16_and_time_major(kind):
    x, labels, ll, tl = case1()
    xb = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    x32 = xb.to(torch.float32).contiguous()  # the same values
    ref = run(kind, 0, x32, labels, ll, tl)
    got = run(kind, 0, xb, labels, ll, tl)
    assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])
    tm = x32.transpose(0, 1).contiguous().transpose(0, 1)  # [B, T, V] view of time-major storage
    assert tm.stride() == (x.shape[2], x.shape[0] * x.shape[2], 1)
    got = run(kind, 0, tm, labels, ll, tl)
    for a, b in zip(ref, got):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("kind", VO.KINDS)
def test_unaligned_vocabulary(kind):
    x, labels, ll, tl = random_input(1, 1200, 31, 1030, (1030,), (1200,), seed=16)
    got = run(kind, 0, x, labels, ll, tl, tf=64)
    check(kind, 0, x, labels, ll, tl, VO.best_path(kind, labels, x, ll, tl), got, what=f"{kind} V=31")


# ---- 7: degenerate utterances, a non-zero blank ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_degenerate_utterances_and_last_column_blank(kind):
    V, U, T = 32, 1040, 1200
    blank = V - 1
    x, labels, ll, tl = random_input(5, T, V, U, (0, 5, 1040, 1041, 1040), (900, 0, T, T, T), seed=17, blank=blank)
    labels[2, 1030] = blank  # a label equal to the blank, in the second label block
    oracle = VO.best_path(kind, labels, x, ll, tl, blank)
    assert [q is None for q in oracle[1]] == [False, True, True, True, False]
    got = run(kind, 0, x, labels, ll, tl, blank=blank, tf=64)
    check(kind, 0, x, labels, ll, tl, oracle, got, blank=blank, what=f"{kind} degenerate")
    assert np.all(got[1][0, :900] == blank)  # label_length = 0: the all-blank path


# ---- 8: ownership ----

def _guarded(shape, dtype, pattern, guard=64):
    n = int(np.prod(shape))
    buf = OWN.filled((n + 2 * guard,), dtype, pattern, DEV)
    return buf, buf[guard:guard + n].view(shape)


def _abi_call(inp, tf, pattern):
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U = inp.shape
    ws = OWN.workspace(_lib.long_best_path_workspace_bytes(inp.kind, B, T, V, U, tf) + 512, pattern)
    bufs = {"score": _guarded((B,), torch.float32, pattern), "tokens": _guarded((B, T), torch.int32, pattern),
            "label_index": _guarded((B, T), torch.int32, pattern), "first_frame": _guarded((B, U), torch.int32, pattern),
            "last_frame": _guarded((B, U), torch.int32, pattern)}
    rc = lib.ctc_amd_long_best_path(*inp.common_ex(0), tf, *(v[1].data_ptr() for v in bufs.values()), ws.data_ptr() + 256,
                                    ws.numel() - 512, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():  # nothing around the outputs is written
        keep = OWN.keeps_prefill(buf, pattern)
        assert bool(keep[:64].all()) and bool(keep[-64:].all()), name
    keep = OWN.keeps_prefill(ws, pattern)  # ... nor around the workspace
    assert bool(keep[:256].all()) and bool(keep[-256:].all())
    return {name: view for name, (buf, view) in bufs.items()}


@pytest.mark.parametrize("kind", VO.KINDS)
def test_ownership(kind):
    x, labels, ll, tl = random_input(2, 1200, 32, 1030, (1030, 300), (1200, 500), seed=18)
    clean = OWN.make_inputs(VO.KINDS.index(kind), x, labels, ll, tl)
    a = _abi_call(clean, 64, 0xA5)
    # every output element is written, the tails with -1 (0xA5 and 0x00 are neither -1 nor a plausible result everywhere)
    assert bool((a["tokens"][1, 500:] == -1).all()) and bool((a["label_index"][1, 500:] == -1).all())
    assert bool((a["first_frame"][1, 300:] == -1).all()) and bool((a["last_frame"][1, 300:] == -1).all())
    for name, t in a.items():
        assert not bool(OWN.keeps_prefill(t, 0xA5).any()), name
    # what the utterances do not own may hold anything: padding frames, label tails, the outputs and the workspace on entry
    xt = torch.from_numpy(x).to(DEV)
    for pattern, value in ((0x00, float("nan")), (0xFF, 3.0e38)):
        dirty = clean.replace(x=OWN.poison_padding(xt, tl, value),
                              labels=OWN.poison_labels(clean.labels, ll, OWN.label_poison_cycle(32, 0)))
        b = _abi_call(dirty, 64, pattern)
        diff = OWN.total_diff(a, b)
        assert not any(diff.values()), (pattern, diff)
