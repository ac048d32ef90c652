"""Long-form forced alignment with wildcard labels on the GPU (ctc_amd_long_wildcard_best_path, csrc/ctc_align_long_wild.hip):
partial transcripts beyond 1024 labels, with label_score.  The reference is the float64 oracle tests/tools/wildcard_oracle.py.

Bars: those of tests/test_gpu_wildcard_alignment.py (derived in tests/test_gpu_alignment.py), through that file's own `check`:
the returned (tokens, label_index) is admissible (check_admissible, exact); oracle optimum - float64 value of the returned path
<= OPT_TOL = 1e-6; |score - oracle| <= score_tol; every label_score against the float64 sum over its frames and sum(label_score)
+ the blank frames' lp against score <= score_tol.  Paths are compared by admissibility and value, never with the oracle's path,
except where a planted optimum is unique (tokens element for element) and where two runs of the same recursion are compared
(bits).  Every figure is printed before it is asserted (pytest -s shows them)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import _ownership as OWN
from tests import test_gpu_long_alignment as GL
from tests import test_gpu_wildcard_alignment as WA
from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
UB = 1024  # label positions per label block
W = WA.W
NAMES = ("score", "tokens", "label_index", "first_frame", "last_frame", "label_score")


def run(kind, wrt, x, labels, ll, tl, blank=0, tf=None, **kw):
    """(score, tokens, label_index, first_frame, last_frame, label_score) as NumPy arrays."""
    import tf_seq2seq_losses_amd as ctc
    args = (WA.dev(labels), WA.dev(x), WA.dev(ll), WA.dev(tl), blank)
    if wrt:
        cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
        out = ctc.ctc_long_wildcard_alignment_from_logproba(*args, cls, frames_per_tile=tf, **kw)
    else:
        fn = ctc.classic_ctc_long_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_long_wildcard_alignment
        out = fn(*args, frames_per_tile=tf, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcLongWildcardAlignment)
    assert out.score.dtype == torch.float32 and out.label_score.dtype == torch.float32
    assert all(t.dtype == torch.int32 for t in (out.tokens, out.label_index, out.first_frame, out.last_frame))
    assert not out.score.requires_grad and not out.label_score.requires_grad
    return tuple(t.cpu().numpy() for t in out)


def wild_input(B, T, V, U, ll, tl, seed, wild, blank=0):
    """Random logits and labels (tests/test_gpu_long_alignment.random_input) with wildcards at wild[b]; feasible on both lattices."""
    x, labels, ll, tl = GL.random_input(B, T, V, U, ll, tl, seed, blank)
    for b, positions in enumerate(wild):
        for i in positions:
            assert 0 <= i < ll[b]
            labels[b, i] = W
    for b in range(B):
        assert WA.needed_frames("classic", labels[b, :ll[b]]) <= tl[b], b
    return x, labels, ll, tl


def same_bits(a, b, names=NAMES):
    for name in names:
        k = NAMES.index(name)
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), name


# ---- 1: one position in the second label block, wildcards on both sides of the block boundary ----

@functools.lru_cache(maxsize=None)
def case1():
    return wild_input(2, 1400, 32, 1025, (1025, 900), (1400, 1300), seed=21, wild=((0, 1023, 1024), (450,)))


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_1025_labels_default_tiles(kind, wrt):
    x, labels, ll, tl = case1()
    assert labels[0, 0] == W and labels[0, 1023] == W and labels[0, 1024] == W and ll[0] - 1 == 1024  # (L - 1 = 1024)
    if wrt:
        x = WA.logprobs32(x)
    got = run(kind, wrt, x, labels, ll, tl)
    WA.check(kind, wrt, x, labels, ll, tl, got, what=f"long {kind} wrt={wrt} U=1025")


# ---- 2: three label blocks, blocks wholly beyond label_length and beyond logit_length ----

@functools.lru_cache(maxsize=None)
def case2():
    return wild_input(2, 2700, 32, 2100, (2100, 1500), (2700, 2400), seed=22,
                      wild=((0, 500, 1023, 2048, 2099), (1023, 1024, 1300)))


@functools.lru_cache(maxsize=None)
def case2_run(kind, tf):
    x, labels, ll, tl = case2()
    return run(kind, 0, x, labels, ll, tl, tf=tf)


@pytest.mark.parametrize("tf", [4, 256])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_three_label_blocks(kind, tf):
    x, labels, ll, tl = case2()
    WA.check(kind, 0, x, labels, ll, tl, case2_run(kind, tf), what=f"long {kind} U=2100 tf={tf}")


# ---- 3: planted regions on log-probability input: the optimum is known exactly ----

PLANT_T, PLANT_V, PLANT_U, PLANT_TF = 1400, 32, 1100, 64
FOREIGN = 31  # a token no label uses: only a wildcard takes its frames for nothing


def _junk(n):
    """n frames of untranscribed material: foreign tokens with blanks among them, a foreign token first and last."""
    j = np.full(n, FOREIGN, np.int64)
    j[2:n - 2:3] = 0
    return j


def _planted_cases():
    """(labels[U], L, T_b, path or None) per utterance.  A wildcard at position 1023 and at 1024 whose run starts on the first and on
    the last frame of a time block and spans more than two of them; a free start and a free end; T_b exactly what the positions
    need; T_b one short of that.  Neighbouring labels differ and every known label has exactly one frame, so each optimum is unique."""
    base = (1 + np.arange(PLANT_U) % 30).astype(np.int32)
    out = []
    for w in (UB - 1, UB):
        for tj in (17 * PLANT_TF, 18 * PLANT_TF - 1):  # the wildcard's first frame
            lab, L, n = base.copy(), UB + 6, 150
            lab[w] = W
            path = np.zeros(PLANT_T, np.int64)  # blank = 0
            path[tj - w + np.arange(w)] = lab[:w]
            path[tj:tj + n] = _junk(n)
            path[tj + n + np.arange(L - w - 1)] = lab[w + 1:L]
            out.append((lab, L, PLANT_T, path))
    lab, L, Tb = base.copy(), UB + 6, 1300
    lab[0] = lab[L - 1] = W
    path = np.concatenate([_junk(40), lab[1:L - 1].astype(np.int64), _junk(Tb - 40 - (L - 2))])
    out.append((lab, L, Tb, path))
    lab = base.copy()
    lab[UB - 1] = lab[UB] = W  # adjacent, across the boundary: a frame each
    path = np.where(lab == W, FOREIGN, lab).astype(np.int64)
    out.append((lab, PLANT_U, PLANT_U, path))       # T_b = the number of positions
    out.append((lab, PLANT_U, PLANT_U - 1, None))   # one frame short: infeasible
    return out


@pytest.mark.parametrize("kind", VO.KINDS)
def test_planted_regions_across_the_block_boundary(kind):
    import tf_seq2seq_losses_amd as ctc
    cases = _planted_cases()
    B = len(cases)
    x = np.full((B, PLANT_T, PLANT_V), -5.0, np.float32)
    labels = np.stack([c[0] for c in cases])
    ll = np.array([c[1] for c in cases], np.int32)
    tl = np.array([c[2] for c in cases], np.int32)
    for b, (_, L, Tb, path) in enumerate(cases):
        src = path if path is not None else cases[b - 1][3]  # (the short one: the same material, one frame less)
        x[b, np.arange(Tb), src[:Tb]] = 0.0
    got = run(kind, 1, x, labels, ll, tl, tf=PLANT_TF)
    score, tokens, index, first, last, ls = got
    for b, (_, L, Tb, path) in enumerate(cases):
        if path is None:
            assert score[b] == -np.inf and np.all(tokens[b] == -1) and np.all(index[b] == -1), b
            assert np.all(first[b] == -1) and np.all(last[b] == -1) and np.all(ls[b] == -np.inf), b
            continue
        print(f"LONG-WILD-MEASURE planted {kind} b={b}: score {score[b]} (0 exactly), "
              f"{int((tokens[b, :Tb] != path[:Tb]).sum())} frames off the planted path", flush=True)
        assert score[b] == 0.0, (b, score[b])
        assert np.array_equal(tokens[b, :Tb], path[:Tb]) and np.all(tokens[b, Tb:] == -1), b
        assert np.all(ls[b, :L] == 0.0), b
    WA.check(kind, 1, x, labels, ll, tl, got, what=f"long {kind} planted")
    # what the feature adds: the plain long-form call has no wildcards, so these labels are not a transcript to it
    short = B - 1
    plain = ctc.classic_ctc_long_alignment(WA.dev(labels[short:]), WA.dev(x[short:]), WA.dev(ll[short:]), WA.dev(tl[short:]), 0,
                                           frames_per_tile=PLANT_TF)
    assert float(plain.score.cpu()[0]) == -np.inf


# ---- 4: without a wildcard it is the plain long-form alignment ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_without_a_wildcard_it_is_the_long_alignment(kind):
    x, labels, ll, tl = GL.case2()
    for tf in (64, 256):
        ref = GL.run(kind, 0, x, labels, ll, tl, tf=tf)
        got = run(kind, 0, x, labels, ll, tl, tf=tf)
        for k in (1, 2, 3, 4):
            assert got[k].tobytes() == ref[k].tobytes(), (tf, NAMES[k])
        d = np.abs(got[0] - ref[0])
        print(f"LONG-WILD-MEASURE {kind} no wildcard tf={tf}: |score - long alignment| {d.max():.3e}", flush=True)
        assert np.all(d <= WA.score_tol(ref[0])), (got[0], ref[0])


# ---- 5: one label block gives the path of the whole-utterance wildcard call ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_one_label_block_equals_the_whole_utterance_kernel(kind):
    x, labels, ll, tl = WA.make_inputs(kind, 2, 1000, 32, 700, seed=23)
    assert np.any(labels[0, :700] == W)
    ref = WA.run(kind, 0, x, labels, ll, tl)
    got = run(kind, 0, x, labels, ll, tl, tf=32)
    for k in (1, 2, 3, 4):
        assert np.array_equal(got[k], ref[k]), NAMES[k]
    assert np.all(np.abs(got[0] - ref[0]) <= WA.score_tol(ref[0])), (got[0], ref[0])
    fin = np.isfinite(ref[5])
    assert np.array_equal(fin, np.isfinite(got[5]))
    print(f"LONG-WILD-MEASURE {kind} U=700: |score - whole-utterance| {np.abs(got[0] - ref[0]).max():.3e}, "
          f"|label_score - whole-utterance| {np.abs(got[5][fin] - ref[5][fin]).max():.3e}", flush=True)
    assert np.all(np.abs(got[5][fin] - ref[5][fin]) <= WA.score_tol(ref[5][fin]))


# ---- 6: a lone wildcard is the greedy decoding ----

@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_lone_wildcard_is_the_greedy_decoding(kind, wrt):
    B, T, V, width = 5, 130, 37, 1100
    rng = np.random.default_rng(41)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if wrt:
        x = WA.logprobs32(x)
    tl = np.asarray([T, 1, 64, 65, 99], np.int32)
    labels, ll = np.full((B, width), 5, np.int32), np.ones(B, np.int32)
    labels[:, 0] = W
    got = run(kind, wrt, x, labels, ll, tl, 3, max_label_length=width)  # two label blocks, the second one empty
    assert got[3].shape == (B, width)
    ref = GO.decode(kind, x, tl, 3, wrt)
    assert np.array_equal(got[1], ref.tokens) and np.all(np.abs(got[0] - ref.score) <= WA.score_tol(ref.score))
    WA.check(kind, wrt, x, labels, ll, tl, got, 3, what=f"long {kind} wrt={wrt} lone wildcard")


# ---- 7: the path and the per-label outputs depend on nothing but the utterance ----

INVARIANT = ("tokens", "label_index", "first_frame", "last_frame", "label_score")


@pytest.mark.parametrize("kind", VO.KINDS)
def test_outputs_are_invariant(kind):
    x, labels, ll, tl = case2()
    ref = case2_run(kind, 256)
    for tf in (4, 64):
        got = case2_run(kind, tf) if tf == 4 else run(kind, 0, x, labels, ll, tl, tf=tf)
        same_bits(ref, got, INVARIANT)
        assert np.all(np.abs(ref[0] - got[0]) <= WA.score_tol(ref[0])), tf  # (the order of the LSE sum differs)
    again = run(kind, 0, x, labels, ll, tl, tf=256)
    same_bits(ref, again)  # two runs of the same call: every output, score included
    U = ref[3].shape[1]
    for b in (0, 1):
        alone = run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], tf=256, max_label_length=U)
        same_bits(tuple(a[b:b + 1] for a in ref), alone, INVARIANT)
    swapped = run(kind, 0, x[::-1].copy(), labels[::-1].copy(), ll[::-1].copy(), tl[::-1].copy(), tf=64)
    same_bits(tuple(a[::-1] for a in ref), swapped, INVARIANT)


# ---- 8: formats ----

@functools.lru_cache(maxsize=None)
def case8():
    return wild_input(2, 1400, 33, 1100, (1100, 700), (1400, 1000), seed=28, wild=((0, 1023, 1024, 1099), (3, 350, 699)))


@pytest.mark.parametrize("kind", VO.KINDS)
def test_producer_formats_read_in_place(kind):
    x, labels, ll, tl = case8()  # V = 33: the element-wise access path
    xt = WA.dev(x)
    ref = run(kind, 0, xt, labels, ll, tl)
    WA.check(kind, 0, x, labels, ll, tl, ref, what=f"long {kind} V=33 float32")
    tm = xt.transpose(0, 1).contiguous().transpose(0, 1)  # [B, T, V] view of time-major storage
    assert tm.stride() == (33, 2 * 33, 1)
    same_bits(ref, run(kind, 0, tm, labels, ll, tl))
    offset = torch.zeros(x.size + 1, device=DEV)[1:].view(x.shape).copy_(xt)
    assert offset.data_ptr() % 16 == 4
    same_bits(ref, run(kind, 0, offset, labels, ll, tl))
    for name, xin in (("bfloat16", xt.to(torch.bfloat16)), ("float16", xt.to(torch.float16))):
        got = run(kind, 0, xin, labels, ll, tl)
        WA.check(kind, 0, xin.float().cpu().numpy(), labels, ll, tl, got, what=f"long {kind} V=33 {name}")
        same_bits(got, run(kind, 0, xin.float().contiguous(), labels, ll, tl), INVARIANT)  # the conversions are exact


@pytest.mark.parametrize("kind", VO.KINDS)
def test_vector_and_element_wise_rows_agree(kind):
    """V = 32 from an aligned base (16-byte row accesses) and from a base 4 bytes off (element-wise): the same bits."""
    x, labels, ll, tl = case1()
    xt = WA.dev(x)
    offset = torch.zeros(x.size + 1, device=DEV)[1:].view(x.shape).copy_(xt)
    assert xt.data_ptr() % 16 == 0 and offset.data_ptr() % 16 == 4
    same_bits(run(kind, 0, xt, labels, ll, tl), run(kind, 0, offset, labels, ll, tl))


# ---- 9: a non-zero blank ----

@pytest.mark.parametrize("blank", [31, 13])
@pytest.mark.parametrize("kind", VO.KINDS)
def test_a_nonzero_blank(kind, blank):
    x, labels, ll, tl = wild_input(1, 1300, 32, 1030, (1030,), (1300,), seed=29 + blank, wild=((0, 1023, 1024, 1029),), blank=blank)
    got = run(kind, 0, x, labels, ll, tl, blank, tf=64)
    WA.check(kind, 0, x, labels, ll, tl, got, blank, what=f"long {kind} blank={blank}")


# ---- 10: degenerate and infeasible utterances, optional outputs, empty shapes ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_degenerate_and_infeasible_utterances(kind):
    V, U, T = 32, 1040, 1200
    x, labels, ll, tl = GL.random_input(7, T, V, U, (0, 5, 1040, 1041, 1040, 1040, 1040), (900, 0, T, T, T, T, 1039), seed=30)
    labels[2, 1030] = 0     # a label equal to the blank, in the second label block
    labels[4, 1025] = -3    # not a label and not the wildcard
    labels[5, [0, 1023, 1024, 1039]] = W  # feasible, beside the others
    labels[6, [0, 1039]] = W              # fewer frames than positions
    got = run(kind, 0, x, labels, ll, tl, tf=64)
    WA.check(kind, 0, x, labels, ll, tl, got, what=f"long {kind} degenerate")
    assert np.array_equal(np.isfinite(got[0]), [True, False, False, False, False, True, False])
    assert np.all(got[1][0, :900] == 0) and np.all(got[2][0] == -1)  # label_length = 0: the all-blank path
    alone = run(kind, 0, x[5:6], labels[5:6], ll[5:6], tl[5:6], tf=64)
    same_bits(tuple(a[5:6] for a in got), alone, INVARIANT)


def abi_call(inp, tf, pattern=0xA5, wrt=0, present=(True, True, True, True), guard=64):
    """ctc_amd_long_wildcard_best_path on guarded, prefilled outputs; present: label_index, first_frame, last_frame, label_score."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U = inp.shape
    ws = OWN.workspace(_lib.long_wildcard_best_path_workspace_bytes(inp.kind, B, T, V, U, tf) + 512, pattern)
    shapes = {"score": ((B,), torch.float32), "tokens": ((B, T), torch.int32), "label_index": ((B, T), torch.int32),
              "first_frame": ((B, U), torch.int32), "last_frame": ((B, U), torch.int32), "label_score": ((B, U), torch.float32)}
    bufs = {}
    for name, want in zip(NAMES, (True, True) + tuple(present)):
        if want:
            shape, dtype = shapes[name]
            n = int(np.prod(shape))
            buf = OWN.filled((n + 2 * guard,), dtype, pattern, DEV)
            bufs[name] = (buf, buf[guard:guard + n].view(shape))
    ptrs = [bufs[name][1].data_ptr() if name in bufs else None for name in NAMES]
    rc = lib.ctc_amd_long_wildcard_best_path(*inp.common_ex(wrt), tf, *ptrs, ws.data_ptr() + 256, ws.numel() - 512,
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():  # nothing around the outputs is written
        keep = OWN.keeps_prefill(buf, pattern)
        assert bool(keep[:guard].all()) and bool(keep[-guard:].all()), name
    keep = OWN.keeps_prefill(ws, pattern)  # ... nor around the workspace
    assert bool(keep[:256].all()) and bool(keep[-256:].all())
    return {name: view for name, (buf, view) in bufs.items()}


@pytest.mark.parametrize("kind", VO.KINDS)
def test_optional_outputs_in_every_combination(kind):
    x, labels, ll, tl = wild_input(2, 1100, 32, 1030, (1030, 300), (1100, 500), seed=31, wild=((0, 1023, 1024), (299,)))
    inp = OWN.make_inputs(VO.KINDS.index(kind), x, labels, ll, tl)
    full = abi_call(inp, 64)
    for present in itertools.product((True, False), repeat=4):
        got = abi_call(inp, 64, present=present)
        assert set(got) == {n for n, p in zip(NAMES, (True, True) + present) if p}
        for name, t in got.items():
            assert OWN.same_bits(t, full[name]), (present, name)


def test_empty_shapes():
    import tf_seq2seq_losses_amd as ctc
    i32 = dict(dtype=torch.int32, device=DEV)
    z = ctc.classic_ctc_long_wildcard_alignment(torch.zeros((0, 2), **i32), torch.zeros((0, 4, 3), device=DEV), torch.zeros(0, **i32),
                                                torch.zeros(0, **i32))
    assert z.score.shape == (0,) and z.tokens.shape == (0, 4) and z.label_index.shape == (0, 4)
    assert z.first_frame.shape == z.last_frame.shape == z.label_score.shape == (0, 2)
    z = ctc.simplified_ctc_long_wildcard_alignment(torch.tensor([[W, 2], [1, 2]], **i32), torch.zeros((2, 0, 3), device=DEV),
                                                   torch.tensor([2, 0], **i32), torch.zeros(2, **i32))
    torch.cuda.synchronize()
    assert z.tokens.shape == (2, 0) and z.score.cpu().tolist() == [-np.inf, 0.0]
    assert np.all(z.first_frame.cpu().numpy() == -1) and np.all(z.last_frame.cpu().numpy() == -1)
    assert np.all(z.label_score.cpu().numpy() == -np.inf)


# ---- 11: ownership ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_ownership(kind):
    x, labels, ll, tl = wild_input(2, 1200, 32, 1030, (1030, 300), (1200, 500), seed=32, wild=((0, 1023, 1024, 1029), (0, 150)))
    clean = OWN.make_inputs(VO.KINDS.index(kind), x, labels, ll, tl)
    a = abi_call(clean, 64, 0xA5)
    # every output element is written, the tails with -1 / -inf (0xA5 and 0x00 are neither, nor a plausible result everywhere)
    assert bool((a["tokens"][1, 500:] == -1).all()) and bool((a["label_index"][1, 500:] == -1).all())
    assert bool((a["first_frame"][1, 300:] == -1).all()) and bool((a["last_frame"][1, 300:] == -1).all())
    assert bool((a["label_score"][1, 300:] == -np.inf).all())
    for name, t in a.items():
        assert not bool(OWN.keeps_prefill(t, 0xA5).any()), name
    # what the utterances do not own may hold anything: padding frames, label tails, the outputs and the workspace on entry
    xt = torch.from_numpy(x).to(DEV)
    for pattern, value in ((0x00, float("nan")), (0xFF, 3.0e38)):
        dirty = clean.replace(x=OWN.poison_padding(xt, tl, value),
                              labels=OWN.poison_labels(clean.labels, ll, OWN.label_poison_cycle(32, 0)))
        b = abi_call(dirty, 64, pattern)
        diff = OWN.total_diff(a, b)
        assert not any(diff.values()), (pattern, diff)


# ---- 12: HIP graph ----

@pytest.mark.parametrize("kind", VO.KINDS)
def test_in_a_hip_graph(kind):
    """Launches on one stream, their number fixed by the shapes: captured once and replayed on new data it reproduces the eager call."""
    from tf_seq2seq_losses_amd import _lib, ops
    lib = _lib.load()
    B, T, V, U, tf = 2, 1200, 32, 1030, 128
    k = ops.KINDS[kind]
    x = torch.zeros((B, T, V), device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    labels, ll, tl = torch.zeros((B, U), **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
    outs = [torch.zeros(B, device=DEV), torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.zeros((B, U), **i32),
            torch.zeros((B, U), **i32), torch.zeros((B, U), device=DEV)]
    ws = torch.zeros(_lib.long_wildcard_best_path_workspace_bytes(k, B, T, V, U, tf), dtype=torch.uint8, device=DEV)

    def call():
        rc = lib.ctc_amd_long_wildcard_best_path(k, _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), U,
                                                 ll.data_ptr(), tl.data_ptr(), 0, B, T, V, U, tf, *(o.data_ptr() for o in outs),
                                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    def fill(seed, lengths, frames, wild):
        h = wild_input(B, T, V, U, lengths, frames, seed, wild)
        for dst, src in zip((x, labels, ll, tl), h):
            dst.copy_(torch.from_numpy(src))
        return h

    fill(1, (1030, 600), (1200, 900), ((0, 1023), (5,)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    h = fill(2, (700, 1030), (1000, 1200), ((699,), (1024, 1029)))
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
    WA.check(kind, 0, *h, got, what=f"long {kind} graph replay")


# ---- 13: refusals ----

def test_cpu_tensors_are_refused():
    import tf_seq2seq_losses_amd as ctc
    for fn in (ctc.classic_ctc_long_wildcard_alignment, ctc.simplified_ctc_long_wildcard_alignment,
               ctc.ctc_long_wildcard_alignment_from_logproba):
        with pytest.raises(RuntimeError):
            fn(torch.tensor([[W, 2]], dtype=torch.int32), torch.zeros((1, 4, 3)), torch.tensor([2]), torch.tensor([4]))


def test_check_labels_keeps_rejecting_the_wildcard():
    import tf_seq2seq_losses_amd as ctc
    with pytest.raises(ValueError):
        ctc.check_labels(torch.tensor([[1, W]], dtype=torch.int32, device=DEV), torch.tensor([2], device=DEV), 5, 0)


def test_bad_frames_per_tile_is_refused():
    import tf_seq2seq_losses_amd as ctc
    i32 = dict(dtype=torch.int32, device=DEV)
    with pytest.raises(Exception):
        ctc.classic_ctc_long_wildcard_alignment(torch.tensor([[W, 2]], **i32), torch.zeros((1, 4, 3), device=DEV),
                                                torch.tensor([2], **i32), torch.tensor([4], **i32), frames_per_tile=6)
