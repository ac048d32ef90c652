"""ctc_amd_edit_distance against the dynamic programme of tests/tools/edit_oracle.py.  The distances are
integers: every comparison is torch.equal / array_equal, there is no tolerance.  The shapes are the smallest at which the kernel can
go wrong: every lane and positions-per-lane (NL) edge of the reference, a pipeline shorter than the wavefront, a result inside a
lane's block, the chunk reload of the hypothesis tokens at 64 and 128."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.tools import edit_oracle as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REF_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1024)
LONG_HYP_AT = (64, 128, 255, 257, 1024)  # one r per NL = 1, 2, 4, 8, 16: h = 1500
POISON = (-1, 2 ** 31 - 1)


def dev(a, dtype=np.int32):
    return torch.tensor(np.asarray(a, dtype), device=DEV)


def run(hyp, hl, ref, rl, R=None):
    from tf_seq2seq_losses_amd import ops
    out = ops.edit_distance(dev(hyp), dev(hl), dev(ref), dev(rl), R)
    torch.cuda.synchronize()
    assert out.dtype == torch.int32 and tuple(out.shape) == tuple(np.asarray(hl).shape)
    return out.cpu().numpy()


def oracle(hyp, hl, ref, rl, R=None):
    return E.edit_distances(hyp, hl, ref, rl, R, one=E.edit_distance_rows)


def pack(strings, width=None, poison=POISON[0]):
    """Rows of different lengths as one padded int32 array (padding: poison) and their lengths."""
    width = max([len(s) for s in strings] + [0]) if width is None else width
    out = np.full((len(strings), width), poison, np.int32)
    for i, s in enumerate(strings):
        out[i, :len(s)] = s
    return out, np.asarray([len(s) for s in strings], np.int32)


def hyp_lengths(r):
    return sorted({0, 1, max(r - 1, 0), r, r + 1, 2 * r + 3} | ({1500} if r in LONG_HYP_AT else set()))


@functools.lru_cache(maxsize=None)
def grid_case(r, alphabet):
    """One utterance per hypothesis length, N = 1, the reference exactly as wide as it is long (R = r selects NL); read-only."""
    rng = np.random.default_rng(1000 * alphabet + r)
    hs = hyp_lengths(r)
    hyp, hl = pack([rng.integers(0, alphabet, h) for h in hs])
    ref = rng.integers(0, alphabet, (len(hs), r)).astype(np.int32)
    rl = np.full(len(hs), r, np.int32)
    want = oracle(hyp[:, None], hl[:, None], ref, rl)
    for a in (hyp, hl, ref, rl, want):
        a.setflags(write=False)
    return hyp[:, None], hl[:, None], ref, rl, want


# ---- 1. reference lengths across every lane and NL edge ----
@pytest.mark.parametrize("alphabet", [2, 1000])
@pytest.mark.parametrize("r", REF_LENGTHS)
def test_length_grid(r, alphabet):
    hyp, hl, ref, rl, want = grid_case(r, alphabet)
    got = run(hyp, hl, ref, rl)
    print(f"EDIT-MEASURE r={r} alphabet={alphabet}: h={hl[:, 0].tolist()} distance={got[:, 0].tolist()}", flush=True)
    assert np.array_equal(got, want), (r, alphabet, got[:, 0].tolist(), want[:, 0].tolist())
    assert np.all((got[:, 0] >= np.abs(hl[:, 0] - r)) & (got[:, 0] <= np.maximum(hl[:, 0], r)))


# ---- 2. constructed cases ----
@pytest.mark.parametrize("r", [64, 66, 130, 300, 600])
def test_constructed(r):
    rng = np.random.default_rng(r)
    ref1 = rng.integers(0, 5, r).tolist()
    positions = sorted({p for p in (0, 62, 63, 64, 65, r - 1) if p < r})
    strings, exact = [list(ref1), [7 + t for t in ref1][: r // 2], [7 + t for t in ref1] + [9] * 40], [0, r, r + 40]
    for p in positions:
        strings += [ref1[:p] + ref1[p + 1:], ref1[:p] + [77] + ref1[p:], ref1[:p] + [77] + ref1[p + 1:]]
        exact += [1, 1, 1]
    hyp, hl = pack(strings)
    ref = np.tile(np.asarray(ref1, np.int32), (1, 1))
    rl = np.asarray([r], np.int32)
    got = run(hyp[None], hl[None], ref, rl)
    assert got[0].tolist() == exact, (r, got[0].tolist())
    assert np.array_equal(got, oracle(hyp[None], hl[None], ref, rl))


# ---- 3. list sizes: one writer per element, a result that does not depend on its place ----
@functools.lru_cache(maxsize=None)
def pool():
    rng = np.random.default_rng(77)
    B, P = 3, 64
    strings = [rng.integers(0, 3, int(h)) for h in rng.integers(0, 90, B * P)]
    hyp, hl = pack(strings, width=96)
    ref, rl = pack([rng.integers(0, 3, r) for r in (70, 0, 33)], width=80, poison=POISON[1])
    hyp, hl = hyp.reshape(B, P, -1), hl.reshape(B, P)
    want = oracle(hyp, hl, ref, rl)
    for a in (hyp, hl, ref, rl, want):
        a.setflags(write=False)
    return hyp, hl, ref, rl, want


@pytest.mark.parametrize("N", [1, 7, 8, 9, 64])
def test_list_sizes(N):
    hyp, hl, ref, rl, want = pool()
    for seed in (0, 1):
        pick = np.random.default_rng(10 * N + seed).permutation(64)[:N]
        got = run(hyp[:, pick], hl[:, pick], ref, rl)
        assert np.array_equal(got, want[:, pick]), (N, seed)


# ---- 4. contract edges ----
def test_strides_poison_and_lengths():
    """Strides wider than the lengths with poison beyond them, negative lengths, lengths beyond the stride (clamped)."""
    rng = np.random.default_rng(5)
    for poison in POISON:
        hyp = rng.integers(0, 2, (2, 3, 70)).astype(np.int32)
        ref = rng.integers(0, 2, (2, 90)).astype(np.int32)
        hl = np.asarray([[66, -5, 500], [0, 70, 1]], np.int32)
        rl = np.asarray([65, 2000], np.int32)
        want = oracle(hyp, hl, ref, rl)
        assert want[0, 1] == 65 and want[1, 0] == 90 and want[0, 2] == oracle(hyp, np.full((2, 3), 70), ref, rl)[0, 2]
        poisoned, pref = hyp.copy(), ref.copy()
        poisoned[0, 0, 66:] = poison
        poisoned[0, 1, :] = poison
        poisoned[1, 0, :] = poison
        poisoned[1, 2, 1:] = poison
        pref[0, 65:] = poison
        assert np.array_equal(run(poisoned, hl, pref, rl), want), poison


def test_reference_beyond_R_is_minus_one_for_that_utterance_only():
    rng = np.random.default_rng(6)
    hyp = rng.integers(0, 3, (3, 4, 20)).astype(np.int32)
    hl = rng.integers(0, 21, (3, 4)).astype(np.int32)
    ref = rng.integers(0, 3, (3, 40)).astype(np.int32)
    rl = np.asarray([10, 11, 9], np.int32)
    want = oracle(hyp, hl, ref, rl, R=10)
    assert np.all(want[1] == -1) and np.all(want[[0, 2]] >= 0)
    assert np.array_equal(run(hyp, hl, ref, rl, R=10), want)
    assert np.array_equal(run(hyp, hl, ref, rl, R=11), oracle(hyp, hl, ref, rl))
    assert np.array_equal(run(hyp, hl, ref, rl, R=0), np.full((3, 4), -1))
    with pytest.raises(ValueError, match="R=1025"):
        run(hyp, hl, ref, rl, R=1025)


def test_guard_elements_stay_untouched_and_the_call_is_deterministic():
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    hyp, hl, ref, rl, want = pool()
    B, N = hl.shape
    G = 64
    th, thl, tr, trl = dev(hyp), dev(hl), dev(ref), dev(rl)
    outs = []
    for fill in (-7, 123456):
        buf = torch.full((G + B * N + G,), fill, dtype=torch.int32, device=DEV)
        rc = lib.ctc_amd_edit_distance(th.data_ptr(), hyp.shape[2], thl.data_ptr(), tr.data_ptr(), ref.shape[1], trl.data_ptr(), B, N,
                                       ref.shape[1], buf.data_ptr() + 4 * G, None, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.ctc_amd_last_error()
        got = buf.cpu().numpy()
        assert np.all(got[:G] == fill) and np.all(got[G + B * N:] == fill)
        outs.append(got[G:G + B * N].reshape(B, N))
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)


def test_empty_shapes():
    from tf_seq2seq_losses_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)  # noqa: E731
    assert tuple(ops.edit_distance(z(0, 3, 5), z(0, 3), z(0, 4), z(0)).shape) == (0, 3)
    got = ops.edit_distance(z(2, 3, 0), z(2, 3), z(2, 4), torch.tensor([3, 0], dtype=torch.int32, device=DEV))
    assert got.cpu().tolist() == [[3, 3, 3], [0, 0, 0]]         # no hypothesis tokens at all: the reference's length
    got = ops.edit_distance(z(2, 1, 5), torch.tensor([[5], [2]], dtype=torch.int32, device=DEV), z(2, 0), z(2))
    assert got.cpu().tolist() == [[5], [2]]                     # no reference tokens at all: the hypothesis' length
    with pytest.raises(ValueError):
        ops.edit_distance(z(2, 0, 5), z(2, 0), z(2, 4), z(2))   # N >= 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edit_distance(torch.zeros((1, 1, 2), dtype=torch.int32), z(1, 1), z(1, 2), z(1))


# ---- 5. the public layer ----
def test_public_two_dimensional_form_mask_and_error_rate():
    import tf_seq2seq_losses_amd as ctc
    hyp, hl, ref, rl, want = pool()
    mask = np.random.default_rng(3).random(hl.shape) < 0.7
    out = ctc.ctc_edit_distance(dev(hyp), dev(hl), dev(ref), dev(rl), hypothesis_mask=dev(mask, bool))
    assert isinstance(out, ctc.CtcEditDistance)
    assert out.distance.dtype == torch.int32 and out.error_rate.dtype == torch.float32
    assert torch.equal(out.distance.cpu(), torch.from_numpy(np.where(mask, want, -1).astype(np.int32)))
    rate = (want.astype(np.float32) / np.maximum(rl, 1).astype(np.float32)[:, None])
    got_rate = out.error_rate.cpu().numpy()
    assert np.array_equal(np.isnan(got_rate), ~mask)
    assert np.array_equal(got_rate[mask], rate[mask])
    assert rl[1] == 0 and np.array_equal(got_rate[1][mask[1]], want[1][mask[1]].astype(np.float32)), "an empty reference divides by 1"
    # NumPy inputs, no mask; the 2-D form is the N = 1 list and comes back as [B]
    plain = ctc.ctc_edit_distance(hyp.copy(), hl.copy(), ref.copy(), rl.copy())
    assert torch.equal(plain.distance.cpu(), torch.from_numpy(want.copy())) and not torch.isnan(plain.error_rate).any()
    two = ctc.ctc_edit_distance(dev(hyp[:, 5]), dev(hl[:, 5]), dev(ref), dev(rl), hypothesis_mask=dev([True, False, True], bool))
    assert tuple(two.distance.shape) == (3,) == tuple(two.error_rate.shape)
    assert two.distance.cpu().tolist() == [int(want[0, 5]), -1, int(want[2, 5])]
    assert np.array_equal(two.error_rate.cpu().numpy()[[0, 2]], rate[[0, 2], 5]) and np.isnan(two.error_rate.cpu().numpy()[1])


@pytest.mark.parametrize("kind", ["classic", "simplified"])
def test_decodings_go_in_as_they_stand(kind):
    import tf_seq2seq_losses_amd as ctc
    rng = np.random.default_rng(8)
    B, T, V = 4, 20, 8
    x = torch.tensor((2.0 * rng.standard_normal((B, T, V))).astype(np.float32), device=DEV)
    tl = dev([20, 13, 0, 7])
    ref, rl = pack([rng.integers(1, V, n) for n in (9, 5, 3, 0)], width=10)
    beam = (ctc.classic_ctc_beam_search if kind == "classic" else ctc.simplified_ctc_beam_search)(x, tl, 0, beam_width=8, top_k=4, nbest=6)
    mask = torch.isfinite(beam.score)
    out = ctc.ctc_edit_distance(beam.labels, beam.label_length, dev(ref), dev(rl), hypothesis_mask=mask)
    want = E.edit_distances(beam.labels.cpu().numpy(), beam.label_length.cpu().numpy(), ref, rl)
    m = mask.cpu().numpy()
    assert m.any() and not m.all(), "present and missing hypotheses"
    assert torch.equal(out.distance.cpu(), torch.from_numpy(np.where(m, want, -1).astype(np.int32)))
    greedy = (ctc.classic_ctc_greedy_decode if kind == "classic" else ctc.simplified_ctc_greedy_decode)(x, tl, 0)
    ter = ctc.ctc_edit_distance(greedy.labels, greedy.label_length, dev(ref), dev(rl))
    want1 = E.edit_distances(greedy.labels.cpu().numpy()[:, None], greedy.label_length.cpu().numpy()[:, None], ref, rl)[:, 0]
    assert torch.equal(ter.distance.cpu(), torch.from_numpy(want1))
    assert np.array_equal(ter.error_rate.cpu().numpy(), want1.astype(np.float32) / np.maximum(rl, 1).astype(np.float32))
    assert want1[2] == 3 and want1.max() > 3, "no frames: every reference token is a deletion"
