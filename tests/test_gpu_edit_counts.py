"""ctc_amd_edit_counts against tests/tools/edit_counts_oracle.py.  Everything is an integer: every comparison
is array_equal / torch.equal, there is no tolerance.  The table is tiled over column blocks of 1024 reference tokens and row blocks
of rows_per_tile hypothesis tokens, so the shapes sit on both sides of every block edge, of the 64-token chunk reloads and of the
lane edges inside a block; tokens beyond the lengths are poison, the workspace is filled with 0xFF and the output has guard elements
around it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.tools import edit_counts_oracle as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISON = (-1, 2 ** 31 - 1)
GUARD = 12345
REF_LENGTHS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000)


def dev(a, dtype=np.int32):
    return torch.tensor(np.asarray(a, dtype), device=DEV)


def run(hyp, hl, ref, rl, R=None, rows_per_tile=0):
    """The C entry point on a workspace of exactly the queried size filled with 0xFF, counts between guard elements."""
    from tf_seq2seq_losses_amd import _lib
    hyp, hl, ref, rl = dev(hyp), dev(hl), dev(ref), dev(rl)
    B, N, W = hyp.shape
    Wr = ref.shape[1]
    R = Wr if R is None else R
    n = _lib.edit_counts_workspace_bytes(B, N, R, W, rows_per_tile)
    ws = torch.full((max(n, 1),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((B * N * 4 + 8,), GUARD, dtype=torch.int32, device=DEV)
    rc = _lib.load().ctc_amd_edit_counts(hyp.data_ptr(), W, hl.data_ptr(), ref.data_ptr(), Wr, rl.data_ptr(), B, N, R, rows_per_tile,
                                         out.data_ptr() + 16, ws.data_ptr(), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "ctc_amd_edit_counts")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:4] == GUARD).all() and (out[-4:] == GUARD).all(), "a store outside counts"
    return out[4:-4].reshape(B, N, 4)


def oracle(hyp, hl, ref, rl, R=None):
    return C.edit_counts_batch(hyp, hl, ref, rl, R, one=C.edit_counts_rows)


def pack(strings, width=None, poison=POISON[0]):
    """Rows of different lengths as one padded int32 array (padding: poison) and their lengths."""
    width = max([len(s) for s in strings] + [0]) if width is None else width
    out = np.full((len(strings), width), poison, np.int32)
    for i, s in enumerate(strings):
        out[i, :len(s)] = s
    return out, np.asarray([len(s) for s in strings], np.int32)


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def grid_case(r, alphabet):
    """One utterance per hypothesis length, N = 1; the reference tensor one element wider than r, that element poison; read-only."""
    rng = np.random.default_rng(1000 * alphabet + r)
    hs = sorted({0, 1, max(r - 1, 0), r, r + 1})
    hyp, hl = pack([rng.integers(0, alphabet, h) for h in hs], poison=POISON[r % 2])
    ref = np.full((len(hs), r + 1), POISON[(r + 1) % 2], np.int32)
    ref[:, :r] = rng.integers(0, alphabet, (len(hs), r))
    rl = np.full(len(hs), r, np.int32)
    want = oracle(hyp[:, None], hl[:, None], ref, rl)
    return freeze(hyp, hl, ref, rl, want)


@pytest.mark.parametrize("rows_per_tile", [64, 0])
@pytest.mark.parametrize("alphabet", [2, 1000])
@pytest.mark.parametrize("r", REF_LENGTHS)
def test_grid(r, alphabet, rows_per_tile):
    hyp, hl, ref, rl, want = grid_case(r, alphabet)
    got = run(hyp[:, None], hl[:, None], ref, rl, R=r, rows_per_tile=rows_per_tile)
    assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def row_edge_case():
    rng = np.random.default_rng(11)
    hs = (63, 64, 65, 127, 128, 129, 2 * 64 + 3)
    hyp, hl = pack([rng.integers(0, 3, h) for h in hs])
    ref = np.tile(rng.integers(0, 3, 1500).astype(np.int32), (len(hs), 1))
    rl = np.full(len(hs), 1500, np.int32)
    return freeze(hyp, hl, ref, rl, oracle(hyp[:, None], hl[:, None], ref, rl))


def test_row_tile_edges():
    """Tile origins at 64 and 128 meet the reloads of the two token chunks; r = 1500 makes every row tile hand a column to the right."""
    hyp, hl, ref, rl, want = row_edge_case()
    got = run(hyp[:, None], hl[:, None], ref, rl, rows_per_tile=64)
    assert np.array_equal(got, want)
    assert np.array_equal(run(hyp[:, None], hl[:, None], ref, rl, rows_per_tile=128), want)


EDIT_AT = (0, 1022, 1023, 1024, 1025, 2047, 2048, 2099)


def test_single_edits():
    """One substitution, insertion or deletion in 2100 distinct tokens, at the block edges: exactly that one count."""
    ref = np.arange(100, 2200, dtype=np.int32)
    hyps, want = [], []
    for at in EDIT_AT:
        s = ref.copy()
        s[at] = 7
        hyps.append(s)
        want.append((1, 1, 0, 0))
        hyps.append(np.insert(ref, at, 7))
        want.append((1, 0, 1, 0))
        hyps.append(np.delete(ref, at))
        want.append((1, 0, 0, 1))
    hyps.append(ref.copy())
    want.append((0, 0, 0, 0))
    hyp, hl = pack(hyps, poison=POISON[1])
    for rows_per_tile in (0, 64):
        got = run(hyp[None], hl[None], ref[None], [len(ref)], rows_per_tile=rows_per_tile)
        assert np.array_equal(got[0], np.asarray(want, np.int32)), rows_per_tile


def test_scattered_deletions_and_insertions():
    ref = np.arange(100, 2200, dtype=np.int32)
    rng = np.random.default_rng(5)
    spots = np.sort(rng.choice(len(ref), 20, replace=False))
    dele, ins = spots[::2], spots[1::2]
    pieces = []
    for j, t in enumerate(ref):
        if j in ins:
            pieces.append(10 ** 6 + j)  # a fresh token in front of ref[j]
        if j not in dele:
            pieces.append(int(t))
    hyp, hl = pack([pieces])
    got = run(hyp[None], hl[None], ref[None], [len(ref)])
    assert got.tolist() == [[[20, 0, 10, 10]]]


@functools.lru_cache(maxsize=None)
def limit_case(h, r):
    rng = np.random.default_rng(h + r)
    hyp = rng.integers(0, 8, h).astype(np.int32)  # half its tokens are not in the reference at all
    ref = rng.integers(0, 4, r).astype(np.int32)
    d, s, i = C.edit_counts_rows(hyp, ref)
    return freeze(hyp, ref) + ((d, s, i, d - s - i),)


@pytest.mark.parametrize("h,r", [(70, 65536), (70, 65535), (66000, 3)])
def test_limits(h, r):
    """K = 64 column blocks under a short hypothesis; many row blocks over one column block at the default tile height."""
    hyp, ref, want = limit_case(h, r)
    got = run(hyp[None, None], [[h]], ref[None], [r])
    assert got.tolist() == [[list(want)]]


def test_reference_longer_than_R_marks_its_utterance_only():
    rng = np.random.default_rng(3)
    hyp, hl = pack([rng.integers(0, 3, h) for h in (1100, 900, 1300, 5, 0, 1200)])
    hyp, hl = hyp.reshape(3, 2, -1), hl.reshape(3, 2)
    ref = rng.integers(0, 3, (3, 1301)).astype(np.int32)
    rl = np.asarray([1300, 1301, 1024], np.int32)
    want = oracle(hyp, hl, ref, rl, R=1300)
    assert (want[1] == -1).all() and (want[[0, 2]] >= 0).all()
    assert np.array_equal(run(hyp, hl, ref, rl, R=1300, rows_per_tile=256), want)


@pytest.mark.parametrize("N", [1, 7, 9])
def test_lists(N):
    """One hypothesis moved about the list and across B = 1 / 3: its four numbers do not change."""
    rng = np.random.default_rng(N)
    probe = rng.integers(0, 3, 1100).astype(np.int32)
    ref = rng.integers(0, 3, (3, 1200)).astype(np.int32)
    rl = np.asarray([1200, 1030, 1200], np.int32)
    ref[2] = ref[0]
    d, s, i = C.edit_counts_rows(probe, ref[0])
    want_probe = [d, s, i, d - s - i]
    for B, b, n in ((1, 0, 0), (1, 0, N - 1), (3, 2, N // 2), (3, 0, N - 1)):
        strings = [rng.integers(0, 3, int(rng.integers(0, 1300))) for _ in range(B * N)]
        strings[b * N + n] = probe
        hyp, hl = pack(strings, width=1300, poison=POISON[N % 2])
        hyp, hl = hyp.reshape(B, N, -1), hl.reshape(B, N)
        got = run(hyp, hl, ref[:B], rl[:B], rows_per_tile=192)
        assert got[b, n].tolist() == want_probe, (B, b, n)
        assert np.array_equal(got, oracle(hyp, hl, ref[:B], rl[:B]))


def test_distance_is_edit_distance_up_to_1024():
    from tf_seq2seq_losses_amd import ops
    rng = np.random.default_rng(9)
    for Wr in (64, 100, 200, 500, 1024):  # one per positions-per-lane instantiation
        hyp, hl = pack([rng.integers(0, 3, int(h)) for h in rng.integers(0, Wr + 40, 10)], poison=POISON[1])
        hyp, hl = dev(hyp.reshape(2, 5, -1)), dev(hl.reshape(2, 5))
        ref, rl = dev(rng.integers(0, 3, (2, Wr))), dev([Wr, Wr - 3])
        counts = ops.edit_counts(hyp, hl, ref, rl)
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (2, 5, 4)
        assert torch.equal(counts[..., 0], ops.edit_distance(hyp, hl, ref, rl))
        assert np.array_equal(counts.cpu().numpy(), oracle(hyp.cpu().numpy(), hl.cpu().numpy(), ref.cpu().numpy(), rl.cpu().numpy()))
        assert torch.equal(counts, ops.edit_counts(hyp, hl, ref, rl, rows_per_tile=64))


def test_public_function():
    import tf_seq2seq_losses_amd as ctc
    rng = np.random.default_rng(21)
    hyp, hl = pack([rng.integers(0, 3, h) for h in (1025, 0, 900, 1100, 3, 1200)])
    hyp, hl = hyp.reshape(2, 3, -1), hl.reshape(2, 3)
    ref = rng.integers(0, 3, (2, 1025)).astype(np.int32)
    rl = np.asarray([1025, 700], np.int32)
    want = oracle(hyp, hl, ref, rl)
    res = ctc.ctc_edit_counts(dev(hyp), dev(hl), dev(ref), dev(rl))
    assert isinstance(res, ctc.CtcEditCounts) and not any(t.requires_grad for t in res)
    for k, name in enumerate(("distance", "substitutions", "insertions", "deletions")):
        assert np.array_equal(getattr(res, name).cpu().numpy(), want[..., k]), name
    assert np.array_equal(res.hits.cpu().numpy(), hl - want[..., 1] - want[..., 2])
    assert np.array_equal(res.hits.cpu().numpy(), rl[:, None] - want[..., 1] - want[..., 3])
    assert np.array_equal(res.error_rate.cpu().numpy(), (want[..., 0].astype(np.float32) / rl[:, None].astype(np.float32)))
    with pytest.raises(ValueError):  # 1025 wide: beyond the short call's limit
        ctc.ctc_edit_distance(dev(hyp), dev(hl), dev(ref), dev(rl))
    # one hypothesis per utterance, and a mask
    one = ctc.ctc_edit_counts(dev(hyp[:, 1]), dev(hl[:, 1]), dev(ref), dev(rl), hypothesis_mask=dev([True, False], bool), rows_per_tile=64)
    for k, name in enumerate(("distance", "substitutions", "insertions", "deletions")):
        assert getattr(one, name).cpu().tolist() == [int(want[0, 1, k]), -1], name
    assert one.hits.cpu().tolist() == [int(hl[0, 1] - want[0, 1, 1] - want[0, 1, 2]), -1]
    rate = one.error_rate.cpu().numpy()
    assert rate.shape == (2,) and rate[0] == np.float32(want[0, 1, 0]) / np.float32(1025) and np.isnan(rate[1])
    # a reference longer than the tensor is wide cannot be passed; a clamped length is read as the kernel reads it
    res = ctc.ctc_edit_counts(dev(hyp), dev(hl), dev(ref), dev([5000, -2]))
    assert np.array_equal(res.distance.cpu().numpy(), oracle(hyp, hl, ref, [5000, -2])[..., 0])


def test_public_function_takes_a_greedy_decoding():
    import tf_seq2seq_losses_amd as ctc
    torch.manual_seed(0)
    logits = torch.randn(3, 40, 6, device=DEV)
    dec = ctc.classic_ctc_greedy_decode(logits, dev([40, 33, 0]), 0)
    ref = np.random.default_rng(2).integers(1, 6, (3, 30)).astype(np.int32)
    rl = np.asarray([30, 12, 4], np.int32)
    res = ctc.ctc_edit_counts(dec.labels, dec.label_length, dev(ref), dev(rl))
    want = oracle(dec.labels.cpu().numpy()[:, None], dec.label_length.cpu().numpy()[:, None], ref, rl)[:, 0]
    got = torch.stack([res.distance, res.substitutions, res.insertions, res.deletions], -1).cpu().numpy()
    assert got.shape == (3, 4) and np.array_equal(got, want)
    assert np.array_equal(res.hits.cpu().numpy(), dec.label_length.cpu().numpy() - want[:, 1] - want[:, 2])


def test_graph_capture():
    """K = 2 column blocks, J = 3 row blocks: four launches in one serial chain, replayed on changed inputs."""
    from tf_seq2seq_losses_amd import ops
    rng = np.random.default_rng(8)

    def make():
        hyp, hl = pack([rng.integers(0, 3, int(h)) for h in rng.integers(130, 193, 4)], width=192)
        return hyp.reshape(2, 2, -1), hl.reshape(2, 2), rng.integers(0, 3, (2, 1100)).astype(np.int32), rng.integers(1025, 1101, 2).astype(np.int32)
    cases = [make() for _ in range(3)]
    bufs = [dev(a) for a in cases[0]]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.edit_counts(*bufs, rows_per_tile=64)  # (the size query's cache and the library are warm before the capture)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.edit_counts(*bufs, rows_per_tile=64)
    for case in cases[1:]:
        for buf, a in zip(bufs, case):
            buf.copy_(dev(a))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), oracle(*case))
        assert torch.equal(out, ops.edit_counts(*bufs, rows_per_tile=64))
