"""The definition ctc_amd_edit_counts is held to (tests/tools/edit_counts_oracle.py), pinned on the CPU: the
tuple recurrence, the packed NumPy row form and a recursion over all alignments agree; the distance is the Levenshtein distance;
deletions and hits follow from the identities and are never negative."""
import numpy as np
import pytest

from tests.tools import edit_counts_oracle as C
from tests.tools import edit_oracle as E


def random_pairs(count=300, seed=7):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        alphabet = int(rng.integers(2, 4))
        yield rng.integers(0, alphabet, int(rng.integers(0, 13))), rng.integers(0, alphabet, int(rng.integers(0, 13)))


def test_three_forms_agree_and_the_identities_hold():
    for a, b in random_pairs():
        want = C.edit_counts(a, b)
        assert C.edit_counts_rows(a, b) == want, (a, b)
        assert C.edit_counts_paths(a, b) == want, (a, b)
        d, s, i = want
        assert d == E.edit_distance(a, b), (a, b)
        deletions, hits = d - s - i, len(a) - s - i
        assert deletions >= 0 and hits >= 0 and hits == len(b) - s - deletions, (a, b, want)


def test_the_example():
    assert C.edit_counts([0, 1], [1, 0]) == (2, 0, 1)  # one insertion, one deletion, one hit: not two substitutions
    out = C.edit_counts_batch(np.array([[[0, 1]]]), np.array([[2]]), np.array([[1, 0]]), np.array([2]))
    assert out.tolist() == [[[2, 0, 1, 1]]]


@pytest.mark.parametrize("hyp,ref,want", [
    ([5, 1, 2, 3], [1, 2, 3], (1, 0, 1)),      # a pure insertion
    ([1, 3], [1, 2, 3], (1, 0, 0)),            # a pure deletion
    ([1, 9, 3], [1, 2, 3], (1, 1, 0)),         # a pure substitution
    ([], [1, 2, 3], (3, 0, 0)), ([1, 2], [], (2, 0, 2)), ([], [], (0, 0, 0)),
])
def test_single_kinds(hyp, ref, want):
    for one in (C.edit_counts, C.edit_counts_rows, C.edit_counts_paths):
        assert one(hyp, ref) == want


def test_batch_wrapper_reads_lengths_as_the_c_abi_does():
    hyp = np.array([[[1, 2, 3, 4], [1, 2, 9, 9]], [[7, 7, 7, 7], [1, 1, 1, 1]]])
    hl = np.array([[9, 2], [-3, 1]])          # clamped to [0, 4]
    ref = np.array([[1, 2, 3], [7, 8, 9]])
    rl = np.array([3, 3])
    out = C.edit_counts_batch(hyp, hl, ref, rl)
    assert out.tolist() == [[[1, 0, 1, 0], [1, 0, 0, 1]], [[3, 0, 0, 3], [3, 1, 0, 2]]]
    out = C.edit_counts_batch(hyp, hl, ref, np.array([3, 2]), R=2, one=C.edit_counts_rows)
    assert out[0].tolist() == [[-1] * 4] * 2 and out[1].tolist() == [[2, 0, 0, 2], [2, 1, 0, 1]]
