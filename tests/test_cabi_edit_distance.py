"""Host layer of ctc_amd_edit_distance / ctc_amd_edit_distance_workspace_bytes, in the manner of tests/test_cabi_nbest_loss.py:
nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16.  The call
needs no workspace, so a call that passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes
import os
import re

import pytest

OK, EINVAL = 0, -1
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(hyp=ONE, hyp_stride=5, hyp_length=ONE, ref=ONE, ref_stride=4, ref_length=ONE, B=2, N=3, R=4, distance=ONE, ws=None, ws_bytes=0)
ORDER = ("hyp", "hyp_stride", "hyp_length", "ref", "ref_stride", "ref_length", "B", "N", "R", "distance", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    rc = lib.ctc_amd_edit_distance(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, B, N, R):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_edit_distance_workspace_bytes(B, N, R, ctypes.byref(out))
    return rc, int(out.value)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_edit_distance", "ctc_amd_edit_distance_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint " + name + r"\(", header), name
    assert len(_lib.SIGNATURES["ctc_amd_edit_distance"][1]) == len(ORDER) + 1  # + the stream
    assert "ctc_edit.hip" in [u[0] for u in __import__("__graft_entry__").HIP_UNITS]


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """No workspace: 0 bytes for every valid shape; the limits are those of the call."""
    for s in [(0, 1, 0), (3, 1, 0), (2, 3, 4), (256, 8, 128), (256, 32, 1024), (1, 100000, 64), (2 ** 20, 2047, 7)]:
        assert size(lib, *s) == (OK, 0), s
    for bad in ((-1, 3, 4), (2, 0, 4), (2, -1, 4), (2, 3, -1), (2, 3, 1025), (2 ** 30, 2, 4), (2 ** 16, 2 ** 15, 4)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert size(lib, 2 ** 16, 2 ** 15 - 1, 4) == (OK, 0)
    assert lib.ctc_amd_edit_distance_workspace_bytes(2, 3, 4, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.edit_distance_workspace_bytes(2, 3, 4) == 0
    with pytest.raises(ValueError):
        _lib.edit_distance_workspace_bytes(2, 3, 1025)


@pytest.mark.parametrize("over,text", [
    (dict(B=-1), "negative size"), (dict(R=-1), "negative size"),
    (dict(R=1025), "R=1025"),
    (dict(N=0), "N 0"), (dict(N=-1), "N -1"),
    (dict(B=2 ** 30, N=2), "B * N"), (dict(B=2 ** 16, N=2 ** 15), "B * N"),
    (dict(hyp_stride=-1), "negative stride"), (dict(ref_stride=-1), "negative stride"),
    (dict(hyp_stride=2 ** 31 - 1), "hyp_stride=2147483647"),
    (dict(hyp_length=None), "null length"), (dict(ref_length=None), "null length"),
    (dict(hyp=None), "null hyp"), (dict(ref=None), "null ref"),
    (dict(distance=None), "null distance"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence(lib):
    expect(lib, EINVAL, "negative size", B=-1, R=2000)         # the sizes, then R
    expect(lib, EINVAL, "R=2000", R=2000, N=0)                  # R, then N
    expect(lib, EINVAL, "N 0", N=0, hyp_stride=-1)              # the shape before the strides
    expect(lib, EINVAL, "negative stride", hyp_stride=-1, hyp_length=None)
    expect(lib, EINVAL, "null length", hyp_length=None, hyp=None, distance=None)
    expect(lib, EINVAL, "null hyp", hyp=None, ref=None)
    expect(lib, EINVAL, "null ref", ref=None, distance=None)
    expect(lib, EINVAL, "R=2000", R=2000, B=0)                  # a bad R hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, hyp=None, hyp_length=None, ref=None, ref_length=None, distance=None)
    expect(lib, OK, B=0, N=0)               # no hypotheses to count
    expect(lib, OK, B=0, hyp_stride=-1)     # nor rows to stride over
