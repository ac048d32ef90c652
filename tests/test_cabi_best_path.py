"""Host layer of ctc_amd_best_path / ctc_amd_best_path_workspace_bytes, in the manner of tests/test_cabi_validation.py: nothing
here touches a GPU.  Validation returns before any launch, pointers are the never-dereferenced address 16 and no call is
given a workspace, so a call that passes every check stops at CTC_AMD_EWORKSPACE."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=4, label_length=ONE, logit_length=ONE,
            blank=0, B=2, T=5, V=8, U=4, score=ONE, tokens=ONE, label_index=ONE, ws=None, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "score", "tokens", "label_index", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    rc = lib.ctc_amd_best_path(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_best_path_workspace_bytes(kind, B, T, V, U, ctypes.byref(out))
    return rc, int(out.value)


def test_abi_version_is_6(lib):
    assert lib.ctc_amd_abi_version() == 6


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None),
    (dict(U=-1), None), (dict(label_stride=-1), None), (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=1025, label_stride=1025), "U=1025"), (dict(label_length=None), None), (dict(logit_length=None), None),
    (dict(logits=None), None), (dict(labels=None), None),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(score=None), "null"), (dict(tokens=None), "null"), (dict(V=16385), "V=16385"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence_follows_the_other_entry_points(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=1025)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)       # common checks before the element type
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)          # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)        # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, score=None)     # strides before the outputs
    expect(lib, EINVAL, "null", score=None, V=16385)     # outputs before the vocabulary limit
    expect(lib, EINVAL, "kind", kind=5, B=0)             # a common fault hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, score=None, tokens=None, label_index=None)
    expect(lib, OK, B=0, xst=7)  # no rows to overlap


def test_a_valid_call_stops_at_the_workspace(lib):
    expect(lib, EWORKSPACE)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=1)
    expect(lib, EWORKSPACE, kind=1, wrt=1)
    expect(lib, EWORKSPACE, label_index=None)
    expect(lib, EWORKSPACE, T=0, tokens=None, label_index=None)  # no frames: nothing to write but the score
    expect(lib, EWORKSPACE, V=16384)
    expect(lib, EWORKSPACE, U=1024, label_stride=1024)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, xdtype=dt)
    expect(lib, EWORKSPACE, xsb=8, xst=16)  # time-major


@pytest.mark.parametrize("kind", [0, 1])
def test_size_function(lib, kind):
    B, V = 3, 256
    # monotone in T and in U, and enough for one back-pointer byte per lane and frame
    for U in (0, 1, 64, 65, 128, 129, 256, 257, 512, 513, 1024):
        prev = -1
        for T in (0, 1, 2, 63, 64, 65, 1000, 1001):
            rc, n = size(lib, kind, B, T, V, U)
            assert rc == OK and n >= prev and n >= B * T * 64, (U, T, n)
            prev = n
    for T in (1, 100, 1000):
        prev = -1
        for U in range(0, 1025):
            rc, n = size(lib, kind, B, T, V, U)
            assert rc == OK and n >= prev, (T, U, n)
            prev = n
    # 16 MB at the shape DESIGN.md quotes (one byte per lane and frame up to 128 label positions)
    assert size(lib, kind, 256, 1000, 256, 128) == (OK, 256 * 1000 * 64)
    assert size(lib, kind, 0, 1000, 256, 128)[0] == OK


def test_size_function_limits(lib):
    out = ctypes.c_size_t(0)
    assert size(lib, 0, 4, 50, 256, 1024)[0] == OK
    assert size(lib, 0, 4, 50, 256, 1025)[0] == EINVAL
    assert size(lib, 0, 4, 50, 16384, 64)[0] == OK
    assert size(lib, 0, 4, 50, 16385, 64)[0] == EINVAL
    for bad in ((2, 4, 50, 256, 64), (0, -1, 50, 256, 64), (0, 4, -1, 256, 64), (0, 4, 50, 0, 64), (0, 4, 50, 256, -1)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_best_path_workspace_bytes(0, 4, 50, 256, 64, None) == EINVAL
    # the selectors of ctc_amd_workspace_bytes did not grow
    assert lib.ctc_amd_workspace_bytes(5, 0, 4, 50, 256, 64, ctypes.byref(out)) == EINVAL
