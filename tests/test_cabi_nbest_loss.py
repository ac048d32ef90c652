"""Host layer of ctc_amd_nbest_loss / ctc_amd_nbest_loss_workspace_bytes, in the manner of tests/test_cabi_beam_search.py: nothing
here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16.  The call needs no
workspace, so a call that passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes

import pytest

OK, EINVAL = 0, -1
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, B=2, T=5, V=8, U=4, N=3, loss=ONE, ws=None, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "N", "loss", "ws", "ws_bytes")


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
    rc = lib.ctc_amd_nbest_loss(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, N):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_nbest_loss_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out))
    return rc, int(out.value)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_nbest_loss", "ctc_amd_nbest_loss_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ctc_amd_nbest_loss"][1]) == len(ORDER) + 1  # + the stream
    assert _lib.NBEST_MAX == 64 and _lib.NBEST_GROUP >= 8


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formula: no workspace, 0 bytes for every valid shape (so it is monotone in every argument); the limits are
    those of the call."""
    shapes = [(0, 0, 0, 3, 0, 1), (0, 3, 0, 3, 4, 2), (1, 2, 5, 8, 4, 3), (0, 256, 1000, 256, 128, 32), (1, 3, 63, 16384, 1024, 64)]
    for s in shapes:
        assert size(lib, *s) == (OK, 0), s
    grown = [size(lib, 0, 4 + d[0], 50 + d[1], 64 + d[2], 100 + d[3], 8 + d[4])[1]
             for d in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1))]
    assert all(g >= grown[0] for g in grown)
    for bad in ((2, 2, 5, 8, 4, 3), (-1, 2, 5, 8, 4, 3), (0, -1, 5, 8, 4, 3), (0, 2, -1, 8, 4, 3), (0, 2, 5, 0, 4, 3), (0, 2, 5, 16385, 4, 3),
                (0, 2, 5, 8, 1025, 3), (0, 2, 5, 8, -1, 3), (0, 2, 5, 8, 4, 0), (0, 2, 5, 8, 4, 65), (0, 2, 5, 8, 4, -1),
                (0, 2 ** 30, 5, 8, 4, 64)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_nbest_loss_workspace_bytes(0, 2, 5, 8, 4, 3, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.nbest_loss_workspace_bytes(0, 2, 5, 8, 4, 3) == 0
    with pytest.raises(ValueError):
        _lib.nbest_loss_workspace_bytes(0, 2, 5, 8, 4, 65)


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(V=-3), None), (dict(U=-1), None), (dict(label_stride=-1), None),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=1025), "U=1025"),
    (dict(logit_length=None), "null"), (dict(label_length=None), "null"), (dict(logits=None), "null"), (dict(labels=None), "null"),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(V=16385), "V=16385"),
    (dict(N=0), "N 0"), (dict(N=65), "N 65"), (dict(N=-1), "N -1"),
    (dict(B=2 ** 30, N=64), "B * N"),
    (dict(loss=None), "null"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence_follows_best_path(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "blank", blank=99, xdtype=3)
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, N=0)             # strides before the call's own arguments
    expect(lib, EINVAL, "V=16385", V=16385, N=0)          # the vocabulary limit, then N
    expect(lib, EINVAL, "N 0", N=0, loss=None)            # ... before the output
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None)
    expect(lib, OK, B=0, xst=7)    # no rows to overlap
    expect(lib, OK, B=0, N=0)      # nor hypotheses to count
