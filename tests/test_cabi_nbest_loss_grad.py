"""Host layer of ctc_amd_nbest_loss_grad / ctc_amd_nbest_loss_grad_workspace_bytes, in the manner of tests/test_cabi_nbest_loss.py:
nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16.  A call that
passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, B=2, T=5, V=8, U=4, N=3, weight=ONE, loss=ONE, grad=ONE, gdtype=0, gsb=None, gst=None, ws=ONE, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "N", "weight", "loss", "grad", "gdtype", "gsb", "gst", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    for sb, st in (("xsb", "xst"), ("gsb", "gst")):
        if a[sb] is None:
            a[sb] = max(a["T"], 1) * a["V"]
        if a[st] is None:
            a[st] = a["V"]
    rc = lib.ctc_amd_nbest_loss_grad(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, N):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_nbest_loss_grad_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out))
    return rc, int(out.value)


def documented(kind, B, T, V, U, N):
    """include/ctc_amd.h: r256(8 B N T (S 64 NL + 2)) + r256(16 B T) + r256(8 B N)."""
    def r256(x):
        return (x + 255) // 256 * 256
    S = 2 if kind == 0 else 1
    NL = 1
    while 64 * NL < U:
        NL *= 2
    return r256(8 * B * N * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B * N)


def test_both_symbols_are_exported_and_declared(lib):
    import os
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_nbest_loss_grad", "ctc_amd_nbest_loss_grad_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert f"int {name}(" in header
    assert len(_lib.SIGNATURES["ctc_amd_nbest_loss_grad"][1]) == len(ORDER) + 1  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_nbest_loss_grad_workspace_bytes"][1]) == 7


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    shapes = [(0, 0, 0, 3, 0, 1), (0, 3, 0, 3, 4, 2), (1, 2, 5, 8, 4, 3), (0, 2, 5, 8, 64, 3), (0, 2, 5, 8, 65, 3), (1, 2, 5, 8, 129, 3),
              (0, 256, 1000, 256, 128, 8), (1, 256, 1000, 256, 128, 8), (0, 256, 1000, 256, 128, 32), (1, 3, 63, 16384, 1024, 64)]
    for s in shapes:
        assert size(lib, *s) == (OK, documented(*s)), s
    assert size(lib, 0, 256, 1000, 256, 128, 8)[1] == 4_227_072_000 + 4_096_000 + 16_384  # the figure of DESIGN.md section 5.11
    base = (4, 50, 64, 100, 8)
    grown = [size(lib, 0, *(b + d for b, d in zip(base, delta)))[1]
             for delta in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 29, 0), (0, 0, 0, 0, 1))]
    assert all(g >= grown[0] for g in grown) and grown[1] > grown[0] and grown[2] > grown[0] and grown[5] > grown[0] and grown[6] > grown[0]
    for bad in ((2, 2, 5, 8, 4, 3), (-1, 2, 5, 8, 4, 3), (0, -1, 5, 8, 4, 3), (0, 2, -1, 8, 4, 3), (0, 2, 5, 0, 4, 3), (0, 2, 5, 16385, 4, 3),
                (0, 2, 5, 8, 1025, 3), (0, 2, 5, 8, -1, 3), (0, 2, 5, 8, 4, 0), (0, 2, 5, 8, 4, 65), (0, 2, 5, 8, 4, -1),
                (0, 2 ** 30, 5, 8, 4, 64)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_nbest_loss_grad_workspace_bytes(0, 2, 5, 8, 4, 3, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.nbest_loss_grad_workspace_bytes(0, 2, 5, 8, 4, 3) == documented(0, 2, 5, 8, 4, 3)
    with pytest.raises(ValueError):
        _lib.nbest_loss_grad_workspace_bytes(0, 2, 5, 8, 4, 65)


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(V=-3), None), (dict(U=-1), None), (dict(label_stride=-1), None),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=1025), "U=1025"),
    (dict(logit_length=None), "null"), (dict(label_length=None), "null"), (dict(logits=None), "null"), (dict(labels=None), "null"),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"), (dict(gdtype=-1), "dtype"), (dict(gdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(gsb=7), "stride"), (dict(gst=7), "stride"), (dict(gst=0), "stride"), (dict(gsb=-8), "stride"),
    (dict(V=16385), "V=16385"),
    (dict(N=0), "N 0"), (dict(N=65), "N 65"), (dict(N=-1), "N -1"),
    (dict(B=2 ** 30, N=64), "B * N"),
    (dict(weight=None), "null weight / loss / grad"), (dict(loss=None), "null weight / loss / grad"), (dict(grad=None), "null weight / loss / grad"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence_follows_the_forward_call(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element types
    expect(lib, EINVAL, "blank", blank=99, gdtype=3)
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element types before B == 0
    expect(lib, EINVAL, "dtype", gdtype=3, B=0)
    expect(lib, EINVAL, "dtype", gdtype=3, gst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, N=0)             # strides before the call's own arguments
    expect(lib, EINVAL, "stride", gst=7, N=0)
    expect(lib, EINVAL, "V=16385", V=16385, N=0)          # the vocabulary limit, then N
    expect(lib, EINVAL, "N 0", N=0, grad=None)            # ... before the tensors
    expect(lib, EINVAL, "null weight", weight=None, ws_bytes=0)   # the tensors before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_workspace_too_small(lib):
    need = documented(BASE["kind"], BASE["B"], BASE["T"], BASE["V"], BASE["U"], BASE["N"])
    assert size(lib, 0, 2, 5, 8, 4, 3) == (OK, need) and need > 0
    expect(lib, EWORKSPACE, "workspace too small", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace too small", ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace too small", ws=None, ws_bytes=need)  # a null workspace of any stated size


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, weight=None, loss=None, grad=None, ws=None)
    expect(lib, OK, B=0, xst=7, gst=7)  # no rows to overlap
    expect(lib, OK, B=0, N=0)           # nor hypotheses to count
