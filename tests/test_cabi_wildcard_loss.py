"""Host layer of ctc_amd_wildcard_loss_grad / ctc_amd_wildcard_loss_workspace_bytes, in the manner of
tests/test_cabi_wildcard_best_path.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the
never-dereferenced address 16.  A call that passes every check would launch: only rejected calls and B == 0 are made here (so a
forward-only call, which needs no workspace, is only ever made with another fault in it)."""
import ctypes
import math

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40              # a workspace size that is always enough

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, weight=0.0, B=2, T=5, V=8, U=4, d_loss=ONE, loss=ONE, grad=ONE, gdtype=0, gsb=None, gst=None, ws=ONE, ws_bytes=BIG)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank", "weight",
         "B", "T", "V", "U", "d_loss", "loss", "grad", "gdtype", "gsb", "gst", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def arguments(**over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    for sb, st in (("xsb", "xst"), ("gsb", "gst")):
        if a[sb] is None:
            a[sb] = max(a["T"], 1) * a["V"]
        if a[st] is None:
            a[st] = a["V"]
    return a


def call(lib, **over):
    a = arguments(**over)
    rc = lib.ctc_amd_wildcard_loss_grad(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, want_grad):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, U, want_grad, ctypes.byref(out))
    return rc, int(out.value)


def formula(kind, B, T, V, U, want_grad):
    """include/ctc_amd.h: nothing without a gradient; with one r256(8 * B * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B),
    S = 2 (classic) or 1 (simplified)."""
    if not want_grad:
        return 0
    nl = 1
    while 64 * nl < U:
        nl *= 2
    r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r256(8 * B * T * ((2 - kind) * 64 * nl + 2)) + r256(16 * B * T) + r256(8 * B)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_wildcard_loss_grad", "ctc_amd_wildcard_loss_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    types = _lib.SIGNATURES["ctc_amd_wildcard_loss_grad"][1]
    assert len(types) == len(ORDER) + 1 == 25  # + the stream
    assert types[ORDER.index("weight")] is ctypes.c_float
    assert len(_lib.SIGNATURES["ctc_amd_wildcard_loss_workspace_bytes"][1]) == 7
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    assert "int ctc_amd_wildcard_loss_grad(" in header and "int ctc_amd_wildcard_loss_workspace_bytes(" in header
    assert "NOT A PROBABILITY" in header


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formula on both sides of every U = 64 NL boundary (NL = 1 ... 16), on both lattices, with and without a
    gradient; monotone in U; the limits are those of ctc_amd_wildcard_best_path_workspace_bytes."""
    shapes = [(0, 256, 1000, 256, 128), (0, 0, 0, 3, 0), (0, 3, 0, 3, 4), (1, 2, 5, 8, 4), (1, 3, 63, 16384, 1024), (0, 1, 1, 3, 0),
              (1, 1, 1, 3, 1)]
    shapes += [(k, 3, 7, 9, U) for k in (0, 1) for U in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)]
    for s in shapes:
        for want in (0, 1):
            assert size(lib, *s, want) == (OK, formula(*s, want)), (s, want)
        assert size(lib, *s, 7) == size(lib, *s, 1)  # any non-zero value asks for the gradient
    assert size(lib, 0, 256, 1000, 256, 128, 1) == (OK, 256 * 1000 * (8 * 258 + 16) + 2048)
    assert size(lib, 1, 256, 1000, 256, 128, 1) == (OK, 256 * 1000 * (8 * 130 + 16) + 2048)
    for T in (1, 100, 1000):
        for kind in (0, 1):
            prev = -1
            for U in range(0, 1025):
                rc, n = size(lib, kind, 3, T, 256, U, 1)
                assert rc == OK and n >= prev, (T, U, n)
                prev = n
    for bad in ((2, 2, 5, 8, 4), (-1, 2, 5, 8, 4), (0, -1, 5, 8, 4), (0, 2, -1, 8, 4), (0, 2, 5, 0, 4), (0, 2, 5, 16385, 4),
                (0, 2, 5, 8, 1025), (0, 2, 5, 8, -1)):
        for want in (0, 1):
            assert size(lib, *bad, want)[0] == EINVAL, bad
    assert lib.ctc_amd_wildcard_loss_workspace_bytes(0, 2, 5, 8, 4, 1, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.wildcard_loss_workspace_bytes(0, 2, 5, 8, 4) == formula(0, 2, 5, 8, 4, 1) == 10496 + 256 + 256
    assert _lib.wildcard_loss_workspace_bytes(0, 2, 5, 8, 4, want_grad=False) == 0
    with pytest.raises(ValueError):
        _lib.wildcard_loss_workspace_bytes(0, 2, 5, 8, 1025)


BAD_ARGUMENTS = [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(V=0), "negative"), (dict(V=-3), "negative"), (dict(U=-1), "negative"),
    (dict(label_stride=-1), "negative"),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=1025), "U=1025"),
    (dict(logit_length=None), "null length"), (dict(label_length=None), "null length"), (dict(logits=None), "null logits"),
    (dict(labels=None), "null labels"),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"), (dict(gdtype=-1), "dtype"), (dict(gdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(gsb=7), "stride"), (dict(gst=7), "stride"), (dict(gst=0), "stride"), (dict(gsb=-8), "stride"),
    (dict(weight=0.5), "wildcard_log_weight"), (dict(weight=1e-30), "wildcard_log_weight"), (dict(weight=math.nan), "wildcard_log_weight"),
    (dict(weight=math.inf), "wildcard_log_weight"), (dict(weight=-math.inf), "wildcard_log_weight"),
    (dict(loss=None), "null loss"),
    (dict(V=16385), "V=16385"),
    (dict(B=1 << 20, T=1 << 14), "launch grid"),
]


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS)
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


@pytest.mark.parametrize("over,text", [c for c in BAD_ARGUMENTS if not set(c[0]) & {"weight", "loss", "B"} or c[0].get("B") == -1])
def test_every_shared_message_is_that_of_nbest_loss_grad(lib, over, text):
    """The one argument check of the host layer: code and whole message are those of ctc_amd_nbest_loss_grad for the same arguments."""
    a = arguments(**over)
    rc_ref = lib.ctc_amd_nbest_loss_grad(*(a[k] for k in ORDER[:11]), *(a[k] for k in ("B", "T", "V", "U")), 1, ONE, a["loss"], a["grad"],
                                         a["gdtype"], a["gsb"], a["gst"], a["ws"], a["ws_bytes"], None)
    msg_ref = lib.ctc_amd_last_error().decode()
    rc, msg = call(lib, **over)
    assert rc == rc_ref == EINVAL, (over, msg, msg_ref)
    if "V" not in over or over["V"] <= 0:  # (the vocabulary limit names its own call)
        assert msg == msg_ref, (over, msg, msg_ref)


def test_gradient_strides_are_not_looked_at_without_a_gradient(lib):
    expect(lib, EINVAL, "wildcard_log_weight", grad=None, gsb=0, gst=0, weight=1.0)  # (passes the strides, stops at the weight)
    expect(lib, EINVAL, "stride", grad=None, xst=7, weight=1.0)                      # the logits' strides still count
    expect(lib, EINVAL, "dtype", grad=None, gdtype=5)                                # the element type is checked with the logits'


def test_precedence(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=1025)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)               # common checks before the element type
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)                  # element type before B == 0
    expect(lib, EINVAL, "dtype", gdtype=3, xst=7)                # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, weight=1.0)             # strides before the wildcard weight
    expect(lib, EINVAL, "wildcard_log_weight", weight=1.0, loss=None)  # the weight before the output
    expect(lib, EINVAL, "null loss", loss=None, V=16385)         # the output before the vocabulary limit
    expect(lib, EINVAL, "V=16385", V=16385, ws_bytes=0)          # the vocabulary limit before the workspace
    expect(lib, EINVAL, "launch grid", B=1 << 20, T=1 << 14, ws_bytes=0)
    expect(lib, EINVAL, "kind", kind=5, B=0)                     # a common fault hides B == 0


def test_a_workspace_that_is_too_small_is_eworkspace(lib):
    need = formula(0, 2, 5, 8, 4, 1)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace", ws=None)
    expect(lib, EWORKSPACE, "workspace", ws=None, ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace", d_loss=None, ws_bytes=need - 1)  # d_loss is optional: the workspace is what is refused
    for kind, U in ((1, 513), (0, 1024), (0, 65), (1, 64), (0, 129), (1, 257)):
        need = formula(kind, 3, 7, 9, U, 1)
        assert size(lib, kind, 3, 7, 9, U, 1) == (OK, need)  # grad != NULL needs exactly what want_grad sizes
        expect(lib, EWORKSPACE, "workspace", kind=kind, B=3, T=7, V=9, U=U, label_stride=U, ws_bytes=need - 1)
        expect(lib, EWORKSPACE, f"{need - 1} < {need}", kind=kind, B=3, T=7, V=9, U=U, label_stride=U, ws_bytes=need - 1)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, "workspace", xdtype=dt, gdtype=dt, ws_bytes=1)
    expect(lib, EWORKSPACE, "workspace", xsb=8, xst=16, gsb=8, gst=16, wrt=1, ws_bytes=1)  # time-major log-probabilities
    expect(lib, EWORKSPACE, "workspace", weight=-0.7, ws_bytes=1)                          # a valid penalty gets as far as the workspace


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, d_loss=None, loss=None, grad=None, ws=None,
           ws_bytes=0)
    expect(lib, OK, B=0, xst=7, gst=7)  # no rows to overlap
    expect(lib, OK, B=0, weight=1.0)    # (B == 0 returns before what only this call takes, as in the other entry points)
