"""Host layer of ctc_amd_label_posterior / ctc_amd_label_posterior_workspace_bytes, in the manner of tests/test_cabi_wildcard_loss.py:
nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16.  A call that
passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes
import math
import os

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40              # a workspace size that is always enough

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, weight=0.0, B=2, T=5, V=8, U=4, loss=ONE, post=ONE, blk=ONE, dur=ONE, exf=ONE, ws=ONE, ws_bytes=BIG)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank", "weight",
         "B", "T", "V", "U", "loss", "post", "blk", "dur", "exf", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def arguments(**over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    return a


def call(lib, **over):
    a = arguments(**over)
    rc = lib.ctc_amd_label_posterior(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_label_posterior_workspace_bytes(kind, B, T, V, U, ctypes.byref(out))
    return rc, int(out.value)


def formula(kind, B, T, V, U):
    """include/ctc_amd.h: r256(8 * B * T * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B), S = 2 (classic) or 1 (simplified)."""
    nl = 1
    while 64 * nl < U:
        nl *= 2
    r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r256(8 * B * T * ((2 - kind) * 64 * nl + 2)) + r256(16 * B * T) + r256(8 * B)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_label_posterior", "ctc_amd_label_posterior_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    types = _lib.SIGNATURES["ctc_amd_label_posterior"][1]
    assert len(types) == len(ORDER) + 1 == 24  # + the stream
    assert types[ORDER.index("weight")] is ctypes.c_float
    assert len(_lib.SIGNATURES["ctc_amd_label_posterior_workspace_bytes"][1]) == 6
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    assert "int ctc_amd_label_posterior(" in header and "int ctc_amd_label_posterior_workspace_bytes(" in header
    assert "REDUCTIONS OF THE FLOAT32 label_posterior VALUES" in header


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formula on both sides of every U = 64 NL boundary, on both lattices; never more than the wildcard loss asks
    for with a gradient; the limits are those of ctc_amd_wildcard_loss_workspace_bytes."""
    shapes = [(0, 256, 1000, 256, 128), (0, 0, 0, 3, 0), (0, 3, 0, 3, 4), (1, 2, 5, 8, 4), (1, 3, 63, 16384, 1024), (0, 1, 1, 3, 0),
              (1, 1, 1, 3, 1)]
    shapes += [(k, 3, 7, 9, U) for k in (0, 1) for U in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)]
    for s in shapes:
        assert size(lib, *s) == (OK, formula(*s)), s
        wild = ctypes.c_size_t(0)
        assert lib.ctc_amd_wildcard_loss_workspace_bytes(*s, 1, ctypes.byref(wild)) == OK
        assert size(lib, *s)[1] <= int(wild.value), s
    assert size(lib, 0, 256, 1000, 256, 128) == (OK, 256 * 1000 * (8 * 258 + 16) + 2048)
    for bad in ((2, 2, 5, 8, 4), (-1, 2, 5, 8, 4), (0, -1, 5, 8, 4), (0, 2, -1, 8, 4), (0, 2, 5, 0, 4), (0, 2, 5, 16385, 4),
                (0, 2, 5, 8, 1025), (0, 2, 5, 8, -1)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_label_posterior_workspace_bytes(0, 2, 5, 8, 4, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.label_posterior_workspace_bytes(0, 2, 5, 8, 4) == formula(0, 2, 5, 8, 4) == 10496 + 256 + 256
    with pytest.raises(ValueError):
        _lib.label_posterior_workspace_bytes(0, 2, 5, 8, 1025)


BAD_ARGUMENTS = [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), "negative"), (dict(T=-1), "negative"), (dict(V=0), "negative"), (dict(V=-3), "negative"), (dict(U=-1), "negative"),
    (dict(label_stride=-1), "negative"),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=1025), "U=1025"),
    (dict(logit_length=None), "null length"), (dict(label_length=None), "null length"), (dict(logits=None), "null logits"),
    (dict(labels=None), "null labels"),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(weight=0.5), "wildcard_log_weight"), (dict(weight=1e-30), "wildcard_log_weight"), (dict(weight=math.nan), "wildcard_log_weight"),
    (dict(weight=math.inf), "wildcard_log_weight"), (dict(weight=-math.inf), "wildcard_log_weight"),
    (dict(loss=None), "null loss"), (dict(post=None), "label_posterior"), (dict(blk=None), "blank_posterior"),
    (dict(dur=None), "both"), (dict(exf=None), "both"),
    (dict(V=16385), "V=16385"),
]


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS)
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


@pytest.mark.parametrize("over,text", [c for c in BAD_ARGUMENTS if not set(c[0]) & {"loss", "post", "blk", "dur", "exf"}])
def test_every_shared_message_is_that_of_wildcard_loss_grad(lib, over, text):
    """The one argument check of the host layer: code and whole message are those of ctc_amd_wildcard_loss_grad for the same
    arguments."""
    a = arguments(**over)
    rc_ref = lib.ctc_amd_wildcard_loss_grad(*(a[k] for k in ORDER[:16]), None, a["loss"], ONE, 0, a["xsb"], a["xst"], a["ws"], a["ws_bytes"],
                                            None)
    msg_ref = lib.ctc_amd_last_error().decode()
    rc, msg = call(lib, **over)
    assert rc == rc_ref == EINVAL, (over, msg, msg_ref)
    if "V" not in over or over["V"] <= 0:  # (the vocabulary limit names its own call)
        assert msg == msg_ref, (over, msg, msg_ref)


def test_precedence(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=1025)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)                       # common checks before the element type
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)                          # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)                        # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, weight=1.0)                     # strides before the wildcard weight
    expect(lib, EINVAL, "wildcard_log_weight", weight=1.0, loss=None)    # the weight before the outputs
    expect(lib, EINVAL, "null loss", loss=None, dur=None)                # the outputs that must exist before the optional pair
    expect(lib, EINVAL, "label_posterior", post=None, V=16385)           # the outputs before the vocabulary limit
    expect(lib, EINVAL, "both", dur=None, V=16385)
    expect(lib, EINVAL, "V=16385", V=16385, ws_bytes=0)                  # the vocabulary limit before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)                             # a common fault hides B == 0


def test_outputs_without_elements_may_be_null(lib):
    """T == 0: no frame to write, neither matrix is needed; U == 0: no label_posterior element.  Such a call gets as far as the
    workspace."""
    expect(lib, EWORKSPACE, "workspace", T=0, logits=None, post=None, blk=None, ws_bytes=1)
    expect(lib, EWORKSPACE, "workspace", U=0, post=None, ws_bytes=1)
    expect(lib, EINVAL, "blank_posterior", U=0, post=None, blk=None, ws_bytes=1)
    expect(lib, EWORKSPACE, "workspace", dur=None, exf=None, ws_bytes=1)  # the statistics are optional, as a pair


def test_a_workspace_that_is_too_small_is_eworkspace(lib):
    need = formula(0, 2, 5, 8, 4)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace", ws=None)
    expect(lib, EWORKSPACE, "workspace", ws=None, ws_bytes=0)
    for kind, U in ((1, 513), (0, 1024), (0, 65), (1, 64), (0, 129), (1, 257)):
        need = formula(kind, 3, 7, 9, U)
        assert size(lib, kind, 3, 7, 9, U) == (OK, need)
        expect(lib, EWORKSPACE, f"{need - 1} < {need}", kind=kind, B=3, T=7, V=9, U=U, label_stride=U, ws_bytes=need - 1)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, "workspace", xdtype=dt, ws_bytes=1)
    expect(lib, EWORKSPACE, "workspace", xsb=8, xst=16, wrt=1, ws_bytes=1)  # time-major log-probabilities
    expect(lib, EWORKSPACE, "workspace", weight=-0.7, ws_bytes=1)           # a valid penalty gets as far as the workspace


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None, post=None, blk=None, dur=None,
           exf=None, ws=None, ws_bytes=0)
    expect(lib, OK, B=0, xst=7)        # no rows to overlap
    expect(lib, OK, B=0, weight=1.0)   # (B == 0 returns before what only this call takes, as in the other entry points)
    expect(lib, OK, B=0, dur=None)
