"""Host layer of ctc_amd_wildcard_best_path / ctc_amd_wildcard_best_path_workspace_bytes, in the manner of
tests/test_cabi_nbest_best_path.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the
never-dereferenced address 16.  A call that passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40              # a workspace size that is always enough

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, B=2, T=5, V=8, U=4, score=ONE, tokens=ONE, label_index=ONE, first_frame=ONE, last_frame=ONE, label_score=ONE,
            ws=ONE, ws_bytes=BIG)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "score", "tokens", "label_index", "first_frame", "last_frame", "label_score", "ws", "ws_bytes")


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
    rc = lib.ctc_amd_wildcard_best_path(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_wildcard_best_path_workspace_bytes(kind, B, T, V, U, ctypes.byref(out))
    return rc, int(out.value)


def formula(kind, B, T, V, U):
    """include/ctc_amd.h: r256(B * T * 64 * word) + r256(B * T * 8) + r256(B * T * 4), word = 1, 1, 2, 4, 8 bytes for
    NL = 1, 2, 4, 8, 16."""
    nl = 1
    while 64 * nl < U:
        nl *= 2
    word = {1: 1, 2: 1, 4: 2, 8: 4, 16: 8}[nl]
    r256 = lambda x: (x + 255) // 256 * 256  # noqa: E731
    return r256(B * T * 64 * word) + r256(B * T * 8) + r256(B * T * 4)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_wildcard_best_path", "ctc_amd_wildcard_best_path_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ctc_amd_wildcard_best_path"][1]) == len(ORDER) + 1 == 24  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_wildcard_best_path_workspace_bytes"][1]) == 6
    assert _lib.WILDCARD == -2
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    assert "#define CTC_AMD_WILDCARD (-2)" in header


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formula on both sides of every U = 64 NL boundary; the back-pointers of ctc_amd_best_path plus 12 bytes per
    frame; monotone; the limits are those of ctc_amd_best_path_workspace_bytes."""
    shapes = [(0, 256, 1000, 256, 128), (0, 0, 0, 3, 0), (0, 3, 0, 3, 4), (1, 2, 5, 8, 4), (1, 3, 63, 16384, 1024), (0, 1, 1, 3, 0),
              (1, 1, 1, 3, 1)]
    shapes += [(k, 3, 7, 9, U) for k in (0, 1) for U in (64, 65, 128, 129, 256, 257, 512, 513, 1024)]
    for s in shapes:
        assert size(lib, *s) == (OK, formula(*s)), s
        out = ctypes.c_size_t(0)
        assert lib.ctc_amd_best_path_workspace_bytes(*s, ctypes.byref(out)) == OK
        B, T = s[1], s[2]
        assert size(lib, *s)[1] == out.value + formula(0, B, T, 3, 0) - (B * T * 64 + 255) // 256 * 256
    assert size(lib, 0, 256, 1000, 256, 128) == (OK, 256 * 1000 * (64 + 8 + 4))
    assert size(lib, 1, 256, 1000, 256, 128)[1] == size(lib, 0, 256, 1000, 256, 128)[1]  # the word does not depend on the lattice
    for T in (1, 100, 1000):
        prev = -1
        for U in range(0, 1025):
            rc, n = size(lib, 0, 3, T, 256, U)
            assert rc == OK and n >= prev, (T, U, n)
            prev = n
    for bad in ((2, 2, 5, 8, 4), (-1, 2, 5, 8, 4), (0, -1, 5, 8, 4), (0, 2, -1, 8, 4), (0, 2, 5, 0, 4), (0, 2, 5, 16385, 4),
                (0, 2, 5, 8, 1025), (0, 2, 5, 8, -1)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_wildcard_best_path_workspace_bytes(0, 2, 5, 8, 4, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.wildcard_best_path_workspace_bytes(0, 2, 5, 8, 4) == formula(0, 2, 5, 8, 4) == 768 + 256 + 256
    with pytest.raises(ValueError):
        _lib.wildcard_best_path_workspace_bytes(0, 2, 5, 8, 1025)


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
    (dict(score=None), "null score / tokens"), (dict(tokens=None), "null score / tokens"),
    (dict(V=16385), "V=16385"),
]


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS)
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS)
def test_every_message_is_that_of_best_path(lib, over, text):
    """The shared argument check: the code and the whole message are those of ctc_amd_best_path for the same arguments."""
    a = arguments(**over)
    shared = ORDER[:ORDER.index("first_frame")]
    rc_ref = lib.ctc_amd_best_path(*(a[k] for k in shared), a["ws"], a["ws_bytes"], None)
    msg_ref = lib.ctc_amd_last_error().decode()
    rc, msg = call(lib, **over)
    assert rc == rc_ref == EINVAL and msg == msg_ref, (over, msg, msg_ref)


def test_precedence_follows_best_path(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=1025)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, score=None)      # strides before the outputs
    expect(lib, EINVAL, "null", score=None, V=16385)      # outputs before the vocabulary limit
    expect(lib, EINVAL, "V=16385", V=16385, ws_bytes=0)   # the vocabulary limit before the workspace
    expect(lib, EINVAL, "null", tokens=None, ws=None)
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_a_workspace_that_is_too_small_is_eworkspace(lib):
    need = formula(0, 2, 5, 8, 4)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace", ws=None)
    expect(lib, EWORKSPACE, "workspace", ws=None, ws_bytes=0)
    # ... with the optional outputs absent as well: they are accepted, the workspace is what is refused
    expect(lib, EWORKSPACE, "workspace", label_index=None, first_frame=None, last_frame=None, label_score=None, ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace", T=0, tokens=None, ws=None)  # no frames: nothing to write but the score and the labels' padding
    for kind, U in ((1, 513), (0, 1024), (0, 65)):
        need = formula(kind, 3, 7, 9, U)
        expect(lib, EWORKSPACE, "workspace", kind=kind, B=3, T=7, V=9, U=U, label_stride=U, ws_bytes=need - 1)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, "workspace", xdtype=dt, ws_bytes=1)
    expect(lib, EWORKSPACE, "workspace", xsb=8, xst=16, wrt=1, ws_bytes=1)  # time-major log-probabilities


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, score=None, tokens=None, label_index=None,
           first_frame=None, last_frame=None, label_score=None, ws=None, ws_bytes=0)
    expect(lib, OK, B=0, xst=7)    # no rows to overlap
