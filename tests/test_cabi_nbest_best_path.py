"""Host layer of ctc_amd_nbest_best_path / ctc_amd_nbest_best_path_workspace_bytes, in the manner of tests/test_cabi_nbest_loss.py:
nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16.  A call that
passes every check would launch: only rejected calls and B == 0 are made here."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40              # a workspace size that is always enough

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=5, label_length=ONE, logit_length=ONE,
            blank=0, B=2, T=5, V=8, U=4, N=3, score=ONE, tokens=ONE, label_index=ONE, first_frame=ONE, last_frame=ONE, ws=ONE,
            ws_bytes=BIG)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "N", "score", "tokens", "label_index", "first_frame", "last_frame", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, fn="ctc_amd_nbest_best_path", **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    rc = getattr(lib, fn)(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, N):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_nbest_best_path_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out))
    return rc, int(out.value)


def formula(kind, B, T, V, U, N):
    """include/ctc_amd.h: r256(B * N * T * 64 * word), word = 1, 1, 2, 4, 8 bytes for NL = 1, 2, 4, 8, 16."""
    nl = 1
    while 64 * nl < U:
        nl *= 2
    word = {1: 1, 2: 1, 4: 2, 8: 4, 16: 8}[nl]
    return (B * N * T * 64 * word + 255) // 256 * 256


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_nbest_best_path", "ctc_amd_nbest_best_path_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ctc_amd_nbest_best_path"][1]) == len(ORDER) + 1  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_nbest_best_path_workspace_bytes"][1]) == 7


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formula, the north-star shape and both sides of every U = 64 NL boundary; monotone in every argument; the
    limits are those of the call."""
    shapes = [(0, 256, 1000, 256, 128, 8), (0, 0, 0, 3, 0, 1), (0, 3, 0, 3, 4, 2), (1, 2, 5, 8, 4, 3), (1, 3, 63, 16384, 1024, 64),
              (0, 1, 1, 3, 0, 1), (1, 1, 1, 3, 1, 1)]
    shapes += [(k, 3, 7, 9, U, 5) for k in (0, 1) for U in (64, 65, 128, 129, 256, 257, 512, 513, 1024)]
    for s in shapes:
        assert size(lib, *s) == (OK, formula(*s)), s
    assert size(lib, 0, 256, 1000, 256, 128, 8) == (OK, 256 * 8 * 1000 * 64)
    assert size(lib, 1, 256, 1000, 256, 128, 8)[1] == size(lib, 0, 256, 1000, 256, 128, 8)[1]  # the word does not depend on the lattice
    base = (4, 50, 64, 100, 8)
    grown = [size(lib, 0, *(b + d for b, d in zip(base, delta)))[1]
             for delta in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 29, 0), (0, 0, 0, 0, 1))]
    assert all(g >= grown[0] for g in grown) and grown[1] > grown[0] and grown[2] > grown[0] and grown[5] > grown[0] and grown[6] > grown[0]
    for bad in ((2, 2, 5, 8, 4, 3), (-1, 2, 5, 8, 4, 3), (0, -1, 5, 8, 4, 3), (0, 2, -1, 8, 4, 3), (0, 2, 5, 0, 4, 3), (0, 2, 5, 16385, 4, 3),
                (0, 2, 5, 8, 1025, 3), (0, 2, 5, 8, -1, 3), (0, 2, 5, 8, 4, 0), (0, 2, 5, 8, 4, 65), (0, 2, 5, 8, 4, -1),
                (0, 2 ** 30, 5, 8, 4, 64)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_nbest_best_path_workspace_bytes(0, 2, 5, 8, 4, 3, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.nbest_best_path_workspace_bytes(0, 2, 5, 8, 4, 3) == formula(0, 2, 5, 8, 4, 3) == 2048
    with pytest.raises(ValueError):
        _lib.nbest_best_path_workspace_bytes(0, 2, 5, 8, 4, 65)


BAD_ARGUMENTS = [
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
]


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS + [(dict(score=None), "null"), (dict(tokens=None), "null")])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


@pytest.mark.parametrize("over,text", BAD_ARGUMENTS)
def test_shared_arguments_have_the_message_of_nbest_loss(lib, over, text):
    """Where the argument is one ctc_amd_nbest_loss takes too, the code and the whole message are that call's."""
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    shared = ORDER[:ORDER.index("score")]
    rc_loss = lib.ctc_amd_nbest_loss(*(a[k] for k in shared), ONE, None, 0, None)
    msg_loss = lib.ctc_amd_last_error().decode()
    rc, msg = call(lib, **over)
    assert rc == rc_loss == EINVAL and msg == msg_loss, (over, msg, msg_loss)


def test_precedence_follows_nbest_loss(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "blank", blank=99, xdtype=3)
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, N=0)             # strides before the call's own arguments
    expect(lib, EINVAL, "V=16385", V=16385, N=0)          # the vocabulary limit, then N
    expect(lib, EINVAL, "N 0", N=0, score=None)           # ... before the outputs
    expect(lib, EINVAL, "null", score=None, ws_bytes=0)   # the outputs before the workspace
    expect(lib, EINVAL, "null", tokens=None, ws=None)
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_a_workspace_that_is_too_small_is_eworkspace(lib):
    need = formula(0, 2, 5, 8, 4, 3)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace", ws_bytes=0)
    expect(lib, EWORKSPACE, "workspace", ws=None)
    expect(lib, EWORKSPACE, "workspace", ws=None, ws_bytes=0)
    # ... with the optional outputs absent as well: they are accepted, the workspace is what is refused
    expect(lib, EWORKSPACE, "workspace", label_index=None, first_frame=None, last_frame=None, ws_bytes=need - 1)
    need = formula(1, 3, 7, 9, 513, 64)
    expect(lib, EWORKSPACE, "workspace", kind=1, B=3, T=7, V=9, U=513, N=64, label_stride=513, ws_bytes=need - 1)


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, score=None, tokens=None, label_index=None,
           first_frame=None, last_frame=None, ws=None, ws_bytes=0)
    expect(lib, OK, B=0, xst=7)    # no rows to overlap
    expect(lib, OK, B=0, N=0)      # nor hypotheses to count
