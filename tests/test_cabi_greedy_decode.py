"""Host layer of ctc_amd_greedy_decode / ctc_amd_greedy_decode_workspace_bytes, in the manner of tests/test_cabi_best_path.py:
nothing here touches a GPU.  Validation returns before any launch, pointers are the never-dereferenced address 16 and no call
is given a workspace, so a call that passes every check stops at CTC_AMD_EWORKSPACE."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, logit_length=ONE, blank=0, B=2, T=5, V=8,
            score=ONE, tokens=ONE, decoded=ONE, decoded_length=ONE, frames=ONE, label_score=ONE, ws=None, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "logit_length", "blank", "B", "T", "V",
         "score", "tokens", "decoded", "decoded_length", "frames", "label_score", "ws", "ws_bytes")


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
    rc = lib.ctc_amd_greedy_decode(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, B, T):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_greedy_decode_workspace_bytes(B, T, ctypes.byref(out))
    return rc, int(out.value)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_greedy_decode", "ctc_amd_greedy_decode_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ctc_amd_greedy_decode"][1]) == len(ORDER) + 1  # + the stream


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    for B, T in ((0, 0), (0, 7), (3, 0), (1, 1), (2, 5), (3, 63), (7, 129), (256, 1000), (32, 100000)):
        rc, n = size(lib, B, T)
        assert rc == OK and n >= B * T * 4 and n % 256 == 0 and n < B * T * 4 + 256, (B, T, n)
    assert size(lib, 256, 1000) == (OK, 256 * 1000 * 4)  # 1 MB at the shape DESIGN.md quotes
    assert size(lib, -1, 5)[0] == EINVAL and size(lib, 2, -1)[0] == EINVAL
    assert lib.ctc_amd_greedy_decode_workspace_bytes(2, 5, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.greedy_decode_workspace_bytes(2, 5) == size(lib, 2, 5)[1]
    with pytest.raises(ValueError):
        _lib.greedy_decode_workspace_bytes(-1, 5)


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(V=-3), None),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(logit_length=None), None), (dict(logits=None), None),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(score=None), "null"), (dict(tokens=None), "null"), (dict(decoded=None), "null"), (dict(decoded_length=None), "null"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence_follows_best_path(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "blank", blank=99, xdtype=3)
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, score=None)      # strides before the outputs
    expect(lib, EINVAL, "null", score=None, ws=ONE, ws_bytes=1)  # outputs before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, logit_length=None, score=None, tokens=None, decoded=None, decoded_length=None, frames=None,
           label_score=None)
    expect(lib, OK, B=0, xst=7)  # no rows to overlap


def test_a_valid_call_stops_at_the_workspace(lib):
    expect(lib, EWORKSPACE)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=1)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=2 * 5 * 4 - 1)
    expect(lib, EWORKSPACE, kind=1, wrt=1)
    expect(lib, EWORKSPACE, frames=None)                    # the two optional outputs
    expect(lib, EWORKSPACE, label_score=None)
    expect(lib, EWORKSPACE, frames=None, label_score=None)
    expect(lib, EWORKSPACE, blank=7)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, xdtype=dt)
    expect(lib, EWORKSPACE, xsb=8, xst=16)                  # time-major
    expect(lib, EWORKSPACE, xsb=5 * 11, xst=11)             # padded rows
    expect(lib, EWORKSPACE, logits=ctypes.c_void_p(20))     # a base pointer that is not 16-byte aligned: element-wise rows


def test_there_is_no_vocabulary_limit(lib):
    expect(lib, EWORKSPACE, V=20000)
    expect(lib, EWORKSPACE, V=20000, blank=19999)
    expect(lib, EWORKSPACE, V=16385, xdtype=1)
    expect(lib, EINVAL, "blank", V=20000, blank=20000)
