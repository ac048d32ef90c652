"""Host layer of ctc_amd_beam_search / ctc_amd_beam_search_workspace_bytes, in the manner of tests/test_cabi_greedy_decode.py:
nothing here touches a GPU.  Validation returns before any launch, pointers are the never-dereferenced address 16 and no call
is given a workspace, so a call that passes every check stops at CTC_AMD_EWORKSPACE."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, logit_length=ONE, blank=0, B=2, T=5, V=8,
            W=4, K=3, nbest=2, score=ONE, decoded=ONE, decoded_length=ONE, ws=None, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "logit_length", "blank", "B", "T", "V", "W", "K", "nbest",
         "score", "decoded", "decoded_length", "ws", "ws_bytes")


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
    rc = lib.ctc_amd_beam_search(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, B, T, V, W, K):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_beam_search_workspace_bytes(B, T, V, W, K, ctypes.byref(out))
    return rc, int(out.value)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_beam_search", "ctc_amd_beam_search_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ctc_amd_beam_search"][1]) == len(ORDER) + 1  # + the stream


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The row-stage records (16 + 8 * min(K, V - 1) bytes per frame) plus the trie (8 bytes per node, 1 + W * T nodes per utterance),
    each rounded up to 256 bytes; it grows with every argument until the cut reaches V - 1."""
    for B, T, V, W, K in ((0, 0, 3, 1, 1), (0, 7, 3, 4, 2), (3, 0, 3, 4, 2), (1, 1, 2, 1, 1), (2, 5, 8, 4, 3), (3, 63, 64, 64, 32),
                          (256, 1000, 256, 64, 32), (2, 70, 16384, 5, 32)):
        rc, n = size(lib, B, T, V, W, K)
        k = min(K, V - 1)
        lo = B * T * (16 + 8 * k) + B * (1 + W * T) * 8
        assert rc == OK and n % 256 == 0 and lo <= n < lo + 512, (B, T, V, W, K, n, lo)
    base = size(lib, 4, 50, 64, 8, 8)[1]
    assert size(lib, 5, 50, 64, 8, 8)[1] > base and size(lib, 4, 51, 64, 8, 8)[1] > base
    assert size(lib, 4, 50, 64, 9, 8)[1] > base and size(lib, 4, 50, 64, 8, 9)[1] > base
    assert size(lib, 4, 50, 65, 8, 8)[1] == base                       # V alone changes nothing ...
    assert size(lib, 4, 50, 5, 8, 8)[1] == size(lib, 4, 50, 5, 8, 4)[1]  # ... until it limits the cut
    assert size(lib, 4, 50, 5, 8, 8)[1] < base
    for bad in ((-1, 5, 8, 4, 3), (2, -1, 8, 4, 3), (2, 5, 0, 4, 3), (2, 5, 16385, 4, 3), (2, 5, 8, 0, 3), (2, 5, 8, 65, 3),
                (2, 5, 8, 4, 0), (2, 5, 8, 4, 33)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert size(lib, 2, 5, 16384, 64, 32)[0] == OK
    assert lib.ctc_amd_beam_search_workspace_bytes(2, 5, 8, 4, 3, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.beam_search_workspace_bytes(2, 5, 8, 4, 3) == size(lib, 2, 5, 8, 4, 3)[1]
    with pytest.raises(ValueError):
        _lib.beam_search_workspace_bytes(2, 5, 8, 65, 3)


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(V=-3), None),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(logit_length=None), None), (dict(logits=None), None),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(V=16385), "V=16385"),
    (dict(W=0), "beam_width"), (dict(W=65), "beam_width"), (dict(W=-1), "beam_width"),
    (dict(K=0), "top_k"), (dict(K=33), "top_k"), (dict(K=-1), "top_k"),
    (dict(nbest=0), "nbest"), (dict(nbest=5), "nbest"), (dict(nbest=-1), "nbest"),
    (dict(score=None), "null"), (dict(decoded=None), "null"), (dict(decoded_length=None), "null"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_precedence_follows_greedy_decode(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "blank", blank=99, xdtype=3)
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, W=0)             # strides before the search's own arguments
    expect(lib, EINVAL, "beam_width", W=0, K=0)           # beam_width, top_k, nbest in that order
    expect(lib, EINVAL, "top_k", K=0, nbest=0)
    expect(lib, EINVAL, "nbest", nbest=0, score=None)     # ... before the outputs
    expect(lib, EINVAL, "null", score=None, ws=ONE, ws_bytes=1)  # outputs before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, logit_length=None, score=None, decoded=None, decoded_length=None)
    expect(lib, OK, B=0, xst=7)  # no rows to overlap


def test_a_valid_call_stops_at_the_workspace(lib):
    expect(lib, EWORKSPACE)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=1)
    need = size(lib, 2, 5, 8, 4, 3)[1]
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=need - 1)
    expect(lib, EWORKSPACE, ws=None, ws_bytes=need)         # enough bytes of nothing
    expect(lib, EWORKSPACE, kind=1, wrt=1)
    expect(lib, EWORKSPACE, blank=7)
    expect(lib, EWORKSPACE, W=64, K=32, nbest=64)           # the limits themselves
    expect(lib, EWORKSPACE, W=1, K=1, nbest=1)
    expect(lib, EWORKSPACE, K=32)                           # a cut beyond V - 1 is no fault
    expect(lib, EWORKSPACE, V=16384, blank=16383)
    expect(lib, EWORKSPACE, T=0, decoded=None)              # no frames: nothing to decode into
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, xdtype=dt)
    expect(lib, EWORKSPACE, xsb=8, xst=16)                  # time-major
    expect(lib, EWORKSPACE, xsb=5 * 11, xst=11)             # padded rows
    expect(lib, EWORKSPACE, logits=ctypes.c_void_p(20))     # a base pointer that is not 16-byte aligned: element-wise rows
