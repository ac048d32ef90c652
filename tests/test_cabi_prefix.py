"""Host layer of the four prefix scorer entry points, in the manner of tests/test_cabi_nbest_loss.py: nothing here touches a GPU.
Validation returns before any launch and pointers are the never-dereferenced address 16: only rejected calls and B == 0 are made."""
import ctypes

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40

HEAD = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, logit_length=ONE, blank=0, B=2, T=5, V=8, N=3, rows=ONE, rows_bytes=BIG)
HEAD_ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "logit_length", "blank", "B", "T", "V", "N", "rows", "rows_bytes")
EXTEND = dict(HEAD, state_in=ONE, last_in=ONE, length_in=ONE, parent=ONE, token=ONE, state_out=ctypes.c_void_p(32), state_bytes=BIG,
              last_out=ONE, length_out=ONE, full=ONE)
EXTEND_ORDER = HEAD_ORDER + ("state_in", "last_in", "length_in", "parent", "token", "state_out", "state_bytes", "last_out", "length_out", "full")
SCORE = dict(HEAD, state=ONE, state_bytes=BIG, last=ONE, length=ONE, score=ONE)
SCORE_ORDER = HEAD_ORDER + ("state", "state_bytes", "last", "length", "score")
ROWS = dict(logits=ONE, xdtype=0, xsb=None, xst=None, logit_length=ONE, B=2, T=5, V=8, rows=ONE, rows_bytes=BIG)
ROWS_ORDER = ("logits", "xdtype", "xsb", "xst", "logit_length", "B", "T", "V", "rows", "rows_bytes")
CALLS = {"extend": ("ctc_amd_prefix_extend", EXTEND, EXTEND_ORDER), "score": ("ctc_amd_prefix_score", SCORE, SCORE_ORDER),
         "rows": ("ctc_amd_prefix_rows", ROWS, ROWS_ORDER)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, which, **over):
    name, base, order = CALLS[which]
    assert not set(over) - set(base), over
    a = dict(base, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    rc = getattr(lib, name)(*(a[k] for k in order), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, which, want_rc, text=None, **over):
    rc, msg = call(lib, which, **over)
    assert rc == want_rc, f"{which} {over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{which} {over}: message {msg!r} lacks {text!r}"


def sizes(lib, B, T, V, N):
    rows, state = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    rc = lib.ctc_amd_prefix_workspace_bytes(B, T, V, N, ctypes.byref(rows), ctypes.byref(state))
    return rc, int(rows.value), int(state.value)


def test_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    for name in ("ctc_amd_prefix_workspace_bytes", "ctc_amd_prefix_rows", "ctc_amd_prefix_extend", "ctc_amd_prefix_score"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name, _, order in CALLS.values():
        assert len(_lib.SIGNATURES[name][1]) == len(order) + 1  # + the stream
    assert _lib.PREFIX_MAX == 64 and _lib.PREFIX_GROUP == 8
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


def test_size_function(lib):
    """The documented formulas: 8 B T bytes of row statistics, 8 B N (2 T + 2) bytes of state."""
    for B, T, V, N in [(0, 0, 3, 1), (3, 0, 3, 2), (2, 5, 8, 3), (256, 1000, 256, 16), (3, 63, 16384, 64)]:
        assert sizes(lib, B, T, V, N) == (OK, 8 * B * T, 8 * B * N * (2 * T + 2)), (B, T, V, N)
    for bad in ((-1, 5, 8, 3), (2, -1, 8, 3), (2, 5, 0, 3), (2, 5, 16385, 3), (2, 5, 8, 0), (2, 5, 8, 65), (2, 5, 8, -1), (2 ** 30, 5, 8, 64)):
        assert sizes(lib, *bad)[0] == EINVAL, bad
    one = ctypes.c_size_t(0)
    assert lib.ctc_amd_prefix_workspace_bytes(2, 5, 8, 3, None, ctypes.byref(one)) == EINVAL
    assert lib.ctc_amd_prefix_workspace_bytes(2, 5, 8, 3, ctypes.byref(one), None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.prefix_workspace_bytes(2, 5, 8, 3) == (80, 8 * 2 * 3 * 12)
    with pytest.raises(ValueError):
        _lib.prefix_workspace_bytes(2, 5, 8, 65)


@pytest.mark.parametrize("which", ["extend", "score"])
@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(wrt=-1), "wrt"),
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(V=-3), None),
    (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(logit_length=None), "null"), (dict(logits=None), "null"),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(V=16385), "V=16385"),
    (dict(N=0), "N 0"), (dict(N=65), "N 65"), (dict(N=-1), "N -1"),
    (dict(B=2 ** 30, N=64), "B * N"),
    (dict(rows=None), "rows"),
])
def test_each_bad_shared_argument_is_einval(lib, which, over, text):
    expect(lib, which, EINVAL, text, **over)


@pytest.mark.parametrize("name", ["parent", "token", "state_out", "last_out", "length_out", "full"])
def test_extend_null_pointers(lib, name):
    expect(lib, "extend", EINVAL, "null", **{name: None})


def test_extend_state_rules(lib):
    expect(lib, "extend", EINVAL, "state_in without", last_in=None)
    expect(lib, "extend", EINVAL, "state_in without", length_in=None)
    expect(lib, "extend", EINVAL, "must not be state_in", state_out=ONE)
    expect(lib, "extend", EWORKSPACE, "state buffer too small", state_bytes=8 * 2 * 3 * 12 - 1)
    expect(lib, "extend", EWORKSPACE, "rows buffer too small", rows_bytes=79)
    expect(lib, "extend", EWORKSPACE, "state buffer too small", wrt=1, rows=None, rows_bytes=0, state_bytes=0)  # log-probabilities need no rows


@pytest.mark.parametrize("name", ["state", "last", "length", "score"])
def test_score_null_pointers(lib, name):
    expect(lib, "score", EINVAL, "null", **{name: None})


def test_score_buffer_sizes(lib):
    expect(lib, "score", EWORKSPACE, "state buffer too small", state_bytes=8 * 2 * 3 * 12 - 1)
    expect(lib, "score", EWORKSPACE, "rows buffer too small", rows_bytes=79)
    expect(lib, "score", EWORKSPACE, "state buffer too small", wrt=1, rows=None, rows_bytes=0, state_bytes=0)


@pytest.mark.parametrize("over,text", [
    (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None), (dict(logit_length=None), "null"), (dict(logits=None), "null"),
    (dict(xdtype=3), "dtype"), (dict(xst=7), "stride"), (dict(xsb=7), "stride"), (dict(V=16385), "V=16385"),
])
def test_rows_bad_arguments(lib, over, text):
    expect(lib, "rows", EINVAL, text, **over)


def test_rows_buffer(lib):
    expect(lib, "rows", EWORKSPACE, "rows buffer too small", rows_bytes=79)
    expect(lib, "rows", EWORKSPACE, "rows buffer too small", rows=None)


@pytest.mark.parametrize("which", ["extend", "score"])
def test_precedence_follows_nbest_loss(lib, which):
    expect(lib, which, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, which, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, which, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, which, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, which, EINVAL, "stride", xst=7, N=0)             # strides before the call's own arguments
    expect(lib, which, EINVAL, "V=16385", V=16385, N=0)          # the vocabulary limit, then N
    expect(lib, which, EINVAL, "N 0", N=0, rows=None)            # ... before the buffers
    expect(lib, which, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


@pytest.mark.parametrize("which", ["extend", "score", "rows"])
def test_empty_batch_is_ok(lib, which):
    expect(lib, which, OK, B=0)
    expect(lib, which, OK, B=0, logits=None, logit_length=None, rows=None, rows_bytes=0)
    expect(lib, which, OK, B=0, xst=7)    # no rows to overlap
