"""Host layer of ctc_amd_wildcard_loss_grad_ckpt / ctc_amd_wildcard_loss_ckpt_workspace_bytes: nothing here touches a GPU (only
rejected calls and B == 0 are made, as in tests/test_cabi_wildcard_loss.py, whose call pattern this file reuses).  The checks are
those of ctc_amd_wildcard_loss_grad, by the same code: every rejected call must return what that call returns, message included."""
import ctypes
import os

import pytest

from tests import test_cabi_wildcard_loss as P
from tests.test_cabi_wildcard_loss import lib  # noqa: F401  (the fixture: builds and loads the library)

OK, EINVAL, EWORKSPACE = P.OK, P.EINVAL, P.EWORKSPACE
BENCH = (256, 1000, 256, 128)


def call(lib, **over):
    a = P.arguments(**over)
    rc = lib.ctc_amd_wildcard_loss_grad_ckpt(*(a[k] for k in P.ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def size(lib, kind, B, T, V, U, want_grad=1):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, want_grad, ctypes.byref(out))
    return rc, int(out.value)


def documented(kind, B, T, V, U):
    """include/ctc_amd.h: checkpoints + statistics + log2 Z with F = 32 / 16 / 8 frames per block (U <= 256; above: the per-frame size)."""
    def r256(x):
        return (x + 255) // 256 * 256
    NL = 1
    while 64 * NL < U:
        NL *= 2
    if NL > 4:
        return P.formula(kind, B, T, V, U, 1)
    F = 32 // NL
    return r256(8 * B * ((T + F - 1) // F) * ((2 - kind) * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B)


def test_symbols_and_abi_version(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctc_amd.h")).read()
    for name, twin in (("ctc_amd_wildcard_loss_grad_ckpt", "ctc_amd_wildcard_loss_grad"),
                       ("ctc_amd_wildcard_loss_ckpt_workspace_bytes", "ctc_amd_wildcard_loss_workspace_bytes")):
        assert hasattr(lib, name) and f"int {name}(" in header
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


# U on both sides of every tier edge, T on both sides of a block edge of each tier (F = 32, 16, 8), the benchmark shape
SHAPES = [(k, 3, T, 9, U) for k in (0, 1) for U, F in ((0, 32), (4, 32), (64, 32), (65, 16), (129, 8), (256, 8)) for T in (F, F + 1)]
SHAPES += [(k, 3, 9, 9, U) for k in (0, 1) for U in (257, 1024)] + [(0, 0, 0, 3, 0), (1, 2, 0, 8, 4), (0, *BENCH), (1, *BENCH)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_size_is_the_documented_formula(lib, shape):
    assert size(lib, *shape) == (OK, documented(*shape)), shape
    assert size(lib, *shape, 0) == (OK, 0)
    if shape[4] > 256:
        assert size(lib, *shape) == P.size(lib, *shape, 1)


@pytest.mark.parametrize("kind", [0, 1])
def test_size_at_the_benchmark_shape(lib, kind):
    """63 blocks of 16 frames, no term in B * T * U: below a third of the per-frame call's workspace (it follows from F >= 4)."""
    got = size(lib, kind, *BENCH)[1]
    assert got == 8 * 256 * 63 * ((2 - kind) * 128 + 2) + 4_096_000 + 2048
    assert 3 * got < P.size(lib, kind, *BENCH, 1)[1]


@pytest.mark.parametrize("bad", [(2, 2, 5, 8, 4), (0, -1, 5, 8, 4), (0, 2, -1, 8, 4), (0, 2, 5, 0, 4), (0, 2, 5, 16385, 4), (0, 2, 5, 8, 1025)])
def test_size_rejects_what_the_per_frame_query_rejects(lib, bad):
    assert size(lib, *bad)[0] == EINVAL == P.size(lib, *bad, 1)[0]
    assert lib.ctc_amd_wildcard_loss_ckpt_workspace_bytes(0, 2, 5, 8, 4, 1, None) == EINVAL


@pytest.mark.parametrize("over", [c[0] for c in P.BAD_ARGUMENTS] + [
    # precedence: the first fault in the shared order is the one reported
    dict(kind=5, xdtype=3), dict(blank=99, U=1025), dict(xdtype=3, B=0), dict(xst=7, weight=1.0), dict(weight=1.0, loss=None),
    dict(loss=None, V=16385), dict(V=16385, ws_bytes=0), dict(grad=None, gsb=0, gst=0, weight=1.0), dict(kind=5, B=0)])
def test_rejections_are_those_of_the_per_frame_call(lib, over):
    got = call(lib, **over)
    assert got[0] == EINVAL and got == P.call(lib, **over), over


def test_workspace_too_small_and_empty_batch(lib):
    need = documented(0, 2, 5, 8, 4)
    assert size(lib, 0, 2, 5, 8, 4) == (OK, need) and 0 < need < P.formula(0, 2, 5, 8, 4, 1)
    for over in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=need), dict(d_loss=None, ws_bytes=need - 1)):
        rc, msg = call(lib, **over)
        assert rc == EWORKSPACE and "workspace" in msg, over
    assert f"{need - 1} < {need}" in call(lib, ws_bytes=need - 1)[1]
    assert call(lib, B=0)[0] == OK
    assert call(lib, B=0, logits=None, labels=None, label_length=None, logit_length=None, d_loss=None, loss=None, grad=None, ws=None,
                ws_bytes=0)[0] == OK
