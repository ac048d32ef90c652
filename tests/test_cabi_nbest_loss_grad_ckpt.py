"""Host layer of ctc_amd_nbest_loss_grad_ckpt / ctc_amd_nbest_loss_grad_ckpt_workspace_bytes: nothing here touches a GPU (only
rejected calls and B == 0 are made, as in tests/test_cabi_nbest_loss_grad.py, whose call pattern this file reuses).  The checks are
those of ctc_amd_nbest_loss_grad, by the same code: every rejected call must return what that call returns, message included."""
import ctypes

import pytest

from tests import test_cabi_nbest_loss_grad as P
from tests.test_cabi_nbest_loss_grad import lib  # noqa: F401  (the fixture: builds and loads the library)

OK, EINVAL, EWORKSPACE = P.OK, P.EINVAL, P.EWORKSPACE


def call(lib, **over):
    a = dict(P.BASE, **over)
    for sb, st in (("xsb", "xst"), ("gsb", "gst")):
        a[sb] = max(a["T"], 1) * a["V"] if a[sb] is None else a[sb]
        a[st] = a["V"] if a[st] is None else a[st]
    rc = lib.ctc_amd_nbest_loss_grad_ckpt(*(a[k] for k in P.ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def size(lib, *shape):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_nbest_loss_grad_ckpt_workspace_bytes(*shape, ctypes.byref(out))
    return rc, int(out.value)


def documented(kind, B, T, V, U, N):
    """include/ctc_amd.h: checkpoints + statistics + log2 P + the accumulator when N > 8 (U <= 256; above: the three-launch size)."""
    def r256(x):
        return (x + 255) // 256 * 256
    S = 2 if kind == 0 else 1
    NL = 1
    while 64 * NL < U:
        NL *= 2
    if NL > 4:
        return P.documented(kind, B, T, V, U, N)
    F = 16 // NL
    return r256(8 * B * N * ((T + F - 1) // F) * (S * 64 * NL + 2)) + r256(16 * B * T) + r256(8 * B * N) + (r256(4 * B * T * V) if N > 8 else 0)


def test_symbols_and_abi_version(lib):
    import os
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_nbest_loss_grad_ckpt", "ctc_amd_nbest_loss_grad_ckpt_workspace_bytes"):
        assert hasattr(lib, name) and f"int {name}(" in header
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_ckpt", "")]
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("shape", [(0, 0, 0, 3, 0, 1), (1, 2, 5, 8, 4, 3), (0, 2, 16, 8, 64, 8), (0, 2, 17, 8, 64, 9), (1, 2, 5, 8, 65, 3),
                                   (0, 2, 5, 8, 129, 17), (1, 3, 9, 1030, 256, 64), (0, 2, 5, 8, 257, 3), (1, 3, 63, 16384, 1024, 64),
                                   (0, 256, 1000, 256, 128, 8), (1, 256, 1000, 256, 128, 8), (0, 256, 1000, 256, 128, 32)])
def test_size_is_the_documented_formula(lib, shape):
    assert size(lib, *shape) == (OK, documented(*shape)), shape
    if shape[4] > 256:
        assert size(lib, *shape) == P.size(lib, *shape)


def test_size_at_the_benchmark_shape(lib):
    """125 blocks of 8 frames, 258 doubles each, no term in B * N * T * U: below a quarter of the three-launch call's workspace."""
    got = size(lib, 0, 256, 1000, 256, 128, 8)[1]
    assert got == 8 * 256 * 8 * 125 * 258 + 4_096_000 + 16_384
    assert 4 * got < P.size(lib, 0, 256, 1000, 256, 128, 8)[1]
    assert 4 * size(lib, 1, 256, 1000, 256, 128, 8)[1] < P.size(lib, 1, 256, 1000, 256, 128, 8)[1]


@pytest.mark.parametrize("bad", [(2, 2, 5, 8, 4, 3), (0, -1, 5, 8, 4, 3), (0, 2, -1, 8, 4, 3), (0, 2, 5, 0, 4, 3), (0, 2, 5, 16385, 4, 3),
                                 (0, 2, 5, 8, 1025, 3), (0, 2, 5, 8, 4, 0), (0, 2, 5, 8, 4, 65), (0, 2 ** 30, 5, 8, 4, 64)])
def test_size_rejects_what_the_three_launch_query_rejects(lib, bad):
    assert size(lib, *bad)[0] == EINVAL == P.size(lib, *bad)[0]
    assert lib.ctc_amd_nbest_loss_grad_ckpt_workspace_bytes(0, 2, 5, 8, 4, 3, None) == EINVAL


@pytest.mark.parametrize("over", [
    dict(kind=5), dict(wrt=2), dict(B=-1), dict(T=-1), dict(V=0), dict(U=-1), dict(label_stride=-1), dict(blank=8), dict(U=1025),
    dict(logit_length=None), dict(logits=None), dict(labels=None), dict(xdtype=3), dict(gdtype=3), dict(xst=7), dict(gsb=7), dict(gst=0),
    dict(V=16385), dict(N=0), dict(N=65), dict(B=2 ** 30, N=64), dict(weight=None), dict(loss=None), dict(grad=None),
    # precedence: the first fault in the shared order is the one reported
    dict(kind=5, xdtype=3), dict(blank=99, gdtype=3), dict(xdtype=3, B=0), dict(gdtype=3, gst=7), dict(gst=7, N=0), dict(V=16385, N=0),
    dict(N=0, grad=None), dict(weight=None, ws_bytes=0), dict(kind=5, B=0),
])
def test_rejections_are_those_of_the_three_launch_call(lib, over):
    got = call(lib, **over)
    assert got[0] == EINVAL and got == P.call(lib, **over), over


def test_workspace_too_small_and_empty_batch(lib):
    need = documented(*(P.BASE[k] for k in ("kind", "B", "T", "V", "U", "N")))
    assert size(lib, 0, 2, 5, 8, 4, 3) == (OK, need) and need > 0
    for over in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=need)):
        rc, msg = call(lib, **over)
        assert rc == EWORKSPACE and "workspace too small" in msg, over
    assert call(lib, B=0)[0] == OK
    assert call(lib, B=0, logits=None, labels=None, label_length=None, logit_length=None, weight=None, loss=None, grad=None, ws=None)[0] == OK
