"""Host layer of ctc_amd_star_loss_grad_ckpt / _ckpt_workspace_bytes without a GPU (rejected calls and B == 0 alone): every rejected
call returns what ctc_amd_wildcard_loss_grad returns, message included, under every combination of the two flags."""
import ctypes
import os

import pytest

from tests import test_cabi_wildcard_loss as P
from tests import test_cabi_wildcard_loss_ckpt as C
from tests.test_cabi_wildcard_loss import lib  # noqa: F401  (the fixture: builds and loads the library)

FLAGS = [(1, 0), (0, 1), (1, 1), (0, 0)]  # (optional_wildcards, exclude_next_label)


def call(lib, flags, **over):
    a = P.arguments(**over)
    head, tail = P.ORDER[:P.ORDER.index("weight")], P.ORDER[P.ORDER.index("weight"):]
    rc = lib.ctc_amd_star_loss_grad_ckpt(*(a[k] for k in head), *flags, *(a[k] for k in tail), None)
    return rc, lib.ctc_amd_last_error().decode()


def size(lib, *shape):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_star_loss_ckpt_workspace_bytes(*shape, ctypes.byref(out))
    return rc, int(out.value)


def test_symbols_and_abi_version(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_star_loss_grad_ckpt", "ctc_amd_star_loss_ckpt_workspace_bytes"):
        assert hasattr(lib, name) and f"int {name}(" in header
    twin = _lib.SIGNATURES["ctc_amd_star_loss_grad"]
    assert _lib.SIGNATURES["ctc_amd_star_loss_grad_ckpt"] == (twin[0], twin[1][:12] + [ctypes.c_int] + twin[1][12:])  # + exclude
    assert _lib.SIGNATURES["ctc_amd_star_loss_ckpt_workspace_bytes"] == _lib.SIGNATURES["ctc_amd_wildcard_loss_ckpt_workspace_bytes"]
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_size_is_that_of_the_mandatory_wildcard(lib, shape):
    """U <= 256: the checkpointed size; above: the per-frame one; nothing without a gradient; a bad kind or U is rejected."""
    assert size(lib, *shape, 1) == (P.OK, C.documented(*shape)) and size(lib, *shape, 0) == (P.OK, 0)
    assert size(lib, 2, *shape[1:], 1)[0] == P.EINVAL == size(lib, *shape[:4], 1025, 1)[0]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("over", [c[0] for c in P.BAD_ARGUMENTS] + [
    # precedence: the first fault in the shared order is the one reported
    dict(kind=5, xdtype=3), dict(blank=99, U=1025), dict(xst=7, weight=1.0), dict(weight=1.0, loss=None), dict(V=16385, ws_bytes=0)])
def test_rejections_are_those_of_the_per_frame_call(lib, over, flags):
    got = call(lib, flags, **over)
    assert got[0] == P.EINVAL and got == P.call(lib, **over), over


@pytest.mark.parametrize("flags", FLAGS)
def test_workspace_too_small_and_empty_batch(lib, flags):
    need = C.documented(0, 2, 5, 8, 4)
    for over in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=need)):
        rc, msg = call(lib, flags, **over)
        assert rc == P.EWORKSPACE and "workspace" in msg, over
    assert f"{need - 1} < {need}" in call(lib, flags, ws_bytes=need - 1)[1] and call(lib, flags, B=0)[0] == P.OK
