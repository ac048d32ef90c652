"""Host layer of ctc_amd_label_posterior_ckpt / _workspace_bytes: no GPU (only rejected calls and B == 0 are made, in the pattern of
tests/test_cabi_label_posterior.py).  Every rejected call must return what ctc_amd_label_posterior returns, message included."""
import ctypes
import os

import pytest

from tests import test_cabi_label_posterior as P
from tests.test_cabi_label_posterior import lib  # noqa: F401  (the fixture: builds and loads the library)


def call(lib, **over):
    a = P.arguments(**over)
    rc = lib.ctc_amd_label_posterior_ckpt(*(a[k] for k in P.ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def size(lib, *shape):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_label_posterior_ckpt_workspace_bytes(*shape, ctypes.byref(out))
    return rc, int(out.value)


def test_symbols_signatures_and_abi_version(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctc_amd.h")).read()
    for name, twin in (("ctc_amd_label_posterior_ckpt", "ctc_amd_label_posterior"),
                       ("ctc_amd_label_posterior_ckpt_workspace_bytes", "ctc_amd_label_posterior_workspace_bytes")):
        assert hasattr(lib, name) and f"int {name}(" in header
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("shape", [(k, 3, T, 9, U) for k in (0, 1) for U in (0, 64, 65, 256, 257, 1024) for T in (0, 33)] +
                         [(0, 256, 1000, 256, 128), (1, 256, 1000, 256, 128)], ids=lambda s: "x".join(map(str, s)))
def test_size_is_the_checkpointed_gradients_up_to_256_positions_and_the_per_frame_one_above(lib, shape):
    want = ctypes.c_size_t(0)
    assert lib.ctc_amd_wildcard_loss_ckpt_workspace_bytes(*shape, 1, ctypes.byref(want)) == P.OK
    assert size(lib, *shape) == (P.OK, int(want.value))
    if shape[4] > 256:
        assert size(lib, *shape) == P.size(lib, *shape)
    elif shape[2] > 0:
        assert 3 * size(lib, *shape)[1] < P.size(lib, *shape)[1]


@pytest.mark.parametrize("over", [c[0] for c in P.BAD_ARGUMENTS] + [  # ... and precedence: the first fault in the shared order
    dict(kind=5, xdtype=3), dict(xdtype=3, B=0), dict(xst=7, weight=1.0), dict(weight=1.0, loss=None), dict(loss=None, dur=None),
    dict(post=None, V=16385), dict(V=16385, ws_bytes=0), dict(U=0, post=None, blk=None, ws_bytes=1)])
def test_rejections_are_those_of_the_per_frame_call(lib, over):
    got = call(lib, **over)
    assert got[0] == P.EINVAL and got == P.call(lib, **over), over


def test_workspace_too_small_and_empty_batch(lib):
    need = size(lib, 0, 2, 5, 8, 4)[1]
    assert 0 < need < P.formula(0, 2, 5, 8, 4)
    for over in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=need), dict(T=0, logits=None, post=None, blk=None, ws_bytes=1),
                 dict(dur=None, exf=None, ws_bytes=1)):
        rc, msg = call(lib, **over)
        assert rc == P.EWORKSPACE and "workspace" in msg, over
    assert f"{need - 1} < {need}" in call(lib, ws_bytes=need - 1)[1]
    assert call(lib, B=0)[0] == P.OK
    assert call(lib, B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None, post=None, blk=None, dur=None, exf=None,
                ws=None, ws_bytes=0)[0] == P.OK
