"""Host layer of the four windowed entry points (include/ctc_amd.h, "Frame windows per label"), in the manner of
tests/test_cabi_wildcard_best_path.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the
never-dereferenced address 16.  A call that passes every check would launch: only rejected calls and B == 0 are made here, so
"the window is accepted" is shown by the NEXT check in line, the workspace's, answering instead."""
import ctypes
import os
import re

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40

PAIRS = {  # new entry: counterpart
    "ctc_amd_windowed_loss_grad": "ctc_amd_wildcard_loss_grad",
    "ctc_amd_windowed_label_posterior": "ctc_amd_label_posterior",
    "ctc_amd_windowed_best_path": "ctc_amd_wildcard_best_path",
    "ctc_amd_long_windowed_best_path": "ctc_amd_long_wildcard_best_path",
}
B, T, V, U = 2, 5, 8, 4
LEAD = (0, 0, ONE, 0, T * V, V, ONE, 5, ONE, ONE, 0)  # kind .. blank_index
# what follows (frame_window, window_stride) up to, but without, (workspace, workspace_bytes, stream)
TAIL = {
    "ctc_amd_windowed_loss_grad": (0.0, B, T, V, U, None, ONE, ONE, 0, T * V, V),
    "ctc_amd_windowed_label_posterior": (0.0, B, T, V, U, ONE, ONE, ONE, ONE, ONE),
    "ctc_amd_windowed_best_path": (B, T, V, U, ONE, ONE, ONE, ONE, ONE, ONE),
    "ctc_amd_long_windowed_best_path": (B, T, V, U, 0, ONE, ONE, ONE, ONE, ONE, ONE),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, name, window, stride, ws=ONE, ws_bytes=BIG, tail=None):
    rc = getattr(lib, name)(*LEAD, window, stride, *(TAIL[name] if tail is None else tail), ws, ws_bytes, None)
    return rc, lib.ctc_amd_last_error().decode()


def with_batch(name, batch):
    t = list(TAIL[name])
    t[1 if isinstance(t[0], float) else 0] = batch
    return tuple(t)


def test_symbols_and_signatures(lib):
    """Exported, declared, and each signature is its counterpart's with (pointer, int) behind blank_index."""
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    declared = set(re.findall(r"ctc_amd_[a-z_]+", header))
    for new, old in PAIRS.items():
        assert hasattr(lib, new) and new in _lib.SIGNATURES and new in declared, new
        res, args = _lib.SIGNATURES[new]
        ores, oargs = _lib.SIGNATURES[old]
        assert res is ores
        assert list(args) == list(oargs[:11]) + [ctypes.c_void_p, ctypes.c_int] + list(oargs[11:]), new
        # ... and the header says the same: the counterpart's parameter list with the two arguments behind blank_index
        def params(n):
            text = re.search(r"\bint " + n + r"\(([^;]*)\);", header).group(1)
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            return [" ".join(q.split()) for q in text.split(",")]
        po, pn = params(old), params(new)
        k = po.index("int blank_index") + 1
        assert pn == po[:k] + ["const int32_t *frame_window", "int window_stride"] + po[k:], new
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION
    assert not any("windowed" in n and n.endswith("workspace_bytes") for n in declared)  # the counterparts' size queries serve


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_window_stride_below_2u_is_rejected(lib, name):
    for stride in (2 * U - 1, 0, -1, U):
        rc, msg = call(lib, name, ONE, stride)
        assert rc == EINVAL and "window_stride" in msg, (name, stride, rc, msg)
    # at 2 U and beyond the window passes: the workspace check, next in line, answers
    for stride in (2 * U, 2 * U + 1, 1 << 20):
        rc, msg = call(lib, name, ONE, stride, ws_bytes=0)
        assert rc == EWORKSPACE, (name, stride, rc, msg)
    # the counterpart's own checks come first
    rc, msg = getattr(lib, name)(7, *LEAD[1:], ONE, 0, *TAIL[name], ONE, BIG, None), lib.ctc_amd_last_error().decode()
    assert rc == EINVAL and "kind" in msg


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_null_window_takes_any_stride(lib, name):
    for stride in (0, -7, 1, 2 * U, 1 << 30):
        rc, msg = call(lib, name, None, stride, ws_bytes=0)
        assert rc == EWORKSPACE and "window_stride" not in msg, (name, stride, rc, msg)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_empty_batch_is_a_no_op(lib, name):
    for window, stride in ((None, 0), (ONE, 2 * U), (ONE, 0)):
        rc, msg = call(lib, name, window, stride, ws=None, ws_bytes=0, tail=with_batch(name, 0))
        assert rc == OK, (name, window, stride, msg)
