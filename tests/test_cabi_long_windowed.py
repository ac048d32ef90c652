"""Host layer of the three long-form windowed entry points of the summed lattice (include/ctc_amd.h, "Frame windows per label"),
in the manner of tests/test_cabi_windowed.py: nothing here touches a GPU.  Validation returns before any launch and pointers are
the never-dereferenced address 16.  A call that passes every check would launch: only rejected calls and B == 0 are made here, so
"the window is accepted" is shown by the NEXT check in line, the workspace's, answering instead."""
import ctypes
import os
import re

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40

PAIRS = {  # new entry: counterpart
    "ctc_amd_long_windowed_loss_grad": "ctc_amd_long_wildcard_loss_grad",
    "ctc_amd_long_windowed_loss_grad_ckpt": "ctc_amd_long_wildcard_loss_grad_ckpt",
    "ctc_amd_long_windowed_label_posterior": "ctc_amd_long_label_posterior",
}
B, T, V, U = 2, 5, 8, 4
LEAD = (0, 0, ONE, 0, T * V, V, ONE, 5, ONE, ONE, 0)  # kind .. blank_index
# what follows (frame_window, window_stride) up to, but without, (workspace, workspace_bytes, stream)
LOSS_TAIL = (0.0, B, T, V, U, 0, None, ONE, ONE, 0, T * V, V)  # weight, sizes, frames_per_tile, d_loss, loss, grad and its format
TAIL = {
    "ctc_amd_long_windowed_loss_grad": LOSS_TAIL,
    "ctc_amd_long_windowed_loss_grad_ckpt": LOSS_TAIL,
    "ctc_amd_long_windowed_label_posterior": (0.0, B, T, V, U, 0, ONE, ONE, ONE, ONE, ONE, ONE, ONE),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, name, window, stride, ws=ONE, ws_bytes=BIG, tail=None, lead=LEAD):
    rc = getattr(lib, name)(*lead, window, stride, *(TAIL[name] if tail is None else tail), ws, ws_bytes, None)
    return rc, lib.ctc_amd_last_error().decode()


def with_tail(name, **at):
    """The tail with B (index 1) or frames_per_tile (index 5) replaced."""
    t = list(TAIL[name])
    for k, v in at.items():
        t[{"batch": 1, "frames_per_tile": 5}[k]] = v
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
        assert getattr(lib, new).argtypes == list(args), new  # ... and that is what ctypes converts with

        # the header says the same: the counterpart's parameter list with the two arguments behind blank_index
        def params(n):
            text = re.search(r"\bint " + n + r"\(([^;]*)\);", header).group(1)
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            return [" ".join(q.split()) for q in text.split(",")]
        po, pn = params(old), params(new)
        k = po.index("int blank_index") + 1
        assert pn == po[:k] + ["const int32_t *frame_window", "int window_stride"] + po[k:], new
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION
    # the counterparts' size queries serve: none of its own, in the header or in the library
    assert not any("windowed" in n and n.endswith("workspace_bytes") for n in declared)
    for new in PAIRS:
        for name in (new + "_workspace_bytes", new.replace("_grad", "") + "_workspace_bytes"):
            with pytest.raises(AttributeError):
                getattr(lib, name)
    # the header's table names all three beside their counterparts
    for new, old in PAIRS.items():
        assert re.search(r"\* +" + new + r" +" + old + r"\b", header), new


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_window_stride_below_2u_is_rejected(lib, name):
    for stride in (2 * U - 1, 0, -1, U):
        rc, msg = call(lib, name, ONE, stride)
        assert rc == EINVAL and "window_stride" in msg, (name, stride, rc, msg)
    # at 2 U and beyond the window passes: the workspace check, next in line, answers
    for stride in (2 * U, 2 * U + 1, 1 << 20):
        rc, msg = call(lib, name, ONE, stride, ws_bytes=0)
        assert rc == EWORKSPACE and "window_stride" not in msg, (name, stride, rc, msg)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_the_counterparts_own_checks_come_first(lib, name):
    """With a window whose stride is too small, whatever the counterpart refuses is refused with the counterpart's message."""
    old = PAIRS[name]

    def both(lead=LEAD, tail=None):
        tail = TAIL[name] if tail is None else tail
        got = call(lib, name, ONE, 0, tail=tail, lead=lead)
        rc = getattr(lib, old)(*lead, *tail, ONE, BIG, None)
        return got, (rc, lib.ctc_amd_last_error().decode())

    got, want = both(lead=(7,) + LEAD[1:])
    assert got == want and got[0] == EINVAL and "kind" in got[1], (got, want)
    got, want = both(tail=with_tail(name, frames_per_tile=3))  # no multiple of 4: the tiling is the counterpart's check too
    assert got == want and got[0] == EINVAL and "window_stride" not in got[1], (got, want)
    weight = (1.0,) + TAIL[name][1:]
    got, want = both(tail=weight)
    assert got == want and got[0] == EINVAL and "window_stride" not in got[1], (got, want)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_null_window_takes_any_stride(lib, name):
    for stride in (0, -7, 1, 2 * U, 1 << 30):
        rc, msg = call(lib, name, None, stride, ws_bytes=0)
        assert rc == EWORKSPACE and "window_stride" not in msg, (name, stride, rc, msg)
        # ... and is the counterpart: the same answer, the same words
        old = getattr(lib, PAIRS[name])(*LEAD, *TAIL[name], ONE, 0, None)
        assert (old, lib.ctc_amd_last_error().decode()) == (rc, msg)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_empty_batch_is_a_no_op(lib, name):
    for window, stride in ((None, 0), (ONE, 2 * U), (ONE, 0)):
        rc, msg = call(lib, name, window, stride, ws=None, ws_bytes=0, tail=with_tail(name, batch=0))
        assert rc == OK, (name, window, stride, msg)


def test_python_layer_is_declared():
    """The loss functions take a keyword-only frame_window.  The unwindowed posterior functions and ops.long_wildcard_loss_grad keep
    their signatures, so the window comes through functions of its own: *_long_windowed_label_posterior is its counterpart plus the
    keyword, ops.long_windowed_loss_grad its counterpart behind frame_window."""
    import inspect

    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops
    for name in ("classic_ctc_long_loss", "simplified_ctc_long_loss", "ctc_long_loss_from_logproba"):
        p = inspect.signature(getattr(ctc, name)).parameters
        assert list(p)[-1] == "frame_window" and p["frame_window"].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert p["frame_window"].default is None and "frame_window" in getattr(ctc, name).__doc__, name
    for old in ("classic_ctc_long_label_posterior", "simplified_ctc_long_label_posterior", "ctc_long_label_posterior_from_logproba"):
        new = old.replace("_long_", "_long_windowed_")
        assert new in ctc.__all__ and old in ctc.__all__, new
        po, pn = inspect.signature(getattr(ctc, old)).parameters, inspect.signature(getattr(ctc, new)).parameters
        assert "frame_window" not in po and list(pn) == list(po) + ["frame_window"], new
        assert pn["frame_window"].kind is inspect.Parameter.KEYWORD_ONLY and pn["frame_window"].default is None, new
        assert all(pn[k].kind is po[k].kind and pn[k].default == po[k].default for k in po), new
    po = inspect.signature(ops.long_wildcard_loss_grad).parameters
    pn = inspect.signature(ops.long_windowed_loss_grad).parameters
    assert list(pn) == ["frame_window"] + list(po) and all(pn[k].default == po[k].default for k in po)
    assert list(inspect.signature(ops.long_label_posterior).parameters)[-1] == "frame_window"
