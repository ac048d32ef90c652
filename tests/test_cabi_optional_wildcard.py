"""Host layer of the three optional-wildcard entry points (include/ctc_amd.h, "Optional wildcards"), in the manner of
tests/test_cabi_wildcard_loss.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the
never-dereferenced address 16; only rejected calls and B == 0 are made.  Each entry point is its counterpart in arguments,
validation order and messages, so every rejected call is made to both and must answer alike."""
import ctypes
import os
import re

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
PAIRS = {  # new entry: counterpart
    "ctc_amd_optional_wildcard_loss_grad": "ctc_amd_wildcard_loss_grad",
    "ctc_amd_optional_wildcard_label_posterior": "ctc_amd_label_posterior",
    "ctc_amd_optional_wildcard_best_path": "ctc_amd_wildcard_best_path",
    "ctc_amd_optional_wildcard_best_path_workspace_bytes": "ctc_amd_wildcard_best_path_workspace_bytes",
    "ctc_amd_optional_wildcard_loss_workspace_bytes": "ctc_amd_wildcard_loss_workspace_bytes",
    "ctc_amd_optional_wildcard_label_posterior_workspace_bytes": "ctc_amd_label_posterior_workspace_bytes",
}
CALLS = ("ctc_amd_optional_wildcard_loss_grad", "ctc_amd_optional_wildcard_label_posterior", "ctc_amd_optional_wildcard_best_path")
B, T, V, U = 2, 5, 8, 4


def args(name, kind=0, wrt=0, dtype=0, sb=T * V, st=V, blank=0, weight=0.0, b=B, t=T, v=V, u=U, loss=ONE, ws=ONE, ws_bytes=BIG, gst=V):
    if name.endswith("best_path"):  # no weight; score (here: `loss`), tokens, four optional outputs
        return (kind, wrt, ONE, dtype, sb, st, ONE, 5, ONE, ONE, blank, b, t, v, u, loss, ONE, ONE, ONE, ONE, ONE, ws, ws_bytes, None)
    lead = (kind, wrt, ONE, dtype, sb, st, ONE, 5, ONE, ONE, blank, ctypes.c_float(weight), b, t, v, u)
    if name.endswith("loss_grad"):
        return lead + (None, loss, ONE, 0, T * V, gst, ws, ws_bytes, None)
    return lead + (loss, ONE, ONE, ONE, ONE, ws, ws_bytes, None)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def both(lib, name, **kw):
    """(rc, message) of the new entry point, after checking that its counterpart answers the same."""
    out = []
    for n in (name, PAIRS[name]):
        rc = getattr(lib, n)(*args(name, **kw))
        out.append((rc, lib.ctc_amd_last_error().decode()))
    assert out[0] == out[1], (name, out)
    return out[0]


def test_symbols_signatures_and_constant(lib):
    from tf_seq2seq_losses_amd import _lib
    import tf_seq2seq_losses_amd as ctc
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    declared = set(re.findall(r"ctc_amd_[a-z_]+", header))
    for new, old in PAIRS.items():
        assert hasattr(lib, new) and new in declared, new
        assert _lib.SIGNATURES[new][0] is _lib.SIGNATURES[old][0] and _lib.SIGNATURES[new][1] == _lib.SIGNATURES[old][1], new
    assert re.search(r"#define CTC_AMD_OPTIONAL_WILDCARD \(-3\)", header)
    assert _lib.OPTIONAL_WILDCARD == ctc.OPTIONAL_WILDCARD == -3 and ctc.WILDCARD == -2 and "OPTIONAL_WILDCARD" in ctc.__all__
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("name", CALLS)
def test_validation_is_the_counterparts(lib, name):
    for kw, word in ((dict(kind=5), "kind"), (dict(wrt=3), "wrt"), (dict(blank=V), "blank"), (dict(u=1025), "U=1025"),
                     (dict(dtype=7), ""), (dict(st=V - 1), "stride"), (dict(weight=0.5), "wildcard_log_weight"),
                     (dict(weight=float("nan")), "wildcard_log_weight"), (dict(loss=None), "null")):
        if "weight" in kw and name.endswith("best_path"):
            continue  # (the alignment has no weight)
        rc, msg = both(lib, name, **kw)
        assert rc == EINVAL and word in msg, (kw, msg)
    rc, msg = both(lib, name, ws_bytes=16)
    assert rc == EWORKSPACE, msg
    rc, msg = both(lib, name, ws=None)
    assert rc == EWORKSPACE, msg
    assert both(lib, name, b=0)[0] == OK  # an empty batch: no launch


def test_gradient_stride_is_checked_only_with_a_gradient(lib):
    rc, msg = both(lib, "ctc_amd_optional_wildcard_loss_grad", gst=V - 1)
    assert rc == EINVAL and "stride" in msg


def test_workspace_queries_are_the_counterparts(lib):
    for kind in (0, 1):
        for u in (3, 64, 65, 1024):
            a, b = ctypes.c_size_t(), ctypes.c_size_t()
            for g in (0, 1):
                assert lib.ctc_amd_optional_wildcard_loss_workspace_bytes(kind, B, T, V, u, g, ctypes.byref(a)) == OK
                assert lib.ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, u, g, ctypes.byref(b)) == OK
                assert a.value == b.value and (a.value > 0) == bool(g)
            assert lib.ctc_amd_optional_wildcard_label_posterior_workspace_bytes(kind, B, T, V, u, ctypes.byref(a)) == OK
            assert a.value == b.value
    assert lib.ctc_amd_optional_wildcard_loss_workspace_bytes(0, B, T, V, 1025, 1, ctypes.byref(a)) == EINVAL
    assert lib.ctc_amd_optional_wildcard_label_posterior_workspace_bytes(0, B, T, V, U, None) == EINVAL


def test_python_layer_refuses_a_window_with_optional_wildcards():
    """Raised before anything is looked at: no device needed."""
    import torch
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops
    lab, x, ll, tl = torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 3, 4)), torch.ones(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    win = torch.zeros((1, 2, 2), dtype=torch.int32)
    for fn in (ctc.classic_ctc_wildcard_loss, ctc.simplified_ctc_wildcard_loss, ctc.classic_ctc_label_posterior,
               ctc.simplified_ctc_label_posterior):
        with pytest.raises(ValueError, match="optional_wildcards"):
            fn(lab, x, ll, tl, 0, frame_window=win, optional_wildcards=True)
    for fn in (ctc.ctc_wildcard_loss_from_logproba, ctc.ctc_label_posterior_from_logproba):
        with pytest.raises(ValueError, match="optional_wildcards"):
            fn(lab, x, ll, tl, 0, None, frame_window=win, optional_wildcards=True)
    for fn in (ctc.classic_ctc_wildcard_alignment, ctc.simplified_ctc_wildcard_alignment):
        with pytest.raises(ValueError, match="optional_wildcards"):
            fn(lab, x, ll, tl, 0, frame_window=win, optional_wildcards=True)
    with pytest.raises(ValueError, match="optional_wildcards"):
        ctc.ctc_wildcard_alignment_from_logproba(lab, x, ll, tl, 0, None, frame_window=win, optional_wildcards=True)
    for fn in (ops.wildcard_loss_grad, ops.label_posterior):
        with pytest.raises(ValueError, match="optional_wildcards"):
            fn(0, 0, lab, x, ll, tl, 0, frame_window=win, optional_wildcards=True)


def test_classic_alignment_limit(lib):
    """The one check of its own: the classic optional-wildcard alignment takes U <= 512, behind the counterpart's checks and before
    the workspace; the size query says so too.  The simplified lattice and the counterpart take 1024."""
    from tf_seq2seq_losses_amd import _lib
    name = "ctc_amd_optional_wildcard_best_path"
    n = ctypes.c_size_t()
    for kind, u, want in ((0, 512, OK), (0, 513, EINVAL), (1, 1024, OK)):
        assert lib.ctc_amd_optional_wildcard_best_path_workspace_bytes(kind, B, T, V, u, ctypes.byref(n)) == want
        rc = getattr(lib, name)(*args(name, kind=kind, u=u, ws_bytes=16))
        assert rc == (EWORKSPACE if want == OK else EINVAL), lib.ctc_amd_last_error()
    rc = getattr(lib, name)(*args(name, kind=0, u=513))
    assert rc == EINVAL and b"512" in lib.ctc_amd_last_error()
    rc = getattr(lib, name)(*args(name, kind=0, u=513, loss=None))
    assert rc == EINVAL and b"512" not in lib.ctc_amd_last_error()  # the counterpart's checks come first
    assert _lib.OPTIONAL_CLASSIC_MAX_U == 512
