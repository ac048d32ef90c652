"""Host layer of the three star entry points (include/ctc_amd.h, "Star temporal classification"), in the manner of
tests/test_cabi_optional_wildcard.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the
never-dereferenced address 16; only rejected calls and B == 0 are made.  Each entry point is its counterpart plus
`int optional_wildcards` behind blank_index, so every rejected call is made to both and must answer alike."""
import ctypes
import os
import re

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
PAIRS = {  # new entry: (counterpart with optional_wildcards = 0, with 1)
    "ctc_amd_star_loss_grad": ("ctc_amd_wildcard_loss_grad", "ctc_amd_optional_wildcard_loss_grad"),
    "ctc_amd_star_label_posterior": ("ctc_amd_label_posterior", "ctc_amd_optional_wildcard_label_posterior"),
    "ctc_amd_star_best_path": ("ctc_amd_wildcard_best_path", "ctc_amd_optional_wildcard_best_path"),
}
B, T, V, U = 2, 5, 8, 4


def args(name, opt=None, kind=0, wrt=0, dtype=0, sb=T * V, st=V, blank=0, weight=0.0, b=B, t=T, v=V, u=U, loss=ONE, ws=ONE, ws_bytes=BIG):
    """opt: None for a counterpart, 0 / 1 for the star entry point."""
    lead = (kind, wrt, ONE, dtype, sb, st, ONE, 5, ONE, ONE, blank) + (() if opt is None else (opt,))
    if name.endswith("best_path"):
        return lead + (b, t, v, u, loss, ONE, ONE, ONE, ONE, ONE, ws, ws_bytes, None)
    lead += (ctypes.c_float(weight), b, t, v, u)
    if name.endswith("loss_grad"):
        return lead + (None, loss, ONE, 0, T * V, V, ws, ws_bytes, None)
    return lead + (loss, ONE, ONE, ONE, ONE, ws, ws_bytes, None)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def test_symbols_and_signatures(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctc_amd.h")).read()
    declared = set(re.findall(r"ctc_amd_[a-z_]+", header))
    for new, (old, _) in PAIRS.items():
        assert hasattr(lib, new) and new in declared and new.replace("_grad", "") + "_workspace_bytes" in declared, new
        want = list(_lib.SIGNATURES[old][1])
        want.insert(11, ctypes.c_int)
        assert _lib.SIGNATURES[new][1] == want, new
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


@pytest.mark.parametrize("opt", (0, 1))
@pytest.mark.parametrize("name", PAIRS)
def test_validation_is_the_counterparts(lib, name, opt):
    def both(**kw):
        out = []
        for n, o in ((name, opt), (PAIRS[name][opt], None)):
            rc = getattr(lib, n)(*args(name, o, **kw))
            out.append((rc, lib.ctc_amd_last_error().decode()))
        assert out[0] == out[1], (name, kw, out)
        return out[0]

    for kw, word in ((dict(kind=5), "kind"), (dict(wrt=3), "wrt"), (dict(blank=V), "blank"), (dict(u=1025), "U=1025"),
                     (dict(dtype=7), ""), (dict(st=V - 1), "stride"), (dict(weight=0.5), "wildcard_log_weight"), (dict(loss=None), "null")):
        if "weight" in kw and name.endswith("best_path"):
            continue  # (the alignment has no weight)
        rc, msg = both(**kw)
        assert rc == EINVAL and word in msg, (kw, msg)
    assert both(ws_bytes=16)[0] == EWORKSPACE
    assert both(ws=None)[0] == EWORKSPACE
    assert both(b=0)[0] == OK  # an empty batch: no launch


def test_workspace_queries(lib):
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    r256 = lambda n: (n + 255) & ~255
    for kind in (0, 1):
        for u in (3, 65, 1024):
            for g in (0, 1):
                assert lib.ctc_amd_star_loss_workspace_bytes(kind, B, T, V, u, g, ctypes.byref(a)) == OK
                assert lib.ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, u, g, ctypes.byref(b)) == OK
                assert a.value == b.value
            assert lib.ctc_amd_star_label_posterior_workspace_bytes(kind, B, T, V, u, ctypes.byref(a)) == OK
            assert a.value == b.value
            # the alignment keeps two tokens per frame: the counterpart's last region doubles
            assert lib.ctc_amd_star_best_path_workspace_bytes(kind, 0, B, T, V, u, ctypes.byref(a)) == OK
            assert lib.ctc_amd_wildcard_best_path_workspace_bytes(kind, B, T, V, u, ctypes.byref(b)) == OK
            assert a.value == b.value - r256(4 * B * T) + r256(8 * B * T)
    assert lib.ctc_amd_star_loss_workspace_bytes(0, B, T, V, 1025, 1, ctypes.byref(a)) == EINVAL
    assert lib.ctc_amd_star_best_path_workspace_bytes(0, 0, B, T, V, U, None) == EINVAL
    # the classic limit of the optional alignment stays: 512 with optional wildcards, 1024 without
    for opt, u, want in ((1, 512, OK), (1, 513, EINVAL), (0, 1024, OK)):
        assert lib.ctc_amd_star_best_path_workspace_bytes(0, opt, B, T, V, u, ctypes.byref(a)) == want
        rc = lib.ctc_amd_star_best_path(*args("ctc_amd_star_best_path", opt, u=u, ws_bytes=16))
        assert rc == (EWORKSPACE if want == OK else EINVAL), lib.ctc_amd_last_error()

