"""Host layer of ctc_amd_long_wildcard_loss_grad / ctc_amd_long_wildcard_loss_workspace_bytes, in the manner of
tests/test_cabi_long_wildcard_best_path.py: nothing here touches a GPU.  Validation returns before any launch, pointers are the
never-dereferenced address 16 and no call is given a workspace large enough, so a call that passes every check stops at
CTC_AMD_EWORKSPACE."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=4, label_length=ONE, logit_length=ONE,
            blank=0, weight=0.0, B=2, T=5, V=8, U=4, tf=0, d_loss=ONE, loss=ONE, grad=ONE, gdtype=0, gsb=None, gst=None, ws=None,
            ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank", "weight",
         "B", "T", "V", "U", "tf", "d_loss", "loss", "grad", "gdtype", "gsb", "gst", "ws", "ws_bytes")
SHORT = tuple(k for k in ORDER if k != "tf")  # ctc_amd_wildcard_loss_grad


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def args(**over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    for sb, st in (("xsb", "xst"), ("gsb", "gst")):
        if a[sb] is None:
            a[sb] = max(a["T"], 1) * a["V"]
        if a[st] is None:
            a[st] = a["V"]
    a["weight"] = ctypes.c_float(a["weight"])
    return a


def call(lib, **over):
    a = args(**over)
    rc = lib.ctc_amd_long_wildcard_loss_grad(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, tf=0, want_grad=1):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_long_wildcard_loss_workspace_bytes(kind, B, T, V, U, tf, want_grad, ctypes.byref(out))
    return rc, int(out.value)


def r256(x):
    return (x + 255) // 256 * 256


def formula(kind, B, T, U, want_grad=1):
    """include/ctc_amd.h, ctc_amd_long_wildcard_loss_grad, term by term (frames_per_tile does not enter)."""
    K, S = max(1, -(-U // 1024)), 2 - kind
    n = r256(16 * B * (K - 1) * T) + r256(8 * B * K * 2056) + r256(16 * B * T) + r256(8 * B) + r256(4 * B)
    if want_grad:
        n += r256(8 * B * (K - 1) * T) + r256(8 * B * K * 2056) + r256(8 * B * K * T * (S * 1024 + 2))
    return n


def test_symbols_and_header(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_long_wildcard_loss_grad", "ctc_amd_long_wildcard_loss_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"^int " + name + r"\(", header, re.M), name  # declared, not only mentioned
    assert len(_lib.SIGNATURES["ctc_amd_long_wildcard_loss_grad"][1]) == len(ORDER) + 1 == 26  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_wildcard_loss_grad"][1]) == 25  # the same without frames_per_tile
    assert len(_lib.SIGNATURES["ctc_amd_long_wildcard_loss_workspace_bytes"][1]) == 8
    assert "#define CTC_AMD_LONG_MAX_U 65536" in header and "#define CTC_AMD_MAX_U 1024" in header
    assert lib.ctc_amd_abi_version() == 6
    # the header's worked examples are the formula's values, as printed there
    assert "3 941 783 808 bytes classic and 1 975 703 808 simplified" in header and "3 972 096 without" in header
    assert formula(0, 1, 30000, 8192) == 3941783808 and formula(1, 1, 30000, 8192) == 1975703808
    assert formula(0, 1, 30000, 8192, 0) == 3972096


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None),
    (dict(U=-1), None), (dict(label_stride=-1), None), (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=65537, label_stride=65537), "U=65537"), (dict(label_length=None), None), (dict(logit_length=None), None),
    (dict(logits=None), None), (dict(labels=None), None),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"), (dict(gdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(gst=7), "stride"), (dict(gsb=-8), "stride"),
    (dict(weight=0.5), "wildcard_log_weight"), (dict(weight=float("nan")), "wildcard_log_weight"),
    (dict(weight=float("-inf")), "wildcard_log_weight"),
    (dict(loss=None), "null loss"), (dict(V=16385), "V=16385"),
    (dict(tf=-4), "frames_per_tile"), (dict(tf=1), "frames_per_tile"), (dict(tf=6), "frames_per_tile"), (dict(tf=127), "frames_per_tile"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_messages_are_those_of_the_wildcard_loss(lib):
    """The same faulty arguments give the same code and the same text as ctc_amd_wildcard_loss_grad."""
    for over in (dict(kind=5), dict(wrt=2), dict(T=-1), dict(blank=8), dict(label_length=None), dict(logits=None), dict(xdtype=3),
                 dict(gdtype=3), dict(xst=7), dict(gst=7), dict(weight=0.5), dict(weight=float("nan")), dict(loss=None),
                 dict(V=16385)):
        rc, msg = call(lib, **over)
        a = args(**over)
        rc0 = lib.ctc_amd_wildcard_loss_grad(*(a[k] for k in SHORT), None)
        assert (rc, msg) == (rc0, lib.ctc_amd_last_error().decode()), over
    # the label limit: the same text with the long limit in it
    rc, msg = call(lib, U=65537, label_stride=65537)
    assert rc == EINVAL and msg == "U=65537 exceeds the supported maximum 65536"
    a = args(U=1025, label_stride=1025)
    assert lib.ctc_amd_wildcard_loss_grad(*(a[k] for k in SHORT), None) == EINVAL
    assert lib.ctc_amd_last_error().decode() == "U=1025 exceeds the supported maximum 1024"  # the existing call keeps its limit
    # frames_per_tile and the grid: the text of ctc_amd_long_best_path
    rc, msg = call(lib, tf=6)
    a = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=40, xst=8, labels=ONE, label_stride=4, ll=ONE, tl=ONE, blank=0, B=2, T=5, V=8, U=4, tf=6)
    rc0 = lib.ctc_amd_long_best_path(*a.values(), ONE, ONE, ONE, ONE, ONE, None, 0, None)
    assert (rc, msg) == (rc0, lib.ctc_amd_last_error().decode()) and "frames_per_tile=6" in msg


def test_precedence(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=65537)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)          # common checks before the element types
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)             # element types before B == 0
    expect(lib, EINVAL, "dtype", gdtype=3, xst=7)           # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, weight=0.5)        # strides before the weight
    expect(lib, EINVAL, "wildcard_log_weight", weight=0.5, loss=None)  # the weight before the output
    expect(lib, EINVAL, "null loss", loss=None, V=16385)    # the output before the vocabulary limit
    expect(lib, EINVAL, "V=16385", V=16385, tf=3)           # the vocabulary limit before frames_per_tile
    expect(lib, EINVAL, "frames_per_tile", tf=3, ws=ONE, ws_bytes=1)  # frames_per_tile before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)                # a common fault hides B == 0
    expect(lib, EWORKSPACE, gst=7, grad=None)               # the gradient's strides only with a gradient
    # the row stage's grid (with a gradient only) before frames_per_tile; both before the workspace
    expect(lib, EINVAL, "rows exceed the launch grid", B=2 ** 20, T=2 ** 14, tf=3)
    expect(lib, EINVAL, "frames_per_tile", B=2 ** 20, T=2 ** 14, tf=3, grad=None)
    expect(lib, EWORKSPACE, B=2 ** 20, T=2 ** 14, grad=None)
    expect(lib, EINVAL, "too large", B=2 ** 30, T=1024, U=65536, label_stride=65536, tf=4, grad=None)  # the tile grid


def test_label_limit(lib):
    expect(lib, EWORKSPACE, U=1025, label_stride=1025)      # beyond CTC_AMD_MAX_U: what this call is for
    expect(lib, EWORKSPACE, U=65536, label_stride=65536)
    expect(lib, EINVAL, "U=65537", U=65537, label_stride=65537)
    assert size(lib, 0, 1, 50, 32, 1025)[0] == OK and size(lib, 0, 1, 50, 32, 65536)[0] == OK
    assert size(lib, 0, 1, 50, 32, 65537)[0] == EINVAL
    out = ctypes.c_size_t(0)  # the one-wavefront call keeps its limit
    assert lib.ctc_amd_wildcard_loss_workspace_bytes(0, 1, 50, 32, 1025, 1, ctypes.byref(out)) == EINVAL


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, d_loss=None, loss=None, grad=None)
    expect(lib, OK, B=0, xst=7)        # no rows to overlap
    expect(lib, OK, B=0, tf=3)         # ... no tiles
    expect(lib, OK, B=0, weight=0.5)   # ... and nothing to weigh


def test_a_valid_call_stops_at_the_workspace(lib):
    expect(lib, EWORKSPACE)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=1)
    expect(lib, EWORKSPACE, kind=1, wrt=1)
    expect(lib, EWORKSPACE, grad=None)                 # forward only needs a workspace too
    expect(lib, EWORKSPACE, grad=None, ws=ONE, ws_bytes=1)
    expect(lib, EWORKSPACE, d_loss=None)
    expect(lib, EWORKSPACE, T=0)
    expect(lib, EWORKSPACE, V=16384)
    expect(lib, EWORKSPACE, weight=-0.5)
    expect(lib, EWORKSPACE, weight=-3.0e38)
    for tf in (0, 4, 8, 128, 132, 4096):
        expect(lib, EWORKSPACE, tf=tf)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, xdtype=dt, gdtype=dt)
    expect(lib, EWORKSPACE, xsb=8, xst=16, gsb=8, gst=16)  # time-major
    # one byte short is too small (only the failing side is called with a non-null workspace: nothing may be launched here)
    for want_grad in (1, 0):
        rc, need = size(lib, 0, 2, 5, 8, 4, 0, want_grad)
        assert rc == OK and need > 0
        expect(lib, EWORKSPACE, f"{need - 1} < {need}", ws=ONE, ws_bytes=need - 1, grad=ONE if want_grad else None)
    # a forward-only call is content with the forward-only size: the gradient's size is larger
    assert size(lib, 0, 2, 5, 8, 4, 0, 0)[1] < size(lib, 0, 2, 5, 8, 4, 0, 1)[1]
    expect(lib, EWORKSPACE, f"{size(lib, 0, 2, 5, 8, 4, 0, 0)[1]} < {size(lib, 0, 2, 5, 8, 4, 0, 1)[1]}", ws=ONE,
           ws_bytes=size(lib, 0, 2, 5, 8, 4, 0, 0)[1])


@pytest.mark.parametrize("kind", [0, 1])
def test_size_function(lib, kind):
    assert size(lib, 0, 1, 30000, 32, 8192) == (OK, 3941783808) and size(lib, 1, 1, 30000, 32, 8192) == (OK, 1975703808)
    for B in (0, 1, 3):
        for T in (0, 1, 31, 127, 128, 129, 2700):
            for U in (0, 1, 1024, 1025, 2048, 2049, 65536):
                for tf in (0, 4, 64, 128, 1000):
                    for want_grad in (0, 1, 7):
                        assert size(lib, kind, B, T, 32, U, tf, want_grad) == (OK, formula(kind, B, T, U, want_grad)), (B, T, U, tf, want_grad)
    # forward only keeps no per-frame rows: nothing grows with K * T * 1024
    fwd = size(lib, kind, 1, 30000, 32, 8192, 0, 0)[1]
    assert fwd == formula(kind, 1, 30000, 8192, 0) == 3972096 and fwd < 8 * 30000 * 1024
    # beyond 2^32 bytes: no 32-bit arithmetic on the way
    assert size(lib, kind, 1, 180000, 32, 50000) == (OK, formula(kind, 1, 180000, 50000)) and formula(kind, 1, 180000, 50000) > 2 ** 36
    assert size(lib, kind, 8, 30000, 32, 8192) == (OK, formula(kind, 8, 30000, 8192)) and formula(kind, 8, 30000, 8192) > 2 ** 32
    assert size(lib, kind, 8, 180000, 32, 65536, 4) == (OK, formula(kind, 8, 180000, 65536))
    assert size(lib, kind, 1, 180000, 32, 50000, 0, 0) == (OK, formula(kind, 1, 180000, 50000, 0))
    assert formula(kind, 1, 180000, 50000, 0) < 2 ** 28  # an hour of audio, forward only: 142 MB


def test_size_function_limits(lib):
    for bad in ((2, 4, 50, 256, 64, 0), (0, -1, 50, 256, 64, 0), (0, 4, -1, 256, 64, 0), (0, 4, 50, 0, 64, 0), (0, 4, 50, 256, -1, 0),
                (0, 4, 50, 16385, 64, 0), (0, 4, 50, 256, 64, 3), (0, 4, 50, 256, 64, -4)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_long_wildcard_loss_workspace_bytes(0, 4, 50, 256, 64, 0, 1, None) == EINVAL
    assert size(lib, 0, 2 ** 30, 1024, 32, 65536, 4, 0)[0] == EINVAL  # a tile launch of more than 2^31 - 1 workgroups
    assert size(lib, 0, 2 ** 20, 2 ** 14, 32, 4, 0, 1)[0] == EINVAL and size(lib, 0, 2 ** 20, 2 ** 13, 32, 4, 0, 0)[0] == OK  # the row stage


def test_python_layer_is_declared():
    import inspect

    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops
    for name in ("classic_ctc_long_loss", "simplified_ctc_long_loss", "ctc_long_loss_from_logproba"):
        assert name in ctc.__all__ and hasattr(ctc, name), name
        p = inspect.signature(getattr(ctc, name)).parameters
        for kw in ("wildcard_log_weight", "frames_per_tile", "max_label_length"):
            assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY, (name, kw)
        assert p["blank_index"].default == 0 and p["wildcard_log_weight"].default == 0.0 and p["frames_per_tile"].default is None
    assert list(inspect.signature(ctc.ctc_long_loss_from_logproba).parameters)[4:6] == ["blank_index", "ctc_loss_data_cls"]
    assert callable(ops.long_wildcard_loss_grad) and callable(_lib.long_wildcard_loss_workspace_bytes)


def test_plan_check_program(tmp_path):
    """tests/tools/long_loss_plan_check.cpp: the plan's offsets, its size_t arithmetic and the read-after-write order of every
    launch as a stand-alone host program.  (Built plainly here; the same source builds with -fsanitize=address,undefined.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "long_loss_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "long_loss_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and "ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
