"""Host layer of ctc_amd_long_wildcard_best_path / ctc_amd_long_wildcard_best_path_workspace_bytes, in the manner of
tests/test_cabi_long_best_path.py: nothing here touches a GPU.  Validation returns before any launch, pointers are the
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
            blank=0, B=2, T=5, V=8, U=4, tf=0, score=ONE, tokens=ONE, label_index=ONE, first_frame=ONE, last_frame=ONE,
            label_score=ONE, ws=None, ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
         "B", "T", "V", "U", "tf", "score", "tokens", "label_index", "first_frame", "last_frame", "label_score", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    rc = lib.ctc_amd_long_wildcard_best_path(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, kind, B, T, V, U, tf=0):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_long_wildcard_best_path_workspace_bytes(kind, B, T, V, U, tf, ctypes.byref(out))
    return rc, int(out.value)


def plain_size(lib, kind, B, T, V, U, tf=0):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_long_best_path_workspace_bytes(kind, B, T, V, U, tf, ctypes.byref(out))
    return rc, int(out.value)


def r256(x):
    return (x + 255) // 256 * 256


def formula(B, T, U, tf=0):
    """include/ctc_amd.h, ctc_amd_long_wildcard_best_path, term by term: back-pointers, columns, rows, LSE partials, label_index,
    feasibility; then m_t, a_t and the per-frame log-sum-exp / log-probability."""
    TF = tf or 128
    K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
    return (r256(B * K * T * 512) + r256(B * (K - 1) * T * 16) + r256(B * K * 16448) + r256(B * J * 8) + r256(B * T * 4) + r256(B * 4)
            + r256(B * T * 8) + r256(B * T * 4) + r256(B * T * 8))


def test_symbols_and_header(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_long_wildcard_best_path", "ctc_amd_long_wildcard_best_path_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"^int " + name + r"\(", header, re.M), name  # declared, not only mentioned
    assert len(_lib.SIGNATURES["ctc_amd_long_wildcard_best_path"][1]) == len(ORDER) + 1 == 25  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_long_wildcard_best_path_workspace_bytes"][1]) == 7
    assert "#define CTC_AMD_LONG_MAX_U 65536" in header and "#define CTC_AMD_WILDCARD (-2)" in header
    assert lib.ctc_amd_abi_version() == 6
    # the header's worked example is the formula's value, as printed there
    assert "= 127 094 272 bytes" in header and formula(1, 30000, 8192) == 127094272
    terms = [122880000, 3360000, 131584, 2048, 120064, 256, 240128, 120064, 240128]
    assert " + ".join(f"{t:,}".replace(",", " ") for t in terms) in header and sum(terms) == 127094272


@pytest.mark.parametrize("over,text", [
    (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(wrt=2), "wrt"), (dict(B=-1), None), (dict(T=-1), None), (dict(V=0), None),
    (dict(U=-1), None), (dict(label_stride=-1), None), (dict(blank=8), "blank"), (dict(blank=-1), "blank"),
    (dict(U=65537, label_stride=65537), "U=65537"), (dict(label_length=None), None), (dict(logit_length=None), None),
    (dict(logits=None), None), (dict(labels=None), None),
    (dict(xdtype=-1), "dtype"), (dict(xdtype=3), "dtype"),
    (dict(xsb=7), "stride"), (dict(xst=7), "stride"), (dict(xst=0), "stride"), (dict(xsb=-8), "stride"),
    (dict(score=None), "null"), (dict(tokens=None), "null"), (dict(V=16385), "V=16385"),
    (dict(tf=-4), "frames_per_tile"), (dict(tf=1), "frames_per_tile"), (dict(tf=6), "frames_per_tile"), (dict(tf=127), "frames_per_tile"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_messages_are_those_of_the_long_call(lib):
    """The same faulty arguments give the same code and the same text in both calls."""
    for over in (dict(kind=5), dict(blank=8), dict(U=65537, label_stride=65537), dict(xdtype=3), dict(xst=7), dict(score=None),
                 dict(V=16385), dict(tf=6)):
        rc, msg = call(lib, **over)
        a = dict(BASE, **over)
        a["xsb"] = max(a["T"], 1) * a["V"] if a["xsb"] is None else a["xsb"]
        a["xst"] = a["V"] if a["xst"] is None else a["xst"]
        rc0 = lib.ctc_amd_long_best_path(*(a[k] for k in ORDER if k != "label_score"), None)
        assert (rc, msg) == (rc0, lib.ctc_amd_last_error().decode()), over


def test_precedence_follows_the_long_call(lib):
    expect(lib, EINVAL, "kind", kind=5, wrt=2)
    expect(lib, EINVAL, "blank", blank=99, U=65537)
    expect(lib, EINVAL, "kind", kind=5, xdtype=3)        # common checks before the element type
    expect(lib, EINVAL, "dtype", xdtype=3, B=0)           # element type before B == 0
    expect(lib, EINVAL, "dtype", xdtype=3, xst=7)         # ... and before the strides
    expect(lib, EINVAL, "stride", xst=7, score=None)      # strides before the outputs
    expect(lib, EINVAL, "null", score=None, V=16385)      # outputs before the vocabulary limit
    expect(lib, EINVAL, "V=16385", V=16385, tf=3)         # the vocabulary limit before frames_per_tile
    expect(lib, EINVAL, "frames_per_tile", tf=3, ws=ONE, ws_bytes=1)  # frames_per_tile before the workspace
    expect(lib, EINVAL, "kind", kind=5, B=0)              # a common fault hides B == 0


def test_label_limit(lib):
    expect(lib, EWORKSPACE, U=1025, label_stride=1025)    # beyond CTC_AMD_MAX_U: what this call is for
    expect(lib, EWORKSPACE, U=65536, label_stride=65536)
    expect(lib, EINVAL, "U=65537", U=65537, label_stride=65537)
    assert size(lib, 0, 1, 50, 32, 1025)[0] == OK and size(lib, 0, 1, 50, 32, 65536)[0] == OK
    assert size(lib, 0, 1, 50, 32, 65537)[0] == EINVAL
    # the whole-utterance wildcard call keeps its limit
    out = ctypes.c_size_t(0)
    assert lib.ctc_amd_wildcard_best_path_workspace_bytes(0, 1, 50, 32, 1025, ctypes.byref(out)) == EINVAL


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, score=None, tokens=None, label_index=None,
           first_frame=None, last_frame=None, label_score=None)
    expect(lib, OK, B=0, xst=7)  # no rows to overlap
    expect(lib, OK, B=0, tf=3)   # ... and no tiles


def test_a_valid_call_stops_at_the_workspace(lib):
    expect(lib, EWORKSPACE)
    expect(lib, EWORKSPACE, ws=ONE, ws_bytes=1)
    expect(lib, EWORKSPACE, kind=1, wrt=1)
    for li in (ONE, None):  # every per-label output is optional, label_score among them
        for ff in (ONE, None):
            for lf in (ONE, None):
                for ls in (ONE, None):
                    expect(lib, EWORKSPACE, label_index=li, first_frame=ff, last_frame=lf, label_score=ls)
    expect(lib, EWORKSPACE, T=0, tokens=None, label_index=None)
    expect(lib, EWORKSPACE, V=16384)
    for tf in (0, 4, 8, 128, 132, 4096):
        expect(lib, EWORKSPACE, tf=tf)
    for dt in (0, 1, 2):
        expect(lib, EWORKSPACE, xdtype=dt)
    expect(lib, EWORKSPACE, xsb=8, xst=16)  # time-major
    # one byte short is too small (only the failing side is called with a non-null workspace: nothing may be launched here)
    rc, need = size(lib, 0, 2, 5, 8, 4)
    assert rc == OK and need > 0
    expect(lib, EWORKSPACE, f"{need - 1} < {need}", ws=ONE, ws_bytes=need - 1)


@pytest.mark.parametrize("kind", [0, 1])
def test_size_function(lib, kind):
    # the header's worked example
    assert size(lib, kind, 1, 30000, 32, 8192, 0) == (OK, 127094272) and formula(1, 30000, 8192) == 127094272
    for B in (0, 1, 3):
        for T in (0, 1, 31, 32, 33, 127, 128, 129, 2700):
            for U in (0, 1, 1024, 1025, 2048, 2049, 65536):
                for tf in (0, 4, 64, 128, 256, 1000):
                    assert size(lib, kind, B, T, 32, U, tf) == (OK, formula(B, T, U, tf)), (B, T, U, tf)
                    # the plain call's regions, then three per-frame ones
                    assert size(lib, kind, B, T, 32, U, tf)[1] == (plain_size(lib, kind, B, T, 32, U, tf)[1]
                                                                   + 2 * r256(B * T * 8) + r256(B * T * 4))
    # beyond 2^31 and 2^32 bytes: an hour of audio (no 32-bit arithmetic on the way)
    assert size(lib, kind, 1, 180000, 32, 50000, 0) == (OK, formula(1, 180000, 50000))
    assert formula(1, 180000, 50000) > 2 ** 32 and 2 ** 31 < formula(3, 30000, 65536) < 2 ** 32
    assert size(lib, kind, 3, 30000, 32, 65536, 0) == (OK, formula(3, 30000, 65536))
    assert size(lib, kind, 8, 180000, 32, 65536, 4) == (OK, formula(8, 180000, 65536, 4))


def test_size_function_limits(lib):
    for bad in ((2, 4, 50, 256, 64, 0), (0, -1, 50, 256, 64, 0), (0, 4, -1, 256, 64, 0), (0, 4, 50, 0, 64, 0), (0, 4, 50, 256, -1, 0),
                (0, 4, 50, 16385, 64, 0), (0, 4, 50, 256, 64, 3), (0, 4, 50, 256, 64, -4)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert lib.ctc_amd_long_wildcard_best_path_workspace_bytes(0, 4, 50, 256, 64, 0, None) == EINVAL
    # a batch whose widest launch would pass 2^31 - 1 workgroups
    assert size(lib, 0, 2 ** 30, 1024, 32, 65536, 4)[0] == EINVAL


def test_python_layer_is_declared():
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import ops
    for name in ("classic_ctc_long_wildcard_alignment", "simplified_ctc_long_wildcard_alignment",
                 "ctc_long_wildcard_alignment_from_logproba", "CtcLongWildcardAlignment", "WILDCARD"):
        assert name in ctc.__all__ and hasattr(ctc, name), name
    assert ctc.CtcLongWildcardAlignment._fields == ("score", "tokens", "label_index", "first_frame", "last_frame", "label_score")
    assert callable(ops.long_wildcard_best_path) and ctc.WILDCARD == -2


def test_plan_check_program(tmp_path):
    """tests/tools/long_wild_plan_check.cpp: the plan's offsets and size_t arithmetic as a stand-alone host program.  (Built
    plainly here; the same source builds with -fsanitize=address,undefined.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "long_wild_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "long_wild_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and "ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
