"""Host layer of ctc_amd_edit_counts / ctc_amd_edit_counts_workspace_bytes, in the manner of tests/test_cabi_edit_distance.py:
nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced address 16; a call that
passes every check would launch, so only rejected calls and B == 0 are made here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(hyp=ONE, hyp_stride=5, hyp_length=ONE, ref=ONE, ref_stride=4, ref_length=ONE, B=2, N=3, R=4, rows_per_tile=0, counts=ONE,
            ws=ONE, ws_bytes=1 << 40)
ORDER = ("hyp", "hyp_stride", "hyp_length", "ref", "ref_stride", "ref_length", "B", "N", "R", "rows_per_tile", "counts", "ws", "ws_bytes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    rc = lib.ctc_amd_edit_counts(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, want_rc, text=None, **over):
    rc, msg = call(lib, **over)
    assert rc == want_rc, f"{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{over}: message {msg!r} lacks {text!r}"


def size(lib, B, N, R, hyp_stride, rows_per_tile=0):
    out = ctypes.c_size_t(12345)
    rc = lib.ctc_amd_edit_counts_workspace_bytes(B, N, R, hyp_stride, rows_per_tile, ctypes.byref(out))
    return rc, int(out.value)


def r256(x):
    return (x + 255) // 256 * 256


def formula(B, N, R, hyp_stride):
    """include/ctc_amd.h: the last column of every column block but the last, and one row per column block, in 8-byte words."""
    K = max(1, -(-R // 1024))
    return r256(8 * B * N * (K - 1) * hyp_stride) + r256(8 * B * N * K * 1024)


def test_both_symbols_are_exported_and_declared(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_edit_counts", "ctc_amd_edit_counts_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint " + name + r"\(", header), name
    assert len(_lib.SIGNATURES["ctc_amd_edit_counts"][1]) == len(ORDER) + 1  # + the stream
    assert re.search(r"#define CTC_AMD_EDIT_COUNTS_MAX_STRIDE 1048576\b", header)
    assert "ctc_edit_long.hip" in [u[0] for u in __import__("__graft_entry__").HIP_UNITS]


def test_abi_version_is_still_6(lib):
    from tf_seq2seq_losses_amd import _lib
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION


SHAPES = [(0, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 1), (2, 3, 4, 5), (256, 8, 128, 128), (1, 1, 1024, 70), (1, 1, 1025, 70), (1, 1, 1025, 71),
          (3, 7, 3000, 3001), (1, 1, 65536, 65536), (8, 1, 65536, 65536), (1, 1, 3, 2 ** 20), (1, 9, 65535, 70),
          (5, 2, 65536, 2 ** 20),      # 5 284 823 040 + 5 242 880 bytes: beyond 2^32
          (2 ** 10, 2 ** 10, 65536, 2 ** 20)]


def test_size_function_is_the_documented_formula(lib):
    for s in SHAPES:
        for rows in (0, 64, 512, 4096):
            assert size(lib, *s, rows) == (OK, formula(*s)), (s, rows)  # (the tile height changes the launches, not the bytes)
    assert formula(5, 2, 65536, 2 ** 20) == 5284823040 + 5242880 > 2 ** 32
    assert formula(1, 1, 65536, 65536) == 33554432  # the figure in the header
    assert lib.ctc_amd_edit_counts_workspace_bytes(2, 3, 4, 5, 0, None) == EINVAL
    from tf_seq2seq_losses_amd import _lib
    assert _lib.edit_counts_workspace_bytes(2, 3, 4, 5) == formula(2, 3, 4, 5)
    with pytest.raises(ValueError):
        _lib.edit_counts_workspace_bytes(2, 3, 65537, 5)


def test_size_function_is_monotone(lib):
    base = (3, 5, 2000, 900)
    for axis, steps in enumerate(((3, 4, 64), (5, 6, 100), (2000, 2048, 2049, 4096, 65536), (900, 901, 1024, 2 ** 20))):
        got = [size(lib, *(base[:axis] + (v,) + base[axis + 1:])) for v in steps]
        assert all(rc == OK for rc, _ in got)
        assert [n for _, n in got] == sorted(n for _, n in got), (axis, got)


def test_size_function_limits(lib):
    for bad in ((-1, 3, 4, 5, 0), (2, 0, 4, 5, 0), (2, 3, -1, 5, 0), (2, 3, 65537, 5, 0), (2, 3, 4, -1, 0), (2, 3, 4, 2 ** 20 + 1, 0),
                (2, 3, 4, 5, 63), (2, 3, 4, 5, -64), (2 ** 16, 2 ** 15, 4, 5, 0)):
        assert size(lib, *bad)[0] == EINVAL, bad
    assert size(lib, 2 ** 16, 2 ** 15 - 1, 4, 5)[0] == OK
    # a full diagonal of K = J = 64 tiles for 2^28 pairs is 2^32 workgroups of four tiles
    rc, _ = size(lib, 2 ** 14, 2 ** 14, 65536, 65536, 1024)
    assert rc == EINVAL and "launch grid" in lib.ctc_amd_last_error().decode()


@pytest.mark.parametrize("over,text", [
    (dict(B=-1), "negative size"), (dict(R=-1), "negative size"),
    (dict(R=65537), "R=65537"),
    (dict(N=0), "N 0"), (dict(N=-1), "N -1"),
    (dict(B=2 ** 30, N=2), "B * N"), (dict(B=2 ** 16, N=2 ** 15), "B * N"),
    (dict(hyp_stride=-1), "negative stride"), (dict(ref_stride=-1), "negative stride"),
    (dict(hyp_stride=2 ** 20 + 1), "hyp_stride=1048577"),
    (dict(rows_per_tile=63), "rows_per_tile=63"), (dict(rows_per_tile=-64), "rows_per_tile=-64"),
    (dict(hyp_length=None), "null length"), (dict(ref_length=None), "null length"),
    (dict(hyp=None), "null hyp"), (dict(ref=None), "null ref"),
    (dict(counts=None), "null counts"),
])
def test_each_bad_argument_is_einval(lib, over, text):
    expect(lib, EINVAL, text, **over)


def test_workspace_null_or_one_byte_short(lib):
    need = formula(BASE["B"], BASE["N"], BASE["R"], BASE["hyp_stride"])
    expect(lib, EWORKSPACE, "workspace too small", ws_bytes=need - 1)
    expect(lib, EWORKSPACE, "workspace too small", ws=None)
    big = dict(B=4, N=3, R=65536, hyp_stride=2 ** 20)
    need = formula(**big)
    assert need % 2 ** 32 < 2 ** 32 < need  # a byte count cut to 32 bits would find 2^32 bytes enough
    expect(lib, EWORKSPACE, "workspace too small", ws_bytes=2 ** 32, **big)


def test_precedence(lib):
    expect(lib, EINVAL, "negative size", B=-1, R=70000)          # the sizes, then R
    expect(lib, EINVAL, "R=70000", R=70000, N=0)                  # R, then N
    expect(lib, EINVAL, "N 0", N=0, hyp_stride=-1)                # the shape before the strides
    expect(lib, EINVAL, "negative stride", hyp_stride=-1, rows_per_tile=63)
    expect(lib, EINVAL, "hyp_stride=", hyp_stride=2 ** 20 + 1, rows_per_tile=63)
    expect(lib, EINVAL, "rows_per_tile=63", rows_per_tile=63, hyp_length=None)
    expect(lib, EINVAL, "null length", hyp_length=None, hyp=None, counts=None)
    expect(lib, EINVAL, "null hyp", hyp=None, ref=None)
    expect(lib, EINVAL, "null ref", ref=None, counts=None)
    expect(lib, EINVAL, "null counts", counts=None, ws=None)      # every argument before the workspace
    expect(lib, EINVAL, "R=70000", R=70000, B=0)                  # a bad R hides B == 0


def test_empty_batch_is_ok(lib):
    expect(lib, OK, B=0)
    expect(lib, OK, B=0, hyp=None, hyp_length=None, ref=None, ref_length=None, counts=None, ws=None, ws_bytes=0)
    expect(lib, OK, B=0, N=0)               # no hypotheses to count
    expect(lib, OK, B=0, hyp_stride=-1, rows_per_tile=63)


def test_edit_distance_keeps_its_limit(lib):
    rc = lib.ctc_amd_edit_distance(ONE, 5, ONE, ONE, 4, ONE, 2, 3, 1025, ONE, None, 0, None)
    assert rc == EINVAL and "R=1025" in lib.ctc_amd_last_error().decode()
    out = ctypes.c_size_t(1)
    assert lib.ctc_amd_edit_distance_workspace_bytes(2, 3, 1025, ctypes.byref(out)) == EINVAL


def test_plan_check_program(tmp_path):
    """tests/tools/edit_counts_plan_check.cpp: the launcher's plan (diagonal enumeration, workspace offsets, size_t arithmetic) for K
    and J up to the limits, as a stand-alone host program.  (Built plainly here; the same source builds with
    -fsanitize=address,undefined.)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "edit_counts_plan_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "edit_counts_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and "ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
