"""Host layer of ctc_amd_long_wildcard_loss_grad_ckpt / ctc_amd_long_wildcard_loss_ckpt_workspace_bytes (the long-form gradient from
tile checkpoints), in the manner of tests/test_cabi_long_loss.py, whose helpers it uses: nothing here touches a GPU.  Validation
returns before any launch, pointers are the never-dereferenced address 16 and no call is given a workspace large enough, so a call
that passes every check stops at CTC_AMD_EWORKSPACE."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.test_cabi_long_loss import EINVAL, EWORKSPACE, OK, ONE, ORDER, ROOT, args, lib, r256  # noqa: F401  (lib: the fixture)
from tests.test_cabi_long_loss import formula as formula_existing
from tests.test_cabi_long_loss import size as size_existing


def call(lib, **over):
    a = args(**over)
    rc = lib.ctc_amd_long_wildcard_loss_grad_ckpt(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def call_existing(lib, **over):
    a = args(**over)
    rc = lib.ctc_amd_long_wildcard_loss_grad(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def size(lib, kind, B, T, V, U, tf=0, want_grad=1):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, tf, want_grad, ctypes.byref(out))
    return rc, int(out.value)


def terms(kind, B, T, U, tf=0):
    """include/ctc_amd.h, ctc_amd_long_wildcard_loss_grad_ckpt with a gradient, term by term."""
    TF = tf or 128
    K, S = max(1, -(-U // 1024)), 2 - kind
    J = max(1, -(-T // TF))
    R = min(K, J)
    return dict(alpha_columns=r256(16 * B * (K - 1) * T), checkpoints=r256(8 * B * K * J * 2056), statistics=r256(16 * B * T),
                log2z=r256(8 * B), feasible=r256(4 * B), beta_columns=r256(8 * B * (K - 1) * T), beta_rows=r256(8 * B * K * 2056),
                ring=r256(8 * B * K * min(R * TF, T) * (S * 1024 + 2)))


def formula(kind, B, T, U, tf=0, want_grad=1):
    return sum(terms(kind, B, T, U, tf).values()) if want_grad else formula_existing(kind, B, T, U, 0)


def test_symbols_and_header(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_long_wildcard_loss_grad_ckpt", "ctc_amd_long_wildcard_loss_ckpt_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"^int " + name + r"\(", header, re.M), name  # declared, not only mentioned
    assert _lib.SIGNATURES["ctc_amd_long_wildcard_loss_grad_ckpt"] == _lib.SIGNATURES["ctc_amd_long_wildcard_loss_grad"]
    assert _lib.SIGNATURES["ctc_amd_long_wildcard_loss_ckpt_workspace_bytes"] == _lib.SIGNATURES["ctc_amd_long_wildcard_loss_workspace_bytes"]
    assert lib.ctc_amd_abi_version() == 6
    # the header's worked examples are the formula's values, as printed there
    assert "170 923 264 bytes classic" in header and "103 814 400 simplified" in header
    assert "6 385 200 384 bytes classic, 3 867 569 408 simplified" in header
    assert formula(0, 1, 30000, 8192) == 170923264 and formula(1, 1, 30000, 8192) == 103814400
    assert formula(0, 1, 180000, 50000) == 6385200384 and formula(1, 1, 180000, 50000) == 3867569408
    assert "min(R * TF, T)" in header and "frames_per_tile trades memory" in header


@pytest.mark.parametrize("kind", [0, 1])
def test_size_function(lib, kind):
    for B in (0, 1, 3):
        for T in (0, 1, 31, 127, 128, 129, 2700):
            for U in (0, 1, 1024, 1025, 2048, 2049, 65536):  # (K = 1 among them)
                for tf in (0, 4, 64, 128, 1000):
                    want = formula(kind, B, T, U, tf)
                    assert size(lib, kind, B, T, 32, U, tf, 1) == (OK, want), (B, T, U, tf, terms(kind, B, T, U, tf))
                    assert size(lib, kind, B, T, 32, U, tf, 7) == (OK, want)
                    # without a gradient: the existing function's forward-only size
                    assert size(lib, kind, B, T, 32, U, tf, 0) == size_existing(lib, kind, B, T, 32, U, tf, 0) == (OK, formula(kind, B, T, U, tf, 0))
                    # the ring never exceeds the per-frame rows it replaces
                    S, K = 2 - kind, max(1, -(-U // 1024))
                    assert terms(kind, B, T, U, tf)["ring"] <= r256(8 * B * K * T * (S * 1024 + 2))
    # frames_per_tile trades memory: the ring grows with it, the checkpoints shrink
    a, b = terms(kind, 1, 30000, 8192, 64), terms(kind, 1, 30000, 8192, 256)
    assert a["ring"] < b["ring"] and a["checkpoints"] > b["checkpoints"]
    assert size(lib, kind, 1, 30000, 32, 8192, 64)[1] == sum(a.values()) and size(lib, kind, 1, 30000, 32, 8192, 256)[1] == sum(b.values())
    # beyond 2^32 bytes: no 32-bit arithmetic on the way
    assert size(lib, kind, 8, 180000, 32, 65536, 4) == (OK, formula(kind, 8, 180000, 65536, 4)) and formula(kind, 8, 180000, 65536, 4) > 2 ** 32
    assert size(lib, kind, 8, 180000, 32, 65536, 0) == (OK, formula(kind, 8, 180000, 65536, 0))


def test_an_hour_of_audio(lib):
    rc, n = size(lib, 0, 1, 180000, 32, 50000, 0, 1)
    rc0, n0 = size_existing(lib, 0, 1, 180000, 32, 50000, 0, 1)
    assert (rc, rc0) == (OK, OK) and n == formula(0, 1, 180000, 50000) == 6385200384 and n0 == formula_existing(0, 1, 180000, 50000)
    assert n * 20 < n0
    t = terms(0, 1, 180000, 50000)  # K = 49, J = 1407, R = 49
    assert t["checkpoints"] == r256(8 * 49 * 1407 * 2056) and t["ring"] == r256(8 * 49 * 49 * 128 * 2050)
    assert size(lib, 0, 1, 30000, 32, 8192)[1] * 20 < size_existing(lib, 0, 1, 30000, 32, 8192)[1]


def test_size_function_limits(lib):
    for bad in ((2, 4, 50, 256, 64, 0), (0, -1, 50, 256, 64, 0), (0, 4, -1, 256, 64, 0), (0, 4, 50, 0, 64, 0), (0, 4, 50, 256, -1, 0),
                (0, 4, 50, 16385, 64, 0), (0, 4, 50, 256, 64, 3), (0, 4, 50, 256, 64, -4), (0, 1, 50, 32, 65537, 0)):
        rc = size(lib, *bad)[0]
        msg = lib.ctc_amd_last_error().decode()
        assert rc == EINVAL and (rc, msg) == (size_existing(lib, *bad)[0], lib.ctc_amd_last_error().decode()), bad
    assert lib.ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(0, 4, 50, 256, 64, 0, 1, None) == EINVAL
    assert size(lib, 0, 2 ** 30, 1024, 32, 65536, 4, 0)[0] == EINVAL  # a tile launch of more than 2^31 - 1 workgroups
    assert size(lib, 0, 2 ** 20, 2 ** 14, 32, 4, 0, 1)[0] == EINVAL and size(lib, 0, 2 ** 20, 2 ** 13, 32, 4, 0, 0)[0] == OK  # the row stage


BAD = [dict(kind=5), dict(kind=-1), dict(wrt=2), dict(B=-1), dict(T=-1), dict(V=0), dict(U=-1), dict(label_stride=-1), dict(blank=8),
       dict(blank=-1), dict(U=65537, label_stride=65537), dict(label_length=None), dict(logit_length=None), dict(logits=None),
       dict(labels=None), dict(xdtype=-1), dict(xdtype=3), dict(gdtype=3), dict(xsb=7), dict(xst=7), dict(xst=0), dict(gst=7),
       dict(gsb=-8), dict(weight=0.5), dict(weight=float("nan")), dict(weight=float("-inf")), dict(loss=None), dict(V=16385),
       dict(tf=-4), dict(tf=1), dict(tf=6), dict(tf=127),
       # precedence: the pairs of tests/test_cabi_long_loss.py::test_precedence
       dict(kind=5, wrt=2), dict(blank=99, U=65537), dict(kind=5, xdtype=3), dict(xdtype=3, B=0), dict(gdtype=3, xst=7),
       dict(xst=7, weight=0.5), dict(weight=0.5, loss=None), dict(loss=None, V=16385), dict(V=16385, tf=3),
       dict(tf=3, ws=ONE, ws_bytes=1), dict(kind=5, B=0), dict(B=2 ** 20, T=2 ** 14, tf=3), dict(B=2 ** 20, T=2 ** 14, tf=3, grad=None),
       dict(B=2 ** 30, T=1024, U=65536, label_stride=65536, tf=4, grad=None)]


@pytest.mark.parametrize("over", BAD, ids=[",".join(f"{k}={v}" for k, v in o.items() if k not in ("ws",)) for o in BAD])
def test_validation_is_the_existing_entry_s(lib, over):
    """The same faulty arguments: the same code and the same text as ctc_amd_long_wildcard_loss_grad, which is EINVAL."""
    got, want = call(lib, **over), call_existing(lib, **over)
    assert got == want and got[0] == EINVAL, (over, got, want)


def test_empty_batch_is_ok(lib):
    for over in (dict(B=0), dict(B=0, logits=None, labels=None, label_length=None, logit_length=None, d_loss=None, loss=None, grad=None),
                 dict(B=0, xst=7), dict(B=0, tf=3), dict(B=0, weight=0.5)):
        assert call(lib, **over)[0] == OK, over


def test_a_valid_call_stops_at_the_workspace(lib):
    for over in (dict(), dict(ws=ONE, ws_bytes=1), dict(kind=1, wrt=1), dict(grad=None), dict(grad=None, ws=ONE, ws_bytes=1),
                 dict(d_loss=None), dict(T=0), dict(V=16384), dict(weight=-0.5), dict(U=1025, label_stride=1025),
                 dict(U=65536, label_stride=65536), dict(xsb=8, xst=16, gsb=8, gst=16), dict(gst=7, grad=None),
                 *(dict(tf=tf) for tf in (0, 4, 8, 128, 132, 4096)), *(dict(xdtype=dt, gdtype=dt) for dt in (0, 1, 2))):
        rc, msg = call(lib, **over)
        assert rc == EWORKSPACE, (over, rc, msg)
    # one byte short is too small (only the failing side is called with a non-null workspace: nothing may be launched here)
    for kind in (0, 1):
        for shape in ((2, 5, 4), (2, 300, 2100), (1, 5, 0)):
            for tf in (0, 4):
                for want_grad in (1, 0):
                    B, T, U = shape
                    rc, need = size(lib, kind, B, T, 8, U, tf, want_grad)
                    assert rc == OK and need > 0
                    rc, msg = call(lib, kind=kind, B=B, T=T, U=U, label_stride=max(U, 1), tf=tf, ws=ONE, ws_bytes=need - 1,
                                   grad=ONE if want_grad else None)
                    assert rc == EWORKSPACE and f"{need - 1} < {need}" in msg, (shape, tf, want_grad, rc, msg)
    # the size that suffices is this entry's, not the existing one's: at T = 300, U = 2100 the two differ in both directions by tiling
    assert size(lib, 0, 2, 300, 8, 2100, 4, 1)[1] < size_existing(lib, 0, 2, 300, 8, 2100, 4, 1)[1]
    # a forward-only call is content with the forward-only size, which is the existing call's
    assert size(lib, 0, 2, 5, 8, 4, 0, 0) == size_existing(lib, 0, 2, 5, 8, 4, 0, 0)


def test_python_layer_is_declared():
    import inspect

    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops
    for name in ("classic_ctc_long_loss", "simplified_ctc_long_loss", "ctc_long_loss_from_logproba"):
        p = inspect.signature(getattr(ctc, name)).parameters
        assert p["checkpoint"].kind is inspect.Parameter.KEYWORD_ONLY and p["checkpoint"].default is False, name
        assert "checkpoint" in getattr(ctc, name).__doc__ and "same bits" in getattr(ctc, name).__doc__, name
    p = inspect.signature(ops.long_wildcard_loss_grad).parameters
    assert list(p)[-1] == "checkpoint" and p["checkpoint"].default is False
    assert callable(_lib.long_wildcard_loss_ckpt_workspace_bytes)
    assert _lib.long_wildcard_loss_ckpt_workspace_bytes(0, 1, 30000, 32, 8192) == 170923264
    assert _lib.long_wildcard_loss_ckpt_workspace_bytes(0, 1, 30000, 32, 8192, 0, False) == _lib.long_wildcard_loss_workspace_bytes(0, 1, 30000, 32, 8192, 0, False)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_plan_check_program(tmp_path, flags):
    """tests/tools/long_loss_ckpt_plan_check.cpp: the checkpointed plan's offsets and addressing, the read-after-write order of every
    launch, the ring's liveness and the row stage's cover, as a stand-alone host program, plainly and under the host sanitizers."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "long_loss_ckpt_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "long_loss_ckpt_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "6385200384 bytes checkpointed, 144859852800 existing" in res.stdout and "ring 5040179200" in res.stdout
