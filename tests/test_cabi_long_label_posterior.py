"""Host layer of ctc_amd_long_label_posterior / ctc_amd_long_label_posterior_workspace_bytes (label posteriors above 1024 labels,
DESIGN.md section 5.22), in the manner of tests/test_cabi_long_loss_ckpt.py, whose helpers it uses: nothing here touches a GPU.
Validation returns before any launch, pointers are the never-dereferenced address 16 and no call is given a workspace large enough,
so a call that passes every check stops at CTC_AMD_EWORKSPACE."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from tests import test_cabi_long_loss_ckpt as CK
from tests.test_cabi_long_loss import EINVAL, EWORKSPACE, OK, ONE, ROOT, lib, r256  # noqa: F401  (lib: the fixture)

BASE = dict(kind=0, wrt=0, logits=ONE, xdtype=0, xsb=None, xst=None, labels=ONE, label_stride=4, label_length=ONE, logit_length=ONE,
            blank=0, weight=0.0, B=2, T=5, V=8, U=4, tf=0, loss=ONE, post=ONE, blk=ONE, dur=ONE, exf=ONE, peak=ONE, pfr=ONE, ws=None,
            ws_bytes=0)
ORDER = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank", "weight",
         "B", "T", "V", "U", "tf", "loss", "post", "blk", "dur", "exf", "peak", "pfr", "ws", "ws_bytes")
SHARED = ("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank", "weight",
          "B", "T", "V", "U", "tf", "loss", "ws", "ws_bytes")  # what the checkpointed gradient takes too


def call(lib, **over):
    assert not set(over) - set(BASE), over
    a = dict(BASE, **over)
    if a["xsb"] is None:
        a["xsb"] = max(a["T"], 1) * a["V"]
    if a["xst"] is None:
        a["xst"] = a["V"]
    a["weight"] = ctypes.c_float(a["weight"])
    rc = lib.ctc_amd_long_label_posterior(*(a[k] for k in ORDER), None)
    return rc, lib.ctc_amd_last_error().decode()


def call_ckpt(lib, **over):
    """ctc_amd_long_wildcard_loss_grad_ckpt WITH a gradient on the shared arguments (a float32 gradient with the logits' strides)."""
    assert not set(over) - set(SHARED), over
    return CK.call(lib, **over, gsb=over.get("xsb"), gst=over.get("xst"))


def size(lib, kind, B, T, V, U, tf=0):
    out = ctypes.c_size_t(0)
    rc = lib.ctc_amd_long_label_posterior_workspace_bytes(kind, B, T, V, U, tf, ctypes.byref(out))
    return rc, int(out.value)


def terms(kind, B, T, U, tf=0):
    """include/ctc_amd.h, ctc_amd_long_label_posterior, term by term: section 5.21's terms, then the two of this call."""
    return dict(CK.terms(kind, B, T, U, tf), sums=r256(16 * B * U), peaks=r256(8 * B * U))


def test_symbols_and_header(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    for name in ("ctc_amd_long_label_posterior", "ctc_amd_long_label_posterior_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"^int " + name + r"\(", header, re.M), name  # declared, not only mentioned
    assert len(_lib.SIGNATURES["ctc_amd_long_label_posterior"][1]) == len(ORDER) + 1 == 27  # + the stream
    assert len(_lib.SIGNATURES["ctc_amd_long_label_posterior_workspace_bytes"][1]) == 7
    # the shared arguments are declared as the checkpointed gradient declares them
    ck = _lib.SIGNATURES["ctc_amd_long_wildcard_loss_grad_ckpt"][1]
    assert _lib.SIGNATURES["ctc_amd_long_label_posterior"][1][:17] == ck[:17]
    assert lib.ctc_amd_abi_version() == 6
    # the header's worked examples are the formula's values, as printed there
    assert "171 119 872 bytes classic" in header and "6 386 400 512 classic" in header
    assert sum(terms(0, 1, 30000, 8192).values()) == 171119872 and sum(terms(0, 1, 180000, 50000).values()) == 6386400512
    assert "r256(16 * B * U)" in header and "r256(8 * B * U)" in header and "DESCENDING FRAME ORDER" in header


@pytest.mark.parametrize("kind", [0, 1])
def test_size_function_term_by_term(lib, kind):
    """section 5.21's function plus r256(16 B U) + r256(8 B U): the four shapes of its table first, then a grid."""
    table = ((1, 30000, 8192), (1, 180000, 50000))
    want = {(0, table[0]): 170923264, (1, table[0]): 103814400, (0, table[1]): 6385200384, (1, table[1]): 3867569408}
    for B, T, U in table:
        rc, ck = CK.size(lib, kind, B, T, 32, U, 0, 1)
        assert rc == OK and ck == want[(kind, (B, T, U))]
        t = terms(kind, B, T, U)
        assert sum(v for k, v in t.items() if k not in ("sums", "peaks")) == ck
        assert t["sums"] == r256(16 * U) and t["peaks"] == r256(8 * U)
        assert size(lib, kind, B, T, 32, U) == (OK, ck + t["sums"] + t["peaks"]) == (OK, sum(t.values())), (B, T, U, t)
    for B in (0, 1, 3):
        for T in (0, 1, 127, 128, 129, 2700):
            for U in (0, 1, 5, 1024, 1025, 2049, 65536):
                for tf in (0, 4, 64, 1000):
                    rc, ck = CK.size(lib, kind, B, T, 32, U, tf, 1)
                    assert rc == OK and size(lib, kind, B, T, 32, U, tf) == (OK, ck + r256(16 * B * U) + r256(8 * B * U)), (B, T, U, tf)
                    assert size(lib, kind, B, T, 32, U, tf)[1] == sum(terms(kind, B, T, U, tf).values())
    # beyond 2^32 bytes: no 32-bit arithmetic on the way
    assert size(lib, kind, 8, 180000, 32, 65536, 4) == (OK, sum(terms(kind, 8, 180000, 65536, 4).values()))


def test_size_function_limits(lib):
    """What the checkpointed size function refuses with a gradient, with its words; and this call's own launch grid."""
    for bad in ((2, 4, 50, 256, 64, 0), (0, -1, 50, 256, 64, 0), (0, 4, -1, 256, 64, 0), (0, 4, 50, 0, 64, 0), (0, 4, 50, 256, -1, 0),
                (0, 4, 50, 16385, 64, 0), (0, 4, 50, 256, 64, 3), (0, 4, 50, 256, 64, -4), (0, 1, 50, 32, 65537, 0),
                (0, 2 ** 20, 2 ** 14, 32, 4, 0)):
        rc = size(lib, *bad)[0]
        msg = lib.ctc_amd_last_error().decode()
        assert rc == EINVAL and (rc, msg) == (CK.size(lib, *bad, 1)[0], lib.ctc_amd_last_error().decode()), bad
    assert lib.ctc_amd_long_label_posterior_workspace_bytes(0, 4, 50, 256, 64, 0, None) == EINVAL
    # 2^20 * 1028 workgroups of rows and 2^30 of positions: each fits a grid (the checkpointed call accepts the shape), the sum does not
    assert CK.size(lib, 0, 2 ** 22, 1028, 32, 65536, 1028, 1)[0] == OK and size(lib, 0, 2 ** 22, 1028, 32, 65536, 1028)[0] == EINVAL
    assert size(lib, 0, 2 ** 22, 1020, 32, 65536, 1020)[0] == OK


BAD = [dict(kind=5), dict(kind=-1), dict(wrt=2), dict(B=-1), dict(T=-1), dict(V=0), dict(U=-1), dict(label_stride=-1), dict(blank=8),
       dict(blank=-1), dict(U=65537, label_stride=65537), dict(label_length=None), dict(logit_length=None), dict(logits=None),
       dict(labels=None), dict(xdtype=-1), dict(xdtype=3), dict(xsb=7), dict(xst=7), dict(xst=0), dict(weight=0.5),
       dict(weight=float("nan")), dict(weight=float("-inf")), dict(loss=None), dict(V=16385), dict(tf=-4), dict(tf=1), dict(tf=6),
       dict(tf=127), dict(B=2 ** 20, T=2 ** 14), dict(B=2 ** 30, T=1024, U=65536, label_stride=65536, tf=4),
       # precedence, pair by pair in the order of the checks
       dict(kind=5, wrt=2), dict(blank=99, U=65537), dict(kind=5, xdtype=3), dict(xdtype=3, B=0), dict(xdtype=3, xst=7),
       dict(xst=7, weight=0.5), dict(weight=0.5, loss=None), dict(loss=None, V=16385), dict(V=16385, B=2 ** 20, T=2 ** 14),
       dict(B=2 ** 20, T=2 ** 14, tf=3), dict(V=16385, tf=3), dict(tf=3, ws=ONE, ws_bytes=1), dict(kind=5, B=0)]


@pytest.mark.parametrize("over", BAD, ids=[",".join(f"{k}={v}" for k, v in o.items() if k not in ("ws",)) for o in BAD])
def test_validation_is_the_checkpointed_entry_s(lib, over):
    """The same faulty shared arguments: the code and the text of ctc_amd_long_wildcard_loss_grad_ckpt with a gradient."""
    got, want = call(lib, **over), call_ckpt(lib, **over)
    assert got == want and got[0] == EINVAL, (over, got, want)


def test_validation_of_the_outputs(lib):
    """After the checkpointed entry's checks: blank_posterior when T > 0, the two pairs; then frames_per_tile, the grid, the workspace."""
    rc, msg = call(lib, blk=None)
    assert rc == EINVAL and "null blank_posterior pointer" in msg
    assert call(lib, blk=None, T=0)[0] == EWORKSPACE
    for over in (dict(dur=None), dict(exf=None)):
        rc, msg = call(lib, **over)
        assert rc == EINVAL and msg == "duration and expected_frame must both be given or both be NULL", (over, msg)
    for over in (dict(peak=None), dict(pfr=None)):
        rc, msg = call(lib, **over)
        assert rc == EINVAL and msg == "peak_posterior and peak_frame must both be given or both be NULL", (over, msg)
    # order: loss, V, B * T before the outputs; the outputs in the order above; the outputs before frames_per_tile and the workspace
    assert "null loss pointer" in call(lib, loss=None, blk=None)[1]
    assert "exceeds the supported maximum" in call(lib, V=16385, blk=None)[1]
    assert "rows exceed the launch grid" in call(lib, B=2 ** 20, T=2 ** 14, blk=None)[1]
    assert "blank_posterior" in call(lib, blk=None, dur=None)[1]
    assert "duration" in call(lib, dur=None, peak=None)[1]
    assert "peak_posterior" in call(lib, peak=None, tf=3)[1]
    assert "duration" in call(lib, exf=None, ws=ONE, ws_bytes=1)[1]
    rc, msg = call(lib, tf=3, ws=ONE, ws_bytes=1)
    assert rc == EINVAL and "frames_per_tile=3" in msg
    # the posterior stage's own grid is refused with the tile grid's words
    rc, msg = call(lib, B=2 ** 22, T=1028, U=65536, label_stride=65536, tf=1028)
    assert rc == EINVAL and "is too large for" in msg, msg
    assert call(lib, B=2 ** 22, T=1020, U=65536, label_stride=65536, tf=1020)[0] == EWORKSPACE


def test_empty_batch_is_ok(lib):
    for over in (dict(B=0), dict(B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None, post=None, blk=None,
                               dur=None, exf=None, peak=None, pfr=None),
                 dict(B=0, xst=7), dict(B=0, tf=3), dict(B=0, weight=0.5), dict(B=0, dur=None)):
        assert call(lib, **over)[0] == OK, over


def test_a_valid_call_stops_at_the_workspace(lib):
    for over in (dict(), dict(ws=ONE, ws_bytes=1), dict(kind=1, wrt=1), dict(post=None), dict(dur=None, exf=None), dict(peak=None, pfr=None),
                 dict(post=None, dur=None, exf=None, peak=None, pfr=None), dict(T=0), dict(T=0, blk=None, post=None), dict(U=0, label_stride=0),
                 dict(V=16384), dict(weight=-0.5), dict(U=1025, label_stride=1025), dict(U=65536, label_stride=65536), dict(xsb=8, xst=16),
                 *(dict(tf=tf) for tf in (0, 4, 8, 128, 132, 4096)), *(dict(xdtype=dt) for dt in (0, 1, 2))):
        rc, msg = call(lib, **over)
        assert rc == EWORKSPACE, (over, rc, msg)
    # one byte short is too small, and the checkpointed gradient's size is (only failing calls get a non-null workspace: no launch here)
    for kind in (0, 1):
        for B, T, U in ((2, 5, 4), (2, 300, 2100), (1, 5, 0), (1, 0, 7)):
            for tf in (0, 4):
                rc, need = size(lib, kind, B, T, 8, U, tf)
                assert rc == OK and need > 0
                for n in (need - 1, CK.size(lib, kind, B, T, 8, U, tf, 1)[1] if U else need - 1):
                    rc, msg = call(lib, kind=kind, B=B, T=T, U=U, label_stride=max(U, 1), tf=tf, ws=ONE, ws_bytes=n)
                    assert rc == EWORKSPACE and f"{n} < {need}" in msg, (B, T, U, tf, rc, msg)


def test_python_layer_is_declared():
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops
    want = ["labels", "logits", "label_length", "logit_length", "blank_index", "wildcard_log_weight", "frames_per_tile",
            "max_label_length", "dense"]
    for name in ("classic_ctc_long_label_posterior", "simplified_ctc_long_label_posterior"):
        assert name in ctc.__all__
        p = inspect.signature(getattr(ctc, name)).parameters
        assert list(p) == want, (name, list(p))
        assert p["blank_index"].default == 0 and p["wildcard_log_weight"].default == 0.0 and p["frames_per_tile"].default is None
        assert p["max_label_length"].default is None and p["dense"].default is True
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want[5:])
    p = inspect.signature(ctc.ctc_long_label_posterior_from_logproba).parameters
    assert [k for k in p if k != "ctc_loss_data_cls"] == ["labels", "logprobas"] + want[2:] and p["dense"].default is True
    assert "ctc_long_label_posterior_from_logproba" in ctc.__all__ and "CtcLongLabelPosterior" in ctc.__all__
    assert ctc.CtcLongLabelPosterior._fields == ("loss", "label_posterior", "blank_posterior", "duration", "expected_frame",
                                                 "peak_posterior", "peak_frame")
    assert callable(ops.long_label_posterior)
    assert _lib.long_label_posterior_workspace_bytes(0, 1, 30000, 32, 8192) == 171119872
    assert _lib.long_label_posterior_workspace_bytes(1, 1, 180000, 32, 50000, 0) == 3867569408 + r256(16 * 50000) + r256(8 * 50000)


def test_plan_check_program(tmp_path):
    """tests/tools/long_post_plan_check.cpp: the plan's regions, the posterior stage's reads of the ring, its cover of (b, t) and
    (b, i) and the life of the accumulators, as a stand-alone host program (built plainly here; its header says how to build it
    under the host sanitizers)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "long_post_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "long_post_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "171119872 bytes" in res.stdout and "6386400512 bytes" in res.stdout and "3868769536 bytes" in res.stdout
