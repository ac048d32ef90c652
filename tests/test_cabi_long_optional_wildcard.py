"""Host layer of the three long-form entry points with optional wildcards (include/ctc_amd.h, "Optional wildcards above 1024
labels"), in the manner of tests/test_cabi_long_windowed.py: nothing here touches a GPU.  Validation returns before any launch and
pointers are the never-dereferenced address 16.  A call that passes every check would launch: only rejected calls and B == 0 are
made here."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

PAIRS = {  # new entry: counterpart
    "ctc_amd_long_optional_wildcard_loss_grad": "ctc_amd_long_wildcard_loss_grad",
    "ctc_amd_long_optional_wildcard_loss_grad_ckpt": "ctc_amd_long_wildcard_loss_grad_ckpt",
    "ctc_amd_long_optional_wildcard_label_posterior": "ctc_amd_long_label_posterior",
}
QUERIES = {
    "ctc_amd_long_optional_wildcard_loss_workspace_bytes": "ctc_amd_long_wildcard_loss_workspace_bytes",
    "ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes": "ctc_amd_long_wildcard_loss_ckpt_workspace_bytes",
    "ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes": "ctc_amd_long_label_posterior_workspace_bytes",
}
B, T, V, U = 2, 5, 8, 4


def r256(n):
    return (n + 255) // 256 * 256


def arguments(name, kind=0, wrt=0, logits=ONE, xdtype=0, xsb=T * V, xst=V, labels=ONE, label_stride=5, label_length=ONE,
              logit_length=ONE, blank=0, weight=0.0, B=B, T=T, V=V, U=U, tf=0, loss=ONE, ws=ONE, ws_bytes=BIG):
    lead = (kind, wrt, logits, xdtype, xsb, xst, labels, label_stride, label_length, logit_length, blank, ctypes.c_float(weight), B, T, V, U, tf)
    if name.endswith("label_posterior"):
        return lead + (loss, ONE, ONE, ONE, ONE, ONE, ONE, ws, ws_bytes, None)
    return lead + (None, loss, ONE, 0, xsb, xst, ws, ws_bytes, None)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


def call(lib, name, **over):
    rc = getattr(lib, name)(*arguments(name, **over))
    return rc, lib.ctc_amd_last_error().decode()


def test_symbols_and_signatures(lib):
    from tf_seq2seq_losses_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    declared = set(re.findall(r"ctc_amd_[a-z_]+", header))

    def params(n):
        text = re.search(r"\bint " + n + r"\(([^;]*)\);", header).group(1)
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        return [" ".join(q.split()) for q in text.split(",")]
    for new, old in {**PAIRS, **QUERIES}.items():
        assert hasattr(lib, new) and new in _lib.SIGNATURES and new in declared, new
        assert _lib.SIGNATURES[new][0] is _lib.SIGNATURES[old][0] and list(_lib.SIGNATURES[new][1]) == list(_lib.SIGNATURES[old][1]), new
        assert getattr(lib, new).argtypes == list(_lib.SIGNATURES[new][1]), new
        assert params(new) == params(old), new  # the header: the counterpart's parameter list
    assert lib.ctc_amd_abi_version() == 6 == _lib.ABI_VERSION
    for new, old in PAIRS.items():
        assert re.search(r"\* +" + new + r" +counterpart: " + old + r"\b", header), new


BAD = [dict(kind=5), dict(kind=-1), dict(wrt=2), dict(xdtype=3), dict(xdtype=-1), dict(xsb=7), dict(xst=7), dict(xst=0), dict(tf=3), dict(tf=-4),
       dict(tf=6), dict(U=65537, label_stride=65537), dict(ws=ONE, ws_bytes=1), dict(ws=None, ws_bytes=0), dict(loss=None), dict(weight=0.5),
       dict(weight=float("nan")), dict(blank=8), dict(V=0), dict(V=16385), dict(labels=None), dict(label_length=None),
       dict(kind=5, tf=3), dict(xdtype=3, loss=None), dict(tf=3, ws=ONE, ws_bytes=1), dict(loss=None, tf=3), dict(U=65537, label_stride=65537, tf=3)]


@pytest.mark.parametrize("name", sorted(PAIRS))
@pytest.mark.parametrize("over", BAD, ids=[",".join(f"{k}={v}" for k, v in o.items() if k != "ws") for o in BAD])
def test_validation_is_the_counterparts(lib, name, over):
    """The same faulty arguments: the same code and the same words as the counterpart."""
    got, want = call(lib, name, **over), call(lib, PAIRS[name], **over)
    assert got == want and got[0] in (EINVAL, EWORKSPACE), (name, over, got, want)
    assert (got[0] == EWORKSPACE) == (set(over) <= {"ws", "ws_bytes"}), (name, over, got)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_empty_batch_is_a_no_op(lib, name):
    for over in (dict(B=0), dict(B=0, ws=None, ws_bytes=0), dict(B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None)):
        assert call(lib, name, **over)[0] == OK, (name, over)


def test_a_valid_call_stops_at_its_own_workspace_size(lib):
    """One byte short of the new size is refused, with the new size in the message: at K > 1 the counterpart's size does not do."""
    sz = ctypes.c_size_t(0)
    for name in sorted(PAIRS):
        query = name.replace("_grad_ckpt", "_ckpt").replace("_grad", "") + "_workspace_bytes"
        post = name.endswith("label_posterior")
        for shape in ((2, 5, 4), (2, 300, 2100)):
            b, t, u = shape
            rc = getattr(lib, query)(0, b, t, V, u, 4, *(() if post else (1,)), ctypes.byref(sz))
            assert rc == OK and sz.value > 0
            got = call(lib, name, B=b, T=t, U=u, label_stride=max(u, 1), xsb=t * V, tf=4, ws_bytes=sz.value - 1)
            assert got[0] == EWORKSPACE and f"{sz.value - 1} < {sz.value}" in got[1], (name, shape, got)


@pytest.mark.parametrize("kind", [0, 1])
def test_size_queries_are_the_counterparts_plus_two_columns(lib, kind):
    """K = 1: equal.  K > 1: 16 B (K - 1) T more, and with a gradient (the posteriors: always) 8 B (K - 1) T more, each rounded to 256."""
    new, old = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for b, t, u in ((2, 300, 1000), (2, 300, 1024), (3, 301, 1025), (3, 301, 2048), (1, 999, 8000), (2, 50, 8192)):
        K = (u + 1023) // 1024
        assert K in (1, 2, 8)
        c16, c8 = r256(16 * b * (K - 1) * t), r256(8 * b * (K - 1) * t)
        for tf in (0, 4, 64):
            for q in sorted(QUERIES):
                post = q.endswith("label_posterior_workspace_bytes")
                for g in ((1,) if post else (0, 1)):
                    tail = () if post else (g,)
                    assert getattr(lib, q)(kind, b, t, V, u, tf, *tail, ctypes.byref(new)) == OK
                    assert getattr(lib, QUERIES[q])(kind, b, t, V, u, tf, *tail, ctypes.byref(old)) == OK
                    assert new.value == old.value + c16 + (c8 if g else 0), (q, b, t, u, tf, g, new.value, old.value)
                    assert (new.value == old.value) == (K == 1)
    # what the counterparts refuse, in their words
    for q in sorted(QUERIES):
        post = q.endswith("label_posterior_workspace_bytes")
        for bad in ((2, 4, 50, 256, 64, 0), (0, 4, 50, 256, 64, 3), (0, 1, 50, 32, 65537, 0), (0, 4, 50, 0, 64, 0)):
            tail = () if post else (1,)
            a = (getattr(lib, q)(*bad, *tail, ctypes.byref(new)), lib.ctc_amd_last_error().decode())
            c = (getattr(lib, QUERIES[q])(*bad, *tail, ctypes.byref(old)), lib.ctc_amd_last_error().decode())
            assert a == c and a[0] == EINVAL, (q, bad, a, c)
        assert getattr(lib, q)(0, 4, 50, 256, 64, 0, *(() if post else (1,)), None) == EINVAL


def test_existing_size_queries_keep_their_values(lib):
    from tf_seq2seq_losses_amd import _lib
    assert _lib.long_wildcard_loss_ckpt_workspace_bytes(0, 1, 30000, 32, 8192) == 170923264
    assert _lib.long_optional_wildcard_loss_ckpt_workspace_bytes(0, 1, 30000, 32, 8192) == 170923264 + r256(16 * 7 * 30000) + r256(8 * 7 * 30000)
    assert _lib.long_optional_wildcard_loss_workspace_bytes(0, 1, 30000, 32, 8192, 0, False) == \
        _lib.long_wildcard_loss_workspace_bytes(0, 1, 30000, 32, 8192, 0, False) + r256(16 * 7 * 30000)
    assert _lib.long_optional_wildcard_label_posterior_workspace_bytes(1, 1, 30000, 32, 8192) == \
        _lib.long_label_posterior_workspace_bytes(1, 1, 30000, 32, 8192) + r256(16 * 7 * 30000) + r256(8 * 7 * 30000)


def test_python_layer_is_declared():
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops
    for name in ("classic_ctc_long_loss", "simplified_ctc_long_loss", "ctc_long_loss_from_logproba"):
        p = inspect.signature(getattr(ctc, name)).parameters
        assert list(p)[-2:] == ["optional_wildcards", "frame_window"], name
        assert p["optional_wildcards"].kind is inspect.Parameter.KEYWORD_ONLY and p["optional_wildcards"].default is False, name
        assert p["frame_window"].kind is inspect.Parameter.KEYWORD_ONLY and p["frame_window"].default is None, name
        assert "optional_wildcards" in getattr(ctc, name).__doc__, name
    for old in ("classic_ctc_long_label_posterior", "simplified_ctc_long_label_posterior", "ctc_long_label_posterior_from_logproba"):
        new = old.replace("_long_", "_long_optional_wildcard_")
        assert new in ctc.__all__ and old in ctc.__all__, new
        po, pn = inspect.signature(getattr(ctc, old)).parameters, inspect.signature(getattr(ctc, new)).parameters
        assert list(pn) == list(po) and all(pn[k].kind is po[k].kind and pn[k].default == po[k].default for k in po), new
        assert pn["dense"].default is True
        assert inspect.signature(getattr(ctc, new)).return_annotation == inspect.signature(getattr(ctc, old)).return_annotation, new
        assert "CtcLongLabelPosterior" in str(inspect.signature(getattr(ctc, new)).return_annotation), new
    po = inspect.signature(ops.long_wildcard_loss_grad).parameters
    pn = inspect.signature(ops.long_optional_wildcard_loss_grad).parameters
    assert list(po)[-1] == "checkpoint" and list(pn) == list(po) and all(pn[k].default == po[k].default for k in po)
    assert list(inspect.signature(ops.long_label_posterior).parameters)[-1] == "frame_window"
    assert callable(ops.long_optional_wildcard_label_posterior)
    assert "frame_window" not in inspect.signature(ops.long_optional_wildcard_label_posterior).parameters
    for helper in ("long_optional_wildcard_loss_workspace_bytes", "long_optional_wildcard_loss_ckpt_workspace_bytes",
                   "long_optional_wildcard_label_posterior_workspace_bytes"):
        assert callable(getattr(_lib, helper)), helper
    assert _lib.OPTIONAL_WILDCARD == -3


def test_window_with_optional_wildcards_raises_before_any_launch():
    """CPU tensors and no GPU: the ValueError comes before anything is looked at."""
    import torch

    import tf_seq2seq_losses_amd as ctc
    labels = torch.tensor([[1, -3, 2]], dtype=torch.int32)
    x = torch.zeros((1, 4, V))
    ll, tl = torch.tensor([3], dtype=torch.int32), torch.tensor([4], dtype=torch.int32)
    window = torch.zeros((1, 3, 2), dtype=torch.int32)
    for fn in (ctc.classic_ctc_long_loss, ctc.simplified_ctc_long_loss):
        with pytest.raises(ValueError, match="frame_window and optional_wildcards"):
            fn(labels, x, ll, tl, 0, optional_wildcards=True, frame_window=window)
    with pytest.raises(ValueError, match="frame_window and optional_wildcards"):
        ctc.ctc_long_loss_from_logproba(labels, x, ll, tl, 0, None, optional_wildcards=True, frame_window=window)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_plan_check_program(tmp_path, flags):
    """tests/tools/long_optional_plan_check.cpp: the optional plan's regions, that every reachable state lies in a tile that runs
    (T_b < L included), and the read-after-write order of every launch of both workspaces, the two new columns included, as a
    stand-alone host program, plainly and under the host sanitizers."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    out = str(tmp_path / "long_optional_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "tf_seq2seq_losses_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "long_optional_plan_check.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "175963392 checkpointed" in res.stdout
