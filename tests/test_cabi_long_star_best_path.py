"""Host layer of ctc_amd_long_optional_wildcard_best_path and ctc_amd_long_star_best_path (include/ctc_amd.h, DESIGN.md section
5.31), in the manner of tests/test_cabi_long_star.py: nothing here touches a GPU.  Validation returns before any launch and pointers
are the never-dereferenced address 16; only rejected calls are made, to the new entry point and to ctc_amd_long_wildcard_best_path,
which must answer alike."""
import ctypes
import inspect

import pytest

ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
B, T, V, U = 2, 3000, 8, 2100
NEW = (("ctc_amd_long_optional_wildcard_best_path", None), ("ctc_amd_long_star_best_path", 0), ("ctc_amd_long_star_best_path", 1))


def args(opt=None, kind=0, dtype=0, blank=0, u=U, tf=0, score=ONE, ws=ONE, ws_bytes=BIG):
    """opt: None for the calls without the argument, 0 / 1 for ctc_amd_long_star_best_path."""
    return (kind, 0, ONE, dtype, T * V, V, ONE, U, ONE, ONE, blank) + (() if opt is None else (opt,)) + \
        (B, T, V, u, tf, score, ONE, ONE, ONE, ONE, ONE, ws, ws_bytes, None)


def size(lib, name, opt, kind, u, tf=0, t=T):
    out = ctypes.c_size_t(0)
    rc = getattr(lib, name + "_workspace_bytes")(kind, *(() if opt is None else (opt,)), B, t, V, u, tf, ctypes.byref(out))
    return rc, out.value


def formula(kind, u, tf, t=T):
    """The header's: label blocks of 512 (classic) / 1024 (simplified) positions, every region rounded up to 256 bytes."""
    r = lambda x: (x + 255) // 256 * 256
    ub = 512 if kind == 0 else 1024
    k, j = max(1, -(-u // ub)), max(1, -(-t // (tf or 128)))
    return (r(256 * B * k * t) + r(16 * B * (k - 1) * t) + r(8 * B * k * (2 * ub + 8)) + r(8 * B * j) + r(4 * B * t) + r(4 * B)
            + r(8 * B * t) + r(4 * B * t) + r(8 * B * t) + r(16 * B * (k - 1) * t) + r(8 * B * t) + r(4 * B * t))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name,opt", NEW)
@pytest.mark.parametrize("kind", (0, 1))
def test_size_is_the_documented_formula(lib, name, opt, kind):
    ub = 512 if kind == 0 else 1024
    for u, tf in ((ub, 0), (ub + 1, 0), (2 * ub, 64), (2 * ub + 6, 4), (0, 0)):  # K = 1, 2, 2, 3, 1
        assert size(lib, name, opt, kind, u, tf) == (0, formula(kind, u, tf))
    assert size(lib, name, opt, kind, U, 0, t=0) == (0, formula(kind, U, 0, t=0))
    assert size(lib, name, opt, kind, 65536)[0] == 0 and size(lib, name, opt, kind, 65537)[0] != 0


@pytest.mark.parametrize("bad", (dict(kind=2), dict(dtype=7), dict(blank=V), dict(u=65537), dict(tf=6), dict(score=None)), ids=lambda d: next(iter(d)))
@pytest.mark.parametrize("name,opt", NEW)
def test_argument_checks_answer_as_the_counterpart(lib, name, opt, bad):
    rc = getattr(lib, name)(*args(opt, **bad))
    msg = lib.ctc_amd_last_error()
    ref = lib.ctc_amd_long_wildcard_best_path(*args(None, **bad))
    assert rc != 0 and rc == ref and msg == lib.ctc_amd_last_error()
    if "tf" in bad or "kind" in bad or "u" in bad:  # ... and so do the size queries
        kw = dict(kind=bad.get("kind", 0), u=bad.get("u", U), tf=bad.get("tf", 0))
        rc = size(lib, name, opt, **kw)[0]
        msg = lib.ctc_amd_last_error()
        assert rc != 0 and rc == size(lib, "ctc_amd_long_wildcard_best_path", None, **kw)[0] and msg == lib.ctc_amd_last_error()


@pytest.mark.parametrize("name,opt", NEW)
@pytest.mark.parametrize("kind", (0, 1))
def test_workspace_one_byte_short_is_refused(lib, name, opt, kind):
    need = formula(kind, U, 0)
    for bad in (dict(ws_bytes=need - 1), dict(ws=None, ws_bytes=need)):  # (the plan is the unit's own, so the message names its size)
        rc = getattr(lib, name)(*args(opt, kind=kind, **bad))
        msg = lib.ctc_amd_last_error().decode()
        assert rc != 0 and str(need) in msg
        assert rc == lib.ctc_amd_long_wildcard_best_path(*args(None, kind=kind, ws_bytes=1024))
    assert getattr(lib, name)(*args(opt, kind=kind, tf=6, ws_bytes=need)) not in (0, rc)  # (a bad tiling is still refused first)


def test_signatures():
    import tf_seq2seq_losses_amd as ctc
    for fn in (ctc.classic_ctc_long_wildcard_alignment, ctc.simplified_ctc_long_wildcard_alignment,
               ctc.ctc_long_wildcard_alignment_from_logproba):
        params = inspect.signature(fn).parameters
        assert list(params)[-3:] == ["frame_window", "optional_wildcards", "exclude_next_label"]
        assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY and params[n].default is False for n in list(params)[-2:])
