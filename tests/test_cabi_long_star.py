"""Host layer of the three long-form star entry points (include/ctc_amd.h, "The exclusion above 1024 labels"), in the manner of
tests/test_cabi_star.py: nothing here touches a GPU.  Validation returns before any launch and pointers are the never-dereferenced
address 16; only rejected calls are made.  Each entry point is its counterpart plus `int optional_wildcards` behind blank_index
(size queries: behind kind), so every rejected call is made to both and must answer alike."""
import ctypes
import inspect

import pytest

ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
PAIRS = {  # new entry: (counterpart with optional_wildcards = 0, with 1)
    "ctc_amd_long_star_loss_grad": ("ctc_amd_long_wildcard_loss_grad", "ctc_amd_long_optional_wildcard_loss_grad"),
    "ctc_amd_long_star_loss_grad_ckpt": ("ctc_amd_long_wildcard_loss_grad_ckpt", "ctc_amd_long_optional_wildcard_loss_grad_ckpt"),
    "ctc_amd_long_star_label_posterior": ("ctc_amd_long_label_posterior", "ctc_amd_long_optional_wildcard_label_posterior"),
}
SIZES = {
    "ctc_amd_long_star_loss_workspace_bytes": ("ctc_amd_long_wildcard_loss_workspace_bytes", "ctc_amd_long_optional_wildcard_loss_workspace_bytes"),
    "ctc_amd_long_star_loss_ckpt_workspace_bytes": ("ctc_amd_long_wildcard_loss_ckpt_workspace_bytes",
                                                    "ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes"),
    "ctc_amd_long_star_label_posterior_workspace_bytes": ("ctc_amd_long_label_posterior_workspace_bytes",
                                                          "ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes"),
}
B, T, V, U = 2, 3000, 8, 2100


def args(name, opt=None, kind=0, dtype=0, blank=0, weight=0.0, u=U, tf=0, loss=ONE, ws=ONE, ws_bytes=BIG):
    """opt: None for a counterpart, 0 / 1 for the star entry point."""
    lead = (kind, 0, ONE, dtype, T * V, V, ONE, U, ONE, ONE, blank) + (() if opt is None else (opt,)) + (ctypes.c_float(weight), B, T, V, u, tf)
    if name.endswith("label_posterior"):
        return lead + (loss, ONE, ONE, ONE, ONE, ONE, ONE, ws, ws_bytes, None)
    return lead + (None, loss, ONE, 0, T * V, V, ws, ws_bytes, None)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(SIZES))
def test_sizes_are_the_counterparts(lib, name):
    """Nothing is added to the counterparts' plans: one label block, two and three, both workspaces, with and without a gradient."""
    for opt in (0, 1):
        for u, tf in ((1024, 0), (1030, 0), (2100, 64)):
            for want in ((), ) if name.endswith("posterior_workspace_bytes") else ((0,), (1,)):
                got, ref = ctypes.c_size_t(0), ctypes.c_size_t(0)
                assert getattr(lib, name)(0, opt, B, T, V, u, tf, *want, ctypes.byref(got)) == 0
                assert getattr(lib, SIZES[name][opt])(0, B, T, V, u, tf, *want, ctypes.byref(ref)) == 0
                assert got.value == ref.value and got.value % 256 == 0 and got.value > 0
    assert getattr(lib, name)(0, 0, B, T, V, 65537, 0, *(() if name.endswith("posterior_workspace_bytes") else (1,)), ctypes.byref(got)) != 0


@pytest.mark.parametrize("bad", (dict(kind=2), dict(dtype=7), dict(blank=V), dict(weight=0.5), dict(u=65537), dict(tf=6), dict(loss=None),
                                 dict(ws=None), dict(ws_bytes=1024)), ids=lambda d: next(iter(d)))
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_argument_checks_answer_as_the_counterparts(lib, name, bad):
    for opt in (0, 1):
        rc = getattr(lib, name)(*args(name, opt, **bad))
        msg = lib.ctc_amd_last_error()
        ref = getattr(lib, PAIRS[name][opt])(*args(name, None, **bad))
        assert rc != 0 and rc == ref and msg == lib.ctc_amd_last_error()


def test_signatures():
    import tf_seq2seq_losses_amd as ctc
    for fn in (ctc.classic_ctc_long_loss, ctc.simplified_ctc_long_loss, ctc.ctc_long_loss_from_logproba):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["exclude_next_label"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
        assert names[-2:] == ["optional_wildcards", "frame_window"] and names[-4:-2] == ["checkpoint", "exclude_next_label"]
    for stem in ("classic_ctc_long_star_label_posterior", "simplified_ctc_long_star_label_posterior",
                 "ctc_long_star_label_posterior_from_logproba"):
        assert stem in ctc.__all__
        p = inspect.signature(getattr(ctc, stem)).parameters["optional_wildcards"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert list(inspect.signature(ctc.classic_ctc_long_star_label_posterior).parameters)[:-1] == \
        list(inspect.signature(ctc.classic_ctc_long_label_posterior).parameters)
