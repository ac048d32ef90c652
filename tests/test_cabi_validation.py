"""Characterisation of the C ABI's host layer: which code (and, where it is part of the contract, which text) every compute
entry point returns for a bad argument, which of two coinciding faults is reported, and which pipeline, workspace size and flag
offset a shape gets.  Nothing here touches a GPU: validation returns before any launch, pointers are the never-dereferenced
address 16 and no call is given a workspace, so a call that passes every check stops at CTC_AMD_EWORKSPACE.

tests/golden/cabi_dispatch_grid.json holds the answers of ctc_amd_pipeline_name, ctc_amd_workspace_bytes and the two
flag-offset functions over a grid that crosses every boundary of the tier selection.  It was written by
`python tests/test_cabi_validation.py --regenerate` from the library as it was BEFORE the host dispatch layer was reshaped
(tier enum, launcher table, shared argument checks); regenerate it only for a change that is meant to move a tier boundary
or a workspace layout."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_PATH = os.path.join(ROOT, "tests", "golden", "cabi_dispatch_grid.json")
OK, EINVAL, EWORKSPACE = 0, -1, -2
ONE = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p(20)  # the same, not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------
# one valid call per entry point; a case overrides single arguments of it

BASE = dict(kind=0, wrt=0, logits=ONE, labels=ONE, label_stride=4, label_length=ONE, logit_length=ONE, blank=0, B=2, T=5, V=8, U=4,
            xdtype=0, xsb=None, xst=None, gdtype=0, gsb=None, gst=None, row_offsets=ONE, row_stride=None, grad_row_stride=None,
            loss=ONE, grad=ONE, d_loss=None, sum2=ONE, zero_next=None, alpha=ONE, beta=ONE, lg=ONE, hess=ONE, vec=ONE, out=ONE,
            ws=None, ws_bytes=0)
PLAIN = ("loss_grad", "alpha_beta", "log_posterior", "hessian", "hvp")     # contiguous float32 logits
FORMATS = ("loss_grad_ex", "loss_grad_packed", "loss_grad_sum", "loss_forward", "grad_resume")  # producer formats
STRIDED = ("loss_grad_ex", "loss_grad_sum", "loss_forward", "grad_resume")
ENTRIES = PLAIN + FORMATS


def call(lib, entry, **over):
    unknown = set(over) - set(BASE)
    assert not unknown, unknown
    a = dict(BASE, **over)
    V, rows = a["V"], max(a["T"], 1) * a["V"]
    for k, dflt in (("xsb", rows), ("xst", V), ("gsb", rows), ("gst", V), ("row_stride", V), ("grad_row_stride", V)):
        if a[k] is None:
            a[k] = dflt
    g = lambda *names: tuple(a[n] for n in names)
    common = g("kind", "wrt", "logits", "labels", "label_stride", "label_length", "logit_length", "blank", "B", "T", "V", "U")
    common_ex = g("kind", "wrt", "logits", "xdtype", "xsb", "xst", "labels", "label_stride", "label_length", "logit_length", "blank",
                  "B", "T", "V", "U")
    tail = (a["ws"], a["ws_bytes"], None)
    args = {
        "loss_grad": common + g("loss", "grad", "d_loss"),
        "loss_grad_ex": common_ex + g("loss", "grad", "gdtype", "gsb", "gst", "d_loss"),
        "loss_grad_packed": g("kind", "wrt", "logits", "xdtype", "row_offsets", "row_stride", "labels", "label_stride", "label_length",
                              "logit_length", "blank", "B", "T", "V", "U", "loss", "grad", "gdtype", "grad_row_stride", "d_loss"),
        "loss_grad_sum": common_ex + g("loss", "grad", "gdtype", "gsb", "gst", "d_loss", "sum2", "zero_next"),
        "loss_forward": common_ex + g("loss"),
        "grad_resume": common_ex + g("loss", "grad", "gdtype", "gsb", "gst", "d_loss"),
        "alpha_beta": common + g("loss", "alpha", "beta"),
        "log_posterior": common + g("loss", "lg"),
        "hessian": common + g("loss", "grad", "hess"),
        "hvp": common + g("vec", "loss", "grad", "out"),
    }[entry]
    rc = getattr(lib, "ctc_amd_" + entry)(*args, *tail)
    return rc, lib.ctc_amd_last_error().decode()


def expect(lib, entry, want_rc, text=None, **over):
    rc, msg = call(lib, entry, **over)
    assert rc == want_rc, f"{entry}{over}: returned {rc} ({msg!r}), expected {want_rc}"
    if text is not None:
        assert text in msg, f"{entry}{over}: message {msg!r} lacks {text!r}"


# ---------------------------------------------------------------------------------------------------------------------------
# (name, entry points, overrides, expected code, substring of the message or None)

COMMON_CASES = [
    ("bad kind", dict(kind=5), "kind"),
    ("negative kind", dict(kind=-1), "kind"),
    ("bad wrt", dict(wrt=2), None),
    ("negative B", dict(B=-1), None),
    ("negative T", dict(T=-1), None),
    ("V = 0", dict(V=0), None),
    ("negative U", dict(U=-1), None),
    ("negative label stride", dict(label_stride=-1), None),
    ("blank = V", dict(blank=8), "blank"),
    ("negative blank", dict(blank=-1), "blank"),
    ("U over the limit", dict(U=1025, label_stride=1025), "U=1025"),
    ("null label_length", dict(label_length=None), None),
    ("null logit_length", dict(logit_length=None), None),
    ("null logits", dict(logits=None), None),
    ("null labels", dict(labels=None), None),
    # precedence inside the common checks, in the order they are made
    ("kind before wrt", dict(kind=5, wrt=2), "kind"),
    ("wrt before sizes", dict(wrt=2, B=-1), "wrt"),
    ("sizes before blank", dict(T=-1, blank=99), "negative"),
    ("blank before U", dict(blank=99, U=1025), "blank"),
    ("U before null lengths", dict(U=1025, label_length=None), "U=1025"),
    # a common fault hides everything behind it, B == 0 included
    ("kind before B == 0", dict(kind=5, B=0), "kind"),
    ("blank before B == 0", dict(blank=8, B=0), "blank"),
    ("U before B == 0", dict(U=1025, B=0), "U=1025"),
]


@pytest.mark.parametrize("entry", ENTRIES)
def test_common_argument_faults(lib, entry):
    for name, over, text in COMMON_CASES:
        expect(lib, entry, EINVAL, text, **over)


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_batch_is_ok_and_no_workspace_is_eworkspace(lib, entry):
    # B == 0: nothing to do, whatever else is null (loss_grad_sum with zero_next = NULL launches nothing)
    expect(lib, entry, OK, B=0)
    expect(lib, entry, OK, B=0, logits=None, labels=None, label_length=None, logit_length=None, loss=None, alpha=None,
           beta=None, lg=None, hess=None, vec=None, out=None, row_offsets=None, **({} if entry == "grad_resume" else {"grad": None}))
    # valid arguments: the first thing missing is the workspace
    expect(lib, entry, EWORKSPACE)
    expect(lib, entry, EWORKSPACE, ws=ONE, ws_bytes=1)
    expect(lib, entry, EWORKSPACE, kind=1, wrt=1)
    expect(lib, entry, EWORKSPACE, T=0)
    if entry != "grad_resume":
        expect(lib, entry, EWORKSPACE, grad=None)


def test_loss_alone_has_no_vocabulary_limit(lib):
    expect(lib, "loss_grad", EWORKSPACE, V=20000, grad=None)
    expect(lib, "loss_grad", EINVAL, "V=20000", V=20000)
    expect(lib, "loss_grad_ex", EWORKSPACE, V=20000, grad=None)
    expect(lib, "loss_grad_ex", EINVAL, "V=20000", V=20000)
    expect(lib, "loss_forward", EWORKSPACE, V=20000)
    # the limit is an argument fault: it is reported before the missing workspace, and after the null loss pointer
    expect(lib, "loss_grad", EINVAL, "loss", V=20000, loss=None)


@pytest.mark.parametrize("entry", FORMATS)
def test_element_types(lib, entry):
    for bad in (-1, 3):
        expect(lib, entry, EINVAL, "dtype", xdtype=bad)
        if entry != "loss_forward":  # (takes no gradient)
            expect(lib, entry, EINVAL, "dtype", gdtype=bad)
    for dt in (0, 1, 2):
        expect(lib, entry, EWORKSPACE, xdtype=dt, gdtype=dt)
    # precedence: common checks < dtype < B == 0
    expect(lib, entry, EINVAL, "kind", kind=5, xdtype=3)
    expect(lib, entry, EINVAL, "blank", blank=8, xdtype=3)
    expect(lib, entry, EINVAL, "dtype", xdtype=3, B=0)
    expect(lib, entry, EINVAL, "dtype", xdtype=3, loss=None)


@pytest.mark.parametrize("entry", STRIDED)
def test_strides_smaller_than_a_row(lib, entry):
    strides = ("xsb", "xst") if entry == "loss_forward" else ("xsb", "xst", "gsb", "gst")
    for s in strides:
        expect(lib, entry, EINVAL, "stride", **{s: 7})
        expect(lib, entry, EINVAL, "stride", **{s: 0})
        expect(lib, entry, EINVAL, "stride", **{s: -8})
        expect(lib, entry, EWORKSPACE, **{s: 8})
        expect(lib, entry, EWORKSPACE, **{s: 4096})
        expect(lib, entry, EINVAL, "dtype", xdtype=3, **{s: 7})     # dtype before strides
        expect(lib, entry, EINVAL, "stride", loss=None, **{s: 7})   # strides before the null loss pointer
    if entry in ("loss_grad_ex", "loss_grad_sum"):  # without a gradient its strides are not looked at
        expect(lib, entry, EWORKSPACE, grad=None, gsb=0, gst=0)
    # an empty batch has no rows to overlap -- except in loss_grad_sum, which checks the strides first
    for s in strides:
        expect(lib, entry, EINVAL if entry == "loss_grad_sum" else OK, B=0, **{s: 7})


def test_packed_rows(lib):
    e = "loss_grad_packed"
    expect(lib, e, EINVAL, "row_offsets", row_offsets=None)
    expect(lib, e, EINVAL, "row strides", row_stride=7)
    expect(lib, e, EINVAL, "row strides", grad_row_stride=7)
    expect(lib, e, EWORKSPACE, grad=None, grad_row_stride=0)
    expect(lib, e, EWORKSPACE, row_stride=64, grad_row_stride=32)
    expect(lib, e, EINVAL, "row_offsets", row_offsets=None, row_stride=7)   # row_offsets before the strides
    expect(lib, e, EINVAL, "dtype", row_offsets=None, gdtype=3)              # dtype before row_offsets
    expect(lib, e, OK, B=0, row_offsets=None, row_stride=7)                  # B == 0 before both
    expect(lib, e, EINVAL, "row strides", row_stride=7, loss=None)


def test_loss_grad_sum_accumulator(lib):
    e = "loss_grad_sum"
    expect(lib, e, EINVAL, "sum2", sum2=None)
    expect(lib, e, EINVAL, "sum2", sum2=None, xdtype=3)     # sum2 before dtype
    expect(lib, e, EINVAL, "sum2", sum2=None, xst=7)
    expect(lib, e, EINVAL, "sum2", sum2=None, B=0)          # ... and before B == 0
    expect(lib, e, EINVAL, "kind", sum2=None, kind=5)       # ... and behind the common checks
    expect(lib, e, OK, B=0, zero_next=None)


def test_grad_resume_needs_a_gradient(lib):
    e = "grad_resume"
    expect(lib, e, EINVAL, "grad", grad=None)
    expect(lib, e, EINVAL, "grad", grad=None, B=0)          # before B == 0
    expect(lib, e, EINVAL, "grad", grad=None, xst=7)        # before the strides
    expect(lib, e, EINVAL, "dtype", grad=None, gdtype=3)    # behind dtype
    expect(lib, e, EINVAL, "loss", loss=None)
    expect(lib, e, EINVAL, "V=20000", V=20000)


def test_log_domain_entry_points(lib):
    """alpha_beta, log_posterior, hessian, hvp: B == 0, then null outputs, then the vocabulary limit, then alignment, then workspace."""
    for e, outs in (("alpha_beta", ("loss", "alpha", "beta")), ("log_posterior", ("loss", "lg")), ("hessian", ("loss", "hess")),
                    ("hvp", ("loss", "out", "vec"))):
        for o in outs:
            expect(lib, e, EINVAL, "null", **{o: None})
            expect(lib, e, OK, B=0, **{o: None})
    expect(lib, "log_posterior", EWORKSPACE, T=0, lg=None)   # no frames, nothing to write
    expect(lib, "hvp", EWORKSPACE, T=0, vec=None)
    expect(lib, "log_posterior", EWORKSPACE, V=8192)
    expect(lib, "log_posterior", EINVAL, "V=8193", V=8193)
    expect(lib, "log_posterior", EINVAL, "null", V=8193, loss=None)
    expect(lib, "alpha_beta", EWORKSPACE, V=20000)
    for e in ("hessian", "hvp"):
        expect(lib, e, EWORKSPACE, V=16380)
        expect(lib, e, EINVAL, "V=16381", V=16381)
        expect(lib, e, EINVAL, "null", V=16381, loss=None)
        expect(lib, e, EINVAL, "aligned", logits=ODD)
        expect(lib, e, EINVAL, "aligned", grad=ODD)
        expect(lib, e, EINVAL, "V=16381", V=16381, logits=ODD)   # limit before alignment
        expect(lib, e, EINVAL, "null", loss=None, logits=ODD)    # null output before alignment
        expect(lib, e, EWORKSPACE, grad=None)
    expect(lib, "hessian", EINVAL, "aligned", hess=ODD)
    expect(lib, "hvp", EINVAL, "aligned", vec=ODD)
    expect(lib, "hvp", EINVAL, "aligned", out=ODD)


# ---------------------------------------------------------------------------------------------------------------------------
# tier selection, workspace sizes and flag offsets over a grid that crosses every boundary of the eligibility predicate

GRID_V = (255, 256, 257, 512, 513, 1024, 1025)
GRID_U = (64, 65, 128, 129, 256, 257, 512, 513)
GRID_BT = ((4, 50), (0, 50), (4, 0))
OVERRIDES = ("", "v1", "fused5")


def dispatch_grid(lib):
    """{override: [[kind, B, T, V, U, names, ws0..ws4, flags_offset, hvp_flags_offset], ...]}: `names` = the pipeline for
    (wrt, want_grad) = (0,1), (0,0), (1,1), (1,0); a size or offset the library refuses with CTC_AMD_EINVAL is null."""
    def sized(fn, *args):
        out = ctypes.c_size_t(0)
        rc = fn(*args, ctypes.byref(out))
        assert rc in (OK, EINVAL), rc
        return int(out.value) if rc == OK else None

    table = {}
    try:
        for ov in OVERRIDES:
            assert lib.ctc_amd_debug_override(b"pipeline", ov.encode()) == OK
            rows = table[ov] = []
            for kind in (0, 1):
                for B, T in GRID_BT:
                    for V in GRID_V:
                        for U in GRID_U:
                            names = ",".join(lib.ctc_amd_pipeline_name(kind, wrt, B, T, V, U, wg).decode() for wrt in (0, 1) for wg in (1, 0))
                            ws = [sized(lib.ctc_amd_workspace_bytes, what, kind, B, T, V, U) for what in range(5)]
                            rows.append([kind, B, T, V, U, names, *ws,
                                         sized(lib.ctc_amd_debug_flags_offset, kind, B, T, V, U),
                                         sized(lib.ctc_amd_debug_hvp_flags_offset, kind, B, T, V, U)])
    finally:
        lib.ctc_amd_debug_override(b"pipeline", b"")
    return table


def test_dispatch_grid_matches_the_recorded_one(lib):
    want = json.load(open(GRID_PATH))
    got = dispatch_grid(lib)
    assert sorted(got) == sorted(want)
    for ov in OVERRIDES:
        assert len(got[ov]) == len(want[ov]) == 2 * len(GRID_BT) * len(GRID_V) * len(GRID_U)
        for g, w in zip(got[ov], want[ov]):
            assert g == w, f"override {ov!r}: [kind, B, T, V, U, names, ws x 5, flags, hvp flags] = {g}, recorded {w}"
    # the grid does cross every tier
    seen = {n for ov in OVERRIDES for row in want[ov] for n in row[5].split(",")}
    assert seen == {"fused6", "fused5", "v1"}


def test_shape_guard_of_the_query_functions(lib):
    for bad in (dict(kind=2), dict(B=-1), dict(T=-1), dict(V=0), dict(U=-1), dict(U=1025)):
        a = dict(kind=0, B=4, T=50, V=256, U=64, **{})
        a.update(bad)
        shape = (a["kind"], a["B"], a["T"], a["V"], a["U"])
        assert lib.ctc_amd_pipeline_name(a["kind"], 0, *shape[1:], 1) == b"invalid"
        out = ctypes.c_size_t(0)
        for what in range(5):
            assert lib.ctc_amd_workspace_bytes(what, *shape, ctypes.byref(out)) == EINVAL
        assert lib.ctc_amd_debug_flags_offset(*shape, ctypes.byref(out)) == EINVAL
        assert lib.ctc_amd_debug_hvp_flags_offset(*shape, ctypes.byref(out)) == EINVAL
    out = ctypes.c_size_t(0)
    assert lib.ctc_amd_workspace_bytes(5, 0, 4, 50, 256, 64, ctypes.byref(out)) == EINVAL
    assert lib.ctc_amd_workspace_bytes(-1, 0, 4, 50, 256, 64, ctypes.byref(out)) == EINVAL
    assert lib.ctc_amd_workspace_bytes(0, 0, 4, 50, 256, 64, None) == EINVAL
    assert lib.ctc_amd_debug_flags_offset(0, 4, 50, 256, 64, None) == EINVAL
    assert lib.ctc_amd_debug_hvp_flags_offset(0, 4, 50, 256, 64, None) == EINVAL
    assert lib.ctc_amd_pipeline_name(0, 7, 4, 50, 256, 64, 1) == b"v1"  # (wrt is not validated here: anything but logits is v1)


def test_override_spellings(lib):
    try:
        for value, rc in ((b"v1", OK), (b"fused5", OK), (b"", OK), (b"fused6", EINVAL), (b"wide", EINVAL), (b"V1", EINVAL)):
            assert lib.ctc_amd_debug_override(b"pipeline", value) == rc, value
        assert lib.ctc_amd_debug_override(b"pipeline", None) == EINVAL
        assert lib.ctc_amd_debug_override(None, b"") == EINVAL
        # a refused value leaves the setting alone
        assert lib.ctc_amd_debug_override(b"pipeline", b"v1") == OK
        assert lib.ctc_amd_debug_override(b"pipeline", b"nope") == EINVAL
        assert lib.ctc_amd_pipeline_name(0, 0, 4, 50, 256, 64, 1) == b"v1"
    finally:
        lib.ctc_amd_debug_override(b"pipeline", b"")
    assert lib.ctc_amd_pipeline_name(0, 0, 4, 50, 256, 64, 1) == b"fused6"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--regenerate"], "usage: python tests/test_cabi_validation.py --regenerate"
    sys.path.insert(0, ROOT)
    from tf_seq2seq_losses_amd import _lib
    with open(GRID_PATH, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(ov) + ": [\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]"
                                   for ov, rows in dispatch_grid(_lib.load()).items()) + "\n}\n")
    print("wrote", GRID_PATH)
