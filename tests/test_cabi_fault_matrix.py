"""Fault matrix of the C ABI's host layer, for every compute entry point and size query that tests/test_cabi_validation.py does
not characterise: the return code and the full message of every rejected call, which of two coinciding faults is reported, which
calls answer CTC_AMD_OK for B == 0 before looking further, and what every size query answers over a small grid of shapes.
Nothing here touches a GPU: pointers are the never-dereferenced address 16, no call is given a workspace, and a call that passes
every check would launch, so only rejected calls and B == 0 are made here.

For each entry point there are two hand-written tables: one baseline call (ARGS, BASE and its `base`) and the overrides of it
(`checks`: one fault per check, in the order the checks are made today; `more`: further values of the same checks).  From them
come every fault alone, every fault with B == 0, and every pair of faults of two consecutive checks, which records precedence.

tests/golden/cabi_fault_matrix.json holds the answers.  It was written by `python tests/test_cabi_fault_matrix.py --regenerate`
from the library as it was BEFORE the host layer's checks were gathered into one copy each; regenerate it only for a deliberate
change of a message, a code or the order of two checks.  Regenerate on a machine without a GPU: the writer refuses every answer
that is not CTC_AMD_EINVAL, CTC_AMD_EWORKSPACE, or CTC_AMD_OK from a size query or a B == 0 call, and there a stray launch is a
harmless error code."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX_PATH = os.path.join(ROOT, "tests", "golden", "cabi_fault_matrix.json")
OK, EINVAL, EWORKSPACE = 0, -1, -2
P, Q = 16, 32  # two non-null, 16-byte aligned, never dereferenced addresses
MAX_U, LONG_MAX_U, MAX_V, NBEST_MAX, PREFIX_MAX, BEAM_MAX_WIDTH, BEAM_MAX_TOP_K = 1024, 65536, 16384, 64, 64, 64, 32
EDIT_MAX_STRIDE, EDIT_COUNTS_MAX_STRIDE = 2147479552, 1048576
B_MAX = 65535 * 32767  # the common check's "B too large"
HUGE = 1 << 40         # a buffer size that suffices for every shape here (its pointer is never followed: a later check fails)
OUT = "out"            # a size query's result pointer: the test passes a size_t of its own


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_seq2seq_losses_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------
# the baseline call: every argument any entry point takes, by name; xsb .. gst default to a contiguous [B, T, V] tensor

BASE = dict(kind=0, wrt=0, logits=P, xdtype=0, xsb=None, xst=None, labels=P, label_stride=4, label_length=P, logit_length=P, blank=0,
            weight=-1.0, B=2, T=5, V=8, U=4, N=2, tf=0, want_grad=1, beam_width=4, top_k=4, nbest=2,
            loss=P, grad=P, gdtype=0, gsb=None, gst=None, d_loss=None, nweight=P, score=P, tokens=P, label_index=P, first_frame=P,
            last_frame=P, label_score=P, decoded=P, decoded_length=P, frames=P, label_posterior=P, blank_posterior=P, duration=None,
            expected_frame=None, peak_posterior=None, peak_frame=None, ws=None, ws_bytes=0, stream=None,
            hyp=P, hyp_stride=4, hyp_length=P, ref=P, ref_stride=4, ref_length=P, R=4, rows_per_tile=0, distance=P, counts=P,
            rows=P, rows_bytes=HUGE, state_in=None, last_in=None, length_in=None, parent=P, token=P, state_out=Q, state_bytes=0,
            last_out=P, length_out=P, full_score=P, state=P, last_token=P, length=P,
            out2=P, dst=P, src=P, nbytes=16, threads=64, lds=0, us=1.0, out=OUT, out_b=OUT)

_EX = "kind wrt logits xdtype xsb xst labels label_stride label_length logit_length blank B T V U"
_WEX = "kind wrt logits xdtype xsb xst labels label_stride label_length logit_length blank weight B T V U"
_FREE = "kind wrt logits xdtype xsb xst logit_length blank B T V"  # the label-free entries
_GRAD = "loss grad gdtype gsb gst"
_WS = "ws ws_bytes stream"
ARGS = {
    "best_path": f"{_EX} score tokens label_index {_WS}",
    "greedy_decode": f"{_FREE} score tokens decoded decoded_length frames label_score {_WS}",
    "beam_search": f"{_FREE} beam_width top_k nbest score decoded decoded_length {_WS}",
    "nbest_loss": f"{_EX} N loss {_WS}",
    "nbest_loss_grad": f"{_EX} N nweight {_GRAD} {_WS}",
    "nbest_best_path": f"{_EX} N score tokens label_index first_frame last_frame {_WS}",
    "wildcard_best_path": f"{_EX} score tokens label_index first_frame last_frame label_score {_WS}",
    "long_best_path": f"{_EX} tf score tokens label_index first_frame last_frame {_WS}",
    "long_wildcard_best_path": f"{_EX} tf score tokens label_index first_frame last_frame label_score {_WS}",
    "wildcard_loss_grad": f"{_WEX} d_loss {_GRAD} {_WS}",
    "long_wildcard_loss_grad": f"{_WEX} tf d_loss {_GRAD} {_WS}",
    "long_wildcard_loss_grad_ckpt": f"{_WEX} tf d_loss {_GRAD} {_WS}",
    "label_posterior": f"{_WEX} loss label_posterior blank_posterior duration expected_frame {_WS}",
    "long_label_posterior": f"{_WEX} tf loss label_posterior blank_posterior duration expected_frame peak_posterior peak_frame {_WS}",
    "edit_distance": f"hyp hyp_stride hyp_length ref ref_stride ref_length B N R distance {_WS}",
    "edit_counts": f"hyp hyp_stride hyp_length ref ref_stride ref_length B N R rows_per_tile counts {_WS}",
    "prefix_rows": "logits xdtype xsb xst logit_length B T V rows rows_bytes stream",
    "prefix_extend": f"{_FREE} N rows rows_bytes state_in last_in length_in parent token state_out state_bytes last_out length_out "
                     "full_score stream",
    "prefix_score": f"{_FREE} N rows rows_bytes state state_bytes last_token length score stream",
    "reduce_loss": "loss B out2 stream",
    "probe_copy": "dst src nbytes stream",
    "probe_spin": "threads lds us stream",
    "check_labels": "labels label_stride label_length blank B V U stream",
    # the size queries
    "best_path_workspace_bytes": "kind B T V U out",
    "greedy_decode_workspace_bytes": "B T out",
    "beam_search_workspace_bytes": "B T V beam_width top_k out",
    "nbest_loss_workspace_bytes": "kind B T V U N out",
    "nbest_loss_grad_workspace_bytes": "kind B T V U N out",
    "nbest_best_path_workspace_bytes": "kind B T V U N out",
    "wildcard_best_path_workspace_bytes": "kind B T V U out",
    "long_best_path_workspace_bytes": "kind B T V U tf out",
    "long_wildcard_best_path_workspace_bytes": "kind B T V U tf out",
    "wildcard_loss_workspace_bytes": "kind B T V U want_grad out",
    "long_wildcard_loss_workspace_bytes": "kind B T V U tf want_grad out",
    "long_wildcard_loss_ckpt_workspace_bytes": "kind B T V U tf want_grad out",
    "label_posterior_workspace_bytes": "kind B T V U out",
    "long_label_posterior_workspace_bytes": "kind B T V U tf out",
    "edit_distance_workspace_bytes": "B N R out",
    "edit_counts_workspace_bytes": "B N R hyp_stride rows_per_tile out",
    "prefix_workspace_bytes": "B T V N out out_b",
}
QUERIES = tuple(e for e in ARGS if e.endswith("_workspace_bytes"))


def call(lib, entry, over):
    """(code, message) of a rejected call, (OK, None) of an accepted one, (OK, [sizes]) of an answered size query."""
    names = ARGS[entry].split()
    unknown = set(over) - set(names)
    assert not unknown, (entry, unknown)
    a = dict(BASE, **over)
    rows = max(a["T"], 1) * a["V"]
    for k, dflt in (("xsb", rows), ("xst", a["V"]), ("gsb", rows), ("gst", a["V"])):
        if a[k] is None:
            a[k] = dflt
    outs = [ctypes.c_size_t(0) for n in names if a[n] == OUT]
    it = iter(outs)
    rc = getattr(lib, "ctc_amd_" + entry)(*(ctypes.byref(next(it)) if a[n] == OUT else a[n] for n in names))
    if rc != OK:
        return rc, lib.ctc_amd_last_error().decode()
    return rc, [int(o.value) for o in outs] if entry in QUERIES else None


# ---------------------------------------------------------------------------------------------------------------------------
# the overrides.  `checks`: one fault per check in today's order, EMPTY where B == 0 answers OK; `more`: further cases;
# `stops`: the baseline itself is rejected (no workspace), so single valid values may be tried too.

EMPTY = "B == 0"
XD, GD, XST, GST = dict(xdtype=3), dict(gdtype=3), dict(xst=7), dict(gst=7)
V_OVER = dict(V=MAX_V + 1)
GRID4, GRID16 = dict(B=2 ** 20, T=2 ** 14), dict(B=2 ** 20, T=2 ** 15)  # B * T rows beyond 2^31 - 1 workgroups of 4 / of 16 rows
PAIRS_OVER = dict(B=2 ** 26, N=64)                                       # B * N beyond 2^31 - 1
WEIGHT = dict(weight=1.0)
TF = dict(tf=2)


def common(max_u=MAX_U, labelled=True):
    """check_common, in its order."""
    if labelled:
        return [dict(kind=5), dict(wrt=2), dict(T=-1), dict(blank=99), dict(U=max_u + 1), dict(label_length=None), dict(logits=None),
                dict(labels=None), dict(B=B_MAX + 1)]
    return [dict(kind=5), dict(wrt=2), dict(T=-1), dict(blank=99), dict(logit_length=None), dict(logits=None), dict(B=B_MAX + 1)]


COMMON_MORE = [dict(kind=-1), dict(wrt=-1), dict(B=-1), dict(V=0), dict(blank=-1), dict(blank=8), dict(logit_length=None), dict(xdtype=-1),
               dict(xsb=7), dict(xst=0), dict(xsb=-8)]
T0 = dict(T=0, logits=None)  # no frames, no logits (only where the workspace is still needed then)
LABEL_MORE = [dict(U=-1), dict(label_stride=-1), dict(label_stride=0, labels=None)]
GRAD_MORE = [dict(gdtype=-1), dict(gsb=7), dict(gst=0)]
WS_MORE = [dict(ws=P, ws_bytes=1), dict(ws_bytes=HUGE), dict(kind=1, wrt=1)]  # (a null workspace of any size is refused: the needs here are > 0)
WEIGHT_MORE = [dict(weight=float("nan")), dict(weight=float("-inf")), dict(weight=float("inf")), dict(weight=0.0)]
TF_MORE = [dict(tf=-4), dict(tf=6), dict(tf=4), dict(tf=128), dict(B=2 ** 30, T=1024, U=65536, tf=4), dict(B=2 ** 30, T=1024, U=65536, tf=4, V=MAX_V + 1)]
N_MORE = [dict(N=NBEST_MAX + 1), dict(N=-4), dict(N=NBEST_MAX + 1, B=2 ** 26)]
LONG_U = [dict(U=MAX_U + 1), dict(U=LONG_MAX_U)]

ENTRIES = {
    "best_path": dict(stops=True, checks=[*common(), XD, EMPTY, XST, dict(score=None), V_OVER],
                      more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, dict(tokens=None), dict(T=0, tokens=None), dict(label_index=None), dict(V=MAX_V)]),
    "greedy_decode": dict(stops=True, checks=[*common(labelled=False), XD, EMPTY, XST, dict(score=None), GRID16],
                          more=[*COMMON_MORE, *WS_MORE, dict(decoded_length=None), dict(tokens=None), dict(decoded=None), dict(frames=None, label_score=None),
                                V_OVER, GRID4]),
    "beam_search": dict(stops=True, checks=[*common(labelled=False), XD, EMPTY, XST, V_OVER, dict(beam_width=0), dict(top_k=0), dict(nbest=0),
                                            dict(score=None), GRID16, dict(beam_width=64, T=2 ** 25)],
                        more=[T0, *COMMON_MORE, *WS_MORE, dict(beam_width=BEAM_MAX_WIDTH + 1), dict(beam_width=-4), dict(beam_width=2), dict(top_k=BEAM_MAX_TOP_K + 1),
                              dict(top_k=-4), dict(top_k=2), dict(nbest=5), dict(nbest=-4), dict(nbest=4), dict(beam_width=2, nbest=2, top_k=2),
                              dict(decoded=None), dict(decoded_length=None), dict(V=MAX_V), dict(B=2 ** 20, T=2 ** 25, beam_width=64)]),
    "nbest_loss": dict(stops=False, checks=[*common(), XD, EMPTY, XST, V_OVER, dict(N=0), PAIRS_OVER, dict(loss=None)],
                       more=[*COMMON_MORE, *LABEL_MORE[:2], *N_MORE]),  # (needs no workspace: only with a fault)
    "nbest_loss_grad": dict(stops=True, checks=[*common(), XD, EMPTY, XST, V_OVER, dict(N=0), PAIRS_OVER, dict(nweight=None), GRID4],
                            more=[T0, *COMMON_MORE, *LABEL_MORE, *GRAD_MORE, *WS_MORE, *N_MORE, GD, GST, dict(loss=None), dict(grad=None), dict(N=NBEST_MAX)]),
    "nbest_best_path": dict(stops=True, checks=[*common(), XD, EMPTY, XST, V_OVER, dict(N=0), PAIRS_OVER, dict(score=None)],
                            more=[*COMMON_MORE, *LABEL_MORE, *WS_MORE, *N_MORE, dict(tokens=None), dict(first_frame=None, last_frame=None)]),
    "wildcard_best_path": dict(stops=True, checks=[*common(), XD, EMPTY, XST, dict(score=None), V_OVER],
                               more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, dict(tokens=None), dict(label_score=None, first_frame=None)]),
    "long_best_path": dict(stops=True, checks=[*common(LONG_MAX_U), XD, EMPTY, XST, dict(score=None), V_OVER, TF],
                           more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, *TF_MORE, *LONG_U, dict(tokens=None)]),
    "long_wildcard_best_path": dict(stops=True, checks=[*common(LONG_MAX_U), XD, EMPTY, XST, dict(score=None), V_OVER, TF],
                                    more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, *TF_MORE, *LONG_U, dict(tokens=None), dict(label_score=None)]),
    "wildcard_loss_grad": dict(stops=True, checks=[*common(), XD, EMPTY, XST, WEIGHT, dict(loss=None), V_OVER, GRID4],
                               more=[*COMMON_MORE, *LABEL_MORE, *GRAD_MORE, *WS_MORE, *WEIGHT_MORE, GD, GST, dict(d_loss=P),
                                     # (without a gradient it needs no workspace: only with a fault)
                                     dict(grad=None, loss=None), dict(grad=None, gst=7, loss=None), dict(grad=None, gdtype=3), dict(grad=None, B=2 ** 20, T=2 ** 14, V=MAX_V + 1)]),
    "long_wildcard_loss_grad": dict(stops=True, checks=[*common(LONG_MAX_U), XD, EMPTY, XST, WEIGHT, dict(loss=None), V_OVER, GRID4, TF],
                                    more=[T0, *COMMON_MORE, *LABEL_MORE, *GRAD_MORE, *WS_MORE, *WEIGHT_MORE, *TF_MORE, *LONG_U, GD, GST, dict(grad=None),
                                          dict(grad=None, gst=7), dict(grad=None, B=2 ** 20, T=2 ** 14, tf=3)]),
    "long_wildcard_loss_grad_ckpt": dict(stops=True, checks=[*common(LONG_MAX_U), XD, EMPTY, XST, WEIGHT, dict(loss=None), V_OVER, GRID4, TF],
                                         more=[T0, *COMMON_MORE, *LABEL_MORE, *GRAD_MORE, *WS_MORE, *WEIGHT_MORE, *TF_MORE, *LONG_U, GD, GST, dict(grad=None),
                                               dict(grad=None, gst=7), dict(grad=None, B=2 ** 20, T=2 ** 14, tf=3)]),
    "label_posterior": dict(stops=True, checks=[*common(), XD, EMPTY, XST, WEIGHT, dict(loss=None), dict(duration=P), V_OVER],
                            more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, *WEIGHT_MORE, dict(label_posterior=None), dict(blank_posterior=None),
                                  dict(U=0, label_posterior=None), dict(T=0, label_posterior=None, blank_posterior=None), dict(expected_frame=P),
                                  dict(duration=P, expected_frame=P), GRID4]),
    "long_label_posterior": dict(stops=True, checks=[*common(LONG_MAX_U), XD, EMPTY, XST, WEIGHT, dict(loss=None), V_OVER, GRID4, dict(blank_posterior=None),
                                                     dict(duration=P), dict(peak_posterior=P), TF],
                                 more=[T0, *COMMON_MORE, *LABEL_MORE, *WS_MORE, *WEIGHT_MORE, *TF_MORE, *LONG_U, dict(label_posterior=None), dict(expected_frame=P),
                                       dict(peak_frame=P), dict(duration=P, expected_frame=P, peak_posterior=P, peak_frame=P), dict(T=0, blank_posterior=None)]),
    "edit_distance": dict(stops=False, checks=[dict(R=-1), dict(R=MAX_U + 1), EMPTY, dict(N=0), PAIRS_OVER, dict(hyp_stride=-4), dict(hyp_stride=EDIT_MAX_STRIDE + 1),
                                               dict(hyp_length=None), dict(hyp=None), dict(ref=None), dict(distance=None)],
                          more=[dict(B=-1), dict(N=-4), dict(ref_stride=-4), dict(ref_length=None), dict(hyp_stride=2, hyp=None), dict(ref_stride=0, ref=None, distance=None),
                                dict(hyp_stride=0, hyp=None, ref=None), dict(B=-1, R=MAX_U + 1)]),
    "edit_counts": dict(stops=True, checks=[dict(R=-1), dict(R=LONG_MAX_U + 1), EMPTY, dict(N=0), PAIRS_OVER, dict(ref_stride=-4), dict(hyp_stride=EDIT_COUNTS_MAX_STRIDE + 1),
                                            dict(rows_per_tile=2), dict(B=2 ** 24, N=64, R=65536, hyp_stride=2 ** 20), dict(hyp_length=None), dict(hyp=None), dict(ref=None),
                                            dict(counts=None)],
                        more=[*WS_MORE[:2], dict(B=-1), dict(N=-4), dict(hyp_stride=-4), dict(hyp_stride=2), dict(rows_per_tile=-4), dict(rows_per_tile=64),
                              dict(rows_per_tile=-64), dict(ref_length=None), dict(hyp_stride=0, hyp=None), dict(R=MAX_U + 1), dict(R=LONG_MAX_U),
                              dict(hyp_stride=-4, rows_per_tile=2), dict(B=-1, R=LONG_MAX_U + 1)]),
    "prefix_rows": dict(stops=True, checks=[dict(T=-1), dict(logit_length=None), dict(logits=None), dict(B=B_MAX + 1), XD, EMPTY, XST, V_OVER, GRID4],
                        base=dict(rows_bytes=0),
                        more=[dict(B=-1), dict(V=0), dict(xdtype=-1), dict(xsb=7), dict(xst=0), dict(rows=None), dict(rows=None, rows_bytes=HUGE), dict(rows_bytes=1)]),
    "prefix_extend": dict(stops=True, checks=[*common(labelled=False), XD, EMPTY, XST, V_OVER, dict(N=0), PAIRS_OVER, dict(rows=None), dict(rows_bytes=0), dict(parent=None),
                                              dict(state_in=P, last_in=None), dict(state_in=Q)],
                          more=[*COMMON_MORE, dict(N=PREFIX_MAX + 1), dict(N=-4), dict(N=PREFIX_MAX + 1, B=2 ** 26), dict(wrt=1, rows=None), dict(wrt=1, rows_bytes=0),
                                dict(token=None), dict(state_out=None), dict(last_out=None), dict(length_out=None), dict(full_score=None),
                                dict(state_in=P, last_in=P, length_in=None), dict(state_in=P, last_in=P, length_in=P), dict(state_in=Q, last_in=P, length_in=P),
                                dict(state_bytes=1), dict(rows_bytes=1)]),
    "prefix_score": dict(stops=True, checks=[*common(labelled=False), XD, EMPTY, XST, V_OVER, dict(N=0), PAIRS_OVER, dict(rows=None), dict(rows_bytes=0), dict(state=None)],
                         more=[*COMMON_MORE, dict(N=PREFIX_MAX + 1), dict(N=-4), dict(wrt=1, rows=None), dict(wrt=1, rows_bytes=0), dict(last_token=None),
                               dict(length=None), dict(score=None), dict(state_bytes=1), dict(rows_bytes=1)]),
    # no workspace, no B == 0 answer before a launch (ctc_amd_check_labels has one): documented faults only
    "reduce_loss": dict(stops=False, empty=False, checks=[], more=[dict(B=-1), dict(out2=None), dict(loss=None), dict(B=0, out2=None), dict(B=-1, out2=None, loss=None)]),
    "probe_copy": dict(stops=False, checks=[], more=[dict(dst=None), dict(src=None), dict(nbytes=8), dict(dst=20), dict(src=20), dict(dst=None, nbytes=8)]),
    "probe_spin": dict(stops=False, checks=[], more=[dict(threads=0), dict(threads=32), dict(threads=100), dict(threads=2048), dict(lds=-1), dict(lds=65537),
                                                     dict(us=-1.0), dict(us=float("nan")), dict(us=1001.0)]),
    "check_labels": dict(stops=False, checks=[dict(U=-1), EMPTY, dict(labels=None)],
                         more=[dict(B=-1), dict(V=0), dict(label_stride=-1), dict(label_stride=0), dict(label_stride=0, labels=None, label_length=None),
                               dict(label_length=None)]),
}

# the size queries: null result, the shape guard with its limit on U, the vocabulary limit, then what only the query takes
SHAPE = [dict(kind=2), dict(B=-1), dict(T=-1), dict(V=0), dict(U=-1)]
GRID = [dict(kind=k, B=B, T=T, U=U) for k in (0, 1) for B in (0, 1, 3) for T in (0, 1, 130) for U in (0, 1, 300, MAX_U)]
LONG_GRID = [dict(kind=k, B=B, T=T, U=U, tf=tf) for k in (0, 1) for B in (0, 3) for T in (0, 1, 130) for U in (0, 300, MAX_U + 1, 3000) for tf in (0, 4, 64)]
WG = [dict(want_grad=0), dict(want_grad=7)]
TF_Q = [dict(tf=-4), dict(tf=6), dict(tf=4), dict(B=2 ** 30, T=1024, U=65536, tf=4)]


def _with(cases, *extra):
    return [dict(c, **e) for c in cases for e in extra]


QUERY_CASES = {
    "best_path_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER], more=[*SHAPE, *GRID]),
    "greedy_decode_workspace_bytes": dict(checks=[dict(out=None), dict(T=-1)], more=[dict(B=-1), *(dict(B=B, T=T) for B in (0, 1, 3) for T in (0, 1, 130))]),
    "beam_search_workspace_bytes": dict(checks=[dict(out=None), dict(T=-1), V_OVER, dict(beam_width=0), dict(top_k=0)],
                                        more=[dict(B=-1), dict(V=0), dict(beam_width=BEAM_MAX_WIDTH + 1), dict(beam_width=-4), dict(beam_width=2), dict(top_k=BEAM_MAX_TOP_K + 1),
                                              dict(top_k=-4), dict(top_k=2), *(dict(B=B, T=T, beam_width=W, top_k=K) for B in (0, 3) for T in (0, 130) for W in (1, 64) for K in (1, 32))]),
    "nbest_loss_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER, dict(N=0), PAIRS_OVER], more=[*SHAPE, *N_MORE, *GRID, *_with(GRID[:24], dict(N=9))]),
    "nbest_loss_grad_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER, dict(N=0), PAIRS_OVER], more=[*SHAPE, *N_MORE, *GRID, *_with(GRID[:24], dict(N=9))]),
    "nbest_best_path_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER, dict(N=0), PAIRS_OVER], more=[*SHAPE, *N_MORE, *GRID, *_with(GRID[:24], dict(N=9))]),
    "wildcard_best_path_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER], more=[*SHAPE, *GRID]),
    "long_best_path_workspace_bytes": dict(checks=[dict(out=None), dict(U=LONG_MAX_U + 1), V_OVER, TF], more=[*SHAPE, *TF_Q, *LONG_GRID]),
    "long_wildcard_best_path_workspace_bytes": dict(checks=[dict(out=None), dict(U=LONG_MAX_U + 1), V_OVER, TF], more=[*SHAPE, *TF_Q, *LONG_GRID]),
    "wildcard_loss_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER], more=[*SHAPE, *GRID, *_with(GRID, *WG)]),
    "long_wildcard_loss_workspace_bytes": dict(checks=[dict(out=None), dict(U=LONG_MAX_U + 1), V_OVER, TF],
                                               more=[*SHAPE, *TF_Q, *LONG_GRID, *_with(LONG_GRID, *WG), dict(B=2 ** 20, T=2 ** 14), dict(B=2 ** 20, T=2 ** 13, want_grad=0)]),
    "long_wildcard_loss_ckpt_workspace_bytes": dict(checks=[dict(out=None), dict(U=LONG_MAX_U + 1), V_OVER, TF],
                                                    more=[*SHAPE, *TF_Q, *LONG_GRID, *_with(LONG_GRID, *WG), dict(B=2 ** 20, T=2 ** 14), dict(B=2 ** 20, T=2 ** 13, want_grad=0)]),
    "label_posterior_workspace_bytes": dict(checks=[dict(out=None), dict(U=MAX_U + 1), V_OVER], more=[*SHAPE, *GRID]),
    "long_label_posterior_workspace_bytes": dict(checks=[dict(out=None), dict(U=LONG_MAX_U + 1), V_OVER, TF], more=[*SHAPE, *TF_Q, *LONG_GRID, dict(B=2 ** 20, T=2 ** 14)]),
    "edit_distance_workspace_bytes": dict(checks=[dict(out=None), dict(R=-1), dict(R=MAX_U + 1), dict(N=0), PAIRS_OVER],
                                          more=[dict(B=-1), dict(N=-4), dict(B=0), dict(B=0, N=0), dict(R=0), dict(R=MAX_U)]),
    "edit_counts_workspace_bytes": dict(checks=[dict(out=None), dict(R=-1), dict(R=LONG_MAX_U + 1), dict(N=0), PAIRS_OVER, dict(hyp_stride=-4),
                                                dict(hyp_stride=EDIT_COUNTS_MAX_STRIDE + 1), dict(rows_per_tile=2), dict(B=2 ** 24, N=64, R=65536, hyp_stride=2 ** 20)],
                                        more=[dict(B=-1), dict(N=-4), dict(hyp_stride=2), dict(rows_per_tile=-4), dict(rows_per_tile=-64), dict(B=0, N=0),
                                              *(dict(B=B, N=N, R=R, hyp_stride=s, rows_per_tile=rt) for B in (0, 3) for N in (1, 5) for R in (0, 4, 1025, 65536) for s in (0, 70, 3001)
                                                for rt in (0, 64))]),
    "prefix_workspace_bytes": dict(checks=[dict(out=None), dict(T=-1), V_OVER, dict(N=0), PAIRS_OVER],
                                   more=[dict(out_b=None), dict(B=-1), dict(V=0), dict(N=PREFIX_MAX + 1), dict(N=-4), *(dict(B=B, T=T, N=N) for B in (0, 1, 3) for T in (0, 1, 130) for N in (1, 9, 64))]),
}


def cases_of(entry):
    """Every override of one entry point, in a fixed order and without repeats."""
    spec = ENTRIES.get(entry) or dict(QUERY_CASES[entry], stops=True, query=True)
    base, faults = spec.get("base", {}), [c for c in spec["checks"] if c != EMPTY]
    takes_b = "B" in ARGS[entry].split()
    out = [{}] if spec["stops"] else []
    out += faults + spec["more"]
    if takes_b and not spec.get("query") and spec.get("empty", True):
        out += [dict(B=0)] + [dict(c, B=0) for c in faults + spec["more"]]
        if "ws" in ARGS[entry].split():  # B == 0: nothing to do, whatever else is null
            out.append({n: (0 if n == "B" else None) for n in ARGS[entry].split() if n == "B" or BASE[n] in (P, Q)})
    for a, b in zip(faults, faults[1:]):  # two consecutive checks fail together: the earlier one is reported
        if not set(a) & set(b):
            out.append(dict(a, **b))
    seen, unique = set(), []
    for c in out:
        c = dict(base, **c)
        k = key(c)
        if k not in seen:
            seen.add(k)
            unique.append(c)
    return unique


def key(over):
    return json.dumps(over, sort_keys=True)


def documented(entry, over, rc):
    """What may be recorded: a rejection, a size query's answer, B == 0 (ctc_amd_check_labels: or no labels) answered with OK."""
    if rc in (EINVAL, EWORKSPACE):
        return True
    empty = over.get("B") == 0 or (entry == "check_labels" and over.get("label_stride") == 0)
    return rc == OK and (entry in QUERIES or (empty and entry not in ("reduce_loss", "probe_copy", "probe_spin")))


def matrix(lib):
    """{"messages": [...], "answers": {entry: {key: [code, message index | sizes | null]}}}; refuses a case that is none for this table."""
    messages, answers, refused = [], {}, []
    for entry in ARGS:
        rows = answers[entry] = {}
        for over in cases_of(entry):
            rc, what = call(lib, entry, over)
            if not documented(entry, over, rc):
                refused.append(f"ctc_amd_{entry}{over} returned {rc} ({what!r})")
            if isinstance(what, str):
                if what not in messages:
                    messages.append(what)
                what = messages.index(what)
            rows[key(over)] = [rc, what]
    assert not refused, "not cases for this table (no rejection, size answer or empty batch):\n" + "\n".join(refused)
    return dict(messages=messages, answers=answers)


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(MATRIX_PATH))


@pytest.mark.parametrize("entry", list(ARGS))
def test_answers_match_the_recorded_ones(lib, recorded, entry):
    want = recorded["answers"][entry]
    cases = cases_of(entry)
    assert [key(c) for c in cases] == list(want), "the tables and the fixture differ: regenerate only from the library they were written for"
    for over in cases:
        rc, what = call(lib, entry, over)
        w_rc, w_what = want[key(over)]
        if w_rc != OK:
            w_what = recorded["messages"][w_what]
        assert (rc, what) == (w_rc, w_what), f"ctc_amd_{entry}{over}: ({rc}, {what!r}), recorded ({w_rc}, {w_what!r})"


def test_the_fixture_holds_only_documented_answers(recorded):
    """The fixture holds rejections, size answers and empty batches only, every entry point has its cases, and the limits one step
    outside their range are among them."""
    assert sorted(recorded["answers"]) == sorted(ARGS)
    n = 0
    for entry, rows in recorded["answers"].items():
        assert rows, entry
        for k, (rc, what) in rows.items():
            assert documented(entry, json.loads(k), rc), (entry, k, rc)
            assert rc == OK or 0 <= what < len(recorded["messages"])
            n += 1
        codes = {rc for rc, _ in rows.values()}
        assert EINVAL in codes, entry
        if entry in ENTRIES and ENTRIES[entry]["stops"]:
            assert EWORKSPACE in codes and rows[key(ENTRIES[entry].get("base", {}))][0] == EWORKSPACE, entry
    assert n > 3000 and os.path.getsize(MATRIX_PATH) < 1 << 20
    text = "\n".join(recorded["messages"])
    for literal in ("wildcard_log_weight must be finite", "is neither 0 nor a positive multiple of 4, or B", "rows exceed the launch grid", "bad kind or shape",
                    "out_bytes is null", "workspace too small: 0 < ", "exceeds the supported maximum 16384", "U=1025 exceeds", "U=65537 exceeds", "state_out must not be state_in"):
        assert literal in text, literal


if __name__ == "__main__":
    assert sys.argv[1:] == ["--regenerate"], "usage: python tests/test_cabi_fault_matrix.py --regenerate"
    sys.path.insert(0, ROOT)
    from tf_seq2seq_losses_amd import _lib
    m = matrix(_lib.load())
    with open(MATRIX_PATH, "w") as f:
        f.write('{\n"messages": [\n' + ",\n".join(json.dumps(s) for s in m["messages"]) + '\n],\n"answers": {\n' +
                ",\n".join(json.dumps(e) + ": {\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in rows.items()) + "\n}"
                           for e, rows in m["answers"].items()) + "\n}\n}\n")
    print("wrote", MATRIX_PATH, sum(len(r) for r in m["answers"].values()), "cases,", len(m["messages"]), "messages")
