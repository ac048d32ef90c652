"""Ownership invariance: memory an utterance does not own cannot change any result.

Every case makes a CLEAN run, compared with the float64 oracles at the project's 1e-4 exactly as test_gpu_fused.py /
test_gpu_contract.py do, and PERTURBED runs in which only unowned memory differs: padding frames (NaN, +-inf, 3e38), label tails
(-7, V + 100, the blank, INT32_MIN, INT32_MAX), the bytes of outputs and workspace on entry (0x00, 0xFF, 0xA5, or what a call of
another shape and lattice left there), the batch position and the neighbours, the gaps of strided and packed storage.  Perturbed
runs are compared with the clean one BY THEIR BITS; there is no closeness tolerance in this file besides TOL for the oracle.

One exception (test_log_domain_hvp_with_repeats_against_the_oracle): the log-domain Hessian-vector pipeline scatters tangents with
a float LDS atomicAdd (csrc/ctc_hvp_device.h), so with a token that occurs twice in a label the order of two adds is not specified.
Its bitwise cases draw each utterance's labels without replacement; every other tier uses integer atomics and gets repeats.

Every figure is printed before it is asserted (pytest -s): the clean run's oracle error, the number of differing elements, the
flag words."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import ctc_oracle as O
from tests import _ownership as W
from tests.test_gpu_alignment import check_against_oracle
from tests.test_gpu_greedy_decode import check as check_decoding
from tests.tools import greedy_oracle as GO
from tests.tools import viterbi_oracle as VO

pytestmark = pytest.mark.gpu
TOL = 1e-4
KINDS = W.KINDS
KIND_ID = {"classic": 0, "simplified": 1}
# loss + gradient cases and the pipeline a float32 call of theirs selects by default
LG_CASES = {"lg_nl1": "fused6", "lg_nl2": "fused6", "lg_nl4": "fused6", "lg_seg4": "fused6", "lg_nl8": "fused6", "lg_wide": "v1"}


def PERM(B):
    """A fixed permutation that is not the identity (B = 3: a rotation, so that every row moves)."""
    return [1, 2, 0] if B == 3 else list(range(B))[::-1]


@contextlib.contextmanager
def override(key, value):
    from tf_seq2seq_losses_amd import _lib
    _lib.debug_override(key, value)
    try:
        yield
    finally:
        _lib.debug_override(key, "")


def _tiers(name, kind):
    """The loss + gradient tiers that take this shape, after asserting which one is the default."""
    from tf_seq2seq_losses_amd import _lib
    c = W.case(name)
    got = _lib.pipeline_name(KIND_ID[kind], 0, *c.shape, True)
    assert got == LG_CASES[name], (name, got)
    return ("", "fused5", "v1") if got == "fused6" else ("",)


def _assert_pipeline(c, kind, tier):
    from tf_seq2seq_losses_amd import _lib
    want = tier if tier else LG_CASES.get(c.name, "v1")
    for want_grad in (True, False):
        got = _lib.pipeline_name(KIND_ID[kind], 0, *c.shape, want_grad)
        assert got == want, (c.name, kind, tier, want_grad, got)
    return want


def _inputs(c, kind, **kw):
    return W.make_inputs(KIND_ID[kind], kw.pop("x", c.logits), kw.pop("labels", c.labels), kw.pop("ll", c.ll), kw.pop("tl", c.tl),
                         U=c.shape[3], **kw)


def _poisoned(inp, c, value, label_values=None):
    """The same call with every padding frame of the logits (and of vec) holding `value` and every label tail poisoned."""
    B, T, V, U = c.shape
    kw = dict(x=W.poison_padding(inp.x, c.tl, value))
    kw["labels"] = W.poison_labels(inp.labels, c.ll, label_values or W.label_poison_cycle(V, inp.blank))
    if hasattr(inp, "vec"):
        kw["vec"] = W.poison_padding(inp.vec, c.tl, value)
    return inp.replace(**kw)


def _report(what, diff):
    total = sum(diff.values())
    print(f"OWNERSHIP {what}: {total} differing elements {diff if total else ''}", flush=True)
    assert total == 0, (what, diff)


def _no_prefill_left(out, fill, what):
    """0xA5 is no value any output takes (-2.9e-16 as float32, a negative 10-digit integer); 0xFF is a NaN as float."""
    for name, t in out.items():
        if fill == 0xA5:
            kept = int(W.keeps_prefill(t, fill).sum().item())
            assert kept == 0, (what, name, f"{kept} elements keep the 0xA5 prefill")
        if fill == 0xFF and t.is_floating_point():
            assert not bool(torch.isnan(t).any()), (what, name, "NaN left from the 0xFF prefill")


# ---- references (float64 oracles on the clean arrays, computed once) ----

@functools.lru_cache(maxsize=None)
def _ref_lg(name, kind, dtype=None):
    c = W.case(name)
    x = c.logits if dtype is None else torch.tensor(c.logits).to(dtype).float().numpy()
    loss, grad = C.loss_grad(kind, c.labels, x, c.ll, c.tl, 0)
    loss.flags.writeable = grad.flags.writeable = False
    return loss, grad


@functools.lru_cache(maxsize=None)
def _ref_data(name, kind):
    """The NumPy oracle's loss data of the feasible rows (the others are +inf / exactly zero by contract): (rows, data, logits)."""
    c = W.case(name)
    g = np.nonzero(W.feasible_rows(c, kind))[0]
    return g, O.ctc_loss(kind, c.labels[g], c.logits[g], c.ll[g], c.tl[g], 0), c.logits[g]


@functools.lru_cache(maxsize=None)
def _ref_hessian(name, kind):
    g, data, x = _ref_data(name, kind)
    return O.logits_hessian(data, x)


def _check_loss(c, kind, loss, ref_loss, what):
    got = loss.cpu().numpy().astype(np.float64)
    feas = W.feasible_rows(c, kind)
    assert np.array_equal(np.isfinite(ref_loss), feas), (what, ref_loss)
    assert np.all(got[~feas] == np.inf), (what, got)
    assert np.array_equal(np.isfinite(got), feas), (what, got, ref_loss)
    err = (np.abs(got[feas] - ref_loss[feas]) / np.maximum(1, np.abs(ref_loss[feas]))).max()
    print(f"OWNERSHIP {what}: clean loss error {err:.3e}", flush=True)
    assert err < TOL, (what, err)


def _check_abs(got, ref, what):
    got = got.float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref).max()
    print(f"OWNERSHIP {what}: clean error {err:.3e}", flush=True)
    assert err < TOL, (what, err)


def _check_lg_clean(c, kind, out, what, dtype=None):
    rl, rg = _ref_lg(c.name, kind, dtype)
    for key in ("loss", "loss_forward"):
        if key in out:
            _check_loss(c, kind, out[key], rl, f"{what} {key}")
    if "grad" in out and out["grad"].dtype == torch.float32:
        _check_abs(out["grad"], rg, f"{what} gradient")
    elif "grad" in out:  # one rounding to the element type on top: half an ulp, eps / 2 relative (subnormal steps are far below TOL)
        g = out["grad"].float().cpu().numpy().astype(np.float64)
        excess = (np.abs(g - rg) - 0.5 * torch.finfo(out["grad"].dtype).eps * np.abs(rg)).max()
        print(f"OWNERSHIP {what}: clean gradient error beyond the rounding of {out['grad'].dtype} {excess:.3e}", flush=True)
        assert np.isfinite(g).all() and excess < TOL, (what, excess)
    if "sum2" in out:
        fin = np.isfinite(rl)
        s = out["sum2"].cpu().numpy()
        err = abs(s[0] * 2.0 ** -20 - rl[fin].sum()) / max(1.0, abs(rl[fin].sum()))
        print(f"OWNERSHIP {what}: sum2 = {s.tolist()}, error of the sum {err:.3e}", flush=True)
        assert s[1] == fin.sum() and err < TOL, (what, s, rl)
        assert out["zero_next"].tolist() == [0, 0], what


# ---- the operations under test: how to run one, and what its padding frames must hold ----

class Op:
    """run(inp, fill, ws) -> namespace(out, ws); pad(out, mask[B, T]) asserts the contractual values of the padding frames;
    flags(inp, run) -> the fused kernel's flag words or None; ws_bytes(inp)."""

    def __init__(self, label, run, pad, ws_bytes, flags=None):
        self.label, self.run, self.pad, self.ws_bytes, self.flags = label, run, pad, ws_bytes, flags or (lambda i, r: None)


def _pad_zero(*names):
    def pad(out, mask, what):
        for n in names:
            if n in out:
                t = out[n]
                assert bool((t[mask] == 0).all()), (what, n, "padding frames are not exactly 0")
                if t.dim() == 5:  # the Hessian: columns too
                    assert bool((t.permute(0, 3, 4, 1, 2)[mask] == 0).all()), (what, n, "padding columns are not exactly 0")
    return pad


def _lg_flags(tier):
    def flags(inp, run):
        from tf_seq2seq_losses_amd import _lib
        if tier != "" or inp.x.dtype != torch.float32 or LG_CASES.get(getattr(inp, "case_name", ""), "") != "fused6":
            return None
        return W.flag_words(run.ws, _lib.flags_offset(inp.kind, *inp.shape), inp.shape[0])
    return flags


def _lg_ws_bytes(selector=None):
    def n(inp):
        from tf_seq2seq_losses_amd import _lib
        sel = selector
        if sel is None:
            sel = _lib.WS_LOSS_GRAD_LOGITS if inp.x.dtype == torch.float32 else _lib.WS_LOSS_GRAD
        return _lib.workspace_bytes(sel, inp.kind, *inp.shape)
    return n


def lg_op(entry, tier, wrt=0, selector=None):
    return Op(f"{entry}", lambda inp, fill=0xA5, ws=None: W.loss_grad(inp, entry, wrt=wrt, fill=fill, ws=ws, selector=selector),
              _pad_zero("grad"), _lg_ws_bytes(selector), _lg_flags(tier))


def _hvp_flags(inp, run):
    from tf_seq2seq_losses_amd import _lib
    if not getattr(inp, "fused_hvp", False):
        return None
    return W.flag_words(run.ws, _lib.hvp_flags_offset(inp.kind, *inp.shape), inp.shape[0])


def _ws(what):
    def n(inp):
        from tf_seq2seq_losses_amd import _lib
        return _lib.workspace_bytes(what, inp.kind, *inp.shape)
    return n


def _pad_lg(out, mask, what):
    assert bool((out["lg"][mask] == -float("inf")).all()), (what, "log posterior of padding frames is not -inf")


def _pad_align(out, mask, what):
    assert bool((out["tokens"][mask] == -1).all()) and bool((out["label_index"][mask] == -1).all()), (what, "padding frames are not -1")


def _pad_decode(out, mask, what):
    assert bool((out["tokens"][mask] == -1).all()), (what, "tokens of padding frames are not -1")
    B, T = out["tokens"].shape
    beyond = torch.arange(T, device=mask.device)[None, :] >= out["decoded_length"][:, None]
    assert bool((out["decoded"][beyond] == -1).all()) and bool((out["frames"][beyond] == -1).all()), (what, "decoded / frames padding")
    assert bool((out["label_score"][beyond] == -float("inf")).all()), (what, "label_score padding is not -inf")


def _bp_bytes(inp):
    from tf_seq2seq_losses_amd import _lib
    return _lib.best_path_workspace_bytes(inp.kind, *inp.shape)


def _gd_bytes(inp):
    from tf_seq2seq_losses_amd import _lib
    return _lib.greedy_decode_workspace_bytes(inp.shape[0], inp.shape[1])


def _run_hvp(inp, fill=0xA5, ws=None):
    """(the fused kernel serves calls without a gradient only: ctc_amd_hvp with grad == NULL there, with a gradient elsewhere)"""
    return W.hvp(inp, inp.vec, fill=fill, ws=ws, want_grad=not getattr(inp, "fused_hvp", False))


def _ops():
    from tf_seq2seq_losses_amd import _lib
    return {
        "hvp": Op("hvp", _run_hvp, _pad_zero("grad", "hvp"), _ws(_lib.WS_HVP), _hvp_flags),
        "hessian": Op("hessian", W.hessian, _pad_zero("grad", "hess"), _ws(_lib.WS_HESSIAN)),
        "alpha_beta": Op("alpha_beta", W.alpha_beta, lambda o, m, w: None, _ws(_lib.WS_ALPHA_BETA)),
        "log_posterior": Op("log_posterior", W.log_posterior, _pad_lg, _ws(_lib.WS_ALPHA_BETA)),
        "best_path": Op("best_path", W.best_path, _pad_align, _bp_bytes),
        "greedy_decode": Op("greedy_decode", W.greedy_decode, _pad_decode, _gd_bytes),
    }


# ---- the properties ----

def _flags_same(op, inp, clean, run, what):
    f0, f1 = op.flags(inp, clean), op.flags(inp, run)
    if f0 is not None:
        print(f"OWNERSHIP {what}: flag words {f1.tolist()} (clean {f0.tolist()})", flush=True)
        assert torch.equal(f0, f1), (what, f0.tolist(), f1.tolist())
        assert not bool(W.keeps_prefill(f1, 0xA5).any()), (what, "the flag words were not written: another pipeline ran")


def check_padding(op, inp, c, what, clean=None):
    """Property 1 (and 5): poisoned padding frames and label tails change no bit; padding frames hold their contractual values;
    a second clean run is the first one again."""
    mask = W.padding_mask(c.tl, c.shape[1]).to(inp.x.device)
    clean = clean or op.run(inp)
    op.pad(clean.out, mask, what)
    again = op.run(inp)
    _report(f"{what} run-to-run", W.total_diff(clean.out, again.out))
    _flags_same(op, inp, clean, again, f"{what} run-to-run")
    for value in W.poison_values(inp.x.dtype):
        run = op.run(_poisoned(inp, c, value))
        _report(f"{what} padding {value} + label tails", W.total_diff(clean.out, run.out))
        _flags_same(op, inp, clean, run, f"{what} padding {value}")
        op.pad(run.out, mask, what)
    return clean


def check_dirty(op, inp, what, inherit=None):
    """Property 2: the bytes of outputs and workspace on entry change no bit, none survives, the flag words are those of a
    zeroed workspace; `inherit(ws)` runs a call of another shape and lattice on the workspace before the call under test."""
    runs = {fill: op.run(inp, fill=fill) for fill in W.BYTE_PATTERNS}
    base = runs[0x00]
    for fill in W.BYTE_PATTERNS[1:]:
        _report(f"{what} prefill 0x{fill:02X} vs 0x00", W.total_diff(base.out, runs[fill].out))
        _flags_same(op, inp, base, runs[fill], f"{what} prefill 0x{fill:02X}")
        _no_prefill_left(runs[fill].out, fill, what)
    if inherit is not None:
        ws = inherit()
        assert ws.numel() >= op.ws_bytes(inp)
        run = op.run(inp, fill=0xA5, ws=ws)
        _report(f"{what} inherited workspace", W.total_diff(base.out, run.out))
        _flags_same(op, inp, base, run, f"{what} inherited workspace")
    return base


def _rows(inp, perm):
    idx = torch.as_tensor(perm, device=inp.x.device)
    kw = dict(x=inp.x[idx].contiguous(), labels=inp.labels[idx].contiguous(), ll=inp.ll[idx].contiguous(), tl=inp.tl[idx].contiguous())
    if hasattr(inp, "vec"):
        kw["vec"] = inp.vec[idx].contiguous()
    return inp.replace(**kw)


HOSTILE = ("zero-length", "infeasible", "1e10 logits", "label equal to the blank")


def _hostile(inp, how):
    """Utterance 0 as it is; every other one replaced."""
    x, labels, ll, tl = inp.x.clone(), inp.labels.clone(), inp.ll.clone(), inp.tl.clone()
    B, T, V, U = inp.shape
    if how == "zero-length":
        tl[1:] = 0
    elif how == "infeasible":
        tl[1:], ll[1:] = 1, min(U, 3)
    elif how == "1e10 logits":
        x[1:] *= 1e10
        tl[1:], ll[1:] = T, min(U, max(T // 2, 1), 3)
    else:
        labels[1:, 0] = inp.blank
        tl[1:], ll[1:] = T, min(U, max(T // 2, 1), 3)
    return inp.replace(x=x, labels=labels, ll=ll, tl=tl)


def check_neighbours(op, inp, what, clean=None, hostile=HOSTILE):
    """Property 3: (a) a permuted batch gives the permuted rows; (b) utterance 0 keeps its bits and its flag word beside hostile
    neighbours."""
    B = inp.shape[0]
    clean = clean or op.run(inp)
    perm = PERM(B)
    run = op.run(_rows(inp, perm))
    _report(f"{what} batch permuted {perm if B <= 8 else '(reversed)'}", W.total_diff(clean.out, run.out, perm=perm))
    f0, f1 = op.flags(inp, clean), op.flags(inp, run)
    if f0 is not None:
        print(f"OWNERSHIP {what} permuted: flag words {f1.tolist()} (clean {f0.tolist()})", flush=True)
        assert torch.equal(f0[torch.as_tensor(perm, device=f0.device)], f1), what
    for how in hostile:
        run = op.run(_hostile(inp, how))
        _report(f"{what} utterance 0 beside {how} neighbours", W.total_diff(clean.out, run.out, rows=[0]))
        f1 = op.flags(inp, run)
        if f0 is not None:
            print(f"OWNERSHIP {what} beside {how}: flag words {f1.tolist()} (clean {f0.tolist()})", flush=True)
            assert f0[0].item() == f1[0].item(), (what, how)
            if how == "1e10 logits":
                assert bool((f1[1:] != 0).all()), (what, "the 1e10 utterances were not flagged", f1.tolist())


# ---- loss + gradient ----

def _lg_inputs(c, kind, dtype=torch.float32, time_major=False):
    x = W.dev(c.logits, dtype)
    if time_major:
        x = x.transpose(0, 1).contiguous().transpose(0, 1)
    inp = _inputs(c, kind, x=x)
    inp.case_name = c.name
    return inp


def _inherit_lg(inp, kind, tier):
    """A workspace that a loss + gradient call of the other lattice, a larger T and another tier has just used.  It has the
    conservative size (CTC_AMD_WS_LOSS_GRAD, valid for every tier) of the larger of the two calls."""
    def make():
        from tf_seq2seq_losses_amd import _lib
        B, T, V, U = inp.shape
        rng = np.random.default_rng(1)
        T2 = T + 19
        o = W.make_inputs(1 - inp.kind, rng.standard_normal((B, T2, V)).astype(np.float32) * 3, rng.integers(1, V, (B, U)).astype(np.int32),
                          np.full(B, min(U, T2 // 2), np.int32), np.full(B, T2, np.int32), U=U)
        ws = W.workspace(max(_lib.workspace_bytes(_lib.WS_LOSS_GRAD, o.kind, *o.shape), _lib.workspace_bytes(_lib.WS_LOSS_GRAD, inp.kind, *inp.shape)), 0xA5)
        _lib.debug_override("pipeline", {"": "fused5", "fused5": "v1", "v1": ""}[tier])
        try:
            W.loss_grad(o, "loss_grad", ws=ws)
        finally:
            _lib.debug_override("pipeline", tier)
        return ws
    return make


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(LG_CASES))
def test_loss_grad_padding_frames_and_label_tails(name, kind):
    c = W.case(name)
    for tier in _tiers(name, kind):
        with override("pipeline", tier):
            pipe = _assert_pipeline(c, kind, tier)
            for entry in W.LOSS_GRAD_ENTRIES + ("time-major",):
                inp = _lg_inputs(c, kind, time_major=entry == "time-major")
                op = lg_op("ex" if entry == "time-major" else entry, tier)
                what = f"{name} {kind} {pipe} {entry}"
                clean = op.run(inp)
                _check_lg_clean(c, kind, clean.out, what)
                check_padding(op, inp, c, what, clean)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["lg_nl1", "lg_nl2"])
def test_loss_grad_ex_16bit_padding_frames_and_label_tails(name, dtype, kind):
    """The oracle sees the 16-bit values widened.  The loss is float32 and held to TOL; a 16-bit gradient element is the float32
    one rounded once, so its bound is TOL plus half an ulp of the element type at the reference's magnitude (_check_lg_clean).
    bfloat16 rows that are 8-byte aligned (V = 256) run the fused tiers; V = 301 and float16 run the three-kernel pipeline."""
    c = W.case(name)
    fused = dtype == torch.bfloat16 and c.shape[2] % 4 == 0
    for tier in (("", "fused5", "v1") if fused else ("v1",)):
        with override("pipeline", tier):
            pipe = _assert_pipeline(c, kind, tier)
            inp = _lg_inputs(c, kind, dtype)
            wide = inp.replace(x=inp.x.float())
            op, what = lg_op("ex", tier), f"{name} {kind} {pipe} ex {dtype}"
            _check_lg_clean(c, kind, lg_op("ex", tier).run(wide).out, what + " (float32 run on the widened values)", dtype)
            clean = op.run(inp)
            _check_lg_clean(c, kind, clean.out, what, dtype)
            check_padding(op, inp, c, what, clean)
            check_dirty(op, inp, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(LG_CASES))
def test_loss_grad_dirty_outputs_and_workspace(name, kind):
    from tf_seq2seq_losses_amd import _lib
    c = W.case(name)
    for tier in _tiers(name, kind):
        with override("pipeline", tier):
            pipe = _assert_pipeline(c, kind, tier)
            inp = _lg_inputs(c, kind)
            for entry in W.LOSS_GRAD_ENTRIES:
                for selector in (_lib.WS_LOSS_GRAD_LOGITS, _lib.WS_LOSS_GRAD):
                    op = lg_op(entry, tier, selector=selector)
                    what = f"{name} {kind} {pipe} {entry} selector {selector}"
                    # (inherited: once per entry; the inherited workspace has the conservative size whatever the selector)
                    base = check_dirty(op, inp, what, _inherit_lg(inp, kind, tier) if selector == _lib.WS_LOSS_GRAD_LOGITS else None)
                    _check_lg_clean(c, kind, base.out, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(LG_CASES))
def test_loss_grad_neighbours(name, kind):
    c = W.case(name)
    for tier in _tiers(name, kind):
        with override("pipeline", tier):
            pipe = _assert_pipeline(c, kind, tier)
            inp = _lg_inputs(c, kind)
            for entry in ("loss_grad", "loss_only", "two_call"):
                check_neighbours(lg_op(entry, tier), inp, f"{name} {kind} {pipe} {entry}")


@pytest.mark.parametrize("kind", KINDS)
def test_loss_grad_wrt_logprobs(kind):
    """Log-probability input (three-kernel pipeline): padding, label tails, dirty buffers."""
    from tf_seq2seq_losses_amd import _lib
    c = W.case("small")
    assert _lib.pipeline_name(KIND_ID[kind], 1, *c.shape, True) == "v1"
    lp = VO.log_softmax64(c.logits).astype(np.float32)
    inp = _inputs(c, kind, x=lp)
    op = Op("loss_grad wrt logprobs", lambda i, fill=0xA5, ws=None: W.loss_grad(i, "loss_grad", wrt=1, fill=fill, ws=ws),
            _pad_zero("grad"), _lg_ws_bytes(_lib.WS_LOSS_GRAD))
    what = f"small {kind} v1 loss_grad wrt logprobs"
    clean = op.run(inp)
    data = O.LOSS_DATA[kind](c.labels, lp, c.ll, c.tl, 0)
    _check_loss(c, kind, clean.out["loss"], data.loss, what)
    _check_abs(clean.out["grad"], data.gradient, what + " gradient")
    check_padding(op, inp, c, what, clean)
    check_dirty(op, inp, what)


# ---- gaps ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["lg_nl1", "lg_nl2", "lg_wide"])
def test_strided_calls_leave_the_gaps_alone(name, kind):
    """stride_t = V + 5, stride_b = T * stride_t + 11: NaN in the gaps of the logits changes nothing, the gaps of the gradient keep
    their prefill."""
    c = W.case(name)
    B, T, V, U = c.shape
    st, sb = V + 5, T * (V + 5) + 11
    for tier in _tiers(name, kind):
        with override("pipeline", tier):
            pipe = _assert_pipeline(c, kind, tier)
            dense = _lg_inputs(c, kind)
            storage, view, owned = W.strided_storage(dense.x, sb, st, 0x00)
            assert view.stride() == (sb, st, 1)
            for entry in ("ex", "sum", "two_call"):
                what = f"{name} {kind} {pipe} {entry} strided"
                # (not compared bit for bit with the contiguous call: unaligned rows take the element-wise kernels, test_gpu_formats2.py)
                clean = W.loss_grad(dense.replace(x=view), entry, fill=0xA5)
                _check_lg_clean(c, kind, clean.out, what)
                for value in (float("nan"), 3.0e38):
                    pview = W.poison_gaps(storage, owned, value).as_strided((B, T, V), (sb, st, 1))
                    pview.copy_(W.poison_padding(pview, c.tl, value))
                    run = W.loss_grad(dense.replace(x=pview, labels=W.poison_labels(dense.labels, c.ll, W.label_poison_cycle(V, 0))), entry, fill=0xA5)
                    _report(f"{what} gaps and padding {value}", W.total_diff(clean.out, run.out))
                    kept = W.keeps_prefill(run.grad_storage, 0xA5)
                    assert bool(kept[~owned].all()), (what, "a gap of the gradient buffer was written", int((~kept[~owned]).sum().item()))
                    assert not bool(kept[owned].any()), (what, "an owned gradient element keeps its prefill")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,op_name", [("align_a", "best_path"), ("greedy", "greedy_decode")])
def test_strided_alignment_and_decoding_ignore_the_gaps(name, op_name, kind):
    c = W.case(name)
    B, T, V, U = c.shape
    st, sb = V + 5, T * (V + 5) + 11
    op = _ops()[op_name]
    dense = _inputs(c, kind)
    ref = op.run(dense)
    storage, view, owned = W.strided_storage(dense.x, sb, st, 0x00)
    _report(f"{name} {kind} {op_name} strided vs contiguous", W.total_diff(ref.out, op.run(dense.replace(x=view)).out))
    for value in (float("nan"), float("inf")):
        pst = W.poison_gaps(storage, owned, value)
        pv = pst.as_strided((B, T, V), (sb, st, 1))
        pv.copy_(W.poison_padding(pv, c.tl, value))
        _report(f"{name} {kind} {op_name} gaps and padding {value}", W.total_diff(ref.out, op.run(dense.replace(x=pv)).out))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_packed_call_leaves_unowned_rows_and_gaps_alone(kind, dtype):
    """row_stride = V + 3; unowned rows in front of, between and behind the utterances, one utterance without frames."""
    c = W.case("lg_nl1")
    B, T, V, U = c.shape
    rs = V + 3
    offsets, r = [], 2
    for b in range(B):
        offsets.append(r)
        r += int(c.tl[b]) + (b % 3)  # 0, 1 or 2 unowned rows behind each utterance
    total = r + 3
    dense = _lg_inputs(c, kind, dtype)
    odt = None if dtype == torch.float32 else dtype
    what = f"lg_nl1 {kind} packed {dtype}"
    clean = None
    for value, fill in ((None, 0xA5), (float("nan"), 0xA5), (float("nan"), 0x00), (W.poison_values(dtype)[-1], 0xFF)):
        storage, owned = W.packed_storage(dense.x, c.tl, offsets, rs, total, 0x00)
        inp = dense
        if value is not None:
            storage = W.poison_gaps(storage, owned, value)
            inp = dense.replace(labels=W.poison_labels(dense.labels, c.ll, W.label_poison_cycle(V, 0)))
        run = W.loss_grad_packed(inp, storage, offsets, rs, fill=fill)
        g = run.out["grad"]
        kept = W.keeps_prefill(g, fill)
        assert bool(kept[~owned].all()), (what, "an unowned gradient row or gap was written", int((~kept[~owned]).sum().item()))
        if clean is None:
            # Held to the oracle like every clean run, not to the padded call's bits: whether a row takes the 16-byte or the
            # element-wise accesses depends on its own address, which differs between the two layouts (test_packed_batches in
            # test_gpu_formats2.py compares the two calls with a tolerance for that reason).
            clean = run
            unpacked = torch.zeros((B, T, V), dtype=dtype, device=g.device)
            for b in range(B):
                unpacked[b, :int(c.tl[b])] = g[offsets[b]:offsets[b] + int(c.tl[b]), :V]
            _check_lg_clean(c, kind, {"loss": run.out["loss"], "grad": unpacked}, what, odt)
        else:
            _report(f"{what} unowned = {value}, prefill 0x{fill:02X}",
                    {"loss": W.count_diff(clean.out["loss"], run.out["loss"]), "grad": W.count_diff(clean.out["grad"][owned], g[owned])})


# ---- Hessian-vector product ----

def _hvp_inputs(c, kind):
    inp = _inputs(c, kind)
    inp.vec = W.dev(np.random.default_rng(5).standard_normal(c.logits.shape).astype(np.float32))
    return inp


def _hvp_tier(c, kind, tier):
    """Asserts which Hessian-vector pipeline the case runs: `fused` or the log-domain one."""
    from tf_seq2seq_losses_amd import _lib
    if c.name.startswith("hvp_fused"):
        _lib.hvp_flags_offset(KIND_ID[kind], *c.shape)  # (raises unless the shape runs the fused kernel)
        return tier == ""
    with pytest.raises(ValueError):
        _lib.hvp_flags_offset(KIND_ID[kind], *c.shape)
    return False


def _check_hvp_clean(c, kind, op, inp, out, what):
    rl, rg = _ref_lg(c.name, kind)
    _check_loss(c, kind, out["loss"], rl, what)
    if "grad" in out:
        _check_abs(out["grad"], rg, what + " gradient")
    feas = W.feasible_rows(c, kind)
    assert bool((out["hvp"][torch.as_tensor(~feas, device=out["hvp"].device)] == 0).all()), what
    if c.shape[2] <= 8:  # the dense oracle Hessian
        g, _, _ = _ref_data(c.name, kind)
        ref = np.einsum("btkuj,buj->btk", _ref_hessian(c.name, kind), inp.vec.cpu().numpy()[g].astype(np.float64))
        _check_abs(out["hvp"].cpu().numpy()[g], ref, what + " product (dense oracle Hessian)")
        return
    # V = 256: the central difference of the float64 oracle gradient with eps = 1e-3 (derived in test_gpu_contract.py), along the
    # direction the two float32 inputs actually differ by
    eps = 1e-3
    v = inp.vec.cpu().numpy().astype(np.float64)
    xp, xm = ((c.logits.astype(np.float64) + s * eps * v).astype(np.float32) for s in (1, -1))
    taken = ((xp.astype(np.float64) - xm.astype(np.float64)) / (2 * eps)).astype(np.float32)
    fd = (C.loss_grad(kind, c.labels, xp, c.ll, c.tl, 0)[1] - C.loss_grad(kind, c.labels, xm, c.ll, c.tl, 0)[1]) / (2 * eps)
    _check_abs(op.run(inp.replace(vec=W.dev(taken))).out["hvp"], fd, what + " product (central difference of the oracle gradient)")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,tier", [("hvp_fused", ""), ("hvp_fused_distinct", "v1"), ("hvp_log", "")])
def test_hvp_ownership(name, tier, kind):
    """All properties for ctc_amd_hvp: the fused kernel (labels with a run of repeats), the log-domain pipeline forced onto the same
    shape and a shape that runs the log-domain pipeline by itself (both with labels drawn without replacement: module docstring)."""
    c = W.case(name)
    op = _ops()["hvp"]
    with override("hvp", tier):
        fused = _hvp_tier(c, kind, tier)
        inp = _hvp_inputs(c, kind)
        inp.fused_hvp = fused
        what = f"{name} {kind} hvp {'fused' if fused else 'log-domain'}"
        clean = op.run(inp)
        _check_hvp_clean(c, kind, op, inp, clean.out, what)
        check_padding(op, inp, c, what, clean)

        def inherit():  # (the other lattice, another shape and -- from the fused kernel's side -- the other pipeline)
            o = _hvp_inputs(W.case("hvp_log" if name != "hvp_log" else "hvp_fused"), "simplified" if kind == "classic" else "classic")
            ws = W.workspace(max(op.ws_bytes(o), op.ws_bytes(inp)), 0xA5)
            op.run(o, ws=ws)
            return ws
        check_dirty(op, inp, what, inherit)
        check_neighbours(op, inp, what, clean)


@pytest.mark.parametrize("kind", KINDS)
def test_log_domain_hvp_with_repeats_against_the_oracle(kind):
    """The exception: a run of repeats on the tier with float atomics is compared with the oracle at TOL only."""
    c = W.case("hvp_log_repeats")
    assert not _hvp_tier(c, kind, "")
    inp = _hvp_inputs(c, kind)
    op = _ops()["hvp"]
    _check_hvp_clean(c, kind, op, inp, op.run(inp).out, f"hvp_log_repeats {kind}")


# ---- dense Hessian, alpha / beta, log posterior ----

def _check_hessian_clean(c, kind, out, what):
    rl, rg = _ref_lg(c.name, kind)
    _check_loss(c, kind, out["loss"], rl, what)
    _check_abs(out["grad"], rg, what + " gradient")
    g, _, _ = _ref_data(c.name, kind)
    feas = W.feasible_rows(c, kind)
    h = out["hess"].cpu().numpy()
    assert np.all(h[~feas] == 0), what
    _check_abs(h[g], _ref_hessian(c.name, kind), what + " Hessian")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,kernel", [("small", ""), ("small", "slab"), ("hess_long", "")])
def test_hessian_ownership(name, kernel, kind):
    c = W.case(name)
    op = _ops()["hessian"]
    assert (c.shape[3] > 32) == (name == "hess_long")  # labels of more than 32 positions: the general kernel by itself
    with override("hessian", kernel):
        inp = _inputs(c, kind)
        what = f"{name} {kind} hessian '{kernel}'"
        clean = op.run(inp)
        _check_hessian_clean(c, kind, clean.out, what)
        check_padding(op, inp, c, what, clean)

        def inherit():
            o = _inputs(W.case("hess_long" if name == "small" else "small"), "simplified" if kind == "classic" else "classic")
            ws = W.workspace(max(op.ws_bytes(o), op.ws_bytes(inp)), 0xA5)
            op.run(o, ws=ws)
            return ws
        check_dirty(op, inp, what, inherit)
        check_neighbours(op, inp, what, clean)


@pytest.mark.parametrize("kernel", ["", "slab"])
@pytest.mark.parametrize("kind", KINDS)
def test_hessian_plan_kernel_neighbours(kind, kernel):
    """B = 40: the launch goes through the plan kernel and the XCD stride permutation (test_gpu_configs.py)."""
    c = W.case("hess_plan")
    op = _ops()["hessian"]
    with override("hessian", kernel):
        inp = _inputs(c, kind)
        what = f"hess_plan {kind} hessian '{kernel}'"
        clean = op.run(inp)
        _check_hessian_clean(c, kind, clean.out, what)
        check_neighbours(op, inp, what, clean)
        mask = W.padding_mask(c.tl, c.shape[1]).to(inp.x.device)
        op.pad(clean.out, mask, what)


@pytest.mark.parametrize("kind", KINDS)
def test_alpha_beta_and_log_posterior_ownership(kind):
    c = W.case("small")
    ops = _ops()
    inp = _inputs(c, kind)
    rl, _ = _ref_lg("small", kind)
    g, data, _ = _ref_data("small", kind)
    for op_name in ("alpha_beta", "log_posterior"):
        op, what = ops[op_name], f"small {kind} {op_name}"
        clean = op.run(inp)
        _check_loss(c, kind, clean.out["loss"], rl, what)
        for key, ref in (("alpha", data.alpha), ("beta", data.beta), ("lg", data.logarithmic_logproba_gradient)):
            if key not in clean.out:
                continue
            a = clean.out[key].cpu().numpy().astype(np.float64)[g]
            if key != "lg":
                Lo = ref.shape[2]
                assert np.all(a[:, :, Lo:] == -np.inf), key
                a = a[:, :, :Lo]
            assert np.array_equal(np.isfinite(a), np.isfinite(ref)), (what, key)
            m = np.isfinite(ref)
            err = (np.abs(a[m] - ref[m]) / np.maximum(1, np.abs(ref[m]))).max()
            print(f"OWNERSHIP {what}: clean {key} error {err:.3e}", flush=True)
            assert err < TOL, (what, key, err)
        check_padding(op, inp, c, what, clean)

        def inherit():
            o = _inputs(W.case("hvp_log"), "simplified" if kind == "classic" else "classic")
            ws = W.workspace(max(op.ws_bytes(o), op.ws_bytes(inp)), 0xA5)
            ops["alpha_beta"].run(o, ws=ws)
            return ws
        check_dirty(op, inp, what, inherit)
        check_neighbours(op, inp, what, clean)


# ---- best path, greedy decoding ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,wrt", [("align_a", 0), ("align_a", 1), ("align_b", 0)])
def test_best_path_ownership(name, wrt, kind):
    c = W.case(name)
    x = VO.log_softmax64(c.logits).astype(np.float32) if wrt else c.logits
    base = _ops()["best_path"]
    op = Op("best_path", lambda i, fill=0xA5, ws=None: W.best_path(i, wrt=wrt, fill=fill, ws=ws), base.pad, base.ws_bytes)
    inp = _inputs(c, kind, x=x)
    what = f"{name} {kind} best_path wrt={wrt}"
    clean = op.run(inp)
    got = tuple(clean.out[k].cpu().numpy() for k in ("score", "tokens", "label_index"))
    check_against_oracle(kind, wrt, x, c.labels, c.ll, c.tl, got, what=what)
    feas = W.feasible_rows(c, kind)
    assert np.all(got[0][~feas] == -np.inf) and np.all(got[1][~feas] == -1) and np.all(got[2][~feas] == -1)
    check_padding(op, inp, c, what, clean)

    def inherit():
        o = _inputs(W.case("align_b" if name == "align_a" else "align_a"), "simplified" if kind == "classic" else "classic")
        ws = W.workspace(max(op.ws_bytes(o), op.ws_bytes(inp)), 0xA5)
        base.run(o, ws=ws)
        return ws
    check_dirty(op, inp, what, inherit)
    check_neighbours(op, inp, what, clean)


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_decode_ownership(kind):
    c = W.case("greedy")
    op = _ops()["greedy_decode"]
    inp = _inputs(c, kind)
    what = f"greedy {kind} greedy_decode"
    clean = op.run(inp)
    o = clean.out
    check_decoding(tuple(o[k].cpu().numpy() for k in ("score", "tokens", "decoded", "decoded_length", "frames", "label_score")),
                   GO.decode(kind, c.logits, c.tl, 0, 0), what)
    check_padding(op, inp, c, what, clean)

    def inherit():
        B, T, V, _ = c.shape
        rng = np.random.default_rng(2)
        oth = W.make_inputs(KIND_ID["simplified" if kind == "classic" else "classic"], rng.standard_normal((B + 1, T + 40, V)).astype(np.float32),
                            np.ones((B + 1, 1), np.int32), np.zeros(B + 1, np.int32), np.full(B + 1, T + 40, np.int32), U=1)
        ws = W.workspace(max(op.ws_bytes(oth), op.ws_bytes(inp)), 0xA5)
        op.run(oth, ws=ws)
        return ws
    check_dirty(op, inp, what, inherit)
    check_neighbours(op, inp, what, clean, hostile=("zero-length", "1e10 logits"))
