"""Host-side mirror of the reference's Python interface for the CTC hot path.

Same names, argument order, defaults and error behaviour as the reference
(alexeytochin/tf_seq2seq_losses v0.3.0; paths below are relative to it):

    classic_ctc_loss(labels, logits, label_length, logit_length, blank_index=0)      classic_ctc_loss.py:33-70
    simplified_ctc_loss(labels, logits, label_length, logit_length, blank_index=0)   simplified_ctc_loss.py:32-67
    simple_ctc_loss = simplified_ctc_loss       (the name the reference's README/benchmark table uses)
    ctc_loss / ctc_loss_from_logproba                                                 base_loss.py:38-99
    ClassicCtcLossData / SimplifiedCtcLossData  (.loss .gradient .logarithmic_logproba_gradient .hessian
                                                 .alpha .beta)                        base_loss.py:102-298

Tensors are torch tensors on an AMD GPU (TensorFlow is not part of this build); NumPy arrays are accepted
and moved to the current GPU.  Differentiation is wired like the reference's three nested tf.custom_gradient
functions (base_loss.py:140-184): first order = d_loss[:,None,None] * gradient, second order = contraction
with the analytic Hessian, third order raises NotImplementedError.
All arithmetic is done by the HIP kernels behind the C ABI (include/ctc_amd.h); there is no CPU fallback.
"""
from __future__ import annotations

from functools import cached_property, partial
from typing import NamedTuple, Optional, Union

import numpy as np
import torch

from . import _lib, ops

TensorLike = Union[torch.Tensor, np.ndarray]


def _as_tensor(x, dtype=None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    if not torch.cuda.is_available():
        raise RuntimeError("tf_seq2seq_losses_amd needs an AMD GPU (no CPU fallback); torch.cuda.is_available() is False")
    t = torch.as_tensor(np.asarray(x))
    if dtype is not None and t.dtype != dtype and not t.dtype.is_floating_point:
        t = t.to(dtype)
    return t.cuda()


def _blank(blank_index) -> int:
    if isinstance(blank_index, torch.Tensor):
        return int(blank_index.item())  # base_loss.py:122-125 accepts a tensor as well
    return int(blank_index)


def _verify_inputs(labels, x, label_length, logit_length):
    """base_loss.py:129-138 : same assertions, same exception type (AssertionError)."""
    assert x.dim() == 3
    # the reference takes float32 only; bfloat16 / float16 activations are an extension
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    assert labels.dim() == 2
    assert logit_length.dim() == 1
    assert label_length.dim() == 1
    assert x.shape[0] == labels.shape[0]
    assert x.shape[0] == logit_length.shape[0]
    assert x.shape[0] == label_length.shape[0]


# --------------------------------------------------------------------------------------------------
# autograd wiring (base_loss.py:140-184)
# --------------------------------------------------------------------------------------------------
HVP_DENSE = False  # diagnostic: second-order autograd through a materialised [B,T,V,T,V] Hessian, as the reference does


class _HessianContraction(torch.autograd.Function):
    """gradient_fn.backprop (base_loss.py:167-173): out[b,t,k] = sum_{t2,k2} v[b,t2,k2] H[b,t,k,t2,k2].
    Its own backward is the third derivative, which the reference refuses (base_loss.py:179-182)."""

    @staticmethod
    def forward(ctx, x, v, kind, wrt, prep):
        # the reference contracts a materialised [B,T,V,T,V] Hessian here; the tangent-mode kernel (ctc_hvp.hip) gives the
        # same product in O(T*L) memory.  HVP_DENSE keeps the materialised route (parity tests compare both).
        if HVP_DENSE:
            _, _, hess = ops.hessian(kind, wrt, prep, want_grad=False)
            return torch.einsum("btkuj,buj->btk", hess, v.float()).to(x.dtype)
        return ops.hvp(kind, wrt, prep, v)[2].to(x.dtype)

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("Third order derivative over the ctc loss function is not implemented.")


class _CtcGradient(torch.autograd.Function):
    """gradient_fn (base_loss.py:157-175) composed with forward_fn.backprop (base_loss.py:150-153):
    returns d_loss[:,None,None] * gradient and differentiates to the Hessian contraction."""

    @staticmethod
    def forward(ctx, x, d_loss, kind, wrt, prep, pending):
        ctx.kind, ctx.wrt, ctx.prep = kind, wrt, prep
        ctx.save_for_backward(x, d_loss)
        if pending is not None:  # the forward pass left its half of the work in a workspace: run the other half (one launch)
            return ops.grad_resume(kind, wrt, prep, pending, d_loss=d_loss)
        return ops.loss_grad(kind, wrt, prep, True, d_loss=d_loss)[1]  # weighting inside the kernel

    @staticmethod
    def backward(ctx, dd):
        x, d_loss = ctx.saved_tensors
        gx = gd = None
        if ctx.needs_input_grad[0]:
            gx = _HessianContraction.apply(x, dd * d_loss.reshape(-1, 1, 1), ctx.kind, ctx.wrt, ctx.prep)
        if ctx.needs_input_grad[1]:
            grad_unit = ops.loss_grad(ctx.kind, ctx.wrt, ctx.prep, True)[1]
            gd = (dd.float() * grad_unit.float()).sum(dim=(1, 2)).to(d_loss.dtype)
        return gx, gd, None, None, None, None


class _CtcLoss(torch.autograd.Function):
    """forward_fn (base_loss.py:140-155).  On the linear-domain fused tier the forward pass runs the first half of the kernel
    (both lattice chains up to their meeting point: the loss) and keeps its checkpoint workspace (64 MB at the north-star
    shape, saved with the graph and released with it); backward runs the second half from there with d_loss applied inside
    the kernel -- together one loss+gradient call's work, no [B,T,V] tensor kept alive in between, no extra pass over the
    gradient for the d_loss weights (ctc_amd_grad_resume).  Other pipelines keep nothing and compute the gradient in one
    call during backward."""

    @staticmethod
    def forward(ctx, x, kind, wrt, prep):
        ctx.kind, ctx.wrt, ctx.prep = kind, wrt, prep
        if x.requires_grad:
            loss, ws = ops.loss_forward(kind, wrt, prep)
        else:
            loss, ws = ops.loss_grad(kind, wrt, prep, want_grad=False)[0], None
        ctx.has_ws = ws is not None
        if ws is not None:
            ctx.save_for_backward(x, ws)  # freed with the graph, like any saved activation
        else:
            ctx.save_for_backward(x)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        x = ctx.saved_tensors[0]
        ws = ctx.saved_tensors[1] if ctx.has_ws else None
        if not torch.is_grad_enabled():
            # first order only (no create_graph): nobody will differentiate the gradient, so skip the nested autograd node
            # (one Function.apply, its context and saved tensors: ~20 us of host time per step)
            if ws is not None:
                return ops.grad_resume(ctx.kind, ctx.wrt, ctx.prep, ws, d_loss=d_loss), None, None, None
            return ops.loss_grad(ctx.kind, ctx.wrt, ctx.prep, True, d_loss=d_loss)[1], None, None, None
        return _CtcGradient.apply(x, d_loss, ctx.kind, ctx.wrt, ctx.prep, ws), None, None, None


def _host_max(label_length):
    """max(label_length) when the caller's copy lives on the host (NumPy array, list, CPU tensor): free, no device sync."""
    if isinstance(label_length, torch.Tensor):
        if label_length.is_cuda or label_length.numel() == 0:
            return None
        return int(label_length.max())
    a = np.asarray(label_length)
    return int(a.max()) if a.size else None


def _ctc(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, max_label_length=None) -> torch.Tensor:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    kind = ops.KINDS[kind_name]
    # logits keep the producer's format where the kernels read it directly (bfloat16, time-major views): no copy
    prep = ops.Prepared(labels, x.detach(), label_length, logit_length, _blank(blank_index),
                        keep_format=(wrt == _lib.WRT_LOGITS), host_max_label_length=max_label_length)
    return _CtcLoss.apply(x, kind, wrt, prep)


# --------------------------------------------------------------------------------------------------
# public functions
# --------------------------------------------------------------------------------------------------
def classic_ctc_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                     blank_index: Union[int, torch.Tensor] = 0, *, max_label_length: Optional[int] = None) -> torch.Tensor:
    """Classic CTC loss (repeated tokens without a blank in between are merged, then blanks are dropped;
    reference classic_ctc_loss.py:33-70).  Infeasible samples give loss = +inf with zero gradient.

    Args:
        labels:       [batch, max_label_length] int32
        logits:       [batch, max_length, num_tokens] float32
        label_length: [batch] int32
        logit_length: [batch] int32
        blank_index:  integer >= 0 (or a scalar tensor)
        max_label_length: (extension, keyword only) an upper bound on label_length known on the host.  The reference takes
            the dynamic maximum (base_loss.py:482-486); here any bound >= it gives the same results and a tight one selects
            the fastest kernel tier without a device -> host sync.  Not needed when label_length is passed as a NumPy array /
            CPU tensor (its maximum is then taken on the host), nor for label tensors up to 128 wide.
    Returns: [batch] float32 samplewise loss
    """
    return _ctc("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length)


def simplified_ctc_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                        blank_index: Union[int, torch.Tensor] = 0, *, max_label_length: Optional[int] = None) -> torch.Tensor:
    """Simplified CTC loss (blanks are dropped, repeated tokens are NOT merged; reference
    simplified_ctc_loss.py:32-67).  Same arguments and return value as classic_ctc_loss."""
    return _ctc("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length)


simple_ctc_loss = simplified_ctc_loss  # row label used by the reference's README.md:22 and tests/benchmark.py:72,98


def ctc_loss(labels, logits, label_length, logit_length, blank_index, ctc_loss_data_cls) -> torch.Tensor:
    """base_loss.py:38-68 : generic entry point taking the loss-data class."""
    return _ctc(ctc_loss_data_cls.kind_name, _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index)


def ctc_loss_from_logproba(labels, logprobas, label_length, logit_length, blank_index, ctc_loss_data_cls) -> torch.Tensor:
    """base_loss.py:71-99 : loss as a function of log-probabilities treated as independent variables."""
    return _ctc(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length,
                blank_index)


# --------------------------------------------------------------------------------------------------
# best-path (Viterbi) forced alignment: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcAlignment(NamedTuple):
    """score [batch] float32: log-probability of the best path (-inf: no path exists);
    tokens [batch, max_length] int32: the token every frame emits on it (-1 beyond logit_length);
    label_index [batch, max_length] int32: index into labels[b] of the label the frame emits -- on the classic lattice also
    of the label it continues by repeating it -- and -1 on blank frames and beyond logit_length.
    An infeasible sample (loss = +inf) has score = -inf and -1 in every frame."""
    score: torch.Tensor
    tokens: torch.Tensor
    label_index: torch.Tensor


def _align(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, max_label_length=None) -> CtcAlignment:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    with torch.no_grad():  # a path is not differentiable: the result is detached
        prep = ops.Prepared(labels, x.detach(), label_length, logit_length, _blank(blank_index), keep_format=True,
                            host_max_label_length=max_label_length)
        return CtcAlignment(*ops.best_path(ops.KINDS[kind_name], wrt, prep))


def classic_ctc_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                          blank_index: Union[int, torch.Tensor] = 0, *, max_label_length: Optional[int] = None) -> CtcAlignment:
    """Forced alignment on the classic lattice: the most probable path among those classic_ctc_loss sums over (repeats are
    merged, then blanks dropped).  Arguments as classic_ctc_loss (float32 / bfloat16 / float16 logits, any batch / time
    strides); returns CtcAlignment(score, tokens, label_index), not differentiable."""
    return _align("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length)


def simplified_ctc_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                             blank_index: Union[int, torch.Tensor] = 0, *, max_label_length: Optional[int] = None) -> CtcAlignment:
    """Forced alignment on the simplified lattice (blanks are dropped, repeats are not merged: every non-blank frame emits
    exactly one label).  Same arguments and return value as classic_ctc_alignment."""
    return _align("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length)


def ctc_alignment_from_logproba(labels, logprobas, label_length, logit_length, blank_index, ctc_loss_data_cls) -> CtcAlignment:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba)."""
    return _align(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index)


# --------------------------------------------------------------------------------------------------
# forced alignment of partial transcripts (wildcard labels): an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
WILDCARD = _lib.WILDCARD  # -2: the label value of a wildcard position
OPTIONAL_WILDCARD = _lib.OPTIONAL_WILDCARD  # -3: a wildcard position that may be empty (only with optional_wildcards=True)


def ctc_frame_window(first_frame: TensorLike, last_frame: TensorLike, logit_length: TensorLike, *, before: int = 0,
                     after: int = 0) -> torch.Tensor:
    """frame_window [batch, U, 2] int32 for the `frame_window` argument of the (long) wildcard loss, (long) label posterior and
    (long) wildcard alignment functions: (first_frame - before, last_frame + after), clipped to [0, logit_length - 1], on the device of
    first_frame and without a synchronisation.  first_frame / last_frame [batch, U] are an alignment's (CtcWildcardAlignment and
    its long-form twin), or a rounded CtcLabelPosterior.expected_frame given twice; `before` / `after` are the tolerance in frames.
    Positions from label_length on (-1 in both) come out as some clipped pair and are ignored by the calls."""
    first = _as_tensor(first_frame)
    last = _as_tensor(last_frame).to(first.device)
    if first.dim() != 2 or first.shape != last.shape:
        raise ValueError(f"first_frame and last_frame must both be [batch, U], got {tuple(first.shape)} and {tuple(last.shape)}")
    top = (_as_tensor(logit_length).to(device=first.device, dtype=torch.int64) - 1).clamp_min(0).unsqueeze(1)
    if top.shape[0] != first.shape[0]:
        raise ValueError(f"logit_length must be [batch] = {(int(first.shape[0]),)}, got {tuple(top.shape[:1])}")
    lo = torch.minimum((first.to(torch.int64) - int(before)).clamp_min(0), top)
    hi = torch.minimum((last.to(torch.int64) + int(after)).clamp_min(0), top)
    return torch.stack([lo, hi], dim=-1).to(torch.int32)


class CtcWildcardAlignment(NamedTuple):
    """score [batch] float32: log-probability of the best path, the frame-wise best token on wildcard frames (-inf: no path);
    tokens [batch, max_length] int32: the token of every frame on it -- on the frames of a wildcard the frame's argmax, ties to the
    lowest index (-1 beyond logit_length);
    label_index [batch, max_length] int32: index into labels[b] of the label the frame belongs to, a wildcard's index on all of
    its frames; -1 on blank frames outside any label and beyond logit_length;
    first_frame, last_frame [batch, U] int32: the first and last frame of every label (-1 from label_length on), U the bound on the
    label length the call ran with (the width of `labels`, or max_label_length);
    label_score [batch, U] float32: the log-probability of every label's frames (-inf from label_length on).
    An infeasible sample has score = -inf, -1 in every frame and label and -inf in label_score."""
    score: torch.Tensor
    tokens: torch.Tensor
    label_index: torch.Tensor
    first_frame: torch.Tensor
    last_frame: torch.Tensor
    label_score: torch.Tensor


def _wildcard_align(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index,
                    max_label_length=None, frame_window=None,
                    optional_wildcards: bool = False) -> CtcWildcardAlignment:
    if optional_wildcards and frame_window is not None:
        raise ValueError("frame_window and optional_wildcards=True cannot be combined")
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    with torch.no_grad():  # a path is not differentiable: the result is detached
        prep = ops.Prepared(labels, x.detach(), label_length, logit_length, _blank(blank_index), keep_format=True,
                            host_max_label_length=max_label_length)
        if optional_wildcards:
            return CtcWildcardAlignment(*ops.wildcard_best_path(ops.KINDS[kind_name], wrt, prep, optional_wildcards=True))
        if frame_window is None:
            return CtcWildcardAlignment(*ops.wildcard_best_path(ops.KINDS[kind_name], wrt, prep))
        return CtcWildcardAlignment(*ops.wildcard_best_path(ops.KINDS[kind_name], wrt, prep, _as_tensor(frame_window)))


def classic_ctc_wildcard_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                   blank_index: Union[int, torch.Tensor] = 0, *,
                                   max_label_length: Optional[int] = None, frame_window=None,
                    optional_wildcards: bool = False) -> CtcWildcardAlignment:
    """Forced alignment of a partial transcript on the classic lattice.  As classic_ctc_alignment, but a label equal to WILDCARD
    (-2) stands for any non-empty run of frames with any tokens on them: untranscribed speech before, after or inside the known
    words (free start and end are a wildcard as the first and last label).  A wildcard's frames score their best token and report
    it in `tokens`; adjacent wildcards take at least one frame each.  Arguments as classic_ctc_alignment (float32 / bfloat16 /
    float16 logits, any batch / time strides, read in place); returns CtcWildcardAlignment, not differentiable.
    check_labels keeps rejecting -2: it validates transcripts for the loss functions, where a wildcard is an impossible emission.
    frame_window [batch, U, 2] int32 / int64 on the logits' device, (first, last) inclusive per
    label position -- the convention of first_frame / last_frame; see ctc_frame_window -- lets position i own frame t only if
    first <= t <= last (label_index[b, t] == i only inside it; blank frames are free; a wildcard obeys
    its window like any label).  An empty window (first > last), or windows that admit no path, make the sample infeasible.
    optional_wildcards=True also accepts OPTIONAL_WILDCARD (-3), a wildcard position the path may skip: a skipped position has
    first_frame = last_frame = -1 and label_score 0, and score stays the sum of the label scores and the blank frames.  Two of them
    may not be adjacent (score -inf); not with frame_window (ValueError); on the classic lattice at most 512 label positions
    (ValueError).  With False, -3 is a malformed label as before."""
    return _wildcard_align("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length,
                           frame_window, optional_wildcards)


def simplified_ctc_wildcard_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                      blank_index: Union[int, torch.Tensor] = 0, *,
                                      max_label_length: Optional[int] = None, frame_window=None,
                    optional_wildcards: bool = False) -> CtcWildcardAlignment:
    """The same on the simplified lattice (every other non-blank frame emits exactly one label): a wildcard owns every frame from
    its entry until the next label's frame.  Same arguments and return value as classic_ctc_wildcard_alignment; check_labels keeps
    rejecting -2 here as well.  frame_window constrains the frame at which a label is emitted, and every frame a wildcard owns.
    optional_wildcards as in classic_ctc_wildcard_alignment, up to 1024 label positions."""
    return _wildcard_align("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, max_label_length,
                           frame_window, optional_wildcards)


def ctc_wildcard_alignment_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                         max_label_length: Optional[int] = None, frame_window=None,
                    optional_wildcards: bool = False) -> CtcWildcardAlignment:
    """The same for log-probabilities used as they stand (the counterpart of ctc_alignment_from_logproba); ctc_loss_data_cls
    selects the lattice (default: ClassicCtcLossData).  check_labels keeps rejecting -2 here as well."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _wildcard_align(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                           max_label_length, frame_window, optional_wildcards)


# --------------------------------------------------------------------------------------------------
# long-form forced alignment (a whole recording against its transcript): an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcLongAlignment(NamedTuple):
    """score [batch] float32: log-probability of the best path (-inf: no path exists);
    tokens [batch, max_length] int32: the token every frame emits on it (-1 beyond logit_length);
    label_index [batch, max_length] int32: index into labels[b] of the label the frame emits or, on the classic lattice, continues
    by repeating it; -1 on blank frames and beyond logit_length;
    first_frame, last_frame [batch, U] int32: the first and last frame of every label (-1 from label_length on), U the bound on the
    label length the call ran with (the width of `labels`, or max_label_length).
    An infeasible sample has score = -inf and -1 in every frame and label."""
    score: torch.Tensor
    tokens: torch.Tensor
    label_index: torch.Tensor
    first_frame: torch.Tensor
    last_frame: torch.Tensor


def _long_align(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, frames_per_tile=None,
                max_label_length=None) -> CtcLongAlignment:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    with torch.no_grad():  # a path is not differentiable: the result is detached
        prep = ops.Prepared(labels, x.detach(), label_length, logit_length, _blank(blank_index), keep_format=True,
                            host_max_label_length=max_label_length)
        return CtcLongAlignment(*ops.long_best_path(ops.KINDS[kind_name], wrt, prep, 0 if frames_per_tile is None else int(frames_per_tile)))


def classic_ctc_long_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                               blank_index: Union[int, torch.Tensor] = 0, *, frames_per_tile: Optional[int] = None,
                               max_label_length: Optional[int] = None) -> CtcLongAlignment:
    """Forced alignment of a long recording on the classic lattice: the path of classic_ctc_alignment for transcripts of up to
    65536 labels (that call stops at 1024), with the first and last frame of every label.  The lattice is tiled over blocks of 1024
    labels and of `frames_per_tile` frames (None: 128; otherwise a positive multiple of 4) and swept one anti-diagonal of tiles per
    kernel launch, so that one long utterance spreads over many compute units; smaller tiles mean more of them side by side and
    more launches.  The path does not depend on frames_per_tile.  Arguments otherwise as classic_ctc_alignment (float32 /
    bfloat16 / float16 logits, any batch / time strides, read in place); wildcards are not supported here.  Returns
    CtcLongAlignment, not differentiable."""
    return _long_align("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, frames_per_tile,
                       max_label_length)


def simplified_ctc_long_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                  blank_index: Union[int, torch.Tensor] = 0, *, frames_per_tile: Optional[int] = None,
                                  max_label_length: Optional[int] = None) -> CtcLongAlignment:
    """The same on the simplified lattice (every non-blank frame emits exactly one label).  Same arguments and return value as
    classic_ctc_long_alignment."""
    return _long_align("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, frames_per_tile,
                       max_label_length)


def ctc_long_alignment_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                     frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None) -> CtcLongAlignment:
    """The same for log-probabilities used as they stand (the counterpart of ctc_alignment_from_logproba); ctc_loss_data_cls
    selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_align(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index, frames_per_tile,
                       max_label_length)


# --------------------------------------------------------------------------------------------------
# long-form forced alignment of partial transcripts (wildcard labels beyond 1024 labels): an extension, no counterpart in the reference
# --------------------------------------------------------------------------------------------------
class CtcLongWildcardAlignment(NamedTuple):
    """The fields of CtcWildcardAlignment, with their meaning, for transcripts of up to 65536 labels:
    score [batch] float32; tokens, label_index [batch, max_length] int32; first_frame, last_frame [batch, U] int32;
    label_score [batch, U] float32.  An infeasible sample has score = -inf, -1 in every frame and label and -inf in label_score."""
    score: torch.Tensor
    tokens: torch.Tensor
    label_index: torch.Tensor
    first_frame: torch.Tensor
    last_frame: torch.Tensor
    label_score: torch.Tensor


def _long_wildcard_align(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, frames_per_tile=None,
                         max_label_length=None, frame_window=None) -> CtcLongWildcardAlignment:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    with torch.no_grad():  # a path is not differentiable: the result is detached
        prep = ops.Prepared(labels, x.detach(), label_length, logit_length, _blank(blank_index), keep_format=True,
                            host_max_label_length=max_label_length)
        fpt = 0 if frames_per_tile is None else int(frames_per_tile)
        if frame_window is None:
            return CtcLongWildcardAlignment(*ops.long_wildcard_best_path(ops.KINDS[kind_name], wrt, prep, fpt))
        return CtcLongWildcardAlignment(*ops.long_wildcard_best_path(ops.KINDS[kind_name], wrt, prep, fpt, _as_tensor(frame_window)))


def classic_ctc_long_wildcard_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                        blank_index: Union[int, torch.Tensor] = 0, *, frames_per_tile: Optional[int] = None,
                                        max_label_length: Optional[int] = None, frame_window=None) -> CtcLongWildcardAlignment:
    """Forced alignment of a long recording against a partial transcript, on the classic lattice: classic_ctc_wildcard_alignment
    (a label equal to WILDCARD, -2, stands for any non-empty run of frames with any tokens on them; every label gets its first and
    last frame and a label_score) for transcripts of up to 65536 labels, computed on the tiled lattice of
    classic_ctc_long_alignment (`frames_per_tile`: None for 128, otherwise a positive multiple of 4).  The path and the per-label
    outputs do not depend on frames_per_tile.  Returns CtcLongWildcardAlignment, not differentiable.  check_labels keeps rejecting
    -2: it validates transcripts for the loss functions.  frame_window as in classic_ctc_wildcard_alignment, in absolute frames:
    approximate timestamps (subtitles, a coarse first pass) pin every label so the path cannot drift into a repeated phrase; every
    tile of the lattice still runs."""
    return _long_wildcard_align("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, frames_per_tile,
                                max_label_length, frame_window)


def simplified_ctc_long_wildcard_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                           blank_index: Union[int, torch.Tensor] = 0, *, frames_per_tile: Optional[int] = None,
                                           max_label_length: Optional[int] = None, frame_window=None) -> CtcLongWildcardAlignment:
    """The same on the simplified lattice (a wildcard owns every frame from its entry until the next label's frame).  Same arguments
    and return value as classic_ctc_long_wildcard_alignment."""
    return _long_wildcard_align("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                frames_per_tile, max_label_length, frame_window)


def ctc_long_wildcard_alignment_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                              frames_per_tile: Optional[int] = None,
                                              max_label_length: Optional[int] = None, frame_window=None) -> CtcLongWildcardAlignment:
    """The same for log-probabilities used as they stand; ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_wildcard_align(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                                frames_per_tile, max_label_length, frame_window)


# --------------------------------------------------------------------------------------------------
# training on partial transcripts (wildcard labels): an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class _WildcardLossFn(torch.autograd.Function):
    """loss[B] of ops.wildcard_loss_grad with a gradient for the input: forward is the forward-only launch and keeps nothing but
    the inputs; backward is ONE ops.wildcard_loss_grad call with d_loss (where the loss is +inf the incoming gradient is not
    interpreted).  Backward is not itself differentiable: a second derivative raises."""

    @staticmethod
    def forward(ctx, x, labels, label_length, logit_length, kind, wrt, blank, U, weight, frame_window, optional_wildcards=False):
        ctx.save_for_backward(x, labels, label_length, logit_length)
        ctx.call = (kind, wrt, blank, U, weight)
        ctx.window = {} if frame_window is None else {"frame_window": frame_window}  # (no window: the call as it always was)
        if optional_wildcards:
            ctx.window["optional_wildcards"] = True
        return ops.wildcard_loss_grad(kind, wrt, labels, x, label_length, logit_length, blank, None, U,
                                      wildcard_log_weight=weight, want_grad=False, **ctx.window)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        x, labels, label_length, logit_length = ctx.saved_tensors
        kind, wrt, blank, U, weight = ctx.call
        _, grad = ops.wildcard_loss_grad(kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype=x.dtype,
                                         wildcard_log_weight=weight, **ctx.window)
        return grad, None, None, None, None, None, None, None, None, None, None


def _no_window_with_optional(frame_window, optional_wildcards):
    if optional_wildcards and frame_window is not None:
        raise ValueError("frame_window and optional_wildcards=True cannot be combined")


def _wildcard_loss(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, wildcard_log_weight,
                   max_label_length=None, frame_window=None, optional_wildcards=False) -> torch.Tensor:
    _no_window_with_optional(frame_window, optional_wildcards)
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    weight = float(wildcard_log_weight)
    if not (weight <= 0.0) or weight == float("-inf"):
        raise ValueError(f"wildcard_log_weight must be finite and <= 0, got {wildcard_log_weight}")
    U = None if max_label_length is None else max(0, min(int(labels.shape[1]), int(max_label_length)))
    kind = ops.KINDS[kind_name]
    window = {} if frame_window is None else {"frame_window": _as_tensor(frame_window)}
    if optional_wildcards:
        window["optional_wildcards"] = True
    if x.requires_grad and torch.is_grad_enabled():
        return _WildcardLossFn.apply(x, labels, label_length, logit_length, kind, wrt, _blank(blank_index), U, weight,
                                     window.get("frame_window"), bool(optional_wildcards))
    with torch.no_grad():  # forward only: the result is detached
        return ops.wildcard_loss_grad(kind, wrt, labels, x.detach(), label_length, logit_length, _blank(blank_index), None, U,
                                      wildcard_log_weight=weight, want_grad=False, **window)[0]


def classic_ctc_wildcard_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                              blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                              max_label_length: Optional[int] = None, frame_window=None,
                              optional_wildcards: bool = False) -> torch.Tensor:
    """CTC loss of a partial transcript on the classic lattice (wildcard CTC / star temporal classification).  As classic_ctc_loss,
    but a label equal to WILDCARD (-2) stands for any non-empty run of frames with any tokens on them: the lattice of
    classic_ctc_wildcard_alignment, summed over all its paths instead of maximised.  Returns loss [batch] float32 = -ln Z, with a
    first-order gradient when the logits require one (float32 / bfloat16 / float16 logits, any batch / time strides, read in place;
    the gradient comes back in the logits' dtype and layout; a second derivative raises).  Z is a sum over lattice paths, NOT a
    probability: one token sequence can match under several segmentations, so the loss may be negative.  wildcard_log_weight <= 0
    is added to the log-emission of every wildcard frame (STC's per-frame penalty against that).  An infeasible sample (too few
    frames -- every wildcard needs one --, a malformed label) has loss +inf and a zero gradient.  check_labels keeps rejecting -2.
    frame_window [batch, U, 2] int32 / int64 on the logits' device, (first, last) inclusive per
    label position -- the convention of first_frame / last_frame; see ctc_frame_window -- lets position i own frame t only if
    first <= t <= last: the time-restricted loss of latency-controlled training (every token within a
    tolerance of a reference alignment).  Paths outside the windows are left out of Z, so the loss is at least the unconstrained
    one; windows that admit no path give +inf and a zero gradient.  A transcript without wildcards is plain CTC with windows.
    optional_wildcards=True also accepts OPTIONAL_WILDCARD (-3): a wildcard position that may take no frame at all (the star of
    star temporal classification, "something may be missing here").  Z then sums over every choice of used and skipped optional
    positions; two of them may not be adjacent (+inf); it cannot be combined with frame_window (ValueError).  With False, -3 is a
    malformed label as before."""
    return _wildcard_loss("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, wildcard_log_weight,
                          max_label_length, frame_window, optional_wildcards)


def simplified_ctc_wildcard_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                 blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                 max_label_length: Optional[int] = None, frame_window=None,
                                 optional_wildcards: bool = False) -> torch.Tensor:
    """The same on the simplified lattice: entering a wildcard and every stay behind it emit the wildcard's weight instead of a
    token's or the blank's probability.  Same arguments and return value as classic_ctc_wildcard_loss."""
    return _wildcard_loss("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, wildcard_log_weight,
                          max_label_length, frame_window, optional_wildcards)


def ctc_wildcard_loss_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                    wildcard_log_weight: float = 0.0, max_label_length: Optional[int] = None,
                                    frame_window=None, optional_wildcards: bool = False) -> torch.Tensor:
    """The same for log-probabilities used as they stand: a wildcard frame emits wildcard_log_weight + logsumexp(logprobas[t]);
    ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData).  The gradient is with respect to logprobas."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _wildcard_loss(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                          wildcard_log_weight, max_label_length, frame_window, optional_wildcards)


# --------------------------------------------------------------------------------------------------
# long-form loss and gradient (transcripts beyond 1024 labels, wildcards included): an extension, no counterpart in the reference
# --------------------------------------------------------------------------------------------------
def _long_loss_call(frame_window, optional_wildcards=False):
    """ops.long_wildcard_loss_grad, or with a window ops.long_windowed_loss_grad bound to it (no window: the call as it always was);
    with optional wildcards ops.long_optional_wildcard_loss_grad."""
    if optional_wildcards:
        return ops.long_optional_wildcard_loss_grad
    if frame_window is None:
        return ops.long_wildcard_loss_grad
    return partial(ops.long_windowed_loss_grad, frame_window)


class _LongLossFn(torch.autograd.Function):
    """_WildcardLossFn on ops.long_wildcard_loss_grad: forward is the forward-only call and keeps nothing but the inputs; backward is
    ONE call with d_loss.  Backward is not itself differentiable: a second derivative raises."""

    @staticmethod
    def forward(ctx, x, labels, label_length, logit_length, kind, wrt, blank, U, weight, tf, checkpoint, frame_window,
                optional_wildcards=False):
        ctx.save_for_backward(x, labels, label_length, logit_length)
        ctx.call = (kind, wrt, blank, U, weight, tf, checkpoint)
        ctx.window = frame_window
        ctx.optional = optional_wildcards
        return _long_loss_call(frame_window, optional_wildcards)(kind, wrt, labels, x, label_length, logit_length, blank, None, U,
                                             wildcard_log_weight=weight, want_grad=False, frames_per_tile=tf)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        x, labels, label_length, logit_length = ctx.saved_tensors
        kind, wrt, blank, U, weight, tf, checkpoint = ctx.call
        _, grad = _long_loss_call(ctx.window, ctx.optional)(kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U,
                                                            grad_dtype=x.dtype, wildcard_log_weight=weight, frames_per_tile=tf,
                                                            checkpoint=checkpoint)
        return grad, None, None, None, None, None, None, None, None, None, None, None, None


def _long_loss(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, wildcard_log_weight,
               frames_per_tile=None, max_label_length=None, checkpoint=False, frame_window=None, optional_wildcards=False) -> torch.Tensor:
    _no_window_with_optional(frame_window, optional_wildcards)
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    weight = float(wildcard_log_weight)
    if not (weight <= 0.0) or weight == float("-inf"):
        raise ValueError(f"wildcard_log_weight must be finite and <= 0, got {wildcard_log_weight}")
    U = None if max_label_length is None else max(0, min(int(labels.shape[1]), int(max_label_length)))
    kind = ops.KINDS[kind_name]
    tf = 0 if frames_per_tile is None else int(frames_per_tile)
    window = None if frame_window is None else _as_tensor(frame_window)
    if x.requires_grad and torch.is_grad_enabled():
        return _LongLossFn.apply(x, labels, label_length, logit_length, kind, wrt, _blank(blank_index), U, weight, tf, bool(checkpoint),
                                 window, bool(optional_wildcards))
    with torch.no_grad():  # forward only: the result is detached
        return _long_loss_call(window, bool(optional_wildcards))(kind, wrt, labels, x.detach(), label_length, logit_length, _blank(blank_index), None, U,
                                       wildcard_log_weight=weight, want_grad=False, frames_per_tile=tf)[0]


def classic_ctc_long_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                          blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                          frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None,
                          checkpoint: bool = False, optional_wildcards: bool = False, frame_window=None) -> torch.Tensor:
    """CTC loss of a long recording on the classic lattice: classic_ctc_wildcard_loss (without a WILDCARD label, -2, the plain CTC
    loss; with one, the loss of a partial transcript) for transcripts of up to 65536 labels, computed on the tiled lattice of
    classic_ctc_long_alignment (`frames_per_tile`: None for 128, otherwise a positive multiple of 4; the loss and the gradient do not
    depend on it).  Returns loss [batch] float32 = -ln Z with a first-order gradient when the logits require one (float32 / bfloat16
    / float16 logits, any batch / time strides, read in place; the gradient comes back in the logits' dtype and layout; a second
    derivative raises).  An infeasible sample has loss +inf and a zero gradient.  Backward holds the lattice's float64 state of
    every frame: 8 * batch * ceil(U / 1024) * max_length * 2050 bytes (half of that on the simplified lattice); forward alone holds
    no per-frame state.  checkpoint=True gives the same bits in loss and gradient from a backward that keeps one chain row per tile
    and the per-frame state of min(K, J) time blocks only (K = ceil(U / 1024), J = ceil(max_length / TF), TF = frames_per_tile):
    8 * batch * K * (J * 2056 + min(K, J) * TF * 2050) bytes in place of the term above (1026 for 2050 on the simplified lattice),
    23 times less at ten minutes of audio, and an hour (180 000 frames, 50 000 labels) takes 6.4 GB in place of 144.9 GB; it costs
    one more forward sweep, and frames_per_tile then trades memory: the ring grows with it, the checkpoints shrink.  Forward is the
    same call either way.  check_labels keeps rejecting -2.  frame_window [batch, U, 2] as in classic_ctc_wildcard_loss, in absolute
    frames and for every label block: the windows ctc_frame_window makes of a classic_ctc_long_wildcard_alignment hold every token of
    the recording within a tolerance of that alignment, with either `checkpoint` setting and the same bits from both; no result
    depends on where a window's edges fall relative to tiles.  The workspaces are those of the unwindowed call.
    optional_wildcards=True also accepts OPTIONAL_WILDCARD (-3), a wildcard position that may take no frame, as in
    classic_ctc_wildcard_loss and with its definition, at any length up to 65536: a lightly supervised transcript of a long recording,
    or a star between every pair of labels (then L positions need only about L / 2 frames).  Two of them may not be adjacent (+inf, a
    zero gradient), wherever the pair falls; both `checkpoint` settings give the same bits; without a -3 the bits are those of False;
    the workspace holds 24 * batch * (K - 1) * max_length bytes more.  It cannot be combined with frame_window (ValueError).  With
    False, -3 is a bad label as before."""
    return _long_loss("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, wildcard_log_weight,
                      frames_per_tile, max_label_length, checkpoint, frame_window, optional_wildcards)


def simplified_ctc_long_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                             blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                             frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None,
                             checkpoint: bool = False, optional_wildcards: bool = False, frame_window=None) -> torch.Tensor:
    """The same on the simplified lattice.  Same arguments and return value as classic_ctc_long_loss; backward holds
    8 * batch * K * max_length * 1026 bytes, with checkpoint=True 8 * batch * K * (J * 2056 + min(K, J) * TF * 1026), the same bits.
    frame_window as in classic_ctc_long_loss: a wildcard's horizontal frames obey its window too.  optional_wildcards as in
    classic_ctc_long_loss, with the definition of simplified_ctc_wildcard_loss."""
    return _long_loss("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, wildcard_log_weight,
                      frames_per_tile, max_label_length, checkpoint, frame_window, optional_wildcards)


def ctc_long_loss_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                max_label_length: Optional[int] = None, checkpoint: bool = False, optional_wildcards: bool = False,
                                frame_window=None) -> torch.Tensor:
    """The same for log-probabilities used as they stand; ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData).  The
    gradient is with respect to logprobas.  checkpoint and both workspace formulas as in classic_ctc_long_loss /
    simplified_ctc_long_loss: the same bits from the smaller workspace.  frame_window and optional_wildcards as in
    classic_ctc_long_loss."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_loss(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index, wildcard_log_weight,
                      frames_per_tile, max_label_length, checkpoint, frame_window, optional_wildcards)


# --------------------------------------------------------------------------------------------------
# label posteriors (soft alignment over all paths): an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcLabelPosterior(NamedTuple):
    """loss [batch] float32: -ln Z, the bits of the wildcard loss on the same arguments (+inf: no path);
    label_posterior [batch, max_length, U] float32: the probability, over all alignments, that frame t belongs to label position i
    (per position, not per token: a repeated label and every wildcard keep their own columns), U the bound on the label length
    the call ran with (the width of `labels`, or max_label_length);
    blank_posterior [batch, max_length] float32: the probability that frame t is a blank outside any label; each frame's
    label_posterior and blank_posterior sum to 1;
    duration [batch, U] float32: the expected number of frames of every position, the sum of its label_posterior column;
    expected_frame [batch, U] float32: its soft timestamp, sum_t t * label_posterior / duration (-1 from label_length on).
    Frames beyond logit_length and positions from label_length on are 0; an infeasible sample has loss +inf, zeros, and -1 in
    expected_frame."""
    loss: torch.Tensor
    label_posterior: torch.Tensor
    blank_posterior: torch.Tensor
    duration: torch.Tensor
    expected_frame: torch.Tensor


def _label_posterior(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, wildcard_log_weight,
                     max_label_length=None, frame_window=None, optional_wildcards=False) -> CtcLabelPosterior:
    _no_window_with_optional(frame_window, optional_wildcards)
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    weight = float(wildcard_log_weight)
    if not (weight <= 0.0) or weight == float("-inf"):
        raise ValueError(f"wildcard_log_weight must be finite and <= 0, got {wildcard_log_weight}")
    U = None if max_label_length is None else max(0, min(int(labels.shape[1]), int(max_label_length)))
    window = {} if frame_window is None else {"frame_window": _as_tensor(frame_window)}
    if optional_wildcards:
        window["optional_wildcards"] = True
    with torch.no_grad():  # forward only: the result is detached
        return CtcLabelPosterior(*ops.label_posterior(ops.KINDS[kind_name], wrt, labels, x.detach(), label_length, logit_length,
                                                      _blank(blank_index), U, wildcard_log_weight=weight, **window))


def classic_ctc_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                max_label_length: Optional[int] = None, frame_window=None,
                                optional_wildcards: bool = False) -> CtcLabelPosterior:
    """The soft alignment of a transcript on the classic lattice: the occupancy matrix of a forward-backward pass, where
    classic_ctc_alignment returns the single best path.  label_posterior[b, t, i] is the probability that frame t emits label
    position i; a frame's remaining mass is blank_posterior[b, t].  Labels may contain WILDCARD (-2), with the lattice and
    wildcard_log_weight of classic_ctc_wildcard_loss; without one this is plain CTC.  Arguments as classic_ctc_wildcard_loss
    (float32 / bfloat16 / float16 logits, any batch / time strides, read in place); returns CtcLabelPosterior, float32 on the
    logits' device, not differentiable.  check_labels keeps rejecting -2.  frame_window as in classic_ctc_wildcard_loss:
    label_posterior is exactly 0 outside a position's window and every frame still sums to 1.  optional_wildcards as in
    classic_ctc_wildcard_loss: the column of an OPTIONAL_WILDCARD (-3) may sum to less than one frame (duration >= 0, expected_frame
    -1 where it is 0); every frame still sums to 1."""
    return _label_posterior("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, wildcard_log_weight,
                            max_label_length, frame_window, optional_wildcards)


def simplified_ctc_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                   blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                   max_label_length: Optional[int] = None, frame_window=None,
                                   optional_wildcards: bool = False) -> CtcLabelPosterior:
    """The same on the simplified lattice: label_posterior[b, t, i] is the probability that label i is emitted at frame t (so an
    ordinary label's duration is 1 and expected_frame is its expected emission frame); a wildcard also owns the frames spent
    behind it.  Same arguments and return value as classic_ctc_label_posterior."""
    return _label_posterior("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                            wildcard_log_weight, max_label_length, frame_window, optional_wildcards)


def ctc_label_posterior_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                      wildcard_log_weight: float = 0.0, max_label_length: Optional[int] = None,
                                      frame_window=None, optional_wildcards: bool = False) -> CtcLabelPosterior:
    """The same for log-probabilities used as they stand (a wildcard frame emits wildcard_log_weight + logsumexp(logprobas[t]));
    ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _label_posterior(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                            wildcard_log_weight, max_label_length, frame_window, optional_wildcards)


# --------------------------------------------------------------------------------------------------
# long-form label posteriors (soft timestamps of transcripts beyond 1024 labels): an extension, no counterpart in the reference
# --------------------------------------------------------------------------------------------------
class CtcLongLabelPosterior(NamedTuple):
    """loss, label_posterior, blank_posterior, duration, expected_frame: as CtcLabelPosterior, for up to 65536 label positions;
    label_posterior is None when the call ran with dense=False (the [batch, max_length, U] matrix is then never allocated).
    duration and expected_frame are float64 reductions of the float32 label_posterior values, summed sequentially from the last
    frame down to frame 0 and rounded once: a host reduction of the dense matrix in that order gives the same bits;
    peak_posterior [batch, U] float32: the largest label_posterior of every position over the frames, the per-label confidence that
    needs no dense matrix; peak_frame [batch, U] int32: the lowest frame that attains it.  Positions from label_length on and
    infeasible samples have 0 in peak_posterior and -1 in peak_frame."""
    loss: torch.Tensor
    label_posterior: Optional[torch.Tensor]
    blank_posterior: torch.Tensor
    duration: torch.Tensor
    expected_frame: torch.Tensor
    peak_posterior: torch.Tensor
    peak_frame: torch.Tensor


def _long_label_posterior(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, wildcard_log_weight,
                          frames_per_tile=None, max_label_length=None, dense=True, frame_window=None,
                          optional_wildcards=False) -> CtcLongLabelPosterior:
    _no_window_with_optional(frame_window, optional_wildcards)
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    weight = float(wildcard_log_weight)
    if not (weight <= 0.0) or weight == float("-inf"):
        raise ValueError(f"wildcard_log_weight must be finite and <= 0, got {wildcard_log_weight}")
    U = None if max_label_length is None else max(0, min(int(labels.shape[1]), int(max_label_length)))
    tf = 0 if frames_per_tile is None else int(frames_per_tile)
    window = {} if frame_window is None else {"frame_window": _as_tensor(frame_window)}
    with torch.no_grad():  # forward only: the result is detached
        if optional_wildcards:
            return CtcLongLabelPosterior(*ops.long_optional_wildcard_label_posterior(
                ops.KINDS[kind_name], wrt, labels, x.detach(), label_length, logit_length, _blank(blank_index), U,
                wildcard_log_weight=weight, frames_per_tile=tf, dense=bool(dense)))
        return CtcLongLabelPosterior(*ops.long_label_posterior(ops.KINDS[kind_name], wrt, labels, x.detach(), label_length, logit_length,
                                                               _blank(blank_index), U, wildcard_log_weight=weight, frames_per_tile=tf,
                                                               dense=bool(dense), **window))


def classic_ctc_long_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                     blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                     frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None,
                                     dense: bool = True) -> CtcLongLabelPosterior:
    """The soft alignment of a long recording on the classic lattice: classic_ctc_label_posterior for transcripts of up to 65536
    labels, on the tiled lattice and from the workspace of classic_ctc_long_loss(checkpoint=True) (`frames_per_tile`: None for 128,
    otherwise a positive multiple of 4; no output depends on it).  Which stretches of a long alignment to trust: where
    classic_ctc_long_alignment gives the single best path, this gives per label position the probability of every frame, the
    expected duration, the soft timestamp, and the peak posterior with its frame.  dense=False leaves the
    [batch, max_length, U] float32 matrix out (36 GB for an hour of audio with 50 000 labels) and returns None in its place; every
    other output keeps its bits, the per-label statistics coming straight from the sweep.  Labels may contain WILDCARD (-2).
    Arguments as classic_ctc_long_loss; returns CtcLongLabelPosterior on the logits' device, not differentiable.  With frame
    windows: classic_ctc_long_windowed_label_posterior."""
    return _long_label_posterior("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense)


def simplified_ctc_long_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                        blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                        frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None,
                                        dense: bool = True) -> CtcLongLabelPosterior:
    """The same on the simplified lattice (label_posterior as in simplified_ctc_label_posterior).  Same arguments and return value
    as classic_ctc_long_label_posterior."""
    return _long_label_posterior("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense)


def ctc_long_label_posterior_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None, *,
                                           wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                           max_label_length: Optional[int] = None, dense: bool = True) -> CtcLongLabelPosterior:
    """The same for log-probabilities used as they stand; ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_label_posterior(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense)


def classic_ctc_long_optional_wildcard_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike,
                                                       logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                                                       wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                                       max_label_length: Optional[int] = None,
                                                       dense: bool = True) -> CtcLongLabelPosterior:
    """classic_ctc_long_label_posterior for transcripts that may also hold OPTIONAL_WILDCARD (-3), a wildcard position that may take
    no frame: classic_ctc_label_posterior(optional_wildcards=True) at up to 65536 labels.  The loss is
    classic_ctc_long_loss(optional_wildcards=True)'s, bit for bit; the column of an optional position may sum to less than one frame
    and its duration is the expected number of frames it takes (about 0: the position was skipped); every frame's label_posterior and
    blank_posterior still sum to 1.  Two adjacent -3 make the sample infeasible (loss +inf, zeros, expected_frame -1).  dense=False
    as in classic_ctc_long_label_posterior.  (A function of its own because the signature of that one is kept as it is.)  Returns
    CtcLongLabelPosterior on the logits' device, not differentiable."""
    return _long_label_posterior("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, None, True)


def simplified_ctc_long_optional_wildcard_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike,
                                                          logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                                                          wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                                          max_label_length: Optional[int] = None,
                                                          dense: bool = True) -> CtcLongLabelPosterior:
    """The same on the simplified lattice: simplified_ctc_long_label_posterior with optional wildcards.  Same arguments and return
    value as classic_ctc_long_optional_wildcard_label_posterior."""
    return _long_label_posterior("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, None, True)


def ctc_long_optional_wildcard_label_posterior_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0,
                                                             ctc_loss_data_cls=None, *, wildcard_log_weight: float = 0.0,
                                                             frames_per_tile: Optional[int] = None,
                                                             max_label_length: Optional[int] = None,
                                                             dense: bool = True) -> CtcLongLabelPosterior:
    """The same for log-probabilities used as they stand; ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_label_posterior(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, None, True)


def classic_ctc_long_windowed_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                              blank_index: Union[int, torch.Tensor] = 0, *, wildcard_log_weight: float = 0.0,
                                              frames_per_tile: Optional[int] = None, max_label_length: Optional[int] = None,
                                              dense: bool = True, frame_window=None) -> CtcLongLabelPosterior:
    """classic_ctc_long_label_posterior with frame windows: frame_window [batch, U, 2] as in classic_ctc_long_loss, in absolute
    frames and for every label block (see ctc_frame_window).  The loss is the windowed long loss's, label_posterior is exactly 0
    outside a position's window and every frame still sums to 1; dense=False works with windows.  frame_window=None is
    classic_ctc_long_label_posterior, bit for bit.  (A function of its own because the signature of the unwindowed one is kept as it
    is.)  Returns CtcLongLabelPosterior on the logits' device, not differentiable."""
    return _long_label_posterior("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, frame_window)


def simplified_ctc_long_windowed_label_posterior(labels: TensorLike, logits: TensorLike, label_length: TensorLike,
                                                 logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                                                 wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                                 max_label_length: Optional[int] = None, dense: bool = True,
                                                 frame_window=None) -> CtcLongLabelPosterior:
    """The same on the simplified lattice: simplified_ctc_long_label_posterior with frame windows.  Same arguments and return value
    as classic_ctc_long_windowed_label_posterior."""
    return _long_label_posterior("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, frame_window)


def ctc_long_windowed_label_posterior_from_logproba(labels, logprobas, label_length, logit_length, blank_index=0, ctc_loss_data_cls=None,
                                                    *, wildcard_log_weight: float = 0.0, frames_per_tile: Optional[int] = None,
                                                    max_label_length: Optional[int] = None, dense: bool = True,
                                                    frame_window=None) -> CtcLongLabelPosterior:
    """The same for log-probabilities used as they stand; ctc_loss_data_cls selects the lattice (default: ClassicCtcLossData)."""
    kind_name = "classic" if ctc_loss_data_cls is None else ctc_loss_data_cls.kind_name
    return _long_label_posterior(kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                                 wildcard_log_weight, frames_per_tile, max_label_length, dense, frame_window)


# --------------------------------------------------------------------------------------------------
# greedy decoding: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcDecoding(NamedTuple):
    """score [batch] float32: log-probability of the frame-wise argmax path (the best of ALL paths);
    tokens [batch, max_length] int32: the token of every frame on it, ties to the lowest index (-1 beyond logit_length);
    labels [batch, max_length] int32: the path collapsed as the lattice reads it (-1 beyond label_length);
    label_length [batch] int32;
    frames [batch, max_length] int32: the first frame of every decoded label (-1 padding);
    label_score [batch, max_length] float32: the log-probability of every decoded label's frames -- classic: the unbroken repeat
    that starts at its first frame; simplified: that one frame (-inf padding).
    labels and label_length can be passed straight to the loss and alignment functions of the same lattice."""
    score: torch.Tensor
    tokens: torch.Tensor
    labels: torch.Tensor
    label_length: torch.Tensor
    frames: torch.Tensor
    label_score: torch.Tensor


def _decode(kind_name: str, wrt: int, x, logit_length, blank_index) -> CtcDecoding:
    x = _as_tensor(x)
    logit_length = _as_tensor(logit_length, torch.int32)
    assert x.dim() == 3
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    assert logit_length.dim() == 1
    assert x.shape[0] == logit_length.shape[0]
    with torch.no_grad():  # a decoding is not differentiable: the result is detached
        return CtcDecoding(*ops.greedy_decode(ops.KINDS[kind_name], wrt, x.detach(), logit_length, _blank(blank_index)))


def classic_ctc_greedy_decode(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0) -> CtcDecoding:
    """Greedy decoding on the classic lattice: the most probable token of every frame, repeats merged, then blanks dropped.
    logits [batch, max_length, num_tokens] float32 / bfloat16 / float16 (any batch / time strides), logit_length [batch];
    returns CtcDecoding(score, tokens, labels, label_length, frames, label_score), not differentiable."""
    return _decode("classic", _lib.WRT_LOGITS, logits, logit_length, blank_index)


def simplified_ctc_greedy_decode(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0) -> CtcDecoding:
    """Greedy decoding on the simplified lattice (blanks are dropped, repeats are not merged: every non-blank frame is a label).
    Same arguments and return value as classic_ctc_greedy_decode."""
    return _decode("simplified", _lib.WRT_LOGITS, logits, logit_length, blank_index)


def ctc_greedy_decode_from_logproba(logprobas, logit_length, blank_index, ctc_loss_data_cls) -> CtcDecoding:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba)."""
    return _decode(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, logprobas, logit_length, blank_index)


# --------------------------------------------------------------------------------------------------
# prefix beam search: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcBeamDecoding(NamedTuple):
    """score [batch, nbest] float32: ln of each hypothesis' probability, summed over its alignments inside the beam, best first
    (-inf: fewer than nbest hypotheses are alive);
    labels [batch, nbest, max_length] int32 (-1 beyond label_length); label_length [batch, nbest] int32.
    labels[:, n] and label_length[:, n] can be passed straight to the loss and alignment functions of the same lattice."""
    score: torch.Tensor
    labels: torch.Tensor
    label_length: torch.Tensor


def _beam(kind_name: str, wrt: int, x, logit_length, blank_index, beam_width, top_k, nbest) -> CtcBeamDecoding:
    x = _as_tensor(x)
    logit_length = _as_tensor(logit_length, torch.int32)
    assert x.dim() == 3
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    assert logit_length.dim() == 1
    assert x.shape[0] == logit_length.shape[0]
    with torch.no_grad():  # a decoding is not differentiable: the result is detached
        return CtcBeamDecoding(*ops.beam_search(ops.KINDS[kind_name], wrt, x.detach(), logit_length, _blank(blank_index),
                                                beam_width, top_k, nbest))


def classic_ctc_beam_search(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                            beam_width: int = 16, top_k: int = 16, nbest: int = 1) -> CtcBeamDecoding:
    """Prefix beam search on the classic lattice: the `nbest` most probable label sequences among the `beam_width` kept per
    frame, each frame extending prefixes by the blank and its `top_k` most probable non-blank tokens only.
    logits [batch, max_length, num_tokens] float32 / bfloat16 / float16 (any batch / time strides), logit_length [batch];
    beam_width <= 64, top_k <= 32, nbest <= beam_width.  Returns CtcBeamDecoding(score, labels, label_length), not differentiable."""
    return _beam("classic", _lib.WRT_LOGITS, logits, logit_length, blank_index, beam_width, top_k, nbest)


def simplified_ctc_beam_search(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                               beam_width: int = 16, top_k: int = 16, nbest: int = 1) -> CtcBeamDecoding:
    """Prefix beam search on the simplified lattice (every non-blank frame is a label).  Same arguments and return value as
    classic_ctc_beam_search."""
    return _beam("simplified", _lib.WRT_LOGITS, logits, logit_length, blank_index, beam_width, top_k, nbest)


def ctc_beam_search_from_logproba(logprobas, logit_length, blank_index, ctc_loss_data_cls, *, beam_width: int = 16, top_k: int = 16,
                                  nbest: int = 1) -> CtcBeamDecoding:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba)."""
    return _beam(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, logprobas, logit_length, blank_index, beam_width, top_k, nbest)


# --------------------------------------------------------------------------------------------------
# CTC prefix scores, the step-wise scorer of label-synchronous decoding: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcPrefixState(NamedTuple):
    """A beam of N prefixes per utterance.  state [batch, N, 2 * max_length + 2] float64: opaque, the forward variables of every
    prefix; last_token, length [batch, N] int32 (-1 and -1: a dead slot); full_score [batch, N] float32: ln P(prefix | logits), the
    probability of the prefix as the whole label sequence; parent [batch, N] int32: the slot of the beam it was extended from
    (what a caller reorders its own decoder or language-model state by; None for an initial state)."""
    state: torch.Tensor
    last_token: torch.Tensor
    length: torch.Tensor
    full_score: torch.Tensor
    parent: Optional[torch.Tensor] = None


class CtcPrefixScorer:
    """The CTC head as a step-wise scorer (Watanabe et al. 2017): score(state)[b, n, c] = ln psi(g . c), the probability of all
    label sequences that start with prefix g of slot (b, n) followed by token c, and extend(state, parent, token) carries the
    beam forward.  The row statistics of the logits are computed once, here; nothing is differentiable."""

    def __init__(self, kind_name: str, wrt: int, x, logit_length, blank_index):
        x = _as_tensor(x)
        logit_length = _as_tensor(logit_length, torch.int32)
        assert x.dim() == 3
        assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
        assert logit_length.dim() == 1
        assert x.shape[0] == logit_length.shape[0]
        self.kind_name, self.kind, self.wrt, self.blank = kind_name, ops.KINDS[kind_name], wrt, _blank(blank_index)
        with torch.no_grad():
            self.x, self.logit_length, self.rows = ops.prefix_prepare(wrt, x.detach(), logit_length)
        self.batch, self.max_length, self.num_tokens = (int(s) for s in self.x.shape)

    def _args(self):
        return self.kind, self.wrt, self.x, self.logit_length, self.blank, self.rows

    def initial_state(self, N: int) -> CtcPrefixState:
        """N slots per utterance: the empty prefix in slot 0, the others dead."""
        N = int(N)
        parent = torch.full((self.batch, N), -1, dtype=torch.int32, device=self.x.device)
        parent[:, :1] = -2
        with torch.no_grad():
            return CtcPrefixState(*ops.prefix_extend(*self._args(), N, None, None, None, parent, torch.zeros_like(parent)))

    def score(self, state: CtcPrefixState) -> torch.Tensor:
        """[batch, N, num_tokens] float32; -inf in the blank's column and in every dead slot."""
        with torch.no_grad():
            return ops.prefix_score(*self._args(), int(state.state.shape[1]), state.state, state.last_token, state.length)

    def extend(self, state: CtcPrefixState, parent: TensorLike, token: TensorLike) -> CtcPrefixState:
        """New slot (b, n) = slot (b, parent[b, n]) of `state` extended by token[b, n]; parent -1 (or a dead parent, the blank, a
        token outside the vocabulary) gives a dead slot, parent -2 the empty prefix.  parent may repeat and permute."""
        parent, token = _as_tensor(parent, torch.int32), _as_tensor(token, torch.int32)
        with torch.no_grad():
            out = ops.prefix_extend(*self._args(), int(state.state.shape[1]), state.state, state.last_token, state.length, parent, token)
        return CtcPrefixState(*out, parent)


def classic_ctc_prefix_scorer(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0) -> CtcPrefixScorer:
    """Prefix scorer on the classic lattice.  logits [batch, max_length, num_tokens] float32 / bfloat16 / float16 (any batch / time
    strides, read in place every step), logit_length [batch]; num_tokens <= 16384, at most 64 slots per utterance."""
    return CtcPrefixScorer("classic", _lib.WRT_LOGITS, logits, logit_length, blank_index)


def simplified_ctc_prefix_scorer(logits: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0) -> CtcPrefixScorer:
    """Prefix scorer on the simplified lattice (every non-blank frame is a label).  Same arguments as classic_ctc_prefix_scorer."""
    return CtcPrefixScorer("simplified", _lib.WRT_LOGITS, logits, logit_length, blank_index)


def ctc_prefix_scorer_from_logproba(logproba: TensorLike, logit_length: TensorLike, blank_index: Union[int, torch.Tensor] = 0, *,
                                    simplified: bool = False) -> CtcPrefixScorer:
    """The same for log-probabilities used as they stand (no row statistics are computed)."""
    return CtcPrefixScorer("simplified" if simplified else "classic", _lib.WRT_LOGPROBS, logproba, logit_length, blank_index)


def ctc_label_sync_beam_search(scorer: CtcPrefixScorer, beam_width: int, max_length: int, *, extra_score=None,
                               ctc_weight: float = 1.0) -> CtcBeamDecoding:
    """The textbook label-synchronous beam search over a CtcPrefixScorer: per step the prefix scores of the beam, times ctc_weight,
    plus the running sum of extra_score(state) [batch, beam_width, num_tokens] (a language model, an attention decoder, a length
    bonus: the caller's) select the beam_width best extensions among beam_width * num_tokens.  Every prefix visited is a
    candidate result, ranked by ctc_weight * full_score + its sum of extra scores.  Returns the beam_width best as
    CtcBeamDecoding(score, labels [batch, beam_width, max_length], label_length); nothing is copied to the host on the way."""
    N, V, B = int(beam_width), scorer.num_tokens, scorer.batch
    dev = scorer.x.device
    state = scorer.initial_state(N)
    extra = torch.zeros((B, N), dtype=torch.float32, device=dev)           # the beam's sums of extra scores
    labels = torch.full((B, N, int(max_length)), -1, dtype=torch.int32, device=dev)
    best = (torch.where(state.length >= 0, ctc_weight * state.full_score, -torch.inf), labels, state.length.clamp(min=0))
    for step in range(int(max_length)):
        cand = ctc_weight * scorer.score(state) + extra[:, :, None]
        step_extra = None if extra_score is None else extra_score(state).to(torch.float32)
        if step_extra is not None:
            cand = cand + step_extra
        top, idx = cand.reshape(B, N * V).topk(N, dim=1)
        parent = torch.where(top > -torch.inf, idx // V, -1).to(torch.int32)  # (nothing left to extend: a dead slot)
        token = (idx % V).to(torch.int32)
        src = parent.clamp(min=0).long()
        labels = labels.gather(1, src[:, :, None].expand(-1, -1, labels.shape[2]))
        labels[:, :, step] = torch.where(parent >= 0, token, -1)
        extra = extra.gather(1, src)
        if step_extra is not None:
            extra = extra + torch.nan_to_num(step_extra.reshape(B, N * V).gather(1, idx), neginf=0.0)
        state = scorer.extend(state, parent, token)
        final = torch.where(state.length >= 0, ctc_weight * state.full_score + extra, -torch.inf)
        pool = (torch.cat([best[0], final], 1), torch.cat([best[1], labels], 1), torch.cat([best[2], state.length.clamp(min=0)], 1))
        keep = pool[0].topk(N, dim=1).indices
        best = (pool[0].gather(1, keep), pool[1].gather(1, keep[:, :, None].expand(-1, -1, labels.shape[2])), pool[2].gather(1, keep))
    return CtcBeamDecoding(*best)


# --------------------------------------------------------------------------------------------------
# N-best rescoring: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcNbestLoss(NamedTuple):
    """loss [batch, nbest] float32: -ln P(hypothesis | logits), summed over ALL alignments (+inf: infeasible, malformed or masked);
    log_posterior [batch, nbest] float32: -loss - logsumexp(-loss) over the list: the confidence of every hypothesis within ITS
    LIST (-inf where the loss is +inf; a list without a feasible hypothesis is -inf throughout).  The list is taken as it stands:
    a hypothesis that appears twice is counted twice."""
    loss: torch.Tensor
    log_posterior: torch.Tensor


class _NbestLossFn(torch.autograd.Function):
    """loss[B, N] of ops.nbest_loss with a gradient for the logits: forward is the forward-only launch and keeps nothing but the
    inputs; backward is ONE ops.nbest_loss_grad call with weight = d_loss (where the loss is +inf the incoming gradient is not
    interpreted: the NaN / inf that the backward of `where` and `logsumexp` produce there do no harm).  Backward is not itself
    differentiable."""

    @staticmethod
    def forward(ctx, x, labels, label_length, logit_length, kind, wrt, blank, U):
        ctx.save_for_backward(x, labels, label_length, logit_length)
        ctx.call = (kind, wrt, blank, U)
        return ops.nbest_loss(kind, wrt, labels, x, label_length, logit_length, blank, U)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        x, labels, label_length, logit_length = ctx.saved_tensors
        kind, wrt, blank, U = ctx.call
        _, grad = ops.nbest_loss_grad(kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype=x.dtype)
        return grad, None, None, None, None, None, None, None


def _nbest_tail(loss, hypothesis_mask) -> CtcNbestLoss:
    if hypothesis_mask is not None:
        mask = _as_tensor(hypothesis_mask).to(device=loss.device, dtype=torch.bool)
        assert tuple(mask.shape) == tuple(loss.shape)
        loss = torch.where(mask, loss, torch.full_like(loss, float("inf")))
    # (a list of +inf alone: logsumexp is -inf and -inf - -inf would be NaN)
    lse = torch.logsumexp(-loss, dim=1, keepdim=True) if loss.shape[1] else loss.new_zeros((loss.shape[0], 1))
    logp = torch.where(torch.isinf(loss) & (loss > 0), torch.full_like(loss, float("-inf")), -loss - lse)
    return CtcNbestLoss(loss, logp)


def _nbest(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, hypothesis_mask=None,
           max_label_length=None, differentiable=False) -> CtcNbestLoss:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    assert x.dim() == 3
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    assert labels.dim() == 3
    assert label_length.dim() == 2
    assert logit_length.dim() == 1
    assert x.shape[0] == labels.shape[0] == label_length.shape[0] == logit_length.shape[0]
    assert labels.shape[1] == label_length.shape[1]
    U = None if max_label_length is None else max(0, min(int(labels.shape[2]), int(max_label_length)))
    if differentiable and x.requires_grad and torch.is_grad_enabled():
        # the mask and the log_posterior arithmetic are ordinary torch operations on the attached loss
        loss = _NbestLossFn.apply(x, labels, label_length, logit_length, ops.KINDS[kind_name], wrt, _blank(blank_index), U)
        return _nbest_tail(loss, hypothesis_mask)
    with torch.no_grad():  # forward only: the result is detached
        loss = ops.nbest_loss(ops.KINDS[kind_name], wrt, labels, x.detach(), label_length, logit_length, _blank(blank_index), U)
        return _nbest_tail(loss, hypothesis_mask)


def classic_ctc_nbest_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                           blank_index: Union[int, torch.Tensor] = 0, *, hypothesis_mask: Optional[TensorLike] = None,
                           max_label_length: Optional[int] = None, differentiable: bool = False) -> CtcNbestLoss:
    """The exact classic CTC loss of N label sequences per utterance against the same logits, the logits read once per group of
    eight hypotheses instead of once each: what re-ranks an N-best list (the scores of classic_ctc_beam_search are sums inside
    the beam: lower bounds) and turns it into confidences.

    Args:
        labels:       [batch, nbest, max_label_length] int32 -- a CtcBeamDecoding's `labels` as it stands (padding is not read)
        logits:       [batch, max_length, num_tokens] float32 / bfloat16 / float16 (any batch / time strides)
        label_length: [batch, nbest] int32
        logit_length: [batch] int32
        blank_index:  int
        hypothesis_mask: (keyword only) [batch, nbest] bool; where False the loss is +inf and the entry takes no part in the
            normalisation -- pass `isfinite(score)` for the missing hypotheses of a CtcBeamDecoding.
        max_label_length: (keyword only) as in classic_ctc_loss: an upper bound on label_length known on the host.
        differentiable: (keyword only) False (default): the result is detached, whatever the logits require.  True, with logits
            that require grad: `loss` and `log_posterior` carry a gradient for the logits, so that an expected-risk (MWER-style)
            objective such as (log_posterior.exp() * risk).sum() trains end to end.  Backward is ONE call, whatever nbest is: the
            gradient of sum_n d_loss[b, n] * loss[b, n], to which a hypothesis with loss +inf contributes exactly zero.  First
            derivatives only: backward is not itself differentiable.  The values are the same bits either way.
    Returns: CtcNbestLoss(loss, log_posterior), both [batch, nbest] float32 (detached unless `differentiable`; logits that
        require grad are accepted either way).  A duplicate hypothesis is counted twice in log_posterior.  nbest <= 64; a
        hypothesis that is infeasible or malformed (a label outside [0, num_tokens) or equal to the blank, a negative length
        counts as empty) has loss +inf and changes no other entry."""
    return _nbest("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, hypothesis_mask, max_label_length,
                  differentiable)


def simplified_ctc_nbest_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                              blank_index: Union[int, torch.Tensor] = 0, *, hypothesis_mask: Optional[TensorLike] = None,
                              max_label_length: Optional[int] = None, differentiable: bool = False) -> CtcNbestLoss:
    """The same on the simplified lattice (every non-blank frame is a label).  Same arguments and return value as
    classic_ctc_nbest_loss, `differentiable` (first derivatives only) included."""
    return _nbest("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, hypothesis_mask, max_label_length,
                  differentiable)


def ctc_nbest_loss_from_logproba(labels, logprobas, label_length, logit_length, blank_index, ctc_loss_data_cls, *,
                                 hypothesis_mask: Optional[TensorLike] = None, max_label_length: Optional[int] = None,
                                 differentiable: bool = False) -> CtcNbestLoss:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba).  With `differentiable` the
    gradient is the one with respect to the log-probabilities (first derivatives only: backward is not itself differentiable)."""
    return _nbest(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                  hypothesis_mask, max_label_length, differentiable)


# --------------------------------------------------------------------------------------------------
# N-best forced alignment: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcNbestAlignment(NamedTuple):
    """score [batch, nbest] float32: log-probability of each hypothesis' best path (-inf: infeasible, malformed or masked);
    tokens [batch, nbest, max_length] int32: the token every frame emits on it (-1 beyond logit_length);
    label_index [batch, nbest, max_length] int32: index into labels[b, n] of the label the frame emits -- on the classic lattice
    also of the label it continues by repeating it -- and -1 on blank frames and beyond logit_length;
    first_frame, last_frame [batch, nbest, max_label_length] int32: the first and the last frame of every label (equal on the
    simplified lattice), -1 beyond label_length.
    An infeasible, malformed or masked hypothesis has score = -inf and -1 in every frame and label."""
    score: torch.Tensor
    tokens: torch.Tensor
    label_index: torch.Tensor
    first_frame: torch.Tensor
    last_frame: torch.Tensor


def _nbest_align(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, hypothesis_mask=None,
                 max_label_length=None) -> CtcNbestAlignment:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    if max_label_length is None:
        max_label_length = _host_max(label_length)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    assert x.dim() == 3
    assert x.dtype in (torch.float32, torch.bfloat16, torch.float16)
    assert labels.dim() == 3
    assert label_length.dim() == 2
    assert logit_length.dim() == 1
    assert x.shape[0] == labels.shape[0] == label_length.shape[0] == logit_length.shape[0]
    assert labels.shape[1] == label_length.shape[1]
    U = None if max_label_length is None else max(0, min(int(labels.shape[2]), int(max_label_length)))
    with torch.no_grad():  # a path is not differentiable: the result is detached
        out = ops.nbest_best_path(ops.KINDS[kind_name], wrt, labels, x.detach(), label_length, logit_length, _blank(blank_index), U)
        if hypothesis_mask is not None:  # a masked hypothesis reads as infeasible
            score = out[0]
            mask = _as_tensor(hypothesis_mask).to(device=score.device, dtype=torch.bool)
            assert tuple(mask.shape) == tuple(score.shape)
            out = (torch.where(mask, score, torch.full_like(score, float("-inf"))),
                   *(torch.where(mask[:, :, None], t, torch.full_like(t, -1)) for t in out[1:]))
        return CtcNbestAlignment(*out)


def classic_ctc_nbest_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                blank_index: Union[int, torch.Tensor] = 0, *, hypothesis_mask: Optional[TensorLike] = None,
                                max_label_length: Optional[int] = None) -> CtcNbestAlignment:
    """Forced alignment of N label sequences per utterance on the classic lattice, in one call: what classic_ctc_alignment gives
    for labels[:, n], for every n, with the logits read once per group of eight hypotheses, plus the first and last frame of
    every label.  Timestamps for an N-best list.

    Args:
        labels:       [batch, nbest, max_label_length] int32 -- a CtcBeamDecoding's `labels` as it stands (padding is not read)
        logits:       [batch, max_length, num_tokens] float32 / bfloat16 / float16 (any batch / time strides)
        label_length: [batch, nbest] int32
        logit_length: [batch] int32
        blank_index:  int
        hypothesis_mask: (keyword only) [batch, nbest] bool; where False the hypothesis reads as infeasible (score -inf, -1
            everywhere) -- pass `isfinite(score)` for the missing hypotheses of a CtcBeamDecoding.
        max_label_length: (keyword only) as in classic_ctc_loss: an upper bound on label_length known on the host; it is also the
            width of first_frame / last_frame (default: the width of `labels`, or the largest label_length when that is large).
    Returns: CtcNbestAlignment(score, tokens, label_index, first_frame, last_frame), not differentiable.  nbest <= 64; a hypothesis
        that is infeasible or malformed has score -inf and -1 everywhere and changes no other entry.  Among paths of equal value
        the choice is deterministic but unspecified."""
    return _nbest_align("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, hypothesis_mask,
                        max_label_length)


def simplified_ctc_nbest_alignment(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                                   blank_index: Union[int, torch.Tensor] = 0, *, hypothesis_mask: Optional[TensorLike] = None,
                                   max_label_length: Optional[int] = None) -> CtcNbestAlignment:
    """The same on the simplified lattice (every non-blank frame emits exactly one label: first_frame equals last_frame).  Same
    arguments and return value as classic_ctc_nbest_alignment."""
    return _nbest_align("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, hypothesis_mask,
                        max_label_length)


def ctc_nbest_alignment_from_logproba(labels, logprobas, label_length, logit_length, blank_index, ctc_loss_data_cls, *,
                                      hypothesis_mask: Optional[TensorLike] = None,
                                      max_label_length: Optional[int] = None) -> CtcNbestAlignment:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba)."""
    return _nbest_align(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                        hypothesis_mask, max_label_length)


# --------------------------------------------------------------------------------------------------
# edit distance of N-best lists and the MWER loss: an extension, the reference has no counterpart
# --------------------------------------------------------------------------------------------------
class CtcEditDistance(NamedTuple):
    """distance [batch, nbest] int32: the Levenshtein distance (unit cost for insertion, deletion and substitution) of every
    hypothesis to its utterance's reference, -1 where masked;
    error_rate [batch, nbest] float32: distance / max(reference_length, 1), NaN where masked.
    Both are [batch] when the hypotheses were passed as [batch, width]."""
    distance: torch.Tensor
    error_rate: torch.Tensor


def ctc_edit_distance(hypotheses: TensorLike, hypothesis_length: TensorLike, references: TensorLike, reference_length: TensorLike, *,
                      hypothesis_mask: Optional[TensorLike] = None) -> CtcEditDistance:
    """How wrong a decoding is: the edit distance of every hypothesis to the reference transcript of its utterance, on the device,
    in one launch and without a synchronisation.  Tokens are any int32 values compared for equality (characters, sub-word units,
    word ids mapped on the host); there is no blank and no vocabulary limit.

    Args:
        hypotheses:        [batch, nbest, width] int32 -- a CtcBeamDecoding's `labels` as it stands (padding is not read) -- or
                           [batch, width] with a [batch] length: one hypothesis per utterance, e.g. a CtcDecoding's `labels` (the
                           token error rate of greedy decoding); the result is then [batch].
        hypothesis_length: [batch, nbest] (or [batch]) int32
        references:        [batch, max_label_length] int32, at most 1024 wide
        reference_length:  [batch] int32
        hypothesis_mask:   (keyword only) [batch, nbest] (or [batch]) bool; where False the distance is -1 and the error rate NaN
                           -- pass `isfinite(score)` for the missing hypotheses of a CtcBeamDecoding.
    Returns: CtcEditDistance(distance, error_rate), not differentiable."""
    hyp = _as_tensor(hypotheses, torch.int32)
    hyp_length = _as_tensor(hypothesis_length, torch.int32)
    ref = _as_tensor(references, torch.int32)
    ref_length = _as_tensor(reference_length, torch.int32)
    single = hyp.dim() == 2
    if single:
        assert hyp_length.dim() == 1
        hyp, hyp_length = hyp[:, None, :], hyp_length[:, None]
    assert hyp.dim() == 3
    assert hyp_length.dim() == 2
    assert ref.dim() == 2
    assert ref_length.dim() == 1
    assert hyp.shape[0] == hyp_length.shape[0] == ref.shape[0] == ref_length.shape[0]
    assert hyp.shape[1] == hyp_length.shape[1]
    with torch.no_grad():
        distance = ops.edit_distance(hyp, hyp_length, ref, ref_length)
        ref_length = ref_length.to(device=distance.device)
        # (the lengths as the kernel reads them: clamped to the tensor's width)
        rate = distance.to(torch.float32) / ref_length.clamp(1, max(int(ref.shape[1]), 1)).to(torch.float32)[:, None]
        if hypothesis_mask is not None:
            mask = _as_tensor(hypothesis_mask).to(device=distance.device, dtype=torch.bool)
            if single:
                mask = mask[:, None]
            assert tuple(mask.shape) == tuple(distance.shape)
            distance = torch.where(mask, distance, torch.full_like(distance, -1))
            rate = torch.where(mask, rate, torch.full_like(rate, float("nan")))
        if single:
            distance, rate = distance[:, 0], rate[:, 0]
        return CtcEditDistance(distance, rate)


class CtcEditCounts(NamedTuple):
    """distance, substitutions, insertions, deletions, hits [batch, nbest] int32: the lexicographic minimum of (distance,
    substitutions, insertions) over all alignments of a hypothesis with its utterance's reference -- among the alignments of
    minimum distance the one with the most hits, then the fewest insertions --, deletions = distance - substitutions - insertions
    and hits = hypothesis length - substitutions - insertions; all -1 where masked or where the reference is longer than the
    reference tensor is wide;
    error_rate [batch, nbest] float32: distance / max(reference_length, 1), NaN where masked.
    All are [batch] when the hypotheses were passed as [batch, width]."""
    distance: torch.Tensor
    substitutions: torch.Tensor
    insertions: torch.Tensor
    deletions: torch.Tensor
    hits: torch.Tensor
    error_rate: torch.Tensor


def ctc_edit_counts(hypotheses: TensorLike, hypothesis_length: TensorLike, references: TensorLike, reference_length: TensorLike, *,
                    hypothesis_mask: Optional[TensorLike] = None, rows_per_tile: Optional[int] = None) -> CtcEditCounts:
    """What an error-rate report prints: distance, substitutions, insertions, deletions and hits of every hypothesis against the
    reference transcript of its utterance, on the device and without a synchronisation, for references of up to 65536 tokens and
    hypotheses of up to 2^20 (ctc_edit_distance stops at 1024 and returns the distance alone).  Tokens are any int32 values
    compared for equality.

    Args:
        hypotheses:        [batch, nbest, width] int32 -- a CtcBeamDecoding's `labels` as it stands (padding is not read) -- or
                           [batch, width] with a [batch] length: one hypothesis per utterance, e.g. a CtcDecoding's `labels`; the
                           result is then [batch].
        hypothesis_length: [batch, nbest] (or [batch]) int32
        references:        [batch, max_label_length] int32, at most 65536 wide
        reference_length:  [batch] int32
        hypothesis_mask:   (keyword only) [batch, nbest] (or [batch]) bool; where False the five counts are -1 and the error rate
                           NaN -- pass `isfinite(score)` for the missing hypotheses of a CtcBeamDecoding.
        rows_per_tile:     (keyword only) hypothesis tokens per tile of the table, a multiple of 64 (None: the library's default);
                           the result does not depend on it.
    Returns: CtcEditCounts(distance, substitutions, insertions, deletions, hits, error_rate), not differentiable."""
    hyp = _as_tensor(hypotheses, torch.int32)
    hyp_length = _as_tensor(hypothesis_length, torch.int32)
    ref = _as_tensor(references, torch.int32)
    ref_length = _as_tensor(reference_length, torch.int32)
    single = hyp.dim() == 2
    if single:
        assert hyp_length.dim() == 1
        hyp, hyp_length = hyp[:, None, :], hyp_length[:, None]
    assert hyp.dim() == 3
    assert hyp_length.dim() == 2
    assert ref.dim() == 2
    assert ref_length.dim() == 1
    assert hyp.shape[0] == hyp_length.shape[0] == ref.shape[0] == ref_length.shape[0]
    assert hyp.shape[1] == hyp_length.shape[1]
    with torch.no_grad():
        counts = ops.edit_counts(hyp, hyp_length, ref, ref_length, rows_per_tile=rows_per_tile)
        dev = counts.device
        distance, subs, ins, dels = counts.unbind(-1)
        # (the lengths as the kernel reads them: clamped to the tensors' widths)
        h = hyp_length.to(device=dev).clamp(0, int(hyp.shape[2]))
        ref_length = ref_length.to(device=dev)
        valid = distance >= 0
        hits = torch.where(valid, h - subs - ins, torch.full_like(distance, -1))
        rate = distance.to(torch.float32) / ref_length.clamp(1, max(int(ref.shape[1]), 1)).to(torch.float32)[:, None]
        fields = [distance, subs, ins, dels, hits]
        if hypothesis_mask is not None:
            mask = _as_tensor(hypothesis_mask).to(device=dev, dtype=torch.bool)
            if single:
                mask = mask[:, None]
            assert tuple(mask.shape) == tuple(distance.shape)
            fields = [torch.where(mask, f, torch.full_like(f, -1)) for f in fields]
            rate = torch.where(mask, rate, torch.full_like(rate, float("nan")))
        fields = [f.contiguous() for f in fields]
        if single:
            fields, rate = [f[:, 0] for f in fields], rate[:, 0]
        return CtcEditCounts(*fields, rate)


class CtcMwerLoss(NamedTuple):
    """loss [batch] float32: the expected risk of the N-best list relative to its mean risk (differentiable);
    risk [batch, nbest] float32: the edit distance of every hypothesis to the labels (a constant);
    log_posterior [batch, nbest] float32: the confidence of every hypothesis within its list, as a CtcNbestLoss defines it
    (differentiable; -inf for a masked or infeasible hypothesis);
    hypotheses: the CtcBeamDecoding the list was taken from."""
    loss: torch.Tensor
    risk: torch.Tensor
    log_posterior: torch.Tensor
    hypotheses: CtcBeamDecoding


def _mwer(kind_name: str, wrt: int, labels, x, label_length, logit_length, blank_index, beam_width, top_k, nbest, hypotheses,
          max_label_length) -> CtcMwerLoss:
    x = _as_tensor(x)
    labels = _as_tensor(labels, torch.int32)
    label_length = _as_tensor(label_length, torch.int32)
    logit_length = _as_tensor(logit_length, torch.int32)
    _verify_inputs(labels, x, label_length, logit_length)
    if hypotheses is None:  # (on the detached logits, under no_grad: the search leaves the logits' graph alone)
        hypotheses = _beam(kind_name, wrt, x, logit_length, blank_index, beam_width, top_k, nbest)
    else:
        hypotheses = CtcBeamDecoding(_as_tensor(hypotheses[0]), _as_tensor(hypotheses[1], torch.int32), _as_tensor(hypotheses[2], torch.int32))
    mask = torch.isfinite(hypotheses.score)
    with torch.no_grad():
        risk = ops.edit_distance(hypotheses.labels, hypotheses.label_length, labels, label_length).to(torch.float32)
    nb = _nbest(kind_name, wrt, hypotheses.labels, x, hypotheses.label_length, logit_length, blank_index, mask, max_label_length,
                differentiable=True)
    used = torch.isfinite(nb.loss)  # unmasked and feasible
    zero = torch.zeros_like(risk)
    mean = torch.where(used, risk, zero).sum(dim=1, keepdim=True) / used.sum(dim=1, keepdim=True).clamp(min=1).to(torch.float32)
    loss = torch.where(used, nb.log_posterior.exp() * (risk - mean), zero).sum(dim=1)
    return CtcMwerLoss(loss, risk, nb.log_posterior, hypotheses)


def classic_ctc_mwer_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                          blank_index: Union[int, torch.Tensor] = 0, *, beam_width: int = 16, top_k: int = 16, nbest: int = 8,
                          hypotheses: Optional[CtcBeamDecoding] = None, max_label_length: Optional[int] = None) -> CtcMwerLoss:
    """Minimum word error rate (expected risk) training on the classic lattice, end to end on the device: an N-best list, the edit
    distance of every hypothesis to the labels as its risk, the exact posterior of every hypothesis within the list, and
        loss[b] = sum over the used n of  exp(log_posterior[b, n]) * (risk[b, n] - mean risk of the used hypotheses of b)
    (Prabhavalkar et al. 2018).  A hypothesis is used when it is not missing from the list (finite `score`) and feasible on the
    lattice (finite loss); an utterance without a used hypothesis has loss 0 and a zero gradient.

    Args:
        labels, logits, label_length, logit_length, blank_index: as classic_ctc_loss (labels at most 1024 wide)
        beam_width, top_k, nbest: (keyword only) the arguments of classic_ctc_beam_search, which the function runs on the detached
            logits when `hypotheses` is not given.
        hypotheses: (keyword only) a CtcBeamDecoding to take the list from instead: (score [batch, nbest], labels [batch, nbest,
            width], label_length [batch, nbest]); an entry whose score is not finite is masked.
        max_label_length: (keyword only) an upper bound, known on the host, on the HYPOTHESES' lengths, as
            classic_ctc_nbest_loss takes it (a beam search's label tensor is as wide as the logits are long).
    Returns: CtcMwerLoss(loss [batch], risk [batch, nbest], log_posterior [batch, nbest], hypotheses).  The gradient reaches the
        logits through log_posterior only (risk is a constant); backward is the one call of classic_ctc_nbest_loss's.  First
        derivatives only.  No host synchronisation beyond the one look at max(label_length) that classic_ctc_nbest_loss takes for
        a wide label tensor without `max_label_length`."""
    return _mwer("classic", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, beam_width, top_k, nbest,
                 hypotheses, max_label_length)


def simplified_ctc_mwer_loss(labels: TensorLike, logits: TensorLike, label_length: TensorLike, logit_length: TensorLike,
                             blank_index: Union[int, torch.Tensor] = 0, *, beam_width: int = 16, top_k: int = 16, nbest: int = 8,
                             hypotheses: Optional[CtcBeamDecoding] = None, max_label_length: Optional[int] = None) -> CtcMwerLoss:
    """The same on the simplified lattice (every non-blank frame is a label).  Same arguments and return value as
    classic_ctc_mwer_loss."""
    return _mwer("simplified", _lib.WRT_LOGITS, labels, logits, label_length, logit_length, blank_index, beam_width, top_k, nbest,
                 hypotheses, max_label_length)


def ctc_mwer_loss_from_logproba(labels, logprobas, label_length, logit_length, blank_index, ctc_loss_data_cls, *, beam_width: int = 16,
                                top_k: int = 16, nbest: int = 8, hypotheses: Optional[CtcBeamDecoding] = None,
                                max_label_length: Optional[int] = None) -> CtcMwerLoss:
    """The same for log-probabilities used as they stand (the counterpart of ctc_loss_from_logproba); the gradient is the one with
    respect to the log-probabilities."""
    return _mwer(ctc_loss_data_cls.kind_name, _lib.WRT_LOGPROBS, labels, logprobas, label_length, logit_length, blank_index,
                 beam_width, top_k, nbest, hypotheses, max_label_length)


# --------------------------------------------------------------------------------------------------
# loss-data objects (what the reference's unit tests poke at directly)
# --------------------------------------------------------------------------------------------------
class BaseCtcLossData:
    """Mirror of BaseCtcLossData (base_loss.py:102-298) over log-probabilities.  Properties are computed on
    first use by the HIP kernels and memoised, like the reference's cached_property chain."""

    kind_name = ""

    def __init__(self, labels, logprobas, label_length, logit_length, blank_index=0, swap_memory: bool = False):
        logprobas = _as_tensor(logprobas)
        labels = _as_tensor(labels, torch.int32)
        label_length = _as_tensor(label_length, torch.int32)
        logit_length = _as_tensor(logit_length, torch.int32)
        _verify_inputs(labels, logprobas, label_length, logit_length)
        self._kind = ops.KINDS[self.kind_name]
        self._blank_index = _blank(blank_index)
        self._args = (labels, logprobas.detach(), label_length, logit_length)

    @cached_property
    def _max_label_length(self) -> int:
        """base_loss.py:482-486 (dynamic max; costs one device->host sync, only the debug properties use it)."""
        ll = self._args[2]
        return int(ll.max().item()) if ll.numel() else 0

    def _prep(self, exact_u: bool = False) -> ops.Prepared:
        labels, lp, ll, tl = self._args
        return ops.Prepared(labels, lp, ll, tl, self._blank_index, U=self._max_label_length if exact_u else None)

    @cached_property
    def _loss_grad(self):
        return ops.loss_grad(self._kind, _lib.WRT_LOGPROBS, self._prep(), want_grad=True)

    @property
    def loss(self) -> torch.Tensor:
        """[batch]  (classic_ctc_loss.py:152-165, simplified_ctc_loss.py:73-83)"""
        return self._loss_grad[0]

    @property
    def gradient(self) -> torch.Tensor:
        """[batch, max_logit_length, num_tokens]: d loss / d logproba = -posterior (base_loss.py:262-268)"""
        return self._loss_grad[1]

    @cached_property
    def logarithmic_logproba_gradient(self) -> torch.Tensor:
        """log of the posterior = log(-gradient), computed in log space like the reference does (base_loss.py:270-298): finite
        where the float32 gradient underflows (e^-150 comes out as -150); -inf on padded frames, for infeasible samples and
        for tokens no lattice state emits."""
        return ops.log_posterior(self._kind, _lib.WRT_LOGPROBS, self._prep())[1]

    @cached_property
    def _alpha_beta(self):
        return ops.alpha_beta(self._kind, _lib.WRT_LOGPROBS, self._prep(exact_u=True))

    @property
    def alpha(self) -> torch.Tensor:
        """classic [batch, T+1, U+1, 2], simplified [batch, T+1, U+1]; natural log, -inf = impossible"""
        return self._alpha_beta[1]

    @property
    def beta(self) -> torch.Tensor:
        return self._alpha_beta[2]

    @cached_property
    def hessian(self) -> torch.Tensor:
        """[batch, T, V, T, V]: second derivative w.r.t. log-probabilities (base_loss.py:186-260)"""
        return ops.hessian(self._kind, _lib.WRT_LOGPROBS, self._prep(), want_grad=False)[2]

    def hessian_vector_product(self, vec: TensorLike) -> torch.Tensor:
        """sum_{t2,k2} hessian[b,t,k,t2,k2] vec[b,t2,k2] without building `hessian` (extension: tangent-mode
        alpha/beta, ctc_amd_hvp); equals torch.einsum("btkuj,buj->btk", self.hessian, vec)."""
        return ops.hvp(self._kind, _lib.WRT_LOGPROBS, self._prep(), _as_tensor(vec))[2]

    @property
    def gamma(self):
        raise NotImplementedError(
            "gamma (classic_ctc_loss.py:167-308, simplified_ctc_loss.py:85-191) is an O(T^2 L^2) intermediate "
            "of the reference's Hessian; this implementation never materialises it (see DESIGN.md).")


class ClassicCtcLossData(BaseCtcLossData):
    kind_name = "classic"


class SimplifiedCtcLossData(BaseCtcLossData):
    kind_name = "simplified"
