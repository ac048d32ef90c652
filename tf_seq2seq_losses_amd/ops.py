"""Thin torch<->C-ABI plumbing: device pointers, the current HIP stream and workspace allocation.
torch is used for device memory and streams only; all arithmetic happens in libctc_amd.so."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib

KINDS = {"classic": _lib.CLASSIC, "simplified": _lib.SIMPLIFIED}
# Label tensors wider than this are worth one look at max(label_length): up to 128 positions run the fastest instantiation
# (two positions per lane) whatever the width says; beyond, every doubling selects a slower tier (four / eight positions per
# lane, then the three-kernel pipeline) although the labels inside may be short (tests/common.py:89-94 pads labels to T).
WIDTH_WORTH_A_LOOK = 128
_MAXLEN_CACHE = {}  # id(label_length tensor) -> (weak reference to it, its version, its maximum): one sync per distinct tensor


def _device_max_label_length(t: torch.Tensor) -> int:
    """max(label_length) of a device tensor, fetched once per tensor OBJECT and version (a data pointer is no identity: the
    caching allocator hands the same address to the next batch's tensor)."""
    import weakref
    hit = _MAXLEN_CACHE.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    if len(_MAXLEN_CACHE) > 64:
        _MAXLEN_CACHE.clear()
    m = int(t.max().item())  # device -> host sync (pass max_label_length= to avoid it)
    _MAXLEN_CACHE[id(t)] = (weakref.ref(t), t._version, m)
    return m


def _require_gpu(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            "tf_seq2seq_losses_amd runs on an AMD GPU only (HIP kernels for gfx950); got a CPU tensor and "
            "there is no CPU fallback. Move the inputs to the GPU (tensor.cuda()).")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


class Prepared:
    """Validated device inputs of one call.  By default the logits are made contiguous float32 [B,T,V]; with
    keep_format=True a float32/bfloat16 tensor whose token axis is contiguous is passed as it is (time-major views,
    bfloat16 activations: ctc_amd_loss_grad_ex) -- only loss_grad takes such inputs, the other entry points use plain()."""

    def __init__(self, labels, x, label_length, logit_length, blank_index, U=None, keep_format=False, host_max_label_length=None):
        _require_gpu(x)
        dev = x.device
        V = int(x.shape[2]) if x.dim() == 3 else 0
        native = (keep_format and x.dim() == 3 and x.dtype in _DTYPES and x.numel() > 0 and x.stride(2) == 1
                  and x.stride(0) >= V and x.stride(1) >= V)
        self.native = bool(native) and not (x.dtype == torch.float32 and x.is_contiguous())
        self.x = x if (native or (x.dtype == torch.float32 and x.is_contiguous())) else x.to(torch.float32).contiguous()
        def i32(t):
            if t.dtype == torch.int32 and t.device == dev and t.is_contiguous():
                return t
            return t.to(device=dev, dtype=torch.int32).contiguous()
        src_label_length = label_length  # (the caller's own tensor: what the cache of its maximum is keyed on)
        self.labels, self.label_length, self.logit_length = i32(labels), i32(label_length), i32(logit_length)
        self.blank = int(blank_index)
        self.B, self.T, self.V = (int(s) for s in x.shape)
        self.stride = int(self.labels.shape[1])
        # static bound on the label length: any U >= max(label_length) gives the reference's results (it uses the dynamic
        # maximum, base_loss.py:482-486).  The width of the label tensor always works; a tighter bound selects a faster kernel
        # tier.  Sources, in order: the caller's hint (`max_label_length=` of the public functions), the host copy of
        # label_length when the caller passed one (free), and -- only for tensors wide enough that it matters -- the
        # device-side maximum, fetched once per distinct label_length tensor (one sync, not capturable into a graph).
        if U is None:
            U = self.stride
            if host_max_label_length is not None:
                U = max(0, min(U, int(host_max_label_length)))
            elif U > WIDTH_WORTH_A_LOOK and self.label_length.numel() > 0:
                # the maximum of the CALLER's tensor: a host tensor costs nothing; a device tensor one sync per tensor object and
                # version (keyed on the caller's object -- the converted copy made above is a new object every call and never hit
                # the cache); under stream capture no sync is possible and the width stands
                if not src_label_length.is_cuda:
                    U = max(0, min(U, int(src_label_length.max())))
                elif not torch.cuda.is_current_stream_capturing():
                    U = max(0, min(U, _device_max_label_length(src_label_length)))
        self.U = int(U)
        self.device = dev

    def plain(self) -> "Prepared":
        """The same inputs with contiguous float32 logits (Hessian, HVP and alpha/beta read that format only), 16-byte aligned
        (ctc_amd_hvp / ctc_amd_hessian refuse other base pointers: a batch-sliced view whose offset is not a multiple of 16 bytes is
        copied once here)."""
        if self.native:
            return self._with_plain_x(self.x.to(torch.float32).contiguous())
        if self.x.numel() > 0 and (self.x.data_ptr() & 15) != 0:
            return self._with_plain_x(self.x.clone())
        return self

    def _with_plain_x(self, x) -> "Prepared":
        q = Prepared.__new__(Prepared)
        q.__dict__.update(self.__dict__)
        q.x, q.native = x, False
        return q

    def common(self, kind: int, wrt: int):
        """The twelve leading arguments of the entry points that read contiguous float32 logits."""
        assert not self.native, "this entry point takes contiguous float32 logits: use Prepared.plain()"
        return (kind, wrt, _ptr(self.x), _ptr(self.labels), self.stride, _ptr(self.label_length),
                _ptr(self.logit_length), self.blank, self.B, self.T, self.V, self.U)

    def common_ex(self, kind: int, wrt: int):
        """The fifteen leading arguments of the producer-format entry points; [3:6] is the logits' (dtype, stride_b, stride_t)."""
        x = self.x
        return (kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(self.labels), self.stride,
                _ptr(self.label_length), _ptr(self.logit_length), self.blank, self.B, self.T, self.V, self.U)


_WS_BYTES = {}   # (what, kind, B, T, V, U) -> bytes: no ctypes round trip per call
_WS_CACHE = {}   # (device, stream) -> the loss+gradient workspace last used there (reused while it is large enough)
_PIPELINE = {}   # (kind, wrt, B, T, V, U) -> pipeline name of a contiguous float32 call


def _ws_bytes(what: int, kind: int, p: "Prepared") -> int:
    key = (what, kind, p.B, p.T, p.V, p.U, _lib.override_generation)
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.workspace_bytes(what, kind, p.B, p.T, p.V, p.U)
    return n


def _loss_grad_selector(wrt: int, p: "Prepared") -> int:
    """Workspace selector of a loss+gradient call: the pipeline's own (small) layout for logits input in a format the
    fused tiers read (float32; bfloat16 with 8-byte aligned rows), the conservative one otherwise (include/ctc_amd.h)."""
    if wrt != _lib.WRT_LOGITS:
        return _lib.WS_LOSS_GRAD
    x = p.x
    if x.dtype == torch.bfloat16 and ((p.V | x.stride(0) | x.stride(1)) & 3 or x.data_ptr() & 7):
        return _lib.WS_LOSS_GRAD
    if x.dtype == torch.float16:  # read by the three-kernel pipeline only
        return _lib.WS_LOSS_GRAD
    return _lib.WS_LOSS_GRAD_LOGITS


def pipeline_of(kind: int, wrt: int, p: "Prepared") -> str:
    key = (kind, wrt, p.B, p.T, p.V, p.U, _lib.override_generation)
    name = _PIPELINE.get(key)
    if name is None:
        name = _PIPELINE[key] = _lib.pipeline_name(kind, wrt, p.B, p.T, p.V, p.U, True)
    return name


def _workspace(what: int, kind: int, p: Prepared) -> torch.Tensor:
    n = _ws_bytes(what, kind, p)
    if what not in (_lib.WS_LOSS_GRAD, _lib.WS_LOSS_GRAD_LOGITS):
        return torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    # The loss+gradient workspace is scratch that lives only for the duration of one call.  Calls on one stream are
    # ordered, so they can share one buffer; another stream gets its own.
    ck = (p.device, _stream(p.device))
    ws = _WS_CACHE.get(ck)
    if ws is None or ws.numel() < n:
        ws = _WS_CACHE[ck] = torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    return ws


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev) -> int:
    """hipStream_t of torch's current stream on `dev` (torch.cuda.current_stream builds a Stream object: ~15 us per call)."""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` costs ~10 us of host time per call; most calls already run on the right device."""

    __slots__ = ("dev", "ctx")

    def __init__(self, dev):
        self.dev, self.ctx = dev, None

    def __enter__(self):
        if self.dev.index is not None and torch.cuda.current_device() != self.dev.index:
            self.ctx = torch.cuda.device(self.dev)
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _new_grad(p: Prepared, want_grad: bool = True) -> Optional[torch.Tensor]:
    """Uninitialised gradient of p.x: in the producer's format (same element type, same strides) for native inputs,
    contiguous float32 [B,T,V] otherwise."""
    if not want_grad:
        return None
    if p.native:
        return torch.empty_strided(p.x.shape, p.x.stride(), dtype=p.x.dtype, device=p.device)
    return torch.empty((p.B, p.T, p.V), dtype=torch.float32, device=p.device)


def _d_loss(d_loss: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    return None if d_loss is None else d_loss.to(device=dev, dtype=torch.float32).contiguous()


def loss_grad(kind: int, wrt: int, p: Prepared, want_grad: bool, d_loss: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    lib = _lib.load()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    grad = _new_grad(p, want_grad)
    if p.B == 0:
        return loss, grad
    ws = workspace if workspace is not None else _workspace(_loss_grad_selector(wrt, p), kind, p)
    d_loss = _d_loss(d_loss, p.device)
    with _on_device(p.device):
        if p.native:
            ex = p.common_ex(kind, wrt)
            rc = lib.ctc_amd_loss_grad_ex(*ex, _ptr(loss), _ptr(grad), *ex[3:6], _ptr(d_loss),  # (the gradient has the logits' format)
                                          ws.data_ptr(), ws.numel(), _stream(p.device))
        else:
            rc = lib.ctc_amd_loss_grad(*p.common(kind, wrt), _ptr(loss), _ptr(grad), _ptr(d_loss),
                                       ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_loss_grad")
    return loss, grad


def loss_grad_packed(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, row_offsets: torch.Tensor,
                     label_length: torch.Tensor, logit_length: torch.Tensor, blank_index: int, max_length: int,
                     U: Optional[int] = None, want_grad: bool = True, d_loss: Optional[torch.Tensor] = None):
    """Packed (ragged) batch, ctc_amd_loss_grad_packed: `x` is [total_rows, V] (float32 / bfloat16 / float16, rows contiguous
    in the token axis), utterance b owns the rows row_offsets[b] .. row_offsets[b] + logit_length[b] - 1; the gradient comes
    back with the same packing and element type.  max_length >= max(logit_length) sizes the workspace."""
    lib = _lib.load()
    _require_gpu(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype in _DTYPES
    dev = x.device
    B, V, T = int(labels.shape[0]), int(x.shape[1]), int(max_length)
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    labels, label_length, logit_length = i32(labels), i32(label_length), i32(logit_length)
    row_offsets = row_offsets.to(device=dev, dtype=torch.int64).contiguous()
    U = int(labels.shape[1]) if U is None else int(U)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    grad = torch.zeros_like(x) if want_grad else None  # (rows no utterance owns stay zero)
    if B == 0:
        return loss, grad
    ws = torch.empty(max(_lib.workspace_bytes(_lib.WS_LOSS_GRAD, kind, B, T, V, U), 1), dtype=torch.uint8, device=dev)
    d_loss = _d_loss(d_loss, dev)
    dt = _DTYPES[x.dtype]
    with _on_device(dev):
        rc = lib.ctc_amd_loss_grad_packed(kind, wrt, _ptr(x), dt, _ptr(row_offsets), x.stride(0), _ptr(labels), int(labels.shape[1]),
                                          _ptr(label_length), _ptr(logit_length), int(blank_index), B, T, V, U, _ptr(loss),
                                          _ptr(grad), dt, grad.stride(0) if grad is not None else V, _ptr(d_loss),
                                          ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "ctc_amd_loss_grad_packed")
    return loss, grad


LOSS_SUM_SCALE = 1.0 / 1048576.0  # unit of the fixed-point loss sum (ctc_amd_loss_grad_sum)


def loss_grad_sum(kind: int, wrt: int, p: Prepared, sum2: torch.Tensor, zero_next: Optional[torch.Tensor] = None,
                  want_grad: bool = True, d_loss: Optional[torch.Tensor] = None):
    """loss_grad that also adds [sum of the finite losses in units of 2^-20, their number] to the int64[2] tensor `sum2`
    inside the same launch (exact integer adds: deterministic) and clears `zero_next` for the following step."""
    lib = _lib.load()
    assert sum2.dtype == torch.int64 and sum2.numel() == 2 and sum2.device == p.device
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    grad = _new_grad(p, want_grad)
    ws = _workspace(_loss_grad_selector(wrt, p), kind, p)
    d_loss = _d_loss(d_loss, p.device)
    gs = (grad.stride(0), grad.stride(1)) if grad is not None else (p.T * p.V, p.V)
    with _on_device(p.device):
        rc = lib.ctc_amd_loss_grad_sum(*p.common_ex(kind, wrt), _ptr(loss), _ptr(grad), _DTYPES[p.x.dtype], gs[0], gs[1],
                                       _ptr(d_loss), _ptr(sum2), _ptr(zero_next), ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_loss_grad_sum")
    return loss, grad


def loss_forward(kind: int, wrt: int, p: Prepared, keep_always: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Loss only.  Where the two-call form exists (the linear-domain fused tier) the call gets a workspace of its own that
    grad_resume continues from (returned; keep it alive until then: checkpoint rows only, ~64 MB at the north-star shape);
    every other pipeline would recompute everything in the second call anyway, so nothing is kept (None) unless
    keep_always (the parity tests call ctc_amd_grad_resume behind every pipeline)."""
    sel = _loss_grad_selector(wrt, p)
    two_call = p.B > 0 and (keep_always or sel == _lib.WS_LOSS_GRAD_LOGITS) and pipeline_of(kind, wrt, p) == "fused6"
    if not two_call and (p.B == 0 or not keep_always):  # nothing kept
        return loss_grad(kind, wrt, p, False)[0], None
    ws = torch.empty(max(_ws_bytes(sel, kind, p), 1), dtype=torch.uint8, device=p.device)
    if not two_call:  # kept for the tests: an ordinary loss-only call into a workspace of its own
        return loss_grad(kind, wrt, p, False, workspace=ws)[0], ws
    # first half of a forward / backward pair (ctc_amd_loss_forward, ABI v5): the resume call verifies every utterance's posterior
    # mass, so the linear-domain kernel keeps its conservative loss-only signs for binding alignments only
    lib = _lib.load()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    with _on_device(p.device):
        rc = lib.ctc_amd_loss_forward(*p.common_ex(kind, wrt), _ptr(loss), ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_loss_forward")
    return loss, ws


def grad_resume(kind: int, wrt: int, p: Prepared, ws: torch.Tensor, d_loss: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient for the loss that loss_forward computed into `ws` (ctc_amd_grad_resume), weighted by d_loss.  The losses the
    call rewrites (utterances redone in the log domain) go to a scratch buffer: the tensor the forward pass returned to the
    user is never written again."""
    if ws is None:  # the forward call kept nothing (its pipeline has no two-call form): one loss+gradient call
        return loss_grad(kind, wrt, p, True, d_loss=d_loss)[1]
    lib = _lib.load()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    grad = _new_grad(p)
    if p.B == 0 or p.T == 0:
        return grad
    d_loss = _d_loss(d_loss, p.device)
    with _on_device(p.device):
        rc = lib.ctc_amd_grad_resume(*p.common_ex(kind, wrt), _ptr(loss), _ptr(grad), _DTYPES[p.x.dtype], grad.stride(0), grad.stride(1),
                                     _ptr(d_loss), ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_grad_resume")
    return grad


def fused_flags(ws: torch.Tensor, kind: int, p: Prepared) -> torch.Tensor:
    """Diagnostic: int32[B] flag words the linear-domain kernel left in `ws` (0 = linear domain, else redone in the log domain)."""
    off = _lib.flags_offset(kind, p.B, p.T, p.V, p.U)
    return ws[off:off + 4 * p.B].view(torch.int32)


def alpha_beta(kind: int, wrt: int, p: Prepared):
    lib = _lib.load()
    p = p.plain()
    L = p.U + 1
    shape = (p.B, p.T + 1, L, 2) if kind == _lib.CLASSIC else (p.B, p.T + 1, L)
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    alpha = torch.empty(shape, dtype=torch.float32, device=p.device)
    beta = torch.empty(shape, dtype=torch.float32, device=p.device)
    if p.B == 0:
        return loss, alpha, beta
    ws = _workspace(_lib.WS_ALPHA_BETA, kind, p)
    with _on_device(p.device):
        rc = lib.ctc_amd_alpha_beta(*p.common(kind, wrt), _ptr(loss), _ptr(alpha), _ptr(beta),
                                    ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_alpha_beta")
    return loss, alpha, beta


def log_posterior(kind: int, wrt: int, p: Prepared):
    """(loss[B], lg[B,T,V]): natural log of the posterior of "frame t emits token k", in log space (ctc_amd_log_posterior)."""
    lib = _lib.load()
    p = p.plain()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    lg = torch.empty((p.B, p.T, p.V), dtype=torch.float32, device=p.device)
    if p.B == 0:
        return loss, lg
    ws = _workspace(_lib.WS_ALPHA_BETA, kind, p)
    with _on_device(p.device):
        rc = lib.ctc_amd_log_posterior(*p.common(kind, wrt), _ptr(loss), _ptr(lg), ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_log_posterior")
    return loss, lg


def hessian(kind: int, wrt: int, p: Prepared, want_grad: bool = True):
    lib = _lib.load()
    p = p.plain()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    grad = torch.empty((p.B, p.T, p.V), dtype=torch.float32, device=p.device) if want_grad else None
    hess = torch.empty((p.B, p.T, p.V, p.T, p.V), dtype=torch.float32, device=p.device)
    if p.B == 0 or p.T == 0:
        if p.B and not p.T:
            loss, _ = loss_grad(kind, wrt, p, False)
        return loss, grad, hess
    ws = _workspace(_lib.WS_HESSIAN, kind, p)
    with _on_device(p.device):
        rc = lib.ctc_amd_hessian(*p.common(kind, wrt), _ptr(loss), _ptr(grad), _ptr(hess),
                                 ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_hessian")
    return loss, grad, hess


def hvp(kind: int, wrt: int, p: Prepared, vec: torch.Tensor, want_grad: bool = False, return_workspace: bool = False):
    """out[b,t,k] = sum_{t2,k2} H[b,t,k,t2,k2] vec[b,t2,k2] through ctc_amd_hvp (no [B,T,V,T,V] tensor).
    return_workspace (diagnostics): also the workspace, whose flag words say which utterances the fused kernel redid in the log
    domain (_lib.hvp_flags_offset)."""
    lib = _lib.load()
    p = p.plain()
    assert tuple(vec.shape) == (p.B, p.T, p.V), f"vec must be [B,T,V] = {(p.B, p.T, p.V)}, got {tuple(vec.shape)}"
    vec = vec.to(device=p.device, dtype=torch.float32).contiguous()
    if vec.numel() > 0 and (vec.data_ptr() & 15) != 0:  # (an offset view: ctc_amd_hvp wants 16-byte aligned rows)
        vec = vec.clone()
    loss = torch.empty(p.B, dtype=torch.float32, device=p.device)
    grad = torch.empty((p.B, p.T, p.V), dtype=torch.float32, device=p.device) if want_grad else None
    out = torch.empty((p.B, p.T, p.V), dtype=torch.float32, device=p.device)
    if p.B == 0 or p.T == 0:
        if p.B and not p.T:
            loss, _ = loss_grad(kind, wrt, p, False)
        return loss, grad, out
    ws = _workspace(_lib.WS_HVP, kind, p)
    with _on_device(p.device):
        rc = lib.ctc_amd_hvp(*p.common(kind, wrt), _ptr(vec), _ptr(loss), _ptr(grad), _ptr(out),
                             ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_hvp")
    if return_workspace:
        return loss, grad, out, ws
    return loss, grad, out


def best_path(kind: int, wrt: int, p: Prepared) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(score[B] float32, tokens[B,T] int32, label_index[B,T] int32): the best path of the lattice and which label every frame
    emits (ctc_amd_best_path).  Reads the logits in the format `p` holds them in (Prepared(keep_format=True): bfloat16 /
    float16 activations and time-major views in place)."""
    lib = _lib.load()
    score = torch.empty(p.B, dtype=torch.float32, device=p.device)
    tokens = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    label_index = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    if p.B == 0:
        return score, tokens, label_index
    key = ("best_path", kind, p.B, p.T, p.V, p.U)
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.best_path_workspace_bytes(kind, p.B, p.T, p.V, p.U)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    with _on_device(p.device):
        rc = lib.ctc_amd_best_path(*p.common_ex(kind, wrt), _ptr(score), _ptr(tokens), _ptr(label_index),
                                   ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_best_path")
    return score, tokens, label_index


def _frame_window(what: str, frame_window: torch.Tensor, B: int, U: int, dev) -> Tuple[torch.Tensor, int]:
    """(int32 contiguous tensor, window_stride) of a [B, >= U, 2] frame window as the windowed entry points take it: (first, last)
    inclusive per label position.  int64 values are narrowed on the device; nothing is looked at on the host."""
    if frame_window.dim() != 3 or int(frame_window.shape[0]) != B or int(frame_window.shape[1]) < U or int(frame_window.shape[2]) != 2:
        raise ValueError(f"{what}: frame_window must be [B, U, 2] with B = {B} and U >= {U}, got {tuple(frame_window.shape)}")
    if frame_window.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: frame_window must be int32 or int64, got {frame_window.dtype}")
    if frame_window.device != dev:
        raise ValueError(f"{what}: frame_window must be on the logits' device {dev}, got {frame_window.device}")
    if frame_window.dtype == torch.int64:  # (frames beyond int32 do not exist: clamping keeps "before everything" / "behind everything")
        frame_window = frame_window.clamp(-2**31, 2**31 - 1).to(torch.int32)
    frame_window = frame_window.contiguous()
    return frame_window, 2 * int(frame_window.shape[1])


def wildcard_best_path(kind: int, wrt: int, p: Prepared, frame_window: Optional[torch.Tensor] = None, optional_wildcards: bool = False):
    """(score[B] float32, tokens[B,T] int32, label_index[B,T] int32, first_frame[B,U] int32, last_frame[B,U] int32,
    label_score[B,U] float32): the best path of the lattice whose labels may be wildcards (_lib.WILDCARD), and where every label
    lies on it (ctc_amd_wildcard_best_path).  Reads the logits in the format `p` holds them in, as best_path does.  frame_window
    [B, U, 2] (first, last inclusive per label position): ctc_amd_windowed_best_path.  optional_wildcards: labels may also hold
    _lib.OPTIONAL_WILDCARD, a wildcard that may be skipped (ctc_amd_optional_wildcard_best_path; not with a window; classic:
    U <= _lib.OPTIONAL_CLASSIC_MAX_U)."""
    if optional_wildcards and frame_window is not None:
        raise ValueError("wildcard_best_path: frame_window and optional_wildcards cannot be combined")
    if optional_wildcards and kind == _lib.CLASSIC and p.U > _lib.OPTIONAL_CLASSIC_MAX_U:
        raise ValueError(f"wildcard_best_path: optional wildcards on the classic lattice take at most {_lib.OPTIONAL_CLASSIC_MAX_U} "
                         f"label positions, got U = {p.U}")
    lib = _lib.load()
    score = torch.empty(p.B, dtype=torch.float32, device=p.device)
    tokens = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    label_index = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    first_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    last_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    label_score = torch.empty((p.B, p.U), dtype=torch.float32, device=p.device)
    out = (score, tokens, label_index, first_frame, last_frame, label_score)
    if p.B == 0:
        return out
    key = ("wildcard_best_path", kind, p.B, p.T, p.V, p.U)
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.wildcard_best_path_workspace_bytes(kind, p.B, p.T, p.V, p.U)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    if frame_window is not None:
        fw, fws = _frame_window("wildcard_best_path", frame_window, p.B, p.U, p.device)
        with _on_device(p.device):
            rc = lib.ctc_amd_windowed_best_path(*p.common_ex(kind, wrt)[:11], _ptr(fw), fws, p.B, p.T, p.V, p.U, *(_ptr(t) for t in out),
                                                ws.data_ptr(), ws.numel(), _stream(p.device))
        _lib.check(rc, "ctc_amd_windowed_best_path")
        return out
    if optional_wildcards:
        with _on_device(p.device):
            rc = lib.ctc_amd_optional_wildcard_best_path(*p.common_ex(kind, wrt), *(_ptr(t) for t in out), ws.data_ptr(), ws.numel(),
                                                         _stream(p.device))
        _lib.check(rc, "ctc_amd_optional_wildcard_best_path")
        return out
    with _on_device(p.device):
        rc = lib.ctc_amd_wildcard_best_path(*p.common_ex(kind, wrt), *(_ptr(t) for t in out), ws.data_ptr(), ws.numel(),
                                            _stream(p.device))
    _lib.check(rc, "ctc_amd_wildcard_best_path")
    return out


def long_best_path(kind: int, wrt: int, p: Prepared, frames_per_tile: int = 0):
    """(score[B] float32, tokens[B,T] int32, label_index[B,T] int32, first_frame[B,U] int32, last_frame[B,U] int32): the best path
    of a lattice of up to _lib.LONG_MAX_U label positions, tiled over label blocks x time blocks (ctc_amd_long_best_path).  Reads
    the logits in the format `p` holds them in, as best_path does.  The workspace is large (0.5 KB per frame and 1024 labels): it
    is the stream's cached one, shared with the loss calls, which run in order on that stream."""
    lib = _lib.load()
    score = torch.empty(p.B, dtype=torch.float32, device=p.device)
    tokens = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    label_index = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    first_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    last_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    out = (score, tokens, label_index, first_frame, last_frame)
    if p.B == 0:
        return out
    key = ("long_best_path", kind, p.B, p.T, p.V, p.U, int(frames_per_tile))
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.long_best_path_workspace_bytes(kind, p.B, p.T, p.V, p.U, int(frames_per_tile))
    ck = (p.device, _stream(p.device))
    ws = _WS_CACHE.get(ck)
    if ws is None or ws.numel() < n:
        ws = _WS_CACHE[ck] = torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    with _on_device(p.device):
        rc = lib.ctc_amd_long_best_path(*p.common_ex(kind, wrt), int(frames_per_tile), *(_ptr(t) for t in out), ws.data_ptr(),
                                        ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_long_best_path")
    return out


def long_wildcard_best_path(kind: int, wrt: int, p: Prepared, frames_per_tile: int = 0, frame_window: Optional[torch.Tensor] = None):
    """(score[B] float32, tokens[B,T] int32, label_index[B,T] int32, first_frame[B,U] int32, last_frame[B,U] int32,
    label_score[B,U] float32): wildcard_best_path for up to _lib.LONG_MAX_U label positions, on the tiled lattice of long_best_path
    (ctc_amd_long_wildcard_best_path).  Reads the logits in the format `p` holds them in; the workspace is the stream's cached
    one, as in long_best_path.  frame_window as in wildcard_best_path, frames absolute: ctc_amd_long_windowed_best_path."""
    lib = _lib.load()
    score = torch.empty(p.B, dtype=torch.float32, device=p.device)
    tokens = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    label_index = torch.empty((p.B, p.T), dtype=torch.int32, device=p.device)
    first_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    last_frame = torch.empty((p.B, p.U), dtype=torch.int32, device=p.device)
    label_score = torch.empty((p.B, p.U), dtype=torch.float32, device=p.device)
    out = (score, tokens, label_index, first_frame, last_frame, label_score)
    if p.B == 0:
        return out
    key = ("long_wildcard_best_path", kind, p.B, p.T, p.V, p.U, int(frames_per_tile))
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.long_wildcard_best_path_workspace_bytes(kind, p.B, p.T, p.V, p.U, int(frames_per_tile))
    ck = (p.device, _stream(p.device))
    ws = _WS_CACHE.get(ck)
    if ws is None or ws.numel() < n:
        ws = _WS_CACHE[ck] = torch.empty(max(n, 1), dtype=torch.uint8, device=p.device)
    if frame_window is not None:
        fw, fws = _frame_window("long_wildcard_best_path", frame_window, p.B, p.U, p.device)
        with _on_device(p.device):
            rc = lib.ctc_amd_long_windowed_best_path(*p.common_ex(kind, wrt)[:11], _ptr(fw), fws, p.B, p.T, p.V, p.U, int(frames_per_tile),
                                                     *(_ptr(t) for t in out), ws.data_ptr(), ws.numel(), _stream(p.device))
        _lib.check(rc, "ctc_amd_long_windowed_best_path")
        return out
    with _on_device(p.device):
        rc = lib.ctc_amd_long_wildcard_best_path(*p.common_ex(kind, wrt), int(frames_per_tile), *(_ptr(t) for t in out),
                                                 ws.data_ptr(), ws.numel(), _stream(p.device))
    _lib.check(rc, "ctc_amd_long_wildcard_best_path")
    return out


def greedy_decode(kind: int, wrt: int, x: torch.Tensor, logit_length: torch.Tensor, blank: int):
    """(score[B] float32, tokens[B,T] int32, labels[B,T] int32, label_length[B] int32, frames[B,T] int32, label_score[B,T] float32):
    the frame-wise argmax path and the labels it collapses to (ctc_amd_greedy_decode).  Takes the logits as they stand -- float32 /
    bfloat16 / float16, any batch and time strides with a contiguous token axis, read in place; anything else is copied to
    contiguous float32 once -- passes no labels and does not synchronise."""
    _require_gpu(x)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if not (x.dtype in _DTYPES and (x.numel() == 0 or (x.stride(2) == 1 and x.stride(0) >= V and x.stride(1) >= V))):
        x = x.to(torch.float32).contiguous()
    if x.numel() == 0:
        x = torch.empty((B, T, V), dtype=x.dtype if x.dtype in _DTYPES else torch.float32, device=dev)
    if not (logit_length.dtype == torch.int32 and logit_length.device == dev and logit_length.is_contiguous()):
        logit_length = logit_length.to(device=dev, dtype=torch.int32).contiguous()
    score = torch.empty(B, dtype=torch.float32, device=dev)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    labels = torch.empty((B, T), dtype=torch.int32, device=dev)
    label_length = torch.empty(B, dtype=torch.int32, device=dev)
    frames = torch.empty((B, T), dtype=torch.int32, device=dev)
    label_score = torch.empty((B, T), dtype=torch.float32, device=dev)
    if B == 0:
        return score, tokens, labels, label_length, frames, label_score
    key = ("greedy_decode", B, T)
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = _lib.greedy_decode_workspace_bytes(B, T)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        rc = lib.ctc_amd_greedy_decode(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(logit_length), int(blank),
                                       B, T, V, _ptr(score), _ptr(tokens), _ptr(labels), _ptr(label_length), _ptr(frames),
                                       _ptr(label_score), ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "ctc_amd_greedy_decode")
    return score, tokens, labels, label_length, frames, label_score


def beam_search(kind: int, wrt: int, x: torch.Tensor, logit_length: torch.Tensor, blank: int, beam_width: int, top_k: int, nbest: int):
    """(score[B, nbest] float32, labels[B, nbest, T] int32, label_length[B, nbest] int32): the nbest most probable prefixes of a
    prefix beam search (ctc_amd_beam_search).  Takes the logits as greedy_decode does, passes no labels and does not synchronise."""
    _require_gpu(x)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    beam_width, top_k, nbest = int(beam_width), int(top_k), int(nbest)
    if not (x.dtype in _DTYPES and (x.numel() == 0 or (x.stride(2) == 1 and x.stride(0) >= V and x.stride(1) >= V))):
        x = x.to(torch.float32).contiguous()
    if x.numel() == 0:
        x = torch.empty((B, T, V), dtype=x.dtype if x.dtype in _DTYPES else torch.float32, device=dev)
    if not (logit_length.dtype == torch.int32 and logit_length.device == dev and logit_length.is_contiguous()):
        logit_length = logit_length.to(device=dev, dtype=torch.int32).contiguous()
    key = ("beam_search", B, T, V, beam_width, top_k)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, beam_width and top_k, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.beam_search_workspace_bytes(B, T, V, beam_width, top_k)
    if not 1 <= nbest <= beam_width:
        raise ValueError(f"ctc_amd_beam_search: nbest {nbest} outside [1, beam_width = {beam_width}]")
    score = torch.empty((B, nbest), dtype=torch.float32, device=dev)
    labels = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    label_length = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    if B == 0:
        return score, labels, label_length
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        rc = lib.ctc_amd_beam_search(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(logit_length), int(blank),
                                     B, T, V, beam_width, top_k, nbest, _ptr(score), _ptr(labels), _ptr(label_length),
                                     ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "ctc_amd_beam_search")
    return score, labels, label_length


def _nbest_args(what: str, labels, x, label_length, logit_length, U):
    """The inputs of the two N-best entry points as the C ABI takes them: (labels, x, label_length, logit_length, U, N, W)."""
    _require_gpu(x)
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if labels.dim() != 3 or label_length.dim() != 2 or int(labels.shape[0]) != B or tuple(label_length.shape) != tuple(labels.shape[:2]):
        raise ValueError(f"{what}: labels must be [B, N, W] and label_length [B, N] with B = {B}, got {tuple(labels.shape)} and "
                         f"{tuple(label_length.shape)}")
    N, W = int(labels.shape[1]), int(labels.shape[2])
    if U is None:  # as Prepared: the width always works; a wide tensor is worth one look at the maximum inside (a beam search's is T wide)
        U = W
        if U > WIDTH_WORTH_A_LOOK and label_length.numel() > 0:
            if not label_length.is_cuda:
                U = max(0, min(U, int(label_length.max())))
            elif not torch.cuda.is_current_stream_capturing():
                U = max(0, min(U, _device_max_label_length(label_length)))
    U = int(U)
    if not (x.dtype in _DTYPES and (x.numel() == 0 or (x.stride(2) == 1 and x.stride(0) >= V and x.stride(1) >= V))):
        x = x.to(torch.float32).contiguous()
    if x.numel() == 0:
        x = torch.empty((B, T, V), dtype=x.dtype if x.dtype in _DTYPES else torch.float32, device=dev)

    def i32(t):
        return t if (t.dtype == torch.int32 and t.device == dev and t.is_contiguous()) else t.to(device=dev, dtype=torch.int32).contiguous()
    return i32(labels), x, i32(label_length), i32(logit_length), U, N, W


def nbest_loss(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor, logit_length: torch.Tensor,
               blank: int, U: Optional[int] = None) -> torch.Tensor:
    """loss[B, N] float32: the exact loss of the N label sequences labels[b, n, :label_length[b, n]] of every utterance against the
    same logits[b] (ctc_amd_nbest_loss), the logits read once per group of _lib.NBEST_GROUP hypotheses.  labels [B, N, W] and
    label_length [B, N] in the layout beam_search returns; U bounds every label_length (a longer hypothesis is +inf; default: the
    labels' width W, or the maximum inside when W is large, as Prepared finds it).  Takes the logits as greedy_decode does and does not synchronise."""
    labels, x, label_length, logit_length, U, N, W = _nbest_args("nbest_loss", labels, x, label_length, logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    key = ("nbest_loss", kind, B, T, V, U, N)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, U and N, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.nbest_loss_workspace_bytes(kind, B, T, V, U, N)
    loss = torch.empty((B, N), dtype=torch.float32, device=dev)
    if B == 0:
        return loss
    ws = torch.empty(n, dtype=torch.uint8, device=dev) if n else None
    with _on_device(dev):
        rc = lib.ctc_amd_nbest_loss(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W, _ptr(label_length),
                                    _ptr(logit_length), int(blank), B, T, V, U, N, _ptr(loss), _ptr(ws), n, _stream(dev))
    _lib.check(rc, "ctc_amd_nbest_loss")
    return loss


def nbest_loss_grad(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor, logit_length: torch.Tensor,
                    blank: int, weight: torch.Tensor, U: Optional[int] = None,
                    grad_dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss[B, N] float32, grad[B, T, V]): the losses of nbest_loss, bit for bit, and the gradient of sum_n weight[b, n] * loss[b, n]
    with respect to x (ctc_amd_nbest_loss_grad).  A hypothesis whose loss is +inf contributes nothing and its weight is not
    interpreted (it may be NaN or infinite).  Arguments as nbest_loss; weight [B, N]; grad is contiguous, of grad_dtype (default:
    the element type the logits are passed in).  Does not synchronise."""
    labels, x, label_length, logit_length, U, N, W = _nbest_args("nbest_loss_grad", labels, x, label_length, logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if tuple(weight.shape) != (B, N):
        raise ValueError(f"nbest_loss_grad: weight must be [B, N] = {(B, N)}, got {tuple(weight.shape)}")
    if not (weight.dtype == torch.float32 and weight.device == dev and weight.is_contiguous()):
        weight = weight.to(device=dev, dtype=torch.float32).contiguous()
    if grad_dtype is None:
        grad_dtype = x.dtype
    if grad_dtype not in _DTYPES:
        raise ValueError(f"nbest_loss_grad: grad_dtype must be float32, bfloat16 or float16, got {grad_dtype}")
    key = ("nbest_loss_grad", kind, B, T, V, U, N)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, U and N, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.nbest_loss_grad_workspace_bytes(kind, B, T, V, U, N)
    loss = torch.empty((B, N), dtype=torch.float32, device=dev)
    grad = torch.empty((B, T, V), dtype=grad_dtype, device=dev)
    if B == 0:
        return loss, grad
    if T == 0:  # no row to write (and no gradient pointer to pass): the loss alone
        return nbest_loss(kind, wrt, labels, x, label_length, logit_length, blank, U), grad
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    with _on_device(dev):
        rc = lib.ctc_amd_nbest_loss_grad(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                         _ptr(label_length), _ptr(logit_length), int(blank), B, T, V, U, N, _ptr(weight), _ptr(loss),
                                         _ptr(grad), _DTYPES[grad_dtype], T * V, V, _ptr(ws), n, _stream(dev))
    _lib.check(rc, "ctc_amd_nbest_loss_grad")
    return loss, grad


def wildcard_loss_grad(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor, logit_length: torch.Tensor,
                       blank: int, d_loss: Optional[torch.Tensor] = None, U: Optional[int] = None,
                       grad_dtype: Optional[torch.dtype] = None, wildcard_log_weight: float = 0.0,
                       want_grad: bool = True, frame_window: Optional[torch.Tensor] = None,
                       optional_wildcards: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(loss[B] float32, grad[B, T, V] or None): the CTC loss of transcripts whose labels may be wildcards (_lib.WILDCARD), summed
    over all paths of the lattice, and its gradient times d_loss[b] (default: ones) with respect to x (ctc_amd_wildcard_loss_grad).
    want_grad=False is the forward-only launch and returns None for the gradient.  An utterance whose loss is +inf gets a zero
    gradient and its d_loss is not interpreted.  labels [B, W]; U bounds every label_length (default: W, or the maximum inside when
    W is large).  Takes the logits as greedy_decode does (float32 / bfloat16 / float16, any batch and time strides, read in place);
    grad has grad_dtype (default: the logits') and the logits' layout where that is dense, a contiguous one otherwise.
    frame_window [B, U, 2] (first, last inclusive per label position): ctc_amd_windowed_loss_grad.  optional_wildcards: labels may
    also hold _lib.OPTIONAL_WILDCARD, a wildcard that may be empty (ctc_amd_optional_wildcard_loss_grad; not with a window).  Does not
    synchronise."""
    if optional_wildcards and frame_window is not None:
        raise ValueError("wildcard_loss_grad: frame_window and optional_wildcards cannot be combined")
    if labels.dim() != 2 or label_length.dim() != 1:
        raise ValueError(f"wildcard_loss_grad: labels must be [B, W] and label_length [B], got {tuple(labels.shape)} and {tuple(label_length.shape)}")
    labels, x, label_length, logit_length, U, _, W = _nbest_args("wildcard_loss_grad", labels.unsqueeze(1), x, label_length.unsqueeze(1),
                                                                 logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if d_loss is not None:
        if tuple(d_loss.shape) != (B,):
            raise ValueError(f"wildcard_loss_grad: d_loss must be [B] = {(B,)}, got {tuple(d_loss.shape)}")
        if not (d_loss.dtype == torch.float32 and d_loss.device == dev and d_loss.is_contiguous()):
            d_loss = d_loss.to(device=dev, dtype=torch.float32).contiguous()
    if grad_dtype is None:
        grad_dtype = x.dtype
    if grad_dtype not in _DTYPES:
        raise ValueError(f"wildcard_loss_grad: grad_dtype must be float32, bfloat16 or float16, got {grad_dtype}")
    with_grad = bool(want_grad) and T > 0  # (T == 0: no row to write and no gradient pointer to pass)
    key = ("wildcard_loss_grad", kind, B, T, V, U, with_grad)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V and U, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.wildcard_loss_workspace_bytes(kind, B, T, V, U, with_grad)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    grad = torch.empty_like(x, dtype=grad_dtype) if want_grad else None  # (a dense permuted layout is kept, anything else is contiguous)
    if B == 0:
        return loss, grad
    ws = torch.empty(n, dtype=torch.uint8, device=dev) if n else None
    gsb, gst = (grad.stride(0), grad.stride(1)) if with_grad else (T * V, V)
    if frame_window is not None:
        fw, fws = _frame_window("wildcard_loss_grad", frame_window, B, U, dev)
        with _on_device(dev):
            rc = lib.ctc_amd_windowed_loss_grad(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                                _ptr(label_length), _ptr(logit_length), int(blank), _ptr(fw), fws,
                                                float(wildcard_log_weight), B, T, V, U, _ptr(d_loss), _ptr(loss),
                                                _ptr(grad) if with_grad else None, _DTYPES[grad_dtype], gsb, gst, _ptr(ws), n, _stream(dev))
        _lib.check(rc, "ctc_amd_windowed_loss_grad")
        return loss, grad
    if optional_wildcards:
        with _on_device(dev):
            rc = lib.ctc_amd_optional_wildcard_loss_grad(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                                         _ptr(label_length), _ptr(logit_length), int(blank), float(wildcard_log_weight),
                                                         B, T, V, U, _ptr(d_loss), _ptr(loss), _ptr(grad) if with_grad else None,
                                                         _DTYPES[grad_dtype], gsb, gst, _ptr(ws), n, _stream(dev))
        _lib.check(rc, "ctc_amd_optional_wildcard_loss_grad")
        return loss, grad
    with _on_device(dev):
        rc = lib.ctc_amd_wildcard_loss_grad(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                            _ptr(label_length), _ptr(logit_length), int(blank), float(wildcard_log_weight), B, T, V, U,
                                            _ptr(d_loss), _ptr(loss), _ptr(grad) if with_grad else None, _DTYPES[grad_dtype], gsb, gst,
                                            _ptr(ws), n, _stream(dev))
    _lib.check(rc, "ctc_amd_wildcard_loss_grad")
    return loss, grad


def long_wildcard_loss_grad(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor,
                            logit_length: torch.Tensor, blank: int, d_loss: Optional[torch.Tensor] = None, U: Optional[int] = None,
                            grad_dtype: Optional[torch.dtype] = None, wildcard_log_weight: float = 0.0, want_grad: bool = True,
                            frames_per_tile: int = 0, checkpoint: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(loss[B] float32, grad[B, T, V] or None): wildcard_loss_grad for up to _lib.LONG_MAX_U label positions, on the tiled lattice
    of long_wildcard_best_path (ctc_amd_long_wildcard_loss_grad).  frames_per_tile: 0 is the default tile, otherwise a positive
    multiple of _lib.LONG_FRAMES_MULTIPLE; the result does not depend on it.  Every other argument and the return value as
    wildcard_loss_grad.  The workspace is allocated per call: with a gradient it holds the lattice's float64 state of every frame
    (8 * B * ceil(U / 1024) * T * (S * 1024 + 2) bytes, S = 2 classic / 1 simplified).  checkpoint=True is
    ctc_amd_long_wildcard_loss_grad_ckpt: the same bits from a workspace of one checkpoint per tile and a ring of
    min(K, J) * frames_per_tile frames of that state (K = ceil(U / 1024), J = ceil(T / frames_per_tile)) in place of T frames, for
    one more alpha sweep; frames_per_tile then trades memory (the ring grows with it, the checkpoints shrink).  With frame windows:
    long_windowed_loss_grad.  Does not synchronise."""
    return _long_loss_grad(None, kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype, wildcard_log_weight,
                           want_grad, frames_per_tile, checkpoint)


def long_optional_wildcard_loss_grad(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor,
                                     logit_length: torch.Tensor, blank: int, d_loss: Optional[torch.Tensor] = None, U: Optional[int] = None,
                                     grad_dtype: Optional[torch.dtype] = None, wildcard_log_weight: float = 0.0, want_grad: bool = True,
                                     frames_per_tile: int = 0, checkpoint: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """long_wildcard_loss_grad whose labels may also hold _lib.OPTIONAL_WILDCARD, a wildcard position that may take no frame (as in
    wildcard_loss_grad(optional_wildcards=True); two of them may not be adjacent: +inf and a zero gradient):
    ctc_amd_long_optional_wildcard_loss_grad / _grad_ckpt.  The same arguments and return value; the workspace holds two more column
    buffers (24 * B * (ceil(U / 1024) - 1) * T bytes with a gradient, 16 without).  Without such a label the bits of
    long_wildcard_loss_grad.  Not with frame windows.  Does not synchronise."""
    return _long_loss_grad(None, kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype, wildcard_log_weight,
                           want_grad, frames_per_tile, checkpoint, optional_wildcards=True)


def long_windowed_loss_grad(frame_window: torch.Tensor, kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor,
                            label_length: torch.Tensor, logit_length: torch.Tensor, blank: int, d_loss: Optional[torch.Tensor] = None,
                            U: Optional[int] = None, grad_dtype: Optional[torch.dtype] = None, wildcard_log_weight: float = 0.0,
                            want_grad: bool = True, frames_per_tile: int = 0,
                            checkpoint: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """long_wildcard_loss_grad with frame_window [B, U, 2] in front of its arguments, as in wildcard_loss_grad and in absolute
    frames: ctc_amd_long_windowed_loss_grad / _grad_ckpt, on the same workspaces.  Every other argument and the return value as
    long_wildcard_loss_grad, whose signature stays as it is.  Does not synchronise."""
    if frame_window is None:
        raise ValueError("long_windowed_loss_grad: frame_window is required (without one: long_wildcard_loss_grad)")
    return _long_loss_grad(frame_window, kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype,
                           wildcard_log_weight, want_grad, frames_per_tile, checkpoint)


def _long_loss_grad(frame_window, kind, wrt, labels, x, label_length, logit_length, blank, d_loss, U, grad_dtype, wildcard_log_weight,
                    want_grad, frames_per_tile, checkpoint, optional_wildcards=False):
    if optional_wildcards and frame_window is not None:
        raise ValueError("long_wildcard_loss_grad: frame_window and optional_wildcards cannot be combined")
    if labels.dim() != 2 or label_length.dim() != 1:
        raise ValueError(f"long_wildcard_loss_grad: labels must be [B, W] and label_length [B], got {tuple(labels.shape)} and {tuple(label_length.shape)}")
    labels, x, label_length, logit_length, U, _, W = _nbest_args("long_wildcard_loss_grad", labels.unsqueeze(1), x, label_length.unsqueeze(1),
                                                                 logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if d_loss is not None:
        if tuple(d_loss.shape) != (B,):
            raise ValueError(f"long_wildcard_loss_grad: d_loss must be [B] = {(B,)}, got {tuple(d_loss.shape)}")
        if not (d_loss.dtype == torch.float32 and d_loss.device == dev and d_loss.is_contiguous()):
            d_loss = d_loss.to(device=dev, dtype=torch.float32).contiguous()
    if grad_dtype is None:
        grad_dtype = x.dtype
    if grad_dtype not in _DTYPES:
        raise ValueError(f"long_wildcard_loss_grad: grad_dtype must be float32, bfloat16 or float16, got {grad_dtype}")
    with_grad = bool(want_grad) and T > 0  # (T == 0: no row to write and no gradient pointer to pass)
    stem = "long_optional_wildcard_loss_grad" if optional_wildcards else "long_wildcard_loss_grad"
    name = stem + "_ckpt" if checkpoint else stem
    key = (name, kind, B, T, V, U, int(frames_per_tile), with_grad)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, U and frames_per_tile, which an empty batch would otherwise skip)
        if optional_wildcards:
            size = _lib.long_optional_wildcard_loss_ckpt_workspace_bytes if checkpoint else _lib.long_optional_wildcard_loss_workspace_bytes
        else:
            size = _lib.long_wildcard_loss_ckpt_workspace_bytes if checkpoint else _lib.long_wildcard_loss_workspace_bytes
        n = _WS_BYTES[key] = size(kind, B, T, V, U, int(frames_per_tile), with_grad)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    grad = torch.empty_like(x, dtype=grad_dtype) if want_grad else None  # (a dense permuted layout is kept, anything else is contiguous)
    if B == 0:
        return loss, grad
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    gsb, gst = (grad.stride(0), grad.stride(1)) if with_grad else (T * V, V)
    if frame_window is not None:
        fw, fws = _frame_window("long_windowed_loss_grad", frame_window, B, U, dev)
        wname = "long_windowed_loss_grad_ckpt" if checkpoint else "long_windowed_loss_grad"
        with _on_device(dev):
            call = lib.ctc_amd_long_windowed_loss_grad_ckpt if checkpoint else lib.ctc_amd_long_windowed_loss_grad
            rc = call(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                      _ptr(label_length), _ptr(logit_length), int(blank), _ptr(fw), fws, float(wildcard_log_weight), B, T, V, U,
                      int(frames_per_tile), _ptr(d_loss), _ptr(loss), _ptr(grad) if with_grad else None,
                      _DTYPES[grad_dtype], gsb, gst, _ptr(ws), n, _stream(dev))
        _lib.check(rc, "ctc_amd_" + wname)
        return loss, grad
    with _on_device(dev):
        if optional_wildcards:
            call = lib.ctc_amd_long_optional_wildcard_loss_grad_ckpt if checkpoint else lib.ctc_amd_long_optional_wildcard_loss_grad
        else:
            call = lib.ctc_amd_long_wildcard_loss_grad_ckpt if checkpoint else lib.ctc_amd_long_wildcard_loss_grad
        rc = call(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                  _ptr(label_length), _ptr(logit_length), int(blank), float(wildcard_log_weight), B, T, V, U,
                  int(frames_per_tile), _ptr(d_loss), _ptr(loss), _ptr(grad) if with_grad else None,
                  _DTYPES[grad_dtype], gsb, gst, _ptr(ws), n, _stream(dev))
    _lib.check(rc, "ctc_amd_" + name)
    return loss, grad


def label_posterior(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor, logit_length: torch.Tensor,
                    blank: int, U: Optional[int] = None, wildcard_log_weight: float = 0.0, want_stats: bool = True,
                    frame_window: Optional[torch.Tensor] = None, optional_wildcards: bool = False):
    """(loss[B], label_posterior[B, T, U], blank_posterior[B, T], duration[B, U], expected_frame[B, U]), all float32: with what
    probability every frame belongs to every label position (or to the blank) over all paths of the lattice, and per position the
    expected number of frames and the soft timestamp (ctc_amd_label_posterior).  Labels may be wildcards (_lib.WILDCARD); the loss
    is wildcard_loss_grad's forward-only one, bit for bit.  want_stats=False skips the statistics launch and returns None for the
    last two.  Arguments as wildcard_loss_grad (frame_window: ctc_amd_windowed_label_posterior; optional_wildcards:
    ctc_amd_optional_wildcard_label_posterior); every element of every output is written.  Does not synchronise."""
    if optional_wildcards and frame_window is not None:
        raise ValueError("label_posterior: frame_window and optional_wildcards cannot be combined")
    if labels.dim() != 2 or label_length.dim() != 1:
        raise ValueError(f"label_posterior: labels must be [B, W] and label_length [B], got {tuple(labels.shape)} and {tuple(label_length.shape)}")
    labels, x, label_length, logit_length, U, _, W = _nbest_args("label_posterior", labels.unsqueeze(1), x, label_length.unsqueeze(1),
                                                                 logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    key = ("label_posterior", kind, B, T, V, U)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V and U, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.label_posterior_workspace_bytes(kind, B, T, V, U)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    post = torch.empty((B, T, U), dtype=torch.float32, device=dev)
    blk = torch.empty((B, T), dtype=torch.float32, device=dev)
    dur = torch.empty((B, U), dtype=torch.float32, device=dev) if want_stats else None
    exf = torch.empty((B, U), dtype=torch.float32, device=dev) if want_stats else None
    if B == 0:
        return loss, post, blk, dur, exf
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    if frame_window is not None:
        fw, fws = _frame_window("label_posterior", frame_window, B, U, dev)
        with _on_device(dev):
            rc = lib.ctc_amd_windowed_label_posterior(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                                      _ptr(label_length), _ptr(logit_length), int(blank), _ptr(fw), fws,
                                                      float(wildcard_log_weight), B, T, V, U, _ptr(loss), _ptr(post), _ptr(blk),
                                                      _ptr(dur), _ptr(exf), _ptr(ws), n, _stream(dev))
        _lib.check(rc, "ctc_amd_windowed_label_posterior")
        return loss, post, blk, dur, exf
    if optional_wildcards:
        with _on_device(dev):
            rc = lib.ctc_amd_optional_wildcard_label_posterior(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels),
                                                               W, _ptr(label_length), _ptr(logit_length), int(blank),
                                                               float(wildcard_log_weight), B, T, V, U, _ptr(loss), _ptr(post), _ptr(blk),
                                                               _ptr(dur), _ptr(exf), _ptr(ws), n, _stream(dev))
        _lib.check(rc, "ctc_amd_optional_wildcard_label_posterior")
        return loss, post, blk, dur, exf
    with _on_device(dev):
        rc = lib.ctc_amd_label_posterior(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                         _ptr(label_length), _ptr(logit_length), int(blank), float(wildcard_log_weight), B, T, V, U,
                                         _ptr(loss), _ptr(post), _ptr(blk), _ptr(dur), _ptr(exf), _ptr(ws), n, _stream(dev))
    _lib.check(rc, "ctc_amd_label_posterior")
    return loss, post, blk, dur, exf


def long_label_posterior(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor,
                         logit_length: torch.Tensor, blank: int, U: Optional[int] = None, wildcard_log_weight: float = 0.0,
                         frames_per_tile: int = 0, dense: bool = True, want_stats: bool = True, want_peak: bool = True,
                         frame_window: Optional[torch.Tensor] = None):
    """(loss[B], label_posterior[B, T, U] or None, blank_posterior[B, T], duration[B, U], expected_frame[B, U], peak_posterior[B, U]
    float32, peak_frame[B, U] int32): label_posterior for up to _lib.LONG_MAX_U label positions, on the tiled lattice and from the
    workspace of long_wildcard_loss_grad(checkpoint=True) (ctc_amd_long_label_posterior).  dense=False returns None for the
    [B, T, U] matrix, which is then neither allocated nor written; every other output keeps its bits.  peak_posterior is
    max_t label_posterior and peak_frame the lowest frame that attains it (0 / -1 from label_length on).  want_stats=False /
    want_peak=False return None for the pair.  frames_per_tile as in long_wildcard_loss_grad; no output depends on it.  frame_window
    as in label_posterior, frames absolute: ctc_amd_long_windowed_label_posterior.  Every element of every output is written.  Does
    not synchronise."""
    return _long_label_posterior("long_label_posterior", False, kind, wrt, labels, x, label_length, logit_length, blank, U,
                                 wildcard_log_weight, frames_per_tile, dense, want_stats, want_peak, frame_window)


def long_optional_wildcard_label_posterior(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor,
                                           logit_length: torch.Tensor, blank: int, U: Optional[int] = None,
                                           wildcard_log_weight: float = 0.0, frames_per_tile: int = 0, dense: bool = True,
                                           want_stats: bool = True, want_peak: bool = True):
    """long_label_posterior whose labels may also hold _lib.OPTIONAL_WILDCARD (ctc_amd_long_optional_wildcard_label_posterior): the
    same arguments but the window, the same seven outputs.  The column of an optional position may sum to less than one frame, and
    its duration is the expected number of frames it takes; the loss is long_optional_wildcard_loss_grad's, bit for bit.  Does not
    synchronise."""
    return _long_label_posterior("long_optional_wildcard_label_posterior", True, kind, wrt, labels, x, label_length, logit_length, blank, U,
                                 wildcard_log_weight, frames_per_tile, dense, want_stats, want_peak, None)


def _long_label_posterior(what, optional_wildcards, kind, wrt, labels, x, label_length, logit_length, blank, U, wildcard_log_weight,
                          frames_per_tile, dense, want_stats, want_peak, frame_window):
    if labels.dim() != 2 or label_length.dim() != 1:
        raise ValueError(f"{what}: labels must be [B, W] and label_length [B], got {tuple(labels.shape)} and {tuple(label_length.shape)}")
    labels, x, label_length, logit_length, U, _, W = _nbest_args(what, labels.unsqueeze(1), x, label_length.unsqueeze(1), logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    key = (what, kind, B, T, V, U, int(frames_per_tile))
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, U and frames_per_tile, which an empty batch would otherwise skip)
        size = _lib.long_optional_wildcard_label_posterior_workspace_bytes if optional_wildcards else _lib.long_label_posterior_workspace_bytes
        n = _WS_BYTES[key] = size(kind, B, T, V, U, int(frames_per_tile))
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    post = torch.empty((B, T, U), dtype=torch.float32, device=dev) if dense else None
    blk = torch.empty((B, T), dtype=torch.float32, device=dev)
    dur = torch.empty((B, U), dtype=torch.float32, device=dev) if want_stats else None
    exf = torch.empty((B, U), dtype=torch.float32, device=dev) if want_stats else None
    peak = torch.empty((B, U), dtype=torch.float32, device=dev) if want_peak else None
    pfr = torch.empty((B, U), dtype=torch.int32, device=dev) if want_peak else None
    if B == 0:
        return loss, post, blk, dur, exf, peak, pfr
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    if frame_window is not None:
        fw, fws = _frame_window("long_label_posterior", frame_window, B, U, dev)
        with _on_device(dev):
            rc = lib.ctc_amd_long_windowed_label_posterior(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                                           _ptr(label_length), _ptr(logit_length), int(blank), _ptr(fw), fws,
                                                           float(wildcard_log_weight), B, T, V, U, int(frames_per_tile), _ptr(loss),
                                                           _ptr(post), _ptr(blk), _ptr(dur), _ptr(exf), _ptr(peak), _ptr(pfr), _ptr(ws), n,
                                                           _stream(dev))
        _lib.check(rc, "ctc_amd_long_windowed_label_posterior")
        return loss, post, blk, dur, exf, peak, pfr
    name = "ctc_amd_long_optional_wildcard_label_posterior" if optional_wildcards else "ctc_amd_long_label_posterior"
    with _on_device(dev):  # (the two entry points have one argument list)
        rc = getattr(lib, name)(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W, _ptr(label_length),
                                _ptr(logit_length), int(blank), float(wildcard_log_weight), B, T, V, U, int(frames_per_tile), _ptr(loss),
                                _ptr(post), _ptr(blk), _ptr(dur), _ptr(exf), _ptr(peak), _ptr(pfr), _ptr(ws), n, _stream(dev))
    _lib.check(rc, name)
    return loss, post, blk, dur, exf, peak, pfr


def nbest_best_path(kind: int, wrt: int, labels: torch.Tensor, x: torch.Tensor, label_length: torch.Tensor, logit_length: torch.Tensor,
                    blank: int, U: Optional[int] = None):
    """(score[B, N] float32, tokens[B, N, T] int32, label_index[B, N, T] int32, first_frame[B, N, U] int32, last_frame[B, N, U] int32):
    the best path of every one of the N label sequences labels[b, n, :label_length[b, n]] against the same logits[b], and the first
    and last frame of every label on it (ctc_amd_nbest_best_path), the logits read once per group of _lib.NBEST_GROUP hypotheses.
    Arguments as nbest_loss; U (default as there) is also the width of first_frame / last_frame.  Does not synchronise."""
    labels, x, label_length, logit_length, U, N, W = _nbest_args("nbest_best_path", labels, x, label_length, logit_length, U)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    key = ("nbest_best_path", kind, B, T, V, U, N)
    n = _WS_BYTES.get(key)
    if n is None:  # (also the check of V, U and N, which an empty batch would otherwise skip)
        n = _WS_BYTES[key] = _lib.nbest_best_path_workspace_bytes(kind, B, T, V, U, N)
    score = torch.empty((B, N), dtype=torch.float32, device=dev)
    tokens = torch.empty((B, N, T), dtype=torch.int32, device=dev)
    label_index = torch.empty((B, N, T), dtype=torch.int32, device=dev)
    first_frame = torch.empty((B, N, U), dtype=torch.int32, device=dev)
    last_frame = torch.empty((B, N, U), dtype=torch.int32, device=dev)
    if B == 0:
        return score, tokens, label_index, first_frame, last_frame
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        rc = lib.ctc_amd_nbest_best_path(kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(labels), W,
                                         _ptr(label_length), _ptr(logit_length), int(blank), B, T, V, U, N, _ptr(score), _ptr(tokens),
                                         _ptr(label_index), _ptr(first_frame), _ptr(last_frame), ws.data_ptr(), n, _stream(dev))
    _lib.check(rc, "ctc_amd_nbest_best_path")
    return score, tokens, label_index, first_frame, last_frame


def edit_distance(hyp: torch.Tensor, hyp_length: torch.Tensor, ref: torch.Tensor, ref_length: torch.Tensor,
                  R: Optional[int] = None) -> torch.Tensor:
    """distance[B, N] int32: the Levenshtein distance (unit costs) of every hypothesis hyp[b, n, :hyp_length[b, n]] to its utterance's
    reference ref[b, :ref_length[b]] (ctc_amd_edit_distance).  hyp [B, N, W] and hyp_length [B, N] in the layout beam_search
    returns; ref [B, Wr], ref_length [B]; tokens are any int32 values.  R bounds every ref_length (an utterance with a longer
    reference gets -1 throughout; default: the reference tensor's width Wr).  One launch, no workspace; does not synchronise."""
    _require_gpu(hyp)
    dev = hyp.device
    if (hyp.dim() != 3 or hyp_length.dim() != 2 or ref.dim() != 2 or ref_length.dim() != 1
            or tuple(hyp_length.shape) != tuple(hyp.shape[:2]) or int(ref.shape[0]) != int(hyp.shape[0])
            or int(ref_length.shape[0]) != int(hyp.shape[0])):
        raise ValueError(f"edit_distance: hyp must be [B, N, W], hyp_length [B, N], ref [B, Wr] and ref_length [B], got "
                         f"{tuple(hyp.shape)}, {tuple(hyp_length.shape)}, {tuple(ref.shape)} and {tuple(ref_length.shape)}")
    B, N, W = (int(s) for s in hyp.shape)
    Wr = int(ref.shape[1])
    R = Wr if R is None else int(R)
    key = ("edit_distance", B, N, R)
    if key not in _WS_BYTES:  # (0 bytes; the check of N and R, which an empty batch would otherwise skip)
        _WS_BYTES[key] = _lib.edit_distance_workspace_bytes(B, N, R)

    def i32(t):
        return t if (t.dtype == torch.int32 and t.device == dev and t.is_contiguous()) else t.to(device=dev, dtype=torch.int32).contiguous()
    hyp, hyp_length, ref, ref_length = i32(hyp), i32(hyp_length), i32(ref), i32(ref_length)
    distance = torch.empty((B, N), dtype=torch.int32, device=dev)
    if B == 0:
        return distance
    with _on_device(dev):
        rc = _lib.load().ctc_amd_edit_distance(_ptr(hyp), W, _ptr(hyp_length), _ptr(ref), Wr, _ptr(ref_length), B, N, R,
                                               _ptr(distance), None, 0, _stream(dev))
    _lib.check(rc, "ctc_amd_edit_distance")
    return distance


def edit_counts(hyp: torch.Tensor, hyp_length: torch.Tensor, ref: torch.Tensor, ref_length: torch.Tensor,
                R: Optional[int] = None, rows_per_tile: Optional[int] = None) -> torch.Tensor:
    """counts[B, N, 4] int32: (distance, substitutions, insertions, deletions) of every hypothesis hyp[b, n, :hyp_length[b, n]]
    against its utterance's reference ref[b, :ref_length[b]] (ctc_amd_edit_counts): the lexicographic minimum of (distance,
    substitutions, insertions) over all alignments.  The tensors are those of edit_distance; the reference may be up to 65536
    tokens long and the hypotheses up to 2^20.  R bounds every ref_length (an utterance with a longer reference gets -1
    throughout; default: the reference tensor's width Wr).  rows_per_tile (None: the library's default) is the number of
    hypothesis tokens per tile; the result does not depend on it.  Does not synchronise."""
    _require_gpu(hyp)
    dev = hyp.device
    if (hyp.dim() != 3 or hyp_length.dim() != 2 or ref.dim() != 2 or ref_length.dim() != 1
            or tuple(hyp_length.shape) != tuple(hyp.shape[:2]) or int(ref.shape[0]) != int(hyp.shape[0])
            or int(ref_length.shape[0]) != int(hyp.shape[0])):
        raise ValueError(f"edit_counts: hyp must be [B, N, W], hyp_length [B, N], ref [B, Wr] and ref_length [B], got "
                         f"{tuple(hyp.shape)}, {tuple(hyp_length.shape)}, {tuple(ref.shape)} and {tuple(ref_length.shape)}")
    B, N, W = (int(s) for s in hyp.shape)
    Wr = int(ref.shape[1])
    R = Wr if R is None else int(R)
    rt = 0 if rows_per_tile is None else int(rows_per_tile)
    key = ("edit_counts", B, N, R, W, rt)
    if key not in _WS_BYTES:  # (also the check of the shape, which an empty batch would otherwise skip)
        _WS_BYTES[key] = _lib.edit_counts_workspace_bytes(B, N, R, W, rt)
    n = _WS_BYTES[key]

    def i32(t):
        return t if (t.dtype == torch.int32 and t.device == dev and t.is_contiguous()) else t.to(device=dev, dtype=torch.int32).contiguous()
    hyp, hyp_length, ref, ref_length = i32(hyp), i32(hyp_length), i32(ref), i32(ref_length)
    counts = torch.empty((B, N, 4), dtype=torch.int32, device=dev)
    if B == 0:
        return counts
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        rc = _lib.load().ctc_amd_edit_counts(_ptr(hyp), W, _ptr(hyp_length), _ptr(ref), Wr, _ptr(ref_length), B, N, R, rt,
                                             _ptr(counts), ws.data_ptr(), n, _stream(dev))
    _lib.check(rc, "ctc_amd_edit_counts")
    return counts


def prefix_prepare(wrt: int, x: torch.Tensor, logit_length: torch.Tensor):
    """(x, logit_length, rows) of a prefix scorer: the logits as greedy_decode takes them and, for logits, the row statistics
    (ctc_amd_prefix_rows: one launch, once per scorer); rows is None for log-probabilities."""
    _require_gpu(x)
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    if not (x.dtype in _DTYPES and (x.numel() == 0 or (x.stride(2) == 1 and x.stride(0) >= V and x.stride(1) >= V))):
        x = x.to(torch.float32).contiguous()
    if x.numel() == 0:
        x = torch.empty((B, T, V), dtype=x.dtype if x.dtype in _DTYPES else torch.float32, device=dev)
    if not (logit_length.dtype == torch.int32 and logit_length.device == dev and logit_length.is_contiguous()):
        logit_length = logit_length.to(device=dev, dtype=torch.int32).contiguous()
    _lib.prefix_workspace_bytes(B, T, V, 1)  # (the check of V, which an empty batch would otherwise skip)
    if wrt != _lib.WRT_LOGITS:
        return x, logit_length, None
    rows = torch.empty((B, T, 2), dtype=torch.float32, device=dev)
    if B > 0:
        with _on_device(dev):
            rc = lib.ctc_amd_prefix_rows(_ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(logit_length), B, T, V,
                                         _ptr(rows), rows.numel() * 4, _stream(dev))
        _lib.check(rc, "ctc_amd_prefix_rows")
    return x, logit_length, rows


def _prefix_common(kind: int, wrt: int, x, logit_length, blank: int, N: int, rows):
    B, T, V = (int(s) for s in x.shape)
    return (kind, wrt, _ptr(x), _DTYPES[x.dtype], x.stride(0), x.stride(1), _ptr(logit_length), int(blank), B, T, V, int(N),
            _ptr(rows), 0 if rows is None else rows.numel() * 4)


def prefix_extend(kind: int, wrt: int, x, logit_length, blank: int, rows, N: int, state, last_token, length, parent, token):
    """(state [B, N, 2 T + 2] float64, last_token [B, N] int32, length [B, N] int32, full_score [B, N] float32) of the hypotheses
    (parent[b, n], token[b, n]) of the beam (state, last_token, length); state None starts a beam (ctc_amd_prefix_extend)."""
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    _lib.prefix_workspace_bytes(B, T, V, N)

    def i32(t):
        if tuple(t.shape) != (B, N):
            raise ValueError(f"prefix_extend: parent and token must be [B, N] = [{B}, {N}], got {tuple(t.shape)}")
        return t if (t.dtype == torch.int32 and t.device == dev and t.is_contiguous()) else t.to(device=dev, dtype=torch.int32).contiguous()
    parent, token = i32(parent), i32(token)
    new_state = torch.empty((B, N, 2 * T + 2), dtype=torch.float64, device=dev)
    new_last = torch.empty((B, N), dtype=torch.int32, device=dev)
    new_length = torch.empty((B, N), dtype=torch.int32, device=dev)
    full = torch.empty((B, N), dtype=torch.float32, device=dev)
    if B == 0:
        return new_state, new_last, new_length, full
    with _on_device(dev):
        rc = lib.ctc_amd_prefix_extend(*_prefix_common(kind, wrt, x, logit_length, blank, N, rows), _ptr(state), _ptr(last_token),
                                       _ptr(length), _ptr(parent), _ptr(token), _ptr(new_state), new_state.numel() * 8,
                                       _ptr(new_last), _ptr(new_length), _ptr(full), _stream(dev))
    _lib.check(rc, "ctc_amd_prefix_extend")
    return new_state, new_last, new_length, full


def prefix_score(kind: int, wrt: int, x, logit_length, blank: int, rows, N: int, state, last_token, length) -> torch.Tensor:
    """score [B, N, V] float32: ln psi(g . c) of every hypothesis of the beam and every token (ctc_amd_prefix_score)."""
    lib = _lib.load()
    dev = x.device
    B, T, V = (int(s) for s in x.shape)
    score = torch.empty((B, N, V), dtype=torch.float32, device=dev)
    if B == 0:
        return score
    with _on_device(dev):
        rc = lib.ctc_amd_prefix_score(*_prefix_common(kind, wrt, x, logit_length, blank, N, rows), _ptr(state), state.numel() * 8,
                                      _ptr(last_token), _ptr(length), _ptr(score), _stream(dev))
    _lib.check(rc, "ctc_amd_prefix_score")
    return score


def check_labels(labels, label_length, num_tokens: int, blank_index: int = 0) -> None:
    """Opt-in validation (off the hot path: synchronises): raises ValueError if a label inside its `label_length` lies
    outside [0, num_tokens) or equals `blank_index` -- what TF-CPU's gather reports as InvalidArgumentError for
    out-of-range labels (base_loss.py:328-344).  The loss functions themselves treat such a label as an impossible
    emission (loss +inf, zero gradient)."""
    labels = torch.as_tensor(labels)
    label_length = torch.as_tensor(label_length)
    if not labels.is_cuda:
        labels = labels.cuda()
    label_length = label_length.to(labels.device)
    labels = labels.to(torch.int32).contiguous()
    label_length = label_length.to(torch.int32).contiguous()
    B, U = int(labels.shape[0]), int(labels.shape[1])
    if B == 0 or U == 0:
        return
    with _on_device(labels.device):
        _lib.check(_lib.load().ctc_amd_check_labels(_ptr(labels), U, _ptr(label_length), int(blank_index), B, int(num_tokens), U,
                                                    _stream(labels.device)), "ctc_amd_check_labels")
