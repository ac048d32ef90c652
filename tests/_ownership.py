"""Ownership invariance: helpers that change ONLY memory an utterance does not own, and thin wrappers that
call the C ABI directly so that a test controls every output and workspace buffer.

An utterance owns the frames t < clamp(logit_length[b], 0, T) of its logits (and of `vec`), the label positions u < max(label_length[b], 0)
and the V leading elements of each of those rows.  Everything else -- padding frames, label tails, the elements between V and the
row stride, packed rows between utterances, the workspace and the outputs on entry -- may hold anything.

The helpers work on torch tensors (CPU or GPU, any element type) and keep the strides of what they are given; nothing here needs a
GPU until a wrapper is called.  Results are compared by their bits, never by closeness."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

POISON_F32 = (float("nan"), float("inf"), float("-inf"), 3.0e38)
BYTE_PATTERNS = (0x00, 0xFF, 0xA5)  # 0xFF: a NaN as float32 / bfloat16 / float16, -1 as int32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---- bits ----

def bits(t):
    """The tensor's elements as integers of the same width (NaN == NaN, -0.0 != 0.0): what "the same result" means here."""
    return t.view(_BITS[t.element_size()]) if t.is_floating_point() else t


def count_diff(a, b):
    """Number of elements whose bits differ."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum().item())


def same_bits(a, b):
    return count_diff(a, b) == 0


def poison_values(dtype):
    """What to put into padding frames of a tensor of this element type: the four float32 values, or NaN and the largest finite
    value of a 16-bit type."""
    if dtype == torch.float32:
        return POISON_F32
    return (float("nan"), float(torch.finfo(dtype).max))


# ---- byte-pattern fills ----

def byte_fill(nbytes, pattern, device):
    return torch.full((max(int(nbytes), 1),), pattern, dtype=torch.uint8, device=device)


def filled(shape, dtype, pattern, device):
    """A contiguous tensor every byte of which is `pattern`."""
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return byte_fill(n, pattern, device)[:n].view(dtype).reshape(tuple(shape))


def prefill_value(dtype, pattern):
    """The element (as a tensor of one) that `filled` puts everywhere."""
    return filled((1,), dtype, pattern, "cpu")


def keeps_prefill(t, pattern):
    """Mask of the elements that still hold the byte pattern."""
    return bits(t) == bits(prefill_value(t.dtype, pattern)).to(t.device)


# ---- what the utterances do not own ----

def _clone_keeping_strides(x):
    out = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    out.copy_(x)
    return out


def _i64(a):
    return a.detach().cpu().to(torch.int64) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=torch.int64)


def padding_mask(logit_length, T):
    """[B, T] bool: frame t lies at or beyond clamp(logit_length[b], 0, T)."""
    tl = _i64(logit_length).clamp(0, T)
    return torch.arange(T)[None, :] >= tl[:, None]


def poison_padding(x, logit_length, value):
    """A copy of x[B, T, ...] (same strides: a time-major view stays one) whose frames t >= clamp(logit_length[b], 0, T) hold
    `value`."""
    out = _clone_keeping_strides(x)
    out[padding_mask(logit_length, x.shape[1]).to(x.device)] = value
    return out


def label_poison_cycle(V, blank):
    return (-7, V + 100, blank, INT32_MIN, INT32_MAX)


def poison_labels(labels, label_length, values):
    """A copy of labels[B, S] whose positions u >= max(label_length[b], 0) cycle through `values` (starting at another one in
    every row); where a position already holds its value, the next one of the cycle is taken, so that every tail position changes."""
    B, S = labels.shape
    ll = _i64(label_length).clamp(min=0)
    tail = (torch.arange(S)[None, :] >= ll[:, None]).to(labels.device)
    vals = torch.tensor(list(values), dtype=torch.int64, device=labels.device)
    idx = (torch.arange(S, device=labels.device)[None, :] + torch.arange(B, device=labels.device)[:, None]) % len(vals)
    pick = vals[idx]
    pick = torch.where(pick == labels.to(torch.int64), vals[(idx + 1) % len(vals)], pick)
    return torch.where(tail, pick.to(labels.dtype), labels)


def strided_storage(x, stride_b, stride_t, pattern=0x00):
    """Dense x[B, T, V] laid out with element strides (stride_b, stride_t, 1) inside a flat buffer whose other bytes hold `pattern`.
    Returns (storage, view, owned): the flat buffer, its [B, T, V] view, and the mask of the buffer's elements some row owns.
    A time-major layout is stride_b = V (or more), stride_t = B * stride_b (or more)."""
    B, T, V = x.shape
    n = (B - 1) * stride_b + (T - 1) * stride_t + V if B and T else 0
    storage = filled((n,), x.dtype, pattern, x.device)
    view = storage.as_strided((B, T, V), (stride_b, stride_t, 1))
    view.copy_(x)
    owned = torch.zeros(n, dtype=torch.bool, device=x.device)
    owned.as_strided((B, T, V), (stride_b, stride_t, 1)).fill_(True)
    return storage, view, owned


def packed_storage(x, logit_length, row_offsets, row_stride, total_rows, pattern=0x00):
    """Packed (ragged) layout of dense x[B, T, V]: utterance b owns the V leading elements of the rows row_offsets[b] ..
    row_offsets[b] + clamp(logit_length[b], 0, T) - 1 of a [total_rows, row_stride] buffer; everything else holds `pattern`.
    Returns (storage[total_rows, row_stride], owned mask of the same shape)."""
    B, T, V = x.shape
    storage = filled((total_rows, row_stride), x.dtype, pattern, x.device)
    owned = torch.zeros((total_rows, row_stride), dtype=torch.bool, device=x.device)
    for b in range(B):
        n, r0 = min(max(int(logit_length[b]), 0), T), int(row_offsets[b])
        assert r0 >= 0 and r0 + n <= total_rows and not owned[r0:r0 + n].any(), "rows overlap or leave the buffer"
        storage[r0:r0 + n, :V] = x[b, :n]
        owned[r0:r0 + n, :V] = True
    return storage, owned


def poison_gaps(storage, owned, value):
    """A copy of a strided or packed buffer whose unowned elements (between V and the row stride, between the utterances' strides,
    packed rows nobody owns) hold `value`."""
    out = storage.clone()
    out[~owned] = value
    return out


# ---- the C ABI, with every buffer under the caller's control ----

def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    from tf_seq2seq_losses_amd import _lib
    return {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[t.dtype]


def dev(a, dtype=None):
    """A fresh device copy of a NumPy array (the shared inputs are read-only)."""
    t = torch.tensor(np.asarray(a), device=_dev())
    return t if dtype is None else t.to(dtype)


class Inputs(SimpleNamespace):
    """Device inputs of one call: kind (0 / 1), x[B, T, V] (any strides with a contiguous token axis, any of the three element
    types), labels[B, S] int32, ll[B], tl[B] int32, U, blank."""

    @property
    def shape(self):
        B, T, V = self.x.shape
        return B, T, V, self.U

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Inputs(**d)

    def common(self, wrt):
        B, T, V, U = self.shape
        assert self.x.is_contiguous() and self.x.dtype == torch.float32
        return (self.kind, wrt, self.x.data_ptr(), self.labels.data_ptr(), self.labels.shape[1], self.ll.data_ptr(), self.tl.data_ptr(),
                self.blank, B, T, V, U)

    def common_ex(self, wrt):
        B, T, V, U = self.shape
        assert self.x.stride(2) == 1
        return (self.kind, wrt, self.x.data_ptr(), _dt(self.x), self.x.stride(0), self.x.stride(1), self.labels.data_ptr(),
                self.labels.shape[1], self.ll.data_ptr(), self.tl.data_ptr(), self.blank, B, T, V, U)


def make_inputs(kind, x, labels, ll, tl, U=None, blank=0):
    """Inputs from NumPy arrays / tensors: x is taken as it stands when it is a device tensor (views keep their strides)."""
    xt = x if isinstance(x, torch.Tensor) else dev(x)
    lab = labels if isinstance(labels, torch.Tensor) else dev(labels)
    return Inputs(kind=int(kind), x=xt, labels=lab.to(torch.int32), ll=dev(np.asarray(ll, np.int32)), tl=dev(np.asarray(tl, np.int32)),
                  U=int(lab.shape[1] if U is None else U), blank=int(blank))


def workspace(nbytes, pattern):
    return byte_fill(nbytes, pattern, _dev())


def _ok(rc, what):
    from tf_seq2seq_losses_amd import _lib
    assert rc == 0, (what, rc, _lib.load().ctc_amd_last_error())


def _grad_like(x, pattern):
    """Gradient buffer with the logits' element type and strides, every byte `pattern`: (storage, [B, T, V] view)."""
    B, T, V = x.shape
    n = (B - 1) * x.stride(0) + (T - 1) * x.stride(1) + V
    storage = filled((n,), x.dtype, pattern, x.device)
    return storage, storage.as_strided((B, T, V), x.stride())


LOSS_GRAD_ENTRIES = ("loss_grad", "loss_only", "ex", "two_call", "sum")


def loss_grad(inp, entry="loss_grad", wrt=0, fill=0xA5, ws=None, selector=None, d_loss=None):
    """One loss(+gradient) call through `entry`:
        loss_grad  ctc_amd_loss_grad               loss_only  the same with grad == NULL
        ex         ctc_amd_loss_grad_ex            two_call   ctc_amd_loss_forward, then ctc_amd_grad_resume on the untouched workspace
        sum        ctc_amd_loss_grad_sum (sum2 starts at zero: an accumulator by contract; zero_next is prefilled)
    Outputs are prefilled with the byte `fill`; `ws` is the workspace to use as it stands (None: a new one of the selector's size
    filled with `fill`).  Returns a namespace: out = {name: tensor} of everything the call writes, grad_storage, ws."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U = inp.shape
    if selector is None:
        selector = _lib.WS_LOSS_GRAD_LOGITS if (wrt == 0 and inp.x.dtype == torch.float32) else _lib.WS_LOSS_GRAD
    if ws is None:
        ws = workspace(_lib.workspace_bytes(selector, inp.kind, B, T, V, U), fill)
    loss = filled((B,), torch.float32, fill, _dev())
    dl = None if d_loss is None else d_loss.data_ptr()
    out = {"loss": loss}
    gs = grad = None
    if entry != "loss_only":
        gs, grad = _grad_like(inp.x, fill)
        out["grad"] = grad
    st = _stream()
    if entry in ("loss_grad", "loss_only"):
        _ok(lib.ctc_amd_loss_grad(*inp.common(wrt), loss.data_ptr(), None if grad is None else grad.data_ptr(), dl, ws.data_ptr(),
                                  ws.numel(), st), entry)
    else:
        ex = inp.common_ex(wrt)
        gfmt = (grad.data_ptr(), _dt(grad), grad.stride(0), grad.stride(1))
        if entry == "ex":
            _ok(lib.ctc_amd_loss_grad_ex(*ex, loss.data_ptr(), *gfmt, dl, ws.data_ptr(), ws.numel(), st), entry)
        elif entry == "two_call":
            loss1 = filled((B,), torch.float32, fill, _dev())
            _ok(lib.ctc_amd_loss_forward(*ex, loss1.data_ptr(), ws.data_ptr(), ws.numel(), st), "loss_forward")
            _ok(lib.ctc_amd_grad_resume(*ex, loss.data_ptr(), *gfmt, dl, ws.data_ptr(), ws.numel(), st), "grad_resume")
            out["loss_forward"] = loss1
            del out["loss"]  # (the resume call rewrites only the losses of utterances it redoes: not an output of its own)
        elif entry == "sum":
            sum2 = torch.zeros(2, dtype=torch.int64, device=_dev())
            zero_next = filled((2,), torch.int64, fill, _dev())
            _ok(lib.ctc_amd_loss_grad_sum(*ex, loss.data_ptr(), *gfmt, dl, sum2.data_ptr(), zero_next.data_ptr(), ws.data_ptr(),
                                          ws.numel(), st), entry)
            out["sum2"], out["zero_next"] = sum2, zero_next
        else:
            raise ValueError(entry)
    torch.cuda.synchronize()
    return SimpleNamespace(out=out, grad_storage=gs, ws=ws)


def loss_grad_packed(inp, storage, row_offsets, row_stride, fill=0xA5, wrt=0):
    """ctc_amd_loss_grad_packed on a [total_rows, row_stride] buffer; the gradient buffer has the same shape, prefilled."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U = inp.shape
    ws = workspace(_lib.workspace_bytes(_lib.WS_LOSS_GRAD, inp.kind, B, T, V, U), fill)
    loss = filled((B,), torch.float32, fill, _dev())
    grad = filled(tuple(storage.shape), storage.dtype, fill, _dev())
    offs = dev(np.asarray(row_offsets, np.int64))
    _ok(lib.ctc_amd_loss_grad_packed(inp.kind, wrt, storage.data_ptr(), _dt(storage), offs.data_ptr(), row_stride, inp.labels.data_ptr(),
                                     inp.labels.shape[1], inp.ll.data_ptr(), inp.tl.data_ptr(), inp.blank, B, T, V, U, loss.data_ptr(),
                                     grad.data_ptr(), _dt(grad), row_stride, None, ws.data_ptr(), ws.numel(), _stream()), "packed")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"loss": loss, "grad": grad}, ws=ws)


def _log_domain(inp, what, fill, ws):
    from tf_seq2seq_losses_amd import _lib
    B, T, V, U = inp.shape
    if ws is None:
        ws = workspace(_lib.workspace_bytes(what, inp.kind, B, T, V, U), fill)
    return _lib.load(), ws, filled((B,), torch.float32, fill, _dev())


def hvp(inp, vec, wrt=0, fill=0xA5, ws=None, want_grad=True):
    """(want_grad=False: grad == NULL, the only form of the call that the fused kernel serves)"""
    from tf_seq2seq_losses_amd import _lib
    lib, ws, loss = _log_domain(inp, _lib.WS_HVP, fill, ws)
    B, T, V, _ = inp.shape
    out = {"loss": loss, "hvp": filled((B, T, V), torch.float32, fill, _dev())}
    if want_grad:
        out["grad"] = filled((B, T, V), torch.float32, fill, _dev())
    assert vec.is_contiguous() and vec.dtype == torch.float32
    _ok(lib.ctc_amd_hvp(*inp.common(wrt), vec.data_ptr(), loss.data_ptr(), out["grad"].data_ptr() if want_grad else None,
                        out["hvp"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "hvp")
    torch.cuda.synchronize()
    return SimpleNamespace(out=out, ws=ws)


def hessian(inp, wrt=0, fill=0xA5, ws=None):
    from tf_seq2seq_losses_amd import _lib
    lib, ws, loss = _log_domain(inp, _lib.WS_HESSIAN, fill, ws)
    B, T, V, _ = inp.shape
    grad = filled((B, T, V), torch.float32, fill, _dev())
    hess = filled((B, T, V, T, V), torch.float32, fill, _dev())
    _ok(lib.ctc_amd_hessian(*inp.common(wrt), loss.data_ptr(), grad.data_ptr(), hess.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
        "hessian")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"loss": loss, "grad": grad, "hess": hess}, ws=ws)


def alpha_beta(inp, wrt=0, fill=0xA5, ws=None):
    from tf_seq2seq_losses_amd import _lib
    lib, ws, loss = _log_domain(inp, _lib.WS_ALPHA_BETA, fill, ws)
    B, T, _, U = inp.shape
    shape = (B, T + 1, U + 1, 2) if inp.kind == _lib.CLASSIC else (B, T + 1, U + 1)
    alpha, beta = (filled(shape, torch.float32, fill, _dev()) for _ in range(2))
    _ok(lib.ctc_amd_alpha_beta(*inp.common(wrt), loss.data_ptr(), alpha.data_ptr(), beta.data_ptr(), ws.data_ptr(), ws.numel(),
                               _stream()), "alpha_beta")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"loss": loss, "alpha": alpha, "beta": beta}, ws=ws)


def log_posterior(inp, wrt=0, fill=0xA5, ws=None):
    from tf_seq2seq_losses_amd import _lib
    lib, ws, loss = _log_domain(inp, _lib.WS_ALPHA_BETA, fill, ws)
    B, T, V, _ = inp.shape
    lg = filled((B, T, V), torch.float32, fill, _dev())
    _ok(lib.ctc_amd_log_posterior(*inp.common(wrt), loss.data_ptr(), lg.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "log_posterior")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"loss": loss, "lg": lg}, ws=ws)


def best_path(inp, wrt=0, fill=0xA5, ws=None):
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V, U = inp.shape
    if ws is None:
        ws = workspace(_lib.best_path_workspace_bytes(inp.kind, B, T, V, U), fill)
    score = filled((B,), torch.float32, fill, _dev())
    tokens, index = (filled((B, T), torch.int32, fill, _dev()) for _ in range(2))
    _ok(lib.ctc_amd_best_path(*inp.common_ex(wrt), score.data_ptr(), tokens.data_ptr(), index.data_ptr(), ws.data_ptr(), ws.numel(),
                              _stream()), "best_path")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"score": score, "tokens": tokens, "label_index": index}, ws=ws)


def greedy_decode(inp, wrt=0, fill=0xA5, ws=None):
    """(labels, ll and U of `inp` are not passed on: the call takes none)"""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = inp.x.shape
    if ws is None:
        ws = workspace(_lib.greedy_decode_workspace_bytes(B, T), fill)
    score = filled((B,), torch.float32, fill, _dev())
    length = filled((B,), torch.int32, fill, _dev())
    tokens, decoded, frames = (filled((B, T), torch.int32, fill, _dev()) for _ in range(3))
    label_score = filled((B, T), torch.float32, fill, _dev())
    x = inp.x
    _ok(lib.ctc_amd_greedy_decode(inp.kind, wrt, x.data_ptr(), _dt(x), x.stride(0), x.stride(1), inp.tl.data_ptr(), inp.blank, B, T, V,
                                  score.data_ptr(), tokens.data_ptr(), decoded.data_ptr(), length.data_ptr(), frames.data_ptr(),
                                  label_score.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "greedy_decode")
    torch.cuda.synchronize()
    return SimpleNamespace(out={"score": score, "tokens": tokens, "decoded": decoded, "decoded_length": length, "frames": frames,
                                "label_score": label_score}, ws=ws)


def flag_words(ws, offset, B):
    """int32[B] flag words a fused kernel left at `offset` of its workspace (a copy)."""
    return ws[offset:offset + 4 * B].view(torch.int32).clone()


def total_diff(clean, other, rows=None, perm=None):
    """{name: number of differing elements} between the outputs of two runs; `rows` restricts the comparison to those batch rows,
    `perm` compares other[i] with clean[perm[i]]."""
    assert clean.keys() == other.keys(), (clean.keys(), other.keys())
    res = {}
    for name in clean:
        a, b = clean[name], other[name]
        if name in ("sum2", "zero_next"):  # (per call, not per utterance)
            if rows is None and perm is None:
                res[name] = count_diff(a, b)
            continue
        if perm is not None:
            a = a[torch.as_tensor(perm, device=a.device)]
        if rows is not None:
            a, b = a[rows], b[rows]
        res[name] = count_diff(a.contiguous(), b.contiguous())
    return res


# ---- the cases (shared by the CPU test of these helpers and the GPU tests; read-only) ----

# name -> (B, T, V, U), logit_length, label_length, (row, length) of a run of repeats or None, labels drawn without replacement
# Lengths: 0, 1, T and the neighbours of a block boundary (12-frame blocks at one position per lane, 3-frame blocks at eight);
# one empty label and / or one infeasible row (more labels than frames) per batch as far as B allows.
CASES = {
    "lg_nl1": ((8, 50, 256, 12), [50, 0, 1, 11, 12, 13, 24, 25], [12, 0, 1, 12, 6, 0, 12, 4], (0, 6), False),
    "lg_nl2": ((4, 40, 301, 70), [40, 0, 13, 1], [18, 3, 0, 2], (0, 9), False),
    "lg_nl4": ((3, 64, 512, 130), [64, 37, 5], [30, 0, 9], (0, 10), False),
    "lg_seg4": ((2, 45, 1021, 20), [45, 21], [20, 0], (0, 6), False),
    "lg_nl8": ((2, 90, 128, 300), [90, 44], [40, 45], (0, 12), False),
    "lg_wide": ((2, 23, 2050, 9), [23, 10], [9, 0], (0, 4), False),
    "hvp_fused": ((4, 30, 256, 6), [30, 17, 1, 0], [6, 0, 3, 0], (0, 3), False),
    "hvp_fused_distinct": ((4, 30, 256, 6), [30, 17, 1, 0], [6, 0, 3, 0], None, True),
    "hvp_log": ((3, 21, 7, 5), [21, 9, 2], [5, 0, 4], None, True),
    "hvp_log_repeats": ((3, 21, 7, 5), [21, 9, 2], [5, 0, 4], (0, 3), False),
    "small": ((3, 12, 8, 5), [12, 7, 2], [5, 0, 4], (0, 3), False),
    "hess_long": ((2, 45, 4, 40), [45, 20], [36, 33], (0, 3), False),
    "hess_plan": ((40, 10, 6, 4), None, None, None, False),
    "align_a": ((4, 70, 29, 11), [70, 0, 1, 40], [11, 0, 3, 0], (0, 4), False),
    "align_b": ((3, 130, 256, 40), [130, 63, 5], [40, 0, 9], (0, 8), False),
    "greedy": ((4, 300, 37, 1), [300, 0, 257, 64], [0, 0, 0, 0], None, False),
}
KINDS = ("classic", "simplified")


@functools.lru_cache(maxsize=None)
def case(name):
    """Read-only NumPy inputs of one case: shape, logits (N(0, 1) in EVERY frame, padding included), labels in [1, V) in every
    position (tails included), ll, tl; blank = 0."""
    shape, tl, ll, repeat, distinct = CASES[name]
    B, T, V, U = shape
    rng = np.random.default_rng(sum(ord(ch) for ch in name) + 1000 * T + V)
    logits = rng.standard_normal((B, T, V)).astype(np.float32)
    if name == "greedy":
        logits[..., : V // 8] += 2.0  # a few favoured tokens: blanks and repeats do occur on the argmax path
    if distinct:
        labels = np.stack([rng.permutation(np.arange(1, V))[:U] for _ in range(B)]).astype(np.int32)
    elif V <= 4:  # few tokens: cycle through them, so that classic needs no more frames than labels (plus the run below)
        labels = (1 + (np.arange(U)[None, :] + np.arange(B)[:, None]) % (V - 1)).astype(np.int32)
    else:
        labels = rng.integers(1, V, (B, U)).astype(np.int32)
    if tl is None:  # (the plan case: ragged, every row feasible or not as it falls)
        tl = rng.integers(0, T + 1, B)
        ll = rng.integers(0, U + 1, B)
        tl[0], ll[0] = T, U
    if repeat is not None:
        labels[repeat[0], :repeat[1]] = labels[repeat[0], 0]
    tl, ll = np.asarray(tl, np.int32), np.asarray(ll, np.int32)
    assert tl.shape == ll.shape == (B,) and tl.min() >= 0 and tl.max() <= T and ll.min() >= 0 and ll.max() <= U
    for a in (logits, labels, ll, tl):
        a.flags.writeable = False
    return SimpleNamespace(name=name, shape=shape, logits=logits, labels=labels, ll=ll, tl=tl, blank=0)


def frames_needed(kind, label):
    label = [int(k) for k in label]
    return len(label) + (sum(a == b for a, b in zip(label, label[1:])) if kind == "classic" else 0)


def feasible_rows(c, kind):
    """[B] bool: the utterance has at least the frames its label needs."""
    return np.array([frames_needed(kind, c.labels[b, :c.ll[b]]) <= c.tl[b] for b in range(c.shape[0])])
