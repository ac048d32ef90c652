"""Time of the wildcard loss call (ctc_amd_wildcard_loss_grad) beside the caller-side route it replaces and beside the plain loss
on the same logits.

Warm launches timed with device events (one pair of events around each measured item, the items alternating in a fixed order), at
the north-star shape B=256 T=1000 U=128 V=256 unless told otherwise, wildcards at both ends of every label and one in the middle.
  new call           float32 and bfloat16 logits, both lattices, loss only (one launch) and loss + gradient (three launches)
  caller-side route  log_softmax + a zero column + the plain loss on the float32 [B, T, V + 1] log-probabilities with the wildcard
                     mapped to token V, its copies and (with a gradient) its backward through autograd inside the timed region:
                     classic and float32 only, because that is all the route can do
  plain loss         classic_ctc_loss / simplified_ctc_loss forward + backward on the same logits, the wildcards replaced by
                     ordinary labels: a yardstick of different mathematics (the linear-domain fused tier)
The whole measurement is repeated `--repeats` times in the same process; the spread between the repeats' medians is printed beside
the figures.  The script asserts nothing about time: numbers for profiles/wildcard_loss_time.md and DESIGN.md section 5.16.
Needs a GPU (there is no CPU path)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tf_seq2seq_losses_amd as ctc  # noqa: E402
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wildcard_loss_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    plain = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    wild = plain.clone()
    for b in range(B):
        L = int(ll[b])
        wild[b, 0] = wild[b, L - 1] = wild[b, L // 2] = _lib.WILDCARD
    mapped = torch.where(wild == _lib.WILDCARD, torch.full_like(wild, V), wild)
    plain, wild, mapped, ll = plain.to(dev), wild.to(dev), mapped.to(dev), ll.to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    loss_f, loss_g = torch.empty(B, device=dev), torch.empty(B, device=dev)
    zero_col = torch.zeros((B, T, 1), device=dev)
    keep = {}

    rows = {}  # (lattice, input, item) -> [median of every repeat], [minimum of every repeat]
    for kind_name, kind in ops.KINDS.items():
        plain_fn = ctc.classic_ctc_loss if kind_name == "classic" else ctc.simplified_ctc_loss
        for what, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
            dt = ops._DTYPES[x.dtype]
            n = _lib.wildcard_loss_workspace_bytes(kind, B, T, V, U)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            grad = torch.empty_like(x)
            xg = x.clone().requires_grad_(True)

            def new_call(with_grad):
                out = loss_g if with_grad else loss_f
                rc = lib.ctc_amd_wildcard_loss_grad(kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), wild.data_ptr(), U,
                                                    ll.data_ptr(), tl.data_ptr(), 0, 0.0, B, T, V, U, None, out.data_ptr(),
                                                    grad.data_ptr() if with_grad else None, dt, T * V, V,
                                                    ws.data_ptr() if with_grad else None, n if with_grad else 0, st)
                assert rc == 0, lib.ctc_amd_last_error()

            def route(with_grad):
                with torch.set_grad_enabled(with_grad):
                    e = torch.cat([torch.log_softmax(xg, 2), zero_col], -1)
                    loss = ctc.ctc_loss_from_logproba(mapped, e, ll, tl, 0, ctc.ClassicCtcLossData)
                    if with_grad:
                        xg.grad = None
                        loss.sum().backward()
                keep["route"] = loss.detach()

            def plain_call():
                xg.grad = None
                loss = plain_fn(plain, xg, ll, tl, 0)
                loss.sum().backward()
                keep["plain"] = loss.detach()

            items = [("new call, loss only", lambda: new_call(False)), ("new call, loss + gradient", lambda: new_call(True)),
                     ("plain loss, forward + backward", plain_call)]
            if kind_name == "classic" and dt == _lib.F32:
                items[2:2] = [("caller-side route, loss only", lambda: route(False)),
                              ("caller-side route, loss + gradient", lambda: route(True))]
            for _ in range(a.warmup):
                for _, fn in items:
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                t = {name: [] for name, _ in items}
                for _ in range(a.steps):
                    for name, fn in items:
                        t[name].append(timed(fn))
                for name, v in t.items():
                    med, mn = rows.setdefault((kind_name, what, name), ([], []))
                    med.append(float(np.median(v))); mn.append(float(np.min(v)))
            assert torch.isfinite(loss_f).all() and torch.equal(loss_f, loss_g) and torch.isfinite(keep["plain"]).all()
            if kind_name == "classic" and dt == _lib.F32:  # the two routes agree (no adjacent wildcards here)
                assert bool(((loss_g - keep["route"]).abs() <= 2e-4 + 2e-6 * loss_g.abs()).all())
            del ws, grad, xg

    lines = [f"# Wildcard loss beside the caller-side route and the plain loss: B={B} T={T} U={U} V={V}, full-length utterances, "
             f"label_length in [{U // 2}, {U}], wildcards at both ends and one in the middle", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every item, the items alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| lattice | logits | item | time | against the new call with a gradient |", "|---|---|---|---|---|"]
    for (kind_name, what, name), (med, mn) in rows.items():
        ref = float(np.median(rows[(kind_name, what, "new call, loss + gradient")][0]))
        m = float(np.median(med))
        lines.append(f"| {kind_name} | {what} | {name} | {m:.1f} ({min(med):.1f} .. {max(med):.1f}; {min(mn):.1f}) | {m / ref:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
