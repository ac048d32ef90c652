"""Time of the long-form CTC gradient from tile checkpoints (ctc_amd_long_wildcard_loss_grad_ckpt) beside the existing call
(ctc_amd_long_wildcard_loss_grad) in the same process, in the manner of benchmarks/long_loss_time.py, whose inputs these are.

Warm calls timed with device events (one pair of events around each call), float32 logits, full-length utterances, default
frames_per_tile.  Labels: random tokens with a wildcard at both ends and one in the middle of every label block.  Every row is one
(lattice, B, T, U) and shows the forward-only call, the existing call with a gradient and the checkpointed call with a gradient, the
calls alternating; median and (minimum - maximum) of the repeats; the workspace bytes of both; and whether loss and gradient of the
two are the same bits.  --demo B,T,U runs the checkpointed call alone on the classic lattice at a shape whose existing workspace need
not fit the card (an hour of audio: 1,180000,50000).  No gate: numbers for profiles/long_loss_checkpoint_time.md and DESIGN.md section
5.21.  Needs a GPU.

    python benchmarks/long_loss_checkpoint_time.py --demo 1,180000,50000 --out profiles/long_loss_checkpoint_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

EXPECTATION = """Expectation, written before the numbers (nothing had been measured): the checkpointed call costs the existing call plus
about one forward sweep -- roughly 163 + 53 ms (classic) and 95 + 29 ms (simplified) at B = 1, T = 30 000, U = 8 192, the figures of
profiles/long_loss_time.md, which the existing call should reproduce here within its spread.  It may cost less: the saved rows shrink
from 3.9 GB of HBM traffic to a 134 MB ring that may stay in cache.  That last point is a supposition."""


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def inputs(B, T, U, V, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((B, T, V), generator=g).to(dev)
    lab = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    wild = sorted({0, U - 1} | {k * 1024 + 512 for k in range(-(-U // 1024)) if k * 1024 + 512 < U})
    lab[:, wild] = _lib.WILDCARD
    return x, lab.to(dev), torch.full((B,), U, dtype=torch.int32, device=dev), torch.full((B,), T, dtype=torch.int32, device=dev)


def caller(lib, entry, head, B, T, V, U, tf, out, gr, ws, st):
    def fn():
        rc = entry(*head, 0.0, B, T, V, U, tf, None, out.data_ptr(), gr.data_ptr() if gr is not None else None, _lib.F32, T * V, V,
                   ws.data_ptr(), ws.numel(), st)
        assert rc == 0, lib.ctc_amd_last_error()
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="B,T,U; may be given several times")
    ap.add_argument("--demo", action="append", default=[], help="B,T,U for the checkpointed call alone, classic lattice")
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_loss_checkpoint_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192), (8, 30000, 8192), (1, 8192, 1024)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, tf = a.V, 0
    TF = _lib.LONG_FRAMES_DEFAULT
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Long-form CTC gradient from tile checkpoints: V={V}, float32 logits, frames_per_tile={TF}, full-length utterances", "",
             EXPECTATION, "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call, the "
             "calls alternating; microseconds, median (minimum - maximum)", "",
             "| lattice | B | T | U | K x J | existing workspace, bytes | checkpointed workspace, bytes | workspace ratio | forward | "
             "existing, with gradient | checkpointed, with gradient | checkpointed / existing | checkpointed - existing | "
             "(checkpointed - existing) / forward | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in shapes:
        x, labels, ll, tl = inputs(B, T, U, V, dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        for kind_name, kind in ops.KINDS.items():
            loss, loss_g, loss_c = (torch.empty(B, device=dev) for _ in range(3))
            grad, grad_c = torch.empty((B, T, V), device=dev), torch.empty((B, T, V), device=dev)
            n = _lib.long_wildcard_loss_workspace_bytes(kind, B, T, V, U, tf, True)
            nc = _lib.long_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, tf, True)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            wsc = torch.empty(nc, dtype=torch.uint8, device=dev)
            head = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
            calls = {"fwd": caller(lib, lib.ctc_amd_long_wildcard_loss_grad, head, B, T, V, U, tf, loss, None, ws, st),
                     "grad": caller(lib, lib.ctc_amd_long_wildcard_loss_grad, head, B, T, V, U, tf, loss_g, grad, ws, st),
                     "ckpt": caller(lib, lib.ctc_amd_long_wildcard_loss_grad_ckpt, head, B, T, V, U, tf, loss_c, grad_c, wsc, st)}
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in calls}
            for _ in range(a.steps):
                for name, fn in calls.items():
                    times[name].append(timed(fn))
            torch.cuda.synchronize()
            assert torch.isfinite(loss).all() and torch.equal(loss, loss_g) and torch.isfinite(grad).all()
            bits = bool(torch.equal(loss_g.view(torch.int32), loss_c.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad_c.view(torch.int32)))
            t = {name: np.asarray(v) for name, v in times.items()}
            med = {name: float(np.median(v)) for name, v in t.items()}
            cell = {name: f"{med[name]:.0f} ({t[name].min():.0f} - {t[name].max():.0f})" for name in t}
            lines.append(f"| {kind_name} | {B} | {T} | {U} | {K} x {J} | {n} | {nc} | {n / nc:.1f} | {cell['fwd']} | {cell['grad']} | {cell['ckpt']} | "
                         f"{med['ckpt'] / med['grad']:.3f} | {med['ckpt'] - med['grad']:.0f} | {(med['ckpt'] - med['grad']) / med['fwd']:.2f} | "
                         f"{'yes' if bits else 'NO'} |")
            print(lines[-1], flush=True)
            del ws, wsc, grad, grad_c
        del x
    if a.demo:
        lines += ["", "## The checkpointed call alone, classic lattice, at shapes whose existing workspace need not fit the card", "",
                  "| B | T | U | K x J | existing workspace, bytes (not allocated) | checkpointed workspace, bytes | forward | "
                  "checkpointed, with gradient | loss | gradient finite, rows sum to 0 within |", "|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in (tuple(int(v) for v in s.split(",")) for s in a.demo):
        x, labels, ll, tl = inputs(B, T, U, V, dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        kind = ops.KINDS["classic"]
        loss, loss_c = torch.empty(B, device=dev), torch.empty(B, device=dev)
        grad_c = torch.empty((B, T, V), device=dev)
        n = _lib.long_wildcard_loss_workspace_bytes(kind, B, T, V, U, tf, True)
        nc = _lib.long_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, tf, True)
        wsc = torch.empty(nc, dtype=torch.uint8, device=dev)
        head = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
        calls = {"fwd": caller(lib, lib.ctc_amd_long_wildcard_loss_grad_ckpt, head, B, T, V, U, tf, loss, None, wsc, st),
                 "ckpt": caller(lib, lib.ctc_amd_long_wildcard_loss_grad_ckpt, head, B, T, V, U, tf, loss_c, grad_c, wsc, st)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(a.steps):
            for name, fn in calls.items():
                times[name].append(timed(fn))
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all() and torch.equal(loss, loss_c) and torch.isfinite(grad_c).all()
        rows = float(grad_c.sum(-1).abs().max())  # (with respect to logits every gradient row sums to 0)
        t = {name: np.asarray(v) for name, v in times.items()}
        cell = {name: f"{float(np.median(t[name])):.0f} ({t[name].min():.0f} - {t[name].max():.0f})" for name in t}
        lines.append(f"| {B} | {T} | {U} | {K} x {J} | {n} | {nc} | {cell['fwd']} | {cell['ckpt']} | {float(loss_c[0]):.1f} | {rows:.2e} |")
        print(lines[-1], flush=True)
        del x, wsc, grad_c
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
