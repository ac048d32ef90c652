"""Time of the long-form label posteriors (ctc_amd_long_label_posterior), with and without the dense [B, T, U] matrix, beside the
checkpointed gradient (ctc_amd_long_wildcard_loss_grad_ckpt) in the same process on the same inputs, in the manner of
benchmarks/long_loss_checkpoint_time.py, whose inputs these are.

Warm calls timed with device events (one pair around each call), float32 logits, full-length utterances, default frames_per_tile,
the calls alternating; median and (minimum - maximum) of the repeats.  The box's copy rate is taken in the same process: a device
copy of a float32 tensor of the dense matrix's size, whose time is what writing B * T * U * 4 bytes at that rate costs.  Every row
says whether the expectation below held, and whether dense=False gave the bits of the dense call in every other output.
--demo B,T,U runs the call without the dense matrix on the classic lattice at a shape where it would not fit (an hour of audio:
1,180000,50000).  No gate: numbers for profiles/long_label_posterior_time.md and DESIGN.md section 5.22.  Needs a GPU.

    python benchmarks/long_label_posterior_time.py --demo 1,180000,50000 --out profiles/long_label_posterior_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchmarks.long_loss_checkpoint_time import inputs, timed  # noqa: E402
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

EXPECTATION = """Expectation, written before the numbers (nobody had measured any of this): the call runs the checkpointed gradient's
schedule with a posterior stage in the row stage's place, a dense write replacing the row stage's logits read and gradient write.  So
with the dense matrix it costs no more than ctc_amd_long_wildcard_loss_grad_ckpt on the same inputs plus the time to write
B * T * U * 4 bytes at the box's copy rate, beyond that call's own run-to-run spread (maximum - minimum); without the dense matrix no
more than that call beyond its spread.  The per-position walk (one lane per position, TF serial float64 adds per stage behind eight
loads in flight) shares the launch with the row wavefronts and is supposed to hide behind them; at B = 1 there are only 128 such
wavefronts, so that is the part that may not hold."""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="B,T,U; may be given several times")
    ap.add_argument("--demo", action="append", default=[], help="B,T,U for the call without the dense matrix, classic lattice")
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_label_posterior_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192), (8, 30000, 8192)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, tf = a.V, 0
    TF = _lib.LONG_FRAMES_DEFAULT
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Long-form label posteriors: V={V}, float32 logits, frames_per_tile={TF}, full-length utterances", "", EXPECTATION, "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call, the "
             "calls alternating; microseconds, median (minimum - maximum)", "",
             "| lattice | B | T | U | K x J | workspace, bytes | dense matrix, bytes | copy of that size (rate) | checkpointed gradient | "
             "posteriors, dense | posteriors, dense=False | dense - gradient | allowed (copy + spread) | dense=False - gradient | "
             "allowed (spread) | expectation held: dense / dense=False | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def post_caller(head, B, T, U, outs, dense, ws):
        p = [o.data_ptr() for o in outs]
        def fn():
            rc = lib.ctc_amd_long_label_posterior(*head, 0.0, B, T, V, U, tf, p[0], p[1] if dense else None, *p[2:], ws.data_ptr(), ws.numel(), st)
            assert rc == 0, lib.ctc_amd_last_error()
        return fn

    def new_outs(B, T, U, dense):
        return [torch.empty(B, device=dev), torch.empty((B, T, U) if dense else (1,), device=dev), torch.empty((B, T), device=dev),
                torch.empty((B, U), device=dev), torch.empty((B, U), device=dev), torch.empty((B, U), device=dev),
                torch.empty((B, U), dtype=torch.int32, device=dev)]

    for B, T, U in shapes:
        x, labels, ll, tl = inputs(B, T, U, V, dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        src = torch.zeros((B, T, U), device=dev)
        for kind_name, kind in ops.KINDS.items():
            loss_c, grad_c = torch.empty(B, device=dev), torch.empty((B, T, V), device=dev)
            nc = _lib.long_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, tf, True)
            n = _lib.long_label_posterior_workspace_bytes(kind, B, T, V, U, tf)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            head = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
            od, ol = new_outs(B, T, U, True), new_outs(B, T, U, False)

            def grad_call():
                rc = lib.ctc_amd_long_wildcard_loss_grad_ckpt(*head, 0.0, B, T, V, U, tf, None, loss_c.data_ptr(), grad_c.data_ptr(), _lib.F32,
                                                              T * V, V, ws.data_ptr(), nc, st)
                assert rc == 0, lib.ctc_amd_last_error()
            calls = {"grad": grad_call, "dense": post_caller(head, B, T, U, od, True, ws), "lean": post_caller(head, B, T, U, ol, False, ws),
                     "copy": lambda: od[1].copy_(src)}
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in calls}
            for _ in range(a.steps):
                for name in ("grad", "dense", "lean"):
                    times[name].append(timed(calls[name]))
            torch.cuda.synchronize()
            bits = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for i, (p, q) in enumerate(zip(od, ol)) if i != 1)
            bits = bits and torch.equal(od[0].view(torch.int32), loss_c.view(torch.int32)) and bool(torch.isfinite(od[0]).all())
            rows = float((od[1].sum(-1) + od[2] - 1).abs().max())
            for _ in range(a.steps):  # (last: it overwrites the dense matrix)
                times["copy"].append(timed(calls["copy"]))
            t = {name: np.asarray(v) for name, v in times.items()}
            med = {name: float(np.median(v)) for name, v in t.items()}
            cell = {name: f"{med[name]:.0f} ({t[name].min():.0f} - {t[name].max():.0f})" for name in t}
            spread = float(t["grad"].max() - t["grad"].min())
            nbytes = B * T * U * 4
            held = (med["dense"] - med["grad"] <= med["copy"] + spread, med["lean"] - med["grad"] <= spread)
            lines.append(f"| {kind_name} | {B} | {T} | {U} | {K} x {J} | {n} | {nbytes} | {cell['copy']} ({nbytes / med['copy'] / 1e6:.2f} TB/s) | "
                         f"{cell['grad']} | {cell['dense']} | {cell['lean']} | {med['dense'] - med['grad']:.0f} | {med['copy'] + spread:.0f} | "
                         f"{med['lean'] - med['grad']:.0f} | {spread:.0f} | {'yes' if held[0] else 'NO'} / {'yes' if held[1] else 'NO'} | "
                         f"{'yes' if bits else 'NO'} (rows sum to 1 within {rows:.1e}) |")
            print(lines[-1], flush=True)
            del ws, grad_c, od, ol
        del x, src
    if a.demo:
        lines += ["", "## Without the dense matrix, classic lattice, at shapes where it would not fit", "",
                  "| B | T | U | K x J | dense matrix, bytes (not allocated) | workspace, bytes | posteriors, dense=False | loss | "
                  "smallest / mean / largest duration | smallest / median peak_posterior |", "|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in (tuple(int(v) for v in s.split(",")) for s in a.demo):
        x, labels, ll, tl = inputs(B, T, U, V, dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        kind = ops.KINDS["classic"]
        n = _lib.long_label_posterior_workspace_bytes(kind, B, T, V, U, tf)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        head = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
        ol = new_outs(B, T, U, False)
        fn = post_caller(head, B, T, U, ol, False, ws)
        fn()
        torch.cuda.synchronize()
        t = np.asarray([timed(fn) for _ in range(a.steps)])
        torch.cuda.synchronize()
        assert torch.isfinite(ol[0]).all() and bool((ol[6] >= 0).all())
        lines.append(f"| {B} | {T} | {U} | {K} x {J} | {B * T * U * 4} | {n} | {float(np.median(t)):.0f} ({t.min():.0f} - {t.max():.0f}) | "
                     f"{float(ol[0][0]):.1f} | {float(ol[3].min()):.3f} / {float(ol[3].mean()):.3f} / {float(ol[3].max()):.3f} | "
                     f"{float(ol[5].min()):.3f} / {float(ol[5].median()):.3f} |")
        print(lines[-1], flush=True)
        del x, ws
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
