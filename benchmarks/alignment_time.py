"""Time of the best-path alignment call (ctc_amd_best_path) beside the stand-alone loss-only call on the same buffers.

Warm launches timed with device events (one pair of events around each launch, alternating the two calls), at the north-star
shape B=256 T=1000 U=128 V=256 unless told otherwise; float32 and bfloat16 logits, and log-probability input.  The read-once
yardstick is the time the logits alone take at the HBM peak: B * T * V * element bytes / 8 TB/s.  No gate: numbers for
profiles/alignment_time.md and DESIGN.md section 5.6.  Needs a GPU (there is no CPU path)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (datasheet)


def timed(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)  # microseconds
    return np.asarray(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "alignment_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    score = torch.empty(B, device=dev)
    loss = torch.empty(B, device=dev)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    index = torch.empty((B, T), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    lines = [f"# Alignment call beside the loss-only call: B={B} T={T} U={U} V={V}, full-length utterances, label_length in [{U // 2}, {U}]",
             "", f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm launches each after {a.warmup}, device events around every launch, "
             "the two calls alternating; microseconds, median (minimum)", "",
             "| lattice | input | alignment | loss only (grad = NULL) | ratio | read-once yardstick |", "|---|---|---|---|---|---|"]
    for kind_name, kind in ops.KINDS.items():
        for what, wrt, x in (("float32 logits", 0, x32), ("bfloat16 logits", 0, x32.to(torch.bfloat16)),
                             ("float32 log-probabilities", 1, torch.log_softmax(x32, 2))):
            dt = ops._DTYPES[x.dtype]
            ws_a = torch.empty(max(_lib.best_path_workspace_bytes(kind, B, T, V, U), 1), dtype=torch.uint8, device=dev)
            ws_l = torch.empty(max(_lib.workspace_bytes(_lib.WS_LOSS_GRAD, kind, B, T, V, U), 1), dtype=torch.uint8, device=dev)
            common_ex = (kind, wrt, x.data_ptr(), dt, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0, B, T, V, U)

            def align():
                rc = lib.ctc_amd_best_path(*common_ex, score.data_ptr(), tokens.data_ptr(), index.data_ptr(), ws_a.data_ptr(), ws_a.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            def loss_only():
                if dt == _lib.F32:
                    rc = lib.ctc_amd_loss_grad(kind, wrt, x.data_ptr(), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0, B, T, V, U,
                                               loss.data_ptr(), None, None, ws_l.data_ptr(), ws_l.numel(), st)
                else:  # (ctc_amd_loss_grad reads float32 only)
                    rc = lib.ctc_amd_loss_grad_ex(*common_ex, loss.data_ptr(), None, dt, x.stride(0), x.stride(1), None,
                                                  ws_l.data_ptr(), ws_l.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            for _ in range(a.warmup):
                align(); loss_only()
            torch.cuda.synchronize()
            ta, tlo = [], []
            for _ in range(a.steps):
                ta.append(timed(align, 1)[0]); tlo.append(timed(loss_only, 1)[0])
            ta, tlo = np.asarray(ta), np.asarray(tlo)
            assert torch.isfinite(score).all() and torch.isfinite(loss).all() and bool((score <= -loss + 1e-2).all())
            yard = B * T * V * x.element_size() / HBM_PEAK * 1e6
            pipe = _lib.pipeline_name(kind, wrt, B, T, V, U, False) if dt == _lib.F32 else "(producer format)"
            lines.append(f"| {kind_name} | {what} | {np.median(ta):.1f} ({ta.min():.1f}) | {np.median(tlo):.1f} ({tlo.min():.1f}) {pipe} | "
                         f"{np.median(ta) / np.median(tlo):.2f} | {yard:.1f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
