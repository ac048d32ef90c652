"""Time of the label-posterior call (ctc_amd_label_posterior) beside the wildcard loss + gradient (ctc_amd_wildcard_loss_grad) on
the same inputs, in the same process.

Warm launches timed with device events (one pair of events around each measured item, the items alternating in a fixed order), at
the north-star shape B=256 T=1000 U=128 V=256 unless told otherwise, wildcards at both ends of every label and one in the middle
(the inputs of benchmarks/wildcard_loss_time.py).  Both lattices, float32 and bfloat16 logits:
  label posteriors, with statistics      the alpha sweep, the beta sweep that writes [B, T, U], the duration / expected_frame launch
  label posteriors, without statistics   duration = expected_frame = NULL: the two sweeps alone
  wildcard loss + gradient               the same two sweeps, then the row stage that reads and writes [B, T, V]
The expectation this measures: the new call trades the row stage for a [B, T, U] write, so it should take no more device time than
the wildcard loss + gradient beyond that call's own run-to-run spread.  The whole measurement is repeated `--repeats` times; the
spread between the repeats' medians is printed beside the figures.  The script asserts nothing about time: numbers for
profiles/label_posterior_time.md and DESIGN.md section 5.17.  Needs a GPU (there is no CPU path)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

ITEMS = ("label posteriors, with statistics", "label posteriors, without statistics", "wildcard loss + gradient")


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
    assert torch.cuda.is_available(), "label_posterior_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    wild = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    for b in range(B):
        L = int(ll[b])
        wild[b, 0] = wild[b, L - 1] = wild[b, L // 2] = _lib.WILDCARD
    wild, ll = wild.to(dev), ll.to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    loss_p, loss_q, loss_g = (torch.empty(B, device=dev) for _ in range(3))
    post, post_q = torch.empty((B, T, U), device=dev), torch.empty((B, T, U), device=dev)
    blk, blk_q = torch.empty((B, T), device=dev), torch.empty((B, T), device=dev)
    dur, exf = torch.empty((B, U), device=dev), torch.empty((B, U), device=dev)

    rows = {}  # (lattice, input, item) -> [median of every repeat], [minimum of every repeat]
    for kind_name, kind in ops.KINDS.items():
        for what, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
            dt = ops._DTYPES[x.dtype]
            n = _lib.wildcard_loss_workspace_bytes(kind, B, T, V, U)
            assert _lib.label_posterior_workspace_bytes(kind, B, T, V, U) <= n
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            grad = torch.empty_like(x)
            common = (kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), wild.data_ptr(), U, ll.data_ptr(), tl.data_ptr(),
                      0, 0.0, B, T, V, U)

            def posterior(stats):
                out = (loss_p, post, blk, dur, exf) if stats else (loss_q, post_q, blk_q, None, None)
                rc = lib.ctc_amd_label_posterior(*common, *(None if o is None else o.data_ptr() for o in out), ws.data_ptr(), n, st)
                assert rc == 0, lib.ctc_amd_last_error()

            def loss_grad():
                rc = lib.ctc_amd_wildcard_loss_grad(*common, None, loss_g.data_ptr(), grad.data_ptr(), dt, T * V, V, ws.data_ptr(), n, st)
                assert rc == 0, lib.ctc_amd_last_error()

            items = list(zip(ITEMS, (lambda: posterior(True), lambda: posterior(False), loss_grad)))
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
            # the three calls agree: one loss, one matrix; a frame's posteriors sum to 1; the durations to the frames that are no blank
            assert torch.isfinite(loss_p).all() and torch.equal(loss_p, loss_g) and torch.equal(loss_p, loss_q)
            assert torch.equal(post, post_q) and torch.equal(blk, blk_q)
            assert float((post.sum(2) + blk - 1).abs().max()) <= 1e-4 and float(dur.min()) >= 0.0
            del ws, grad

    lines = [f"# Label posteriors beside the wildcard loss + gradient: B={B} T={T} U={U} V={V}, full-length utterances, label_length in "
             f"[{U // 2}, {U}], wildcards at both ends and one in the middle", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every item, the items alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| lattice | logits | item | time | against the wildcard loss + gradient |", "|---|---|---|---|---|"]
    for (kind_name, what, name), (med, mn) in rows.items():
        ref = float(np.median(rows[(kind_name, what, ITEMS[2])][0]))
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
