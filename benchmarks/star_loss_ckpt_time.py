"""Time of the star CTC loss + gradient from block checkpoints (ctc_amd_star_loss_grad_ckpt) beside the per-frame-row call with the
same keywords (ctc_amd_star_loss_grad / ctc_amd_optional_wildcard_loss_grad) in the same process.

Warm launches timed with device events (one pair of events around each call, the two calls alternating), at B=256 T=1000 V=256 with
a star temporal classification transcript: 64 labels with a star before, between and after them (129 positions, four per lane,
blocks of 8 frames).  Both lattices, float32 and bfloat16 logits, with optional_wildcards and exclude_next_label both set; the lines
with one of the two alone (float32; the stars are mandatory without optional_wildcards); and one line at B=1024 (classic, float32).
The whole measurement is repeated `--repeats` times; the spread between the repeats' medians is printed beside the figures.  The
script asserts nothing about time: numbers for profiles/star_loss_ckpt_time.md and DESIGN.md section 5.34.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402
from benchmarks.wildcard_loss_ckpt_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=64)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "star_loss_ckpt_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    T, V, U = a.T, a.V, 2 * a.labels + 1
    st = torch.cuda.current_stream().cuda_stream
    both, f32, bf16 = (True, True), torch.float32, torch.bfloat16
    plan = [(256, k, f, both) for k in ("classic", "simplified") for f in (f32, bf16)]
    plan += [(256, k, f32, fl) for fl in ((True, False), (False, True)) for k in ("classic", "simplified")] + [(1024, "classic", f32, both)]
    rows = {}  # (B, lattice, logits, flags, checkpoint) -> ([median of every repeat], [minimum of every repeat], workspace bytes)
    for B, kind_name, fmt, flags in plan:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn((B, T, V), generator=g).to(dev).to(fmt)
        labels = torch.full((B, U), _lib.OPTIONAL_WILDCARD if flags[0] else _lib.WILDCARD, dtype=torch.int32)
        labels[:, 1::2] = torch.randint(1, V, (B, a.labels), generator=g, dtype=torch.int32)
        labels = labels.to(dev)
        ll = torch.full((B,), U, dtype=torch.int32, device=dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        kind, dt = ops.KINDS[kind_name], ops._DTYPES[fmt]
        calls = {}
        for ck in (False, True):
            n = (_lib.star_loss_ckpt_workspace_bytes if ck else _lib.wildcard_loss_workspace_bytes)(kind, B, T, V, U)
            calls[ck] = (n, torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(B, device=dev), torch.empty_like(x))

        def call(ck):
            n, ws, loss, grad = calls[ck]
            head = (kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
            tail = (0.0, B, T, V, U, None, loss.data_ptr(), grad.data_ptr(), dt, T * V, V, ws.data_ptr(), n, st)
            if ck:
                rc = lib.ctc_amd_star_loss_grad_ckpt(*head, int(flags[0]), int(flags[1]), *tail)
            elif flags[1]:
                rc = lib.ctc_amd_star_loss_grad(*head, int(flags[0]), *tail)
            else:
                rc = lib.ctc_amd_optional_wildcard_loss_grad(*head, *tail)
            assert rc == 0, lib.ctc_amd_last_error()

        for _ in range(a.warmup):
            call(False); call(True)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            t = {False: [], True: []}
            for _ in range(a.steps):
                for ck in (False, True):
                    t[ck].append(timed(lambda: call(ck)))
            for ck, v in t.items():
                med, mn, _ = rows.setdefault((B, kind_name, str(fmt).split(".")[-1], flags, ck), ([], [], calls[ck][0]))
                med.append(float(np.median(v))); mn.append(float(np.min(v)))
        # the two calls agree: the same loss bits, gradients within the sum of both calls' bars
        assert torch.isfinite(calls[True][2]).all() and torch.equal(calls[False][2], calls[True][2])
        err = float((calls[False][3].float() - calls[True][3].float()).abs().max())
        assert err <= (2e-4 if fmt == torch.float32 else 2e-4 + 2.0 ** -7), err
        del calls

    lines = [f"# Star CTC loss + gradient, the per-frame call beside ctc_amd_star_loss_grad_ckpt: T={T} V={V}, full-length utterances, "
             f"{a.labels} labels with a star before, between and after them (U={U})", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every call, the two calls alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| B | lattice | logits | optional, exclude | checkpoints | workspace MB | time | against the per-frame call |",
             "|---|---|---|---|---|---|---|---|"]
    for (B, kind_name, what, flags, ck), (med, mn, n) in rows.items():
        ref = float(np.median(rows[(B, kind_name, what, flags, False)][0]))
        m = float(np.median(med))
        lines.append(f"| {B} | {kind_name} | {what} | {flags[0]}, {flags[1]} | {ck} | {n / 1e6:.1f} | {m:.1f} ({min(med):.1f} .. {max(med):.1f}; "
                     f"{min(mn):.1f}) | {m / ref:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
