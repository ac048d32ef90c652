"""Time of the label posteriors from block checkpoints (ctc_amd_label_posterior_ckpt) beside the per-frame-row call
(ctc_amd_label_posterior) in the same process, in the manner of benchmarks/wildcard_loss_ckpt_time.py.

Warm launches timed with device events (one pair of events around each call, checkpoint=False and True alternating), at B=256
T=1000 U=128 V=256, wildcards at both ends of every label and one in the middle, both lattices, float32 and bfloat16 logits, with
and without duration / expected_frame; plus one line at B=1024 (classic, float32, with statistics).  The whole measurement is
repeated `--repeats` times; the spread between the repeats' medians is printed beside the figures.  The script asserts nothing
about time: numbers for profiles/label_posterior_ckpt_time.md and DESIGN.md section 5.33.  Needs a GPU (there is no CPU path)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "label_posterior_ckpt_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    T, U, V = a.T, a.U, a.V
    st = torch.cuda.current_stream().cuda_stream
    rows = {}  # (B, lattice, logits, statistics, checkpoint) -> ([median of every repeat], [minimum of every repeat], workspace bytes)
    for B, kinds, formats, stats in ((256, ("classic", "simplified"), (torch.float32, torch.bfloat16), (True, False)),
                                     (1024, ("classic",), (torch.float32,), (True,))):
        g = torch.Generator(device="cpu").manual_seed(0)
        x32 = torch.randn((B, T, V), generator=g).to(dev)
        wild = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
        ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
        for b in range(B):
            L = int(ll[b])
            wild[b, 0] = wild[b, L - 1] = wild[b, L // 2] = _lib.WILDCARD
        wild, ll = wild.to(dev), ll.to(dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        for kind_name in kinds:
            kind = ops.KINDS[kind_name]
            for fmt in formats:
                x = x32.to(fmt)
                calls = {}
                for ck in (False, True):
                    n = (_lib.label_posterior_ckpt_workspace_bytes if ck else _lib.label_posterior_workspace_bytes)(kind, B, T, V, U)
                    fn = lib.ctc_amd_label_posterior_ckpt if ck else lib.ctc_amd_label_posterior
                    calls[ck] = (fn, n, torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(B, device=dev),
                                 torch.empty((B, T, U), device=dev), torch.empty((B, T), device=dev), torch.empty((B, U), device=dev),
                                 torch.empty((B, U), device=dev))

                def call(ck, want):
                    fn, n, ws, loss, post, blk, dur, exf = calls[ck]
                    rc = fn(kind, _lib.WRT_LOGITS, x.data_ptr(), ops._DTYPES[fmt], x.stride(0), x.stride(1), wild.data_ptr(), U,
                            ll.data_ptr(), tl.data_ptr(), 0, 0.0, B, T, V, U, loss.data_ptr(), post.data_ptr(), blk.data_ptr(),
                            dur.data_ptr() if want else None, exf.data_ptr() if want else None, ws.data_ptr(), n, st)
                    assert rc == 0, lib.ctc_amd_last_error()

                for want in stats:
                    for _ in range(a.warmup):
                        call(False, want); call(True, want)
                    torch.cuda.synchronize()
                    for _ in range(a.repeats):
                        t = {False: [], True: []}
                        for _ in range(a.steps):
                            for ck in (False, True):
                                t[ck].append(timed(lambda: call(ck, want)))
                        for ck, v in t.items():
                            med, mn, _ = rows.setdefault((B, kind_name, str(fmt).split(".")[-1], want, ck), ([], [], calls[ck][1]))
                            med.append(float(np.median(v))); mn.append(float(np.min(v)))
                # the two calls agree: the same loss bits, every other output within the sum of both calls' bars
                assert torch.isfinite(calls[True][3]).all() and torch.equal(calls[False][3], calls[True][3])
                for i, bar in ((4, 2e-4), (5, 2e-4), (6, 2e-4 * T), (7, 2e-4 * T)):
                    err = float((calls[False][i] - calls[True][i]).abs().max())
                    assert err <= bar, (i, err)
                del calls

    lines = [f"# Label posteriors, checkpoint=False beside checkpoint=True: T={T} U={U} V={V}, full-length utterances, "
             f"label_length in [{U // 2}, {U}], wildcards at both ends and one in the middle", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every call, the two calls alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| B | lattice | logits | statistics | checkpoint | workspace MB | time | against checkpoint=False |", "|---|---|---|---|---|---|---|---|"]
    for (B, kind_name, what, want, ck), (med, mn, n) in rows.items():
        ref = float(np.median(rows[(B, kind_name, what, want, False)][0]))
        m = float(np.median(med))
        lines.append(f"| {B} | {kind_name} | {what} | {want} | {ck} | {n / 1e6:.1f} | {m:.1f} ({min(med):.1f} .. {max(med):.1f}; {min(mn):.1f}) | {m / ref:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
