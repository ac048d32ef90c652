"""Time of the star label posteriors from block checkpoints (ctc_amd_star_label_posterior_ckpt) beside the per-frame-row call with
the same keywords (ctc_amd_star_label_posterior / ctc_amd_optional_wildcard_label_posterior) in the same process.

Warm launches timed with device events (one pair of events around each call, the two calls alternating), at B=256 T=1000 V=256 with
a star temporal classification transcript: 64 labels with a star before, between and after them (129 positions, four per lane,
blocks of 8 frames).  Classic float32 with all three flag pairs (the stars are mandatory without optional_wildcards); with both
keywords also bfloat16, the simplified lattice, and B=1024 (classic, float32); every line with and without duration /
expected_frame.  The whole measurement is repeated `--repeats` times; the spread between the repeats' medians is printed beside the
figures, and the last column says whether the checkpointed call is faster than the per-frame one by more than that spread.  The
script asserts nothing about time: numbers for profiles/star_label_posterior_ckpt_time.md and DESIGN.md section 5.35.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402
from benchmarks.label_posterior_ckpt_time import timed  # noqa: E402


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
    assert torch.cuda.is_available(), "star_label_posterior_ckpt_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    T, V, U = a.T, a.V, 2 * a.labels + 1
    st = torch.cuda.current_stream().cuda_stream
    both, f32, bf16 = (True, True), torch.float32, torch.bfloat16
    plan = [(256, "classic", f32, fl) for fl in (both, (True, False), (False, True))]
    plan += [(256, "classic", bf16, both), (256, "simplified", f32, both), (256, "simplified", bf16, both), (1024, "classic", f32, both)]
    rows = {}  # (B, lattice, logits, flags, statistics, checkpoint) -> ([median of every repeat], [minimum of every repeat], workspace bytes)
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
            n = (_lib.label_posterior_ckpt_workspace_bytes if ck else _lib.label_posterior_workspace_bytes)(kind, B, T, V, U)
            calls[ck] = (n, torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(B, device=dev), torch.empty((B, T, U), device=dev),
                         torch.empty((B, T), device=dev), torch.empty((B, U), device=dev), torch.empty((B, U), device=dev))

        def call(ck, want):
            n, ws, loss, post, blk, dur, exf = calls[ck]
            head = (kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)
            tail = (0.0, B, T, V, U, loss.data_ptr(), post.data_ptr(), blk.data_ptr(), dur.data_ptr() if want else None,
                    exf.data_ptr() if want else None, ws.data_ptr(), n, st)
            if ck:
                rc = lib.ctc_amd_star_label_posterior_ckpt(*head, int(flags[0]), int(flags[1]), *tail)
            elif flags[1]:
                rc = lib.ctc_amd_star_label_posterior(*head, int(flags[0]), *tail)
            else:
                rc = lib.ctc_amd_optional_wildcard_label_posterior(*head, *tail)
            assert rc == 0, lib.ctc_amd_last_error()

        for want in (True, False):
            for _ in range(a.warmup):
                call(False, want); call(True, want)
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                t = {False: [], True: []}
                for _ in range(a.steps):
                    for ck in (False, True):
                        t[ck].append(timed(lambda: call(ck, want)))
                for ck, v in t.items():
                    med, mn, _ = rows.setdefault((B, kind_name, str(fmt).split(".")[-1], flags, want, ck), ([], [], calls[ck][0]))
                    med.append(float(np.median(v))); mn.append(float(np.min(v)))
        # the two calls agree: the same loss bits, every other output within the sum of both calls' bars
        assert torch.isfinite(calls[True][2]).all() and torch.equal(calls[False][2], calls[True][2])
        for i, bar in ((3, 2e-4), (4, 2e-4), (5, 2e-4 * T), (6, 2e-4 * T)):
            err = float((calls[False][i] - calls[True][i]).abs().max())
            assert err <= bar, (i, err)
        del calls

    lines = [f"# Star label posteriors, the per-frame call beside ctc_amd_star_label_posterior_ckpt: T={T} V={V}, full-length utterances, "
             f"{a.labels} labels with a star before, between and after them (U={U})", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every call, the two calls alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum).  Expectation: faster than the per-frame call by more than the larger of the two calls' spreads "
             "between repeats", "",
             "| B | lattice | logits | optional, exclude | statistics | checkpoints | workspace MB | time | against the per-frame call | expectation |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for (B, kind_name, what, flags, want, ck), (med, mn, n) in rows.items():
        rmed = rows[(B, kind_name, what, flags, want, False)][0]
        ref, m = float(np.median(rmed)), float(np.median(med))
        spread = max(max(med) - min(med), max(rmed) - min(rmed))
        verdict = "" if not ck else f"held (spread {spread:.1f})" if ref - m > spread else f"**failed** (spread {spread:.1f})"
        lines.append(f"| {B} | {kind_name} | {what} | {flags[0]}, {flags[1]} | {want} | {ck} | {n / 1e6:.1f} | {m:.1f} ({min(med):.1f} .. "
                     f"{max(med):.1f}; {min(mn):.1f}) | {m / ref:.2f} | {verdict} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
