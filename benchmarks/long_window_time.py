"""Time of the windowed long-form loss, gradient and label posteriors beside their unwindowed counterparts, in one process
(profiles/long_window_time.md), in the manner of benchmarks/window_time.py.

    python benchmarks/long_window_time.py [--runs 5] [--calls 2] [--unwindowed-only] [--root DIR]

Shape: B = 1, T = 30 000, U = 8 192, V = 32, both lattices.  Calls: the forward, the loss + gradient on the per-frame workspace
and from tile checkpoints, the label posteriors with dense=False, and (for expectation 2) the long-form alignment.  Windows: the
unconstrained long-form alignment -/+ 25 frames (ctc_frame_window).  Every figure is the median over `runs` of the mean time of
`calls` back-to-back calls between two device synchronisations, in microseconds; the spread is (max - min) / median over the runs
of the UNWINDOWED call.

Expectations, written before the first run:
  1. An unwindowed call costs what it costs on a build of the parent commit (the WIN = false instantiations are the parent's device
     code): run this with --unwindowed-only --root PARENT_TREE in alternating processes; "the same" is inside the parent's own
     run-to-run spread.
  2. A windowed call costs the unwindowed call of the same build plus what the long-form alignment pays for the same gate
     (profiles/window_time.md: 4-5 %): ratio <= the alignment's ratio measured here, give or take the spread."""
import argparse
import json
import statistics
import sys
import time

import torch

# --root DIR: import the package from DIR, the tree of another commit's build (with --unwindowed-only: the parent's)
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
import tf_seq2seq_losses_amd as ctc  # noqa: E402


def timed(fn, runs, calls):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    med = statistics.median(out)
    return med, (max(out) - min(out)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--unwindowed-only", action="store_true")
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, T, U, V = 1, 30000, 8192, 32
    x = torch.randn((B, T, V), generator=g).to(dev)
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    ll = torch.full((B,), U, dtype=torch.int32, device=dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for kind in ("classic", "simplified"):
        c = kind == "classic"
        loss_fn = ctc.classic_ctc_long_loss if c else ctc.simplified_ctc_long_loss
        post_fn = ctc.classic_ctc_long_label_posterior if c else ctc.simplified_ctc_long_label_posterior
        # (the function that takes frame_window; looked up only with windows, so that --root works on a tree without it)
        wpost_fn = None if a.unwindowed_only else (ctc.classic_ctc_long_windowed_label_posterior if c
                                                    else ctc.simplified_ctc_long_windowed_label_posterior)
        align_fn = ctc.classic_ctc_long_wildcard_alignment if c else ctc.simplified_ctc_long_wildcard_alignment

        def kw(w):
            return dict(max_label_length=U, **({} if w is None else {"frame_window": w}))

        def loss_grad(w, checkpoint):
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(loss_fn(labels, xg, ll, tl, 0, checkpoint=checkpoint, **kw(w)).sum(), xg)

        fns = [("loss", lambda w: loss_fn(labels, x, ll, tl, 0, **kw(w))),
               ("loss+grad", lambda w: loss_grad(w, False)),
               ("loss+grad checkpoint", lambda w: loss_grad(w, True)),
               ("label_posterior dense=False", lambda w: (post_fn if w is None else wpost_fn)(labels, x, ll, tl, 0, dense=False, **kw(w))),
               ("long alignment", lambda w: align_fn(labels, x, ll, tl, 0, **kw(w)))]
        window = None
        if not a.unwindowed_only:
            al = align_fn(labels, x, ll, tl, 0, max_label_length=U)
            window = ctc.ctc_frame_window(al.first_frame, al.last_frame, tl, before=25, after=25)
        for what, fn in fns:
            base, spread = timed(lambda: fn(None), a.runs, a.calls)
            row = dict(case="long B1 T30000 U8192 V32", lattice=kind, call=what, unwindowed_us=round(base, 1), spread=round(spread, 4))
            if window is not None:
                win, _ = timed(lambda: fn(window), a.runs, a.calls)
                row.update(windowed_us=round(win, 1), ratio=round(win / base, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps(dict(summary="long_window_time", rows=len(rows), unwindowed_only=bool(a.unwindowed_only))), flush=True)


if __name__ == "__main__":
    main()
