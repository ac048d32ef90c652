"""Time of the windowed calls beside their unwindowed counterparts, in one process (profiles/window_time.md).

    python benchmarks/window_time.py [--runs 10] [--calls 20] [--skip-long] [--unwindowed-only] [--root DIR]

Shapes: B = 256, T = 1000, U = 128, V = 256 (loss, loss + gradient, label posteriors, alignment) and the long-form alignment at
B = 1, T = 30 000, U = 8 192, V = 32.  Windows: the unconstrained best path -/+ 25 frames (ctc_frame_window).  Every figure is
the median over `runs` of the mean time of `calls` back-to-back calls between two device synchronisations, in microseconds; the
spread is (max - min) / median over the runs of the UNWINDOWED call, which is what "the same" is measured against.

Expectation, written before the first run: a windowed call costs what the unwindowed one does (the gate is two compares per
position and frame in producer wavefronts that already run a block ahead of the chain), i.e. the ratio lies within the spread.
--unwindowed-only prints the unwindowed figures alone: run it in a build of the parent commit as well to compare the two builds."""
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
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--unwindowed-only", action="store_true")
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []

    def case(name, kind, fns, make_window):
        window = None if a.unwindowed_only else make_window()
        for what, fn in fns:
            base, spread = timed(lambda: fn(None), a.runs, a.calls)
            row = dict(case=name, lattice=kind, call=what, unwindowed_us=round(base, 1), spread=round(spread, 4))
            if window is not None:
                win, _ = timed(lambda: fn(window), a.runs, a.calls)
                row.update(windowed_us=round(win, 1), ratio=round(win / base, 4), within_spread=bool(abs(win / base - 1.0) <= spread))
            rows.append(row)
            print(json.dumps(row), flush=True)

    B, T, U, V = 256, 1000, 128, 256
    x = torch.randn((B, T, V), generator=g).to(dev)
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
    ll = torch.full((B,), U, dtype=torch.int32, device=dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    for kind in ("classic", "simplified"):
        c = kind == "classic"
        loss_fn = ctc.classic_ctc_wildcard_loss if c else ctc.simplified_ctc_wildcard_loss
        post_fn = ctc.classic_ctc_label_posterior if c else ctc.simplified_ctc_label_posterior
        align_fn = ctc.classic_ctc_wildcard_alignment if c else ctc.simplified_ctc_wildcard_alignment

        def kw(w):
            return dict(max_label_length=U, **({} if w is None else {"frame_window": w}))

        def loss_grad(w):
            xg = x.detach().requires_grad_(True)
            torch.autograd.grad(loss_fn(labels, xg, ll, tl, 0, **kw(w)).sum(), xg)

        def window():
            al = align_fn(labels, x, ll, tl, 0, max_label_length=U)
            return ctc.ctc_frame_window(al.first_frame, al.last_frame, tl, before=25, after=25)

        case("B256 T1000 U128 V256", kind, [("loss", lambda w: loss_fn(labels, x, ll, tl, 0, **kw(w))), ("loss+grad", loss_grad),
                                            ("label_posterior", lambda w: post_fn(labels, x, ll, tl, 0, **kw(w))),
                                            ("alignment", lambda w: align_fn(labels, x, ll, tl, 0, **kw(w)))], window)
    if not a.skip_long:
        B, T, U, V = 1, 30000, 8192, 32
        x = torch.randn((B, T, V), generator=g).to(dev)
        labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
        ll = torch.full((B,), U, dtype=torch.int32, device=dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        for kind in ("classic", "simplified"):
            long_fn = ctc.classic_ctc_long_wildcard_alignment if kind == "classic" else ctc.simplified_ctc_long_wildcard_alignment

            def window():
                al = long_fn(labels, x, ll, tl, 0, max_label_length=U)
                return ctc.ctc_frame_window(al.first_frame, al.last_frame, tl, before=25, after=25)

            def call(w):
                return long_fn(labels, x, ll, tl, 0, max_label_length=U, **({} if w is None else {"frame_window": w}))

            old_runs, old_calls = a.runs, a.calls
            a.runs, a.calls = min(a.runs, 5), 2  # (tens of milliseconds per call)
            case("long B1 T30000 U8192 V32", kind, [("long alignment", call)], window)
            a.runs, a.calls = old_runs, old_calls
    print(json.dumps(dict(summary="window_time", rows=len(rows),
                          all_within_spread=all(r.get("within_spread", True) for r in rows))), flush=True)


if __name__ == "__main__":
    main()
