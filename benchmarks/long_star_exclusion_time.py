"""Time of the long-form loss, gradient and label posteriors with exclude_next_label=True beside the same calls without it on the
same transcript, in one process (profiles/long_star_exclusion_time.md), in the manner of benchmarks/long_optional_wildcard_time.py.

    python benchmarks/long_star_exclusion_time.py [--runs 5] [--calls 2] [--existing-only] [--root DIR]

Shape: B = 1, T = 30 000, U = 8 192, V = 32, float32, both lattices.  Calls: the forward, the loss + gradient on the per-frame
workspace and from tile checkpoints, and the label posteriors with dense=False.  Transcripts: `few` -- three mandatory stars (1023,
whose label is the next block's first, 3000 and 5000) -- and `stc` -- an optional star before, between and after 4 095 labels, 8 191
positions (optional_wildcards=True on and off).  Every figure is the median over `runs` of the mean time of `calls` back-to-back
calls between two device synchronisations, in microseconds, with the minimum and the maximum over the runs.

Expectations, written before the first run:
  1. An existing long-form call costs what it costs on a build of the parent commit (the XN = false instantiations are the parent's
     device code): run this with --existing-only --root PARENT_TREE in alternating processes; "the same" is a ratio inside the
     parent's own spread between its processes.
  2. The chain step is unchanged but for one add per wildcard position, so the cost is the producers' (one gather, one log2 and one
     exp2 per wildcard position and frame), the (max, sum of the rest) row pass in label block 0, the scan of the transcript at the
     head of every tile, and in the row stage a second set of bins at half the columns per pass (V = 32: still one pass).  The
     short form paid 1.2 - 1.3 x on the loss, 1.3 - 1.4 x on loss + gradient and 1.05 - 1.11 x on the posteriors at U = 128, where
     the producers are the critical path (profiles/star_exclusion_time.md); here the chain wavefront at 16 positions per lane is
     (profiles/long_optional_wildcard_time.md), so `few` is expected at 1.00 - 1.10 x on every row and `stc` below the short form's
     ratios: at most 1.3 x on the loss, 1.4 x on loss + gradient, 1.11 x on the posteriors.  Recorded, not gated."""
import argparse
import json
import statistics
import sys
import time

import torch

# --root DIR: import the package from DIR, the tree of another commit's build (with --existing-only: the parent's)
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
import tf_seq2seq_losses_amd as ctc  # noqa: E402

WILDCARD, OPTIONAL = -2, -3
BOUNDS = {"few": {"loss": 1.10, "loss+grad": 1.10, "loss+grad checkpoint": 1.10, "label_posterior dense=False": 1.10},
          "stc": {"loss": 1.30, "loss+grad": 1.40, "loss+grad checkpoint": 1.40, "label_posterior dense=False": 1.11}}


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
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, T, U, V = 1, 30000, 8192, 32
    x = torch.randn((B, T, V), generator=g).to(dev)
    base = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    few = base.clone()
    few[0, [1023, 3000, 5000]] = WILDCARD
    stc = base.clone()
    stc[0, 0:8191:2] = OPTIONAL
    cases = {"few": (few, U, False), "stc": (stc, 8191, True)}
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for kind in ("classic", "simplified"):
        c = kind == "classic"
        loss_fn = ctc.classic_ctc_long_loss if c else ctc.simplified_ctc_long_loss
        if a.existing_only:  # (the new functions are looked up only where they are called, so that --root works on a tree without them)
            star_post = None
        else:
            star_post = ctc.classic_ctc_long_star_label_posterior if c else ctc.simplified_ctc_long_star_label_posterior
        for case, (lab, L, opt) in cases.items():
            lab = lab.to(dev)
            ll = torch.full((B,), L, dtype=torch.int32, device=dev)
            okw = {"optional_wildcards": True} if opt else {}
            if opt:
                post_fn = ctc.classic_ctc_long_optional_wildcard_label_posterior if c else ctc.simplified_ctc_long_optional_wildcard_label_posterior
            else:
                post_fn = ctc.classic_ctc_long_label_posterior if c else ctc.simplified_ctc_long_label_posterior

            def loss(on, **kw):
                xkw = {"exclude_next_label": True} if on else {}
                return loss_fn(lab, kw.pop("x", x), ll, tl, 0, max_label_length=U, **okw, **xkw, **kw)

            def loss_grad(on, checkpoint):
                xg = x.detach().requires_grad_(True)
                torch.autograd.grad(loss(on, x=xg, checkpoint=checkpoint).sum(), xg)

            def post(on):
                if on:
                    return star_post(lab, x, ll, tl, 0, dense=False, max_label_length=U, **okw)
                return post_fn(lab, x, ll, tl, 0, dense=False, max_label_length=U)

            fns = [("loss", loss), ("loss+grad", lambda on: loss_grad(on, False)), ("loss+grad checkpoint", lambda on: loss_grad(on, True)),
                   ("label_posterior dense=False", post)]
            for what, fn in fns:
                med, lo, hi = timed(lambda: fn(False), a.runs, a.calls)
                row = dict(case=f"long B1 T30000 U8192 V32 {case}", lattice=kind, call=what, off_us=round(med, 1), off_min=round(lo, 1),
                           off_max=round(hi, 1), spread=round((hi - lo) / med, 4))
                if not a.existing_only:
                    nmed, nlo, nhi = timed(lambda: fn(True), a.runs, a.calls)
                    row.update(on_us=round(nmed, 1), on_min=round(nlo, 1), on_max=round(nhi, 1), ratio=round(nmed / med, 4),
                               expected_at_most=BOUNDS[case][what], met=bool(nmed / med <= BOUNDS[case][what]))
                rows.append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps(dict(summary="long_star_exclusion_time", rows=len(rows), existing_only=bool(a.existing_only))), flush=True)


if __name__ == "__main__":
    main()
