"""Time of the long-form loss, gradient and label posteriors with optional wildcards beside the mandatory-wildcard long-form calls
on the same inputs, in one process (profiles/long_optional_wildcard_time.md), in the manner of benchmarks/long_window_time.py.

    python benchmarks/long_optional_wildcard_time.py [--runs 5] [--calls 2] [--existing-only] [--root DIR]

Shape: B = 1, T = 30 000, U = 8 192, V = 32, float32, both lattices.  Calls: the forward, the loss + gradient on the per-frame
workspace and from tile checkpoints, and the label posteriors with dense=False.  Transcripts: `three` -- three optional positions
(1022, 1024 and 5000) -- and `stc` -- a star before, between and after 4 095 labels, 8 191 positions.  The existing call runs the
same transcript with every -3 replaced by -2.  Every figure is the median over `runs` of the mean time of `calls` back-to-back
calls between two device synchronisations, in microseconds, with the minimum and the maximum over the runs.

Expectations, written before the first run:
  1. An existing long-form call costs what it costs on a build of the parent commit (the OPT = false instantiations report the
     parent's resource lines): run this with --existing-only --root PARENT_TREE in alternating processes; "the same" is a ratio
     inside the parent's own run-to-run spread.
  2. A new call costs the mandatory-wildcard call on the same inputs plus the step's added operands.  The short-form calls paid
     1.03 - 1.26 x at U = 128, the only prior there is; no bar is fixed: the ratios are recorded and said to
     fall inside or outside that range.
It also prints the new workspace sizes at this shape and at the hour (T = 180 000, U = 50 000) from the size queries."""
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
    three = base.clone()
    three[0, [1022, 1024, 5000]] = OPTIONAL
    stc = base.clone()
    stc[0, 0:8191:2] = OPTIONAL
    cases = {"three": (three, U), "stc": (stc, 8191)}
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for kind in ("classic", "simplified"):
        c = kind == "classic"
        loss_fn = ctc.classic_ctc_long_loss if c else ctc.simplified_ctc_long_loss
        post_fn = ctc.classic_ctc_long_label_posterior if c else ctc.simplified_ctc_long_label_posterior
        # (looked up only for the new calls, so that --root works on a tree without them)
        opost_fn = None if a.existing_only else (ctc.classic_ctc_long_optional_wildcard_label_posterior if c
                                                 else ctc.simplified_ctc_long_optional_wildcard_label_posterior)
        for case, (lab, L) in cases.items():
            new_lab = lab.to(dev)
            old_lab = torch.where(lab == OPTIONAL, torch.full_like(lab, WILDCARD), lab).to(dev)
            ll = torch.full((B,), L, dtype=torch.int32, device=dev)

            def loss_grad(opt, checkpoint):
                xg = x.detach().requires_grad_(True)
                kw = {"optional_wildcards": True} if opt else {}
                torch.autograd.grad(loss_fn(new_lab if opt else old_lab, xg, ll, tl, 0, checkpoint=checkpoint, max_label_length=U, **kw).sum(), xg)

            fns = [("loss", lambda opt: loss_fn(new_lab if opt else old_lab, x, ll, tl, 0, max_label_length=U,
                                                **({"optional_wildcards": True} if opt else {}))),
                   ("loss+grad", lambda opt: loss_grad(opt, False)),
                   ("loss+grad checkpoint", lambda opt: loss_grad(opt, True)),
                   ("label_posterior dense=False", lambda opt: (opost_fn if opt else post_fn)(new_lab if opt else old_lab, x, ll, tl, 0,
                                                                                              dense=False, max_label_length=U))]
            for what, fn in fns:
                med, lo, hi = timed(lambda: fn(False), a.runs, a.calls)
                row = dict(case=f"long B1 T30000 U8192 V32 {case}", lattice=kind, call=what, existing_us=round(med, 1), existing_min=round(lo, 1),
                           existing_max=round(hi, 1), spread=round((hi - lo) / med, 4))
                if not a.existing_only:
                    nmed, nlo, nhi = timed(lambda: fn(True), a.runs, a.calls)
                    row.update(optional_us=round(nmed, 1), optional_min=round(nlo, 1), optional_max=round(nhi, 1), ratio=round(nmed / med, 4),
                               inside_short_form_range=bool(1.03 <= nmed / med <= 1.26))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if not a.existing_only:
        from tf_seq2seq_losses_amd import _lib
        for shape in ((1, 30000, 32, 8192), (1, 180000, 32, 50000)):
            for k, kind in enumerate(("classic", "simplified")):
                print(json.dumps(dict(workspace=f"B{shape[0]} T{shape[1]} U{shape[3]}", lattice=kind,
                                      loss_forward=_lib.long_optional_wildcard_loss_workspace_bytes(k, *shape, 0, False),
                                      loss_grad=_lib.long_optional_wildcard_loss_workspace_bytes(k, *shape, 0, True),
                                      loss_grad_ckpt=_lib.long_optional_wildcard_loss_ckpt_workspace_bytes(k, *shape, 0, True),
                                      label_posterior=_lib.long_optional_wildcard_label_posterior_workspace_bytes(k, *shape, 0),
                                      existing_loss_grad_ckpt=_lib.long_wildcard_loss_ckpt_workspace_bytes(k, *shape, 0, True))), flush=True)
    print(json.dumps(dict(summary="long_optional_wildcard_time", rows=len(rows), existing_only=bool(a.existing_only))), flush=True)


if __name__ == "__main__":
    main()
