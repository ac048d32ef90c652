"""Time of the N-best gradient call (ctc_amd_nbest_loss_grad: three launches) beside what it replaces, with the protocol of
nbest_loss_time.py: the existing loss + gradient call, ops.loss_grad(..., want_grad=True, d_loss=weight.reshape(-1)), on
logits.repeat_interleave(N, 0) with one hypothesis per row, followed by grad.view(B, N, T, V).sum(1) -- reported without the
expansion copy (the expanded logits already exist) and with it (the copy inside the timed region).

    nbest_grad_time.py --out profiles/nbest_grad_time.md        on the GPU (there is no CPU path)

B=256 T=1000 U=128 V=256, full-length utterances, N in {1, 4, 8, 32}; N(0, 1) logits and blank-biased N(0, 3^2) logits; both
lattices; hypotheses of 64..128 random labels (every one feasible), weights N(0, 1).  Every N is measured by a child process of
its own under a time limit (`--limit` seconds), and nothing more is started once one has failed.  A column whose buffers (the
expansion and its N gradients, or the call's workspace) do not fit in the free device memory is left out and says so.  Device time:
events around every call on a warm device, `--steps` calls after `--warmup`, the calls of a configuration alternating; median,
minimum and the spread (max - min) / median of every column.  No threshold is asserted: the table is the result."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (1, 4, 8, 32)
INPUTS = (("N(0, 1)", 1.0, 0.0), ("blank-biased N(0, 3^2)", 3.0, 6.0))  # name, sigma, what the blank's logit gets on top
KINDS = ("classic", "simplified")


def stats(us):
    us = np.asarray(us)
    return float(np.median(us)), float(us.min()), float((us.max() - us.min()) / np.median(us))


def cell(us):
    med, lo, spread = stats(us)
    return f"{med:.0f} ({lo:.0f}, {100 * spread:.0f}%)"


def measure(a, N):
    import torch
    from tf_seq2seq_losses_amd import _lib, ops
    assert torch.cuda.is_available(), "nbest_grad_time.py needs a GPU"
    dev = torch.device("cuda:0")
    B, T, V, U = a.B, a.T, a.V, a.U
    g = torch.Generator(device="cpu").manual_seed(N)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for name, sigma, bias in INPUTS:
        x = (sigma * torch.randn((B, T, V), generator=g)).to(dev)
        x[..., 0] += bias
        labels = torch.randint(1, V, (B, N, U), generator=g, dtype=torch.int32).to(dev)
        ll = torch.randint(U // 2, U + 1, (B, N), generator=g, dtype=torch.int32).to(dev)
        w = torch.randn((B, N), generator=g).to(dev)
        for kind in KINDS:
            k = ops.KINDS[kind]
            ws_bytes = _lib.nbest_loss_grad_workspace_bytes(k, B, T, V, U, N)
            free = torch.cuda.mem_get_info()[0]
            fits_new = ws_bytes + x.numel() * 4 + (2 << 30) <= free
            fits_base = 3 * N * x.numel() * 4 + (4 << 30) <= free  # the expansion, its gradient, and a second expansion in flight
            out = {}

            def new():
                out["new"] = ops.nbest_loss_grad(k, _lib.WRT_LOGITS, labels, x, ll, tl, 0, w, U)

            t_new = t_base = t_copy = None
            pipeline = "-"
            calls = [new] if fits_new else []
            if fits_base:
                xe = x.repeat_interleave(N, 0)
                tle = tl.repeat_interleave(N, 0)
                prep = ops.Prepared(labels.view(B * N, U), xe, ll.view(B * N), tle, 0, U=U)
                pipeline = ops.pipeline_of(k, _lib.WRT_LOGITS, prep)

                def base():
                    loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, prep, True, d_loss=w.reshape(-1))
                    out["base"] = (loss, grad.view(B, N, T, V).sum(1))

                def base_with_copy():
                    p = ops.Prepared(labels.view(B * N, U), x.repeat_interleave(N, 0), ll.view(B * N), tle, 0, U=U)
                    loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True, d_loss=w.reshape(-1))
                    out["copy"] = (loss, grad.view(B, N, T, V).sum(1))

                calls += [base, base_with_copy]
            for _ in range(a.warmup):  # (every column the same number of warm calls: the buffers come from the allocator's cache then)
                for fn in calls:
                    fn()
            torch.cuda.synchronize()
            times = {fn.__name__: [] for fn in calls}
            for _ in range(a.steps):
                for fn in calls:
                    times[fn.__name__].append(timed(fn))
            t_new, t_base, t_copy = times.get("new"), times.get("base"), times.get("base_with_copy")
            worst = None
            if fits_new and fits_base:
                worst = float((out["new"][1] - out["base"][1]).abs().max())
                assert bool(torch.isfinite(out["new"][0]).all()) and worst <= 1e-3 * float(w.abs().sum(1).max()), worst
            if fits_base:
                del xe, prep
            out.clear()
            torch.cuda.empty_cache()
            rows.append(dict(input=name, N=N, kind=kind, pipeline=pipeline, ws_bytes=ws_bytes, new=t_new, base=t_base, copy=t_copy, diff=worst))
            print(f"{name} N={N} {kind}: new {cell(t_new) if t_new else '-'} us, existing {cell(t_base) if t_base else '-'} us, "
                  f"with its copy {cell(t_copy) if t_copy else '-'} us, workspace {ws_bytes / 1e9:.2f} GB, worst difference {worst}", flush=True)
        del x
    return dict(device=torch.cuda.get_device_name(0), rows=rows)


def table(a, results):
    B, T, V, U = a.B, a.T, a.V, a.U
    mb = B * T * V * 4 / 1e6
    lines = [f"# N-best gradient call beside the existing loss + gradient call on expanded logits: B={B} T={T} U={U} V={V}", "",
             f"device: {results[0]['device'] if results else '-'}; {a.steps} warm calls each after {a.warmup}, the calls of a line alternating, every N in "
             "a process of its own.  Device events around every call, microseconds: median (minimum, spread = (max - min) / median).  "
             f"Logits: {mb:.0f} MB.  `existing`: ops.loss_grad with d_loss = weight on logits.repeat_interleave(N, 0), then "
             ".view(B, N, T, V).sum(1), the expansion made beforehand; `with its copy`: the expansion inside the timed region.  "
             "`new / existing` compares the medians.", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| logits | N | lattice | ctc_amd_nbest_loss_grad | its workspace | existing + sum (pipeline) | existing with its copy | new / existing | new / with copy |",
              "|---|---|---|---|---|---|---|---|---|"]
    for res in results:
        for r in res["rows"]:
            new = cell(r["new"]) if r["new"] else "the workspace does not fit"
            if r["base"] is None:
                lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {new} | {r['ws_bytes'] / 1e9:.2f} GB | the expansion and its gradients do not fit | - | - | - |")
                continue
            b, c = stats(r["base"])[0], stats(r["copy"])[0]
            n = stats(r["new"])[0] if r["new"] else float("nan")
            lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {new} | {r['ws_bytes'] / 1e9:.2f} GB | {cell(r['base'])} ({r['pipeline']}) | "
                         f"{cell(r['copy'])} | {n / b:.2f} | {n / c:.2f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns", type=int, nargs="*", default=list(NS))
    ap.add_argument("--limit", type=int, default=240, help="seconds for the child process of one N")
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--child", default=None, help="(internal) measure --ns[0] in this process and write the result to this JSON file")
    a = ap.parse_args()
    if a.child:
        with open(a.child, "w") as f:
            json.dump(measure(a, a.ns[0]), f)
        return
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for N in a.ns:  # one fresh process per N under its own time limit; nothing more is started after a failure
            path = os.path.join(tmp, f"n{N}.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--ns", str(N), "--B", str(a.B), "--T", str(a.T), "--V", str(a.V),
                   "--U", str(a.U), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            rc = subprocess.run(["timeout", "-k", "10", str(a.limit), *cmd]).returncode
            if rc != 0:
                print(f"N={N}: the child process ended with status {rc}; stopping here", flush=True)
                break
            with open(path) as f:
                results.append(json.load(f))
    text = table(a, results)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if len(results) != len(a.ns):
        sys.exit(1)


if __name__ == "__main__":
    main()
