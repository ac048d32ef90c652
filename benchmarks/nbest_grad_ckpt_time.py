"""Time of the N-best gradient from block checkpoints (ctc_amd_nbest_loss_grad_ckpt: two launches) beside the three-launch call
(ctc_amd_nbest_loss_grad) and beside what both replace, with the method, inputs and columns of nbest_grad_time.py (its docstring
has the protocol): all four calls of a line in the same process, alternating, device events around every call.

    nbest_grad_ckpt_time.py --out profiles/nbest_grad_ckpt_time.md        on the GPU (there is no CPU path)

B=256 T=1000 U=128 V=256, N in {1, 8, 32}.  No threshold is asserted: the table is the result."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nbest_grad_time import INPUTS, KINDS, cell, stats  # noqa: E402

NS = (1, 8, 32)
COLUMNS = ("ckpt", "three", "base", "base_with_copy")


def measure(a, N):
    import torch
    from tf_seq2seq_losses_amd import _lib, ops
    assert torch.cuda.is_available(), "nbest_grad_ckpt_time.py needs a GPU"
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
            ws = {"ckpt": _lib.nbest_loss_grad_ckpt_workspace_bytes(k, B, T, V, U, N), "three": _lib.nbest_loss_grad_workspace_bytes(k, B, T, V, U, N)}
            free = torch.cuda.mem_get_info()[0]
            out = {}

            def ckpt():
                out["ckpt"] = ops.nbest_loss_grad_ckpt(k, _lib.WRT_LOGITS, labels, x, ll, tl, 0, w, U)

            def three():
                out["three"] = ops.nbest_loss_grad(k, _lib.WRT_LOGITS, labels, x, ll, tl, 0, w, U)

            calls = [fn for fn in (ckpt, three) if ws[fn.__name__] + x.numel() * 4 + (2 << 30) <= free]
            if 3 * N * x.numel() * 4 + (4 << 30) <= free:  # the expansion, its gradient, and a second expansion in flight
                xe = x.repeat_interleave(N, 0)
                tle = tl.repeat_interleave(N, 0)
                prep = ops.Prepared(labels.view(B * N, U), xe, ll.view(B * N), tle, 0, U=U)

                def base():
                    loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, prep, True, d_loss=w.reshape(-1))
                    out["base"] = (loss, grad.view(B, N, T, V).sum(1))

                def base_with_copy():
                    p = ops.Prepared(labels.view(B * N, U), x.repeat_interleave(N, 0), ll.view(B * N), tle, 0, U=U)
                    loss, grad = ops.loss_grad(k, _lib.WRT_LOGITS, p, True, d_loss=w.reshape(-1))
                    out["base_with_copy"] = (loss, grad.view(B, N, T, V).sum(1))

                calls += [base, base_with_copy]
            for _ in range(a.warmup):
                for fn in calls:
                    fn()
            torch.cuda.synchronize()
            times = {fn.__name__: [] for fn in calls}
            for _ in range(a.steps):
                for fn in calls:
                    times[fn.__name__].append(timed(fn))
            # the outputs at the size timed: the new call against the three-launch call and against the expanded route
            diff = {}
            for other in ("three", "base"):
                if "ckpt" in out and other in out:
                    diff[other] = float((out["ckpt"][1] - out[other][1]).abs().max())
                    assert diff[other] <= 1e-3 * max(1.0, float(w.abs().sum(1).max())), (other, diff[other])
            if "three" in out and "ckpt" in out:
                assert torch.equal(out["ckpt"][0], out["three"][0]), "the losses differ"
            out.clear()
            xe = prep = None
            torch.cuda.empty_cache()
            rows.append(dict(input=name, N=N, kind=kind, ws=ws, times=times, diff=diff))
            print(f"{name} N={N} {kind}: " + ", ".join(f"{c} {cell(times[c])} us" for c in COLUMNS if c in times) +
                  f"; workspace {ws['ckpt'] / 1e9:.2f} / {ws['three'] / 1e9:.2f} GB; worst difference {diff}", flush=True)
        del x
    return dict(device=torch.cuda.get_device_name(0), rows=rows)


def table(a, results):
    lines = [f"# N-best gradient from block checkpoints beside the three-launch call and the expanded route: B={a.B} T={a.T} U={a.U} V={a.V}", "",
             f"device: {results[0]['device'] if results else '-'}; {a.steps} warm calls each after {a.warmup}, the calls of a line alternating in one "
             "process, every N in a process of its own.  Device events around every call, microseconds: median (minimum, spread = "
             "(max - min) / median).  `existing + sum`: ops.loss_grad on logits.repeat_interleave(N, 0), then .view(B, N, T, V).sum(1); "
             "`with its copy`: the expansion inside the timed region.  The ratios compare medians; `-`: the buffers do not fit.", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| logits | N | lattice | ctc_amd_nbest_loss_grad_ckpt | its workspace | ctc_amd_nbest_loss_grad | its workspace | existing + sum | "
              "with its copy | ckpt / three-launch | ckpt / with copy | worst |ckpt - three-launch| |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for res in results:
        for r in res["rows"]:
            t = r["times"]
            c = [cell(t[k]) if k in t else "-" for k in COLUMNS]

            def ratio(k):
                return f"{stats(t['ckpt'])[0] / stats(t[k])[0]:.2f}" if "ckpt" in t and k in t else "-"
            lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {c[0]} | {r['ws']['ckpt'] / 1e9:.2f} GB | {c[1]} | {r['ws']['three'] / 1e9:.2f} GB | "
                         f"{c[2]} | {c[3]} | {ratio('three')} | {ratio('base_with_copy')} | {r['diff'].get('three', float('nan')):.1e} |")
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
