"""Time of the N-best alignment call (ctc_amd_nbest_best_path: one launch) beside what it replaces, in the manner of
nbest_loss_time.py and alignment_time.py: N consecutive ops.best_path calls, one per list position, on labels[:, n] of the same
list and the same logits (no copy of the logits is needed for that; the N prepared argument sets exist beforehand).

    nbest_align_time.py --out profiles/nbest_align_time.md        on the GPU (there is no CPU path)

B=256 T=1000 U=128 V=256, full-length utterances, N in {1, 4, 8, 32}; both lattices; float32 N(0, 1) logits and their float32
log-probabilities (CTC_AMD_WRT_LOGPROBS: no row statistics); hypotheses of 64..128 random labels (every one feasible).  Device
time: events around every call (the baseline: around its N calls together) on a warm device, `--steps` calls after `--warmup`,
the two columns of a line alternating; median, minimum and the spread (max - min) / median of every column.  The expectation
-- at N = 8 the new call takes less device time than the eight calls together, by more than the baseline's own spread -- is
marked met or not met on every line; no threshold is asserted: the table is the result."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (1, 4, 8, 32)
KINDS = ("classic", "simplified")
INPUTS = (("logits", 0), ("log-probabilities", 1))  # name, wrt


def stats(us):
    us = np.asarray(us)
    return float(np.median(us)), float(us.min()), float((us.max() - us.min()) / np.median(us))


def cell(us):
    med, lo, spread = stats(us)
    return f"{med:.0f} ({lo:.0f}, {100 * spread:.0f}%)"


def measure(a):
    import torch
    from tf_seq2seq_losses_amd import ops
    assert torch.cuda.is_available(), "nbest_align_time.py needs a GPU"
    dev = torch.device("cuda:0")
    B, T, V, U = a.B, a.T, a.V, a.U
    g = torch.Generator(device="cpu").manual_seed(0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    logits = torch.randn((B, T, V), generator=g).to(dev)
    rows = []
    for name, wrt in INPUTS:
        x = torch.log_softmax(logits, dim=-1) if wrt else logits
        for N in NS:
            labels = torch.randint(1, V, (B, N, U), generator=g, dtype=torch.int32).to(dev)
            ll = torch.randint(U // 2, U + 1, (B, N), generator=g, dtype=torch.int32).to(dev)
            for kind in KINDS:
                k = ops.KINDS[kind]
                out = {}
                preps = [ops.Prepared(labels[:, n], x, ll[:, n], tl, 0, keep_format=True, U=U) for n in range(N)]

                def new():
                    out["new"] = ops.nbest_best_path(k, wrt, labels, x, ll, tl, 0, U)

                def base():
                    out["base"] = [ops.best_path(k, wrt, p) for p in preps]

                for _ in range(a.warmup):
                    new(); base()
                torch.cuda.synchronize()
                t_new, t_base = [], []
                for _ in range(a.steps):
                    t_new.append(timed(new)); t_base.append(timed(base))
                same = all(bool((out["new"][1][:, n] == out["base"][n][1]).all()) and bool((out["new"][2][:, n] == out["base"][n][2]).all())
                           for n in range(N))
                diff = max(float((out["new"][0][:, n] - out["base"][n][0]).abs().max()) for n in range(N))
                assert bool(torch.isfinite(out["new"][0]).all()) and diff <= 1e-3, diff
                rows.append(dict(input=name, N=N, kind=kind, new=t_new, base=t_base, same=same, diff=diff))
                print(f"{name} N={N} {kind}: new {cell(t_new)} us, {N} x best_path {cell(t_base)} us, paths {'equal' if same else 'DIFFER'}, "
                      f"largest score difference {diff:.2e}", flush=True)
                del preps
        del x
    return dict(device=torch.cuda.get_device_name(0), rows=rows)


def verdict(r):
    """The new call against the N calls together, read against the baseline's own spread."""
    n, b, spread = stats(r["new"])[0], stats(r["base"])[0], stats(r["base"])[2]
    if n < b * (1 - spread):
        return "faster, by more than the baseline's spread"
    if n > b * (1 + spread):
        return "slower, by more than the baseline's spread"
    return "within the baseline's spread"


def table(a, res):
    B, T, V, U = a.B, a.T, a.V, a.U
    lines = [f"# N-best alignment call beside N consecutive best-path calls: B={B} T={T} U={U} V={V}", "",
             f"device: {res['device']}; {a.steps} warm calls each after {a.warmup}, the two columns of a line alternating.  Device events "
             "around every call (the baseline: around its N calls together), microseconds: median (minimum, spread = (max - min) / "
             "median).  `N x ctc_amd_best_path`: ops.best_path on labels[:, n] for n = 0 .. N - 1, the same logits, arguments prepared "
             "beforehand.  `new / N calls` compares the medians.  Expectation (N = 8): the new call takes less device time than the "
             "eight calls together, by more than the baseline's own spread.", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| input | N | lattice | ctc_amd_nbest_best_path | N x ctc_amd_best_path | new / N calls | reading | expectation (N = 8) | paths equal |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        n, b = stats(r["new"])[0], stats(r["base"])[0]
        v = verdict(r)
        exp = "-" if r["N"] != 8 else ("met" if v.startswith("faster") else "NOT met")
        lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {cell(r['new'])} | {cell(r['base'])} | {n / b:.2f} | {v} | {exp} | "
                     f"{'yes' if r['same'] else 'NO'} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    text = table(a, measure(a))
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
