"""Time of the N-best rescoring call (ctc_amd_nbest_loss: one launch) beside what it replaces, in the manner of
beam_search_time.py: the existing loss-only call, ops.loss_grad(..., want_grad=False), on logits.repeat_interleave(N, 0) with one
hypothesis per row -- reported without the expansion copy (the expanded logits already exist) and with it (the copy inside the
timed region).

    nbest_loss_time.py --out profiles/nbest_loss_time.md        on the GPU (there is no CPU path)

B=256 T=1000 U=128 V=256, full-length utterances, N in {1, 4, 8, 32}; N(0, 1) logits and blank-biased N(0, 3^2) logits; both
lattices; hypotheses of 64..128 random labels (every one feasible).  N = 32 is reported only if its 8.4 GB expansion fits in the
device memory that is free.  Device time: events around every call on a warm device, `--steps` calls after `--warmup`, the calls
of a configuration alternating; median, minimum and the spread (max - min) / median of every column, so that a difference
between two columns can be read against the run-to-run spread of either.  The device's copy rate (ctc_amd_probe_copy over the
logits, read + write) stands in the head: the expansion copy is N such writes.  No threshold is asserted: the table is the result."""
import argparse
import os
import sys

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


def measure(a):
    import torch
    from tf_seq2seq_losses_amd import _lib, ops
    assert torch.cuda.is_available(), "nbest_loss_time.py needs a GPU"
    lib = _lib.load()
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

    # the copy rate of this device, on a buffer of the logits' size
    src = torch.empty(B * T * V, device=dev).normal_()
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream

    def probe():
        assert lib.ctc_amd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel() * 4, st) == 0

    for _ in range(a.warmup):
        probe()
    copy_us = [timed(probe) for _ in range(a.steps)]
    copy_rate = 2 * src.numel() * 4 / (np.median(copy_us) * 1e-6) / 1e12  # TB/s, read + write
    del src, dst

    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for name, sigma, bias in INPUTS:
        x = (sigma * torch.randn((B, T, V), generator=g)).to(dev)
        x[..., 0] += bias
        for N in NS:
            labels = torch.randint(1, V, (B, N, U), generator=g, dtype=torch.int32).to(dev)
            ll = torch.randint(U // 2, U + 1, (B, N), generator=g, dtype=torch.int32).to(dev)
            need = N * x.numel() * 4
            fits = need + (2 << 30) <= torch.cuda.mem_get_info()[0]
            for kind in KINDS:
                k = ops.KINDS[kind]
                out = {}

                def new():
                    out["new"] = ops.nbest_loss(k, _lib.WRT_LOGITS, labels, x, ll, tl, 0, U)

                t_new = t_base = t_copy = None
                if fits:
                    xe = x.repeat_interleave(N, 0)
                    tle = tl.repeat_interleave(N, 0)
                    prep = ops.Prepared(labels.view(B * N, U), xe, ll.view(B * N), tle, 0, U=U)

                    def base():
                        out["base"] = ops.loss_grad(k, _lib.WRT_LOGITS, prep, want_grad=False)[0]

                    def base_with_copy():
                        p = ops.Prepared(labels.view(B * N, U), x.repeat_interleave(N, 0), ll.view(B * N), tle, 0, U=U)
                        out["copy"] = ops.loss_grad(k, _lib.WRT_LOGITS, p, want_grad=False)[0]

                    pipeline = ops.pipeline_of(k, _lib.WRT_LOGITS, prep)
                    for _ in range(a.warmup):  # (every column the same number of warm calls: the expansion's buffer comes from the allocator's cache then)
                        new(); base(); base_with_copy()
                    torch.cuda.synchronize()
                    t_new, t_base, t_copy = [], [], []
                    for _ in range(a.steps):
                        t_new.append(timed(new)); t_base.append(timed(base)); t_copy.append(timed(base_with_copy))
                    diff = (out["new"].view(-1) - out["base"]).abs()
                    assert bool(torch.isfinite(out["new"]).all()) and float(diff.max()) <= 1e-3 * float(out["base"].abs().max()), float(diff.max())
                    del xe, prep
                else:
                    pipeline = "-"
                    for _ in range(a.warmup):
                        new()
                    torch.cuda.synchronize()
                    t_new = [timed(new) for _ in range(a.steps)]
                rows.append(dict(input=name, N=N, kind=kind, pipeline=pipeline, new=t_new, base=t_base, copy=t_copy))
                print(f"{name} N={N} {kind}: new {cell(t_new)} us" + (f", existing {cell(t_base)} us, with its copy {cell(t_copy)} us"
                                                                      if fits else ", the expansion does not fit"), flush=True)
        del x
    return dict(device=torch.cuda.get_device_name(0), copy_us=float(np.median(copy_us)), copy_rate=copy_rate, rows=rows)


def table(a, res):
    B, T, V, U = a.B, a.T, a.V, a.U
    mb = B * T * V * 4 / 1e6
    lines = [f"# N-best rescoring call beside the existing loss-only call on expanded logits: B={B} T={T} U={U} V={V}", "",
             f"device: {res['device']}; {a.steps} warm calls each after {a.warmup}, the calls of a line alternating.  Device events around "
             "every call, microseconds: median (minimum, spread = (max - min) / median).  Logits: "
             f"{mb:.0f} MB; a copy of them (read + write) takes {res['copy_us']:.0f} us here: {res['copy_rate']:.2f} TB/s.  "
             "`existing`: ops.loss_grad(want_grad=False) on logits.repeat_interleave(N, 0), the expansion made beforehand; "
             "`with its copy`: the expansion inside the timed region.  `new / existing` compares the medians.", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| logits | N | lattice | ctc_amd_nbest_loss | existing (pipeline) | existing with its copy | new / existing | new / with copy |",
              "|---|---|---|---|---|---|---|---|"]
    for r in res["rows"]:
        if r["base"] is None:
            lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {cell(r['new'])} | the {r['N'] * mb / 1e3:.1f} GB expansion does not fit | - | - | - |")
            continue
        n, b, c = stats(r["new"])[0], stats(r["base"])[0], stats(r["copy"])[0]
        lines.append(f"| {r['input']} | {r['N']} | {r['kind']} | {cell(r['new'])} | {cell(r['base'])} ({r['pipeline']}) | {cell(r['copy'])} | "
                     f"{n / b:.2f} | {n / c:.2f} |")
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
