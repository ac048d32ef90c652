"""Time of the tiled long-form alignment with optional wildcards and the exclusion of the next label
(ctc_amd_long_optional_wildcard_best_path / ctc_amd_long_star_best_path), in the manner of benchmarks/long_wildcard_alignment_time.py.

Warm calls timed with device events (one pair around each call), float32 logits, full-length utterances, frames_per_tile 128, all
outputs.  Transcripts, those of benchmarks/long_optional_wildcard_time.py: `three` -- optional positions at 1022, 1024 and 5000 (at
U = 1024: 510, 512 and 1000) -- and `stc` -- a star before, between and after the labels, U - 1 positions.  Every row is one
(lattice, B, T, U, transcript) and shows
  existing    ctc_amd_long_wildcard_best_path on the same transcript with -2 for every -3 (that code is untouched);
  OPT, XN, OPT+XN    the three new instantiations on the transcript itself (XN alone: on the -2 transcript),
the calls alternating; the median and (minimum - maximum) over the warm calls, the ratio of medians to `existing`, and the time per
launch of a tile diagonal (K + J - 1 of them; K differs: the classic label block is 512 positions here, 1024 there).  No gate:
numbers for profiles/long_star_alignment_time.md and DESIGN.md section 5.31.  Needs a GPU.

    python benchmarks/long_star_alignment_time.py --out profiles/long_star_alignment_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

EXPECTATION = """Expectation, written before the numbers.  The long-form loss paid 1.27 - 1.41 x for optional wildcards (DESIGN.md section
5.27) and the short-form alignment 1.05 - 1.11 x for the exclusion (section 5.29).  Here the chain is serial over the frames of a
tile and a launch costs what its slowest tile costs.  Simplified: the same 1024-position block with one more candidate per position
and a second DPP shift: 1.1 - 1.3 x with OPT, XN within 1.1 x, on the same K + J - 1 launches.  Classic: the frame of a 512-position
block does half the positions per lane, so a diagonal should cost clearly less than the existing call's (0.6 - 0.8 x per diagonal
with OPT), while K doubles: at T = 30000, U = 8192 that is 250 launches instead of 242 (K - 1 = 15 instead of 7, against J = 235),
so the whole classic call should come out at or below the existing one, 0.7 - 1.0 x; at T = 8192, U = 1024 (K = 2 instead of 1)
likewise.  The trace fetches a window of 34 (classic) / 18 (simplified) words per frame instead of 16: a few percent of the call."""


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="B,T,U; may be given several times")
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_star_alignment_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192), (8, 30000, 8192), (1, 8192, 1024)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, TF = a.V, 128
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Tiled long-form alignment with optional wildcards and the exclusion: V={V}, float32 logits, frames_per_tile={TF}", "",
             EXPECTATION, "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call; "
             "microseconds, median (minimum - maximum)", "",
             "| lattice | B | T | U | transcript | launches existing / new | existing | OPT | XN | OPT+XN | OPT / existing | XN / existing | "
             "OPT+XN / existing | per diagonal existing | per diagonal OPT+XN |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in shapes:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn((B, T, V), generator=g).to(dev)
        base = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
        three, stc = base.clone(), base.clone()
        three[:, [1022, 1024, 5000] if U > 5000 else [U // 2 - 2, U // 2, U - 24]] = _lib.OPTIONAL_WILDCARD
        stc[:, 0:U - 1:2] = _lib.OPTIONAL_WILDCARD
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        J = max(1, -(-T // TF))
        for kind_name, kind in ops.KINDS.items():
            K0, K1 = max(1, -(-U // 1024)), max(1, -(-U // (512 if kind == 0 else 1024)))
            out = [torch.empty(B, device=dev), *(torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(2)),
                   *(torch.empty((B, U), dtype=torch.int32, device=dev) for _ in range(2)), torch.empty((B, U), device=dev)]
            ptrs = [t.data_ptr() for t in out]
            ws0 = torch.empty(max(_lib.long_wildcard_best_path_workspace_bytes(kind, B, T, V, U, TF), 1), dtype=torch.uint8, device=dev)
            ws1 = torch.empty(max(_lib.long_star_best_path_workspace_bytes(kind, B, T, V, U, TF, True), 1), dtype=torch.uint8, device=dev)
            for name, (lab, L) in {"three": (three, U), "stc": (stc, U - 1)}.items():
                opt_lab = lab.to(dev)
                wild_lab = torch.where(opt_lab == _lib.OPTIONAL_WILDCARD, torch.full_like(opt_lab, _lib.WILDCARD), opt_lab)
                ll = torch.full((B,), L, dtype=torch.int32, device=dev)

                def head(lb):
                    return (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), lb.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)

                def existing():
                    rc = lib.ctc_amd_long_wildcard_best_path(*head(wild_lab), B, T, V, U, TF, *ptrs, ws0.data_ptr(), ws0.numel(), st)
                    assert rc == 0, lib.ctc_amd_last_error()

                def star(lb, opt):
                    def fn():
                        rc = lib.ctc_amd_long_star_best_path(*head(lb), opt, B, T, V, U, TF, *ptrs, ws1.data_ptr(), ws1.numel(), st)
                        assert rc == 0, lib.ctc_amd_last_error()
                    return fn

                def optional():
                    rc = lib.ctc_amd_long_optional_wildcard_best_path(*head(opt_lab), B, T, V, U, TF, *ptrs, ws1.data_ptr(), ws1.numel(), st)
                    assert rc == 0, lib.ctc_amd_last_error()

                calls = {"existing": existing, "opt": optional, "xn": star(wild_lab, 0), "both": star(opt_lab, 1)}
                for _ in range(a.warmup):
                    for fn in calls.values():
                        fn()
                torch.cuda.synchronize()
                times = {n: [] for n in calls}
                for _ in range(a.steps):
                    for n, fn in calls.items():
                        times[n].append(timed(fn))
                assert torch.isfinite(out[0]).all()
                t = {n: np.asarray(v) for n, v in times.items()}
                med = {n: float(np.median(v)) for n, v in t.items()}
                cell = {n: f"{med[n]:.0f} ({t[n].min():.0f} - {t[n].max():.0f})" for n in t}
                lines.append(f"| {kind_name} | {B} | {T} | {U} | {name} | {K0 + J - 1} / {K1 + J - 1} | {cell['existing']} | {cell['opt']} | "
                             f"{cell['xn']} | {cell['both']} | {med['opt'] / med['existing']:.3f} | {med['xn'] / med['existing']:.3f} | "
                             f"{med['both'] / med['existing']:.3f} | {med['existing'] / (K0 + J - 1):.1f} | {med['both'] / (K1 + J - 1):.1f} |")
                print(lines[-1], flush=True)
            del ws0, ws1
        del x
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
