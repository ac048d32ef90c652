"""Time of the edit-counts call (ctc_amd_edit_counts: K + J - 1 launches over the tiles of the table), in the manner of
edit_distance_time.py.

    edit_counts_time.py --out profiles/edit_counts_time.md        on the GPU (there is no CPU path)

(a) B=256, N=8, lengths near 128 (96..128, tensors 128 wide): beside ctc_amd_edit_distance on the same tensors.
(b) one hypothesis per utterance, h ~ r in {4096, 16384, 65536}, B in {1, 8}: beside the route a user has without the call --
    hypotheses and references .cpu(), the packed row programme of tests/tools/edit_counts_oracle.py on the host, the result back
    .to(device): host wall time, end to end, the copies included (one call; skipped above --host-cells table cells, where it takes
    minutes: the line then says so).
(c) rows_per_tile in {256, 512, 1024, 2048} at B=1, h ~ r = 16384: the default is chosen by this line.
Tokens from 30 symbols, every hypothesis a corrupted copy of its reference (about 15% edits).  Device time: events around `--reps`
back-to-back calls (time per call), `--steps` timings after `--warmup`; median, minimum and spread.  Every timed result is compared
with the other route's (asserted).  No threshold is asserted: the table is the result."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmarks.edit_distance_time import cell, corrupted, stats  # noqa: E402

LONG = (4096, 16384, 65536)
TILES = (256, 512, 1024, 2048)


def timer(torch):
    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # microseconds per call
    return timed


def series(a, torch, fn, reps):
    timed = timer(torch)
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    return [timed(fn, reps) for _ in range(a.steps)]


def make(rng, B, N, width, low, dev, torch):
    ref_h = rng.integers(0, 30, (B, width)).astype(np.int32)
    rl_h = rng.integers(low, width + 1, B).astype(np.int32)
    hyp_h, hl_h = corrupted(rng, ref_h, rl_h, N, width, 30)
    return tuple(torch.tensor(t, device=dev) for t in (hyp_h, hl_h, ref_h, rl_h))


def measure_short(a, dev, torch):
    from tf_seq2seq_losses_amd import ops
    hyp, hl, ref, rl = make(np.random.default_rng(0), a.B, 8, 128, 96, dev, torch)
    out = {}

    def new():
        out["new"] = ops.edit_counts(hyp, hl, ref, rl)

    def old():
        out["old"] = ops.edit_distance(hyp, hl, ref, rl)

    t_new, t_old = series(a, torch, new, a.reps), series(a, torch, old, a.reps)
    assert torch.equal(out["new"][..., 0], out["old"])
    print(f"(a) B={a.B} N=8 near 128: edit_counts {cell(t_new)} us, edit_distance {cell(t_old)} us", flush=True)
    return dict(new=t_new, old=t_old, mean=out["new"].float().mean((0, 1)).tolist())


def host_route(hyp, hl, ref, rl, dev, torch):
    from tests.tools import edit_counts_oracle as C
    t0 = time.perf_counter()
    d = C.edit_counts_batch(hyp.cpu().numpy(), hl.cpu().numpy(), ref.cpu().numpy(), rl.cpu().numpy(), one=C.edit_counts_rows)
    out = torch.from_numpy(d).to(dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def measure_long(a, dev, torch):
    from tf_seq2seq_losses_amd import ops
    rng = np.random.default_rng(1)
    rows = []
    for width in LONG:
        for B in (1, 8):
            hyp, hl, ref, rl = make(rng, B, 1, width, width - width // 16, dev, torch)
            out = {}

            def new():
                out["new"] = ops.edit_counts(hyp, hl, ref, rl)

            t_new = series(a, torch, new, a.reps)
            t_host = None
            if B * width * width <= a.host_cells:
                t_host, want = host_route(hyp, hl, ref, rl, dev, torch)
                assert torch.equal(out["new"], want)
            K, J = -(-width // 1024), -(-width // a.default_tile)
            rows.append(dict(width=width, B=B, new=t_new, host=t_host, launches=K + J - 1, tiles=K * J, mean=out["new"].float().mean((0, 1)).tolist()))
            print(f"(b) h ~ r = {width} B={B}: edit_counts {cell(t_new)} us, host {t_host if t_host is None else round(t_host)} us", flush=True)
    return rows


def measure_tiles(a, dev, torch):
    from tf_seq2seq_losses_amd import ops
    hyp, hl, ref, rl = make(np.random.default_rng(2), 1, 1, 16384, 16384 - 1024, dev, torch)
    rows, first = [], None
    for tile in TILES:
        out = {}

        def new():
            out["new"] = ops.edit_counts(hyp, hl, ref, rl, rows_per_tile=tile)

        t = series(a, torch, new, a.reps)
        first = out["new"] if first is None else first
        assert torch.equal(out["new"], first)
        rows.append(dict(tile=tile, new=t, launches=16 + -(-16384 // tile) - 1))
        print(f"(c) rows_per_tile={tile}: {cell(t)} us", flush=True)
    return rows


def table(a, dev_name, short, long_rows, tiles):
    lines = [f"# Edit counts (distance, substitutions, insertions, deletions) up to 65536 tokens", "",
             f"device: {dev_name}; {a.steps} timings each after {a.warmup} warm calls; microseconds: median (minimum, spread = (max - min) / "
             f"median).  Device calls by events around {a.reps} calls issued back to back (time per call); the host route by the host's clock "
             "around copy out + the packed NumPy row programme + copy back (one call).  Every pair of routes agrees on every count (asserted).", ""]
    if a.note:
        lines += [a.note, ""]
    n, o = stats(short["new"])[0], stats(short["old"])[0]
    lines += [f"## (a) lengths near 128, N = 8, B = {a.B}: beside `ctc_amd_edit_distance`", "",
              "Expectation before measuring: no more than a small multiple of `ctc_amd_edit_distance`, since the launch dominates both "
              "(one launch each here: R = 128 is one tile of 2 reference tokens per lane; the cells are 64-bit words in place of 32-bit).", "",
              "| mean (d, S, I, D) | ctc_amd_edit_counts | ctc_amd_edit_distance | ratio |", "|---|---|---|---|",
              f"| {', '.join(f'{v:.1f}' for v in short['mean'])} | {cell(short['new'])} | {cell(short['old'])} | {n / o:.2f} |", "",
              f"## (b) one hypothesis per utterance, h ~ r, default rows_per_tile = {a.default_tile}: beside .cpu() + host programme + copy back", "",
              "Expectation before measuring: the time grows with the number of launches K + J - 1 and not with the number of tiles K * J "
              "at B = 1 (the tiles of an anti-diagonal run side by side), and the call beats the host route on every line.", "",
              "| h ~ r | B | mean (d, S, I, D) | launches K + J - 1 | tiles K * J | ctc_amd_edit_counts | per launch | host route | new / host |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in long_rows:
        m = stats(r["new"])[0]
        host = "not run (minutes; B times the B = 1 line)" if r["host"] is None else f"{r['host']:.0f}"
        ratio = "" if r["host"] is None else f"{m / r['host']:.5f}"
        lines.append(f"| {r['width']} | {r['B']} | {', '.join(f'{v:.0f}' for v in r['mean'])} | {r['launches']} | {r['tiles']} | {cell(r['new'])} | "
                     f"{m / r['launches']:.1f} | {host} | {ratio} |")
    lines += ["", "## (c) rows_per_tile at B = 1, h ~ r = 16384", "",
              "Expectation before measuring: a lower tile means more launches of fewer steps each and less of every launch spent filling and "
              "draining the 64 lanes' skew (63 steps per tile); the best of the four becomes the default.", "",
              "| rows_per_tile | launches | ctc_amd_edit_counts |", "|---|---|---|"]
    lines += [f"| {r['tile']} | {r['launches']} | {cell(r['new'])} |" for r in tiles]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--host-cells", type=float, default=4.5e9, help="the host route runs up to this many table cells per line")
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "edit_counts_time.py needs a GPU"
    from tf_seq2seq_losses_amd import _lib
    _lib.load()
    a.default_tile = 256  # EDIT_LONG_RT_DEFAULT (csrc/ctc_edit_long_plan.h)
    dev = torch.device("cuda:0")
    short = measure_short(a, dev, torch)
    tiles = measure_tiles(a, dev, torch)
    long_rows = measure_long(a, dev, torch)
    text = table(a, torch.cuda.get_device_name(0), short, long_rows, tiles)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
