"""Time of the greedy decoding call (ctc_amd_greedy_decode: both launches) beside the torch composition
log_softmax(x, -1).max(-1) on the same buffers -- the row stage's equivalent only, without any collapse.

Warm launches timed with device events (one pair of events around each call, the two alternating), at B=256 T=1000 V=256
unless told otherwise; float32 and bfloat16 logits, and log-probability input (whose composition is x.max(-1) alone).  Beside
each: the read-once yardstick B * T * V * element bytes / 8 TB/s and the same bytes at the rate this box's ctc_amd_probe_copy
moves them (a copy reads and writes: its rate counts both directions).
One requirement (asserted): the decoding call takes no longer than the composition at the float32 and the bfloat16 logits line.
Numbers for profiles/decode_time.md and DESIGN.md section 5.7.  Needs a GPU (there is no CPU path)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (datasheet)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, V = a.B, a.T, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    x32[..., 0] += 3.0  # blank-biased, as a trained model's output is: labels are shorter than frames
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    score = torch.empty(B, device=dev)
    tokens, labels, frames = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(3))
    length = torch.empty(B, dtype=torch.int32, device=dev)
    label_score = torch.empty((B, T), device=dev)
    ws = torch.empty(max(_lib.greedy_decode_workspace_bytes(B, T), 1), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    # the box's copy rate, with the access shape of the kernels' row traffic
    nbytes = x32.numel() * 4
    dst = torch.empty_like(x32)

    def copy():
        assert lib.ctc_amd_probe_copy(dst.data_ptr(), x32.data_ptr(), nbytes, st) == 0, lib.ctc_amd_last_error()

    for _ in range(a.warmup):
        copy()
    tc = np.asarray([timed(copy) for _ in range(a.steps)])
    rate = 2 * nbytes / (np.median(tc) * 1e-6)  # bytes / s, both directions
    del dst

    lines = [f"# Greedy decoding call beside the torch composition log_softmax(x, -1).max(-1): B={B} T={T} V={V}, full-length utterances",
             "", f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call, "
             "the two alternating; microseconds, median (minimum).  The decoding call is both of its launches (row stage and collapse, "
             "all six outputs); the composition is the row stage's equivalent only.",
             f"ctc_amd_probe_copy of {nbytes / 1e6:.0f} MB: {np.median(tc):.1f} ({tc.min():.1f}) us = {rate / 1e12:.2f} TB/s read + write."]
    if a.note:
        lines.append(a.note)
    lines += ["", "| lattice | input | decoding call | torch composition | ratio | read-once yardstick (8 TB/s) | fraction of the yardstick | the same bytes at the copy rate |",
              "|---|---|---|---|---|---|---|---|"]
    worst = {}
    for kind_name, kind in ops.KINDS.items():
        for what, wrt, x in (("float32 logits", 0, x32), ("bfloat16 logits", 0, x32.to(torch.bfloat16)),
                             ("float32 log-probabilities", 1, torch.log_softmax(x32, 2))):
            dt = ops._DTYPES[x.dtype]

            def decode():
                rc = lib.ctc_amd_greedy_decode(kind, wrt, x.data_ptr(), dt, x.stride(0), x.stride(1), tl.data_ptr(), 0, B, T, V,
                                               score.data_ptr(), tokens.data_ptr(), labels.data_ptr(), length.data_ptr(),
                                               frames.data_ptr(), label_score.data_ptr(), ws.data_ptr(), ws.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            res = {}

            def compose():
                res["v"] = (x if wrt else torch.log_softmax(x, -1)).max(-1)

            for _ in range(a.warmup):
                decode(); compose()
            torch.cuda.synchronize()
            td, tt = [], []
            for _ in range(a.steps):
                td.append(timed(decode)); tt.append(timed(compose))
            td, tt = np.asarray(td), np.asarray(tt)
            # the two agree: same tokens wherever the row maximum is unique, same score
            val, idx = res["v"]
            same = (idx.to(torch.int32) == tokens).float().mean().item()
            assert same > (0.5 if x.dtype == torch.bfloat16 else 0.999), same  # (bfloat16: ties at the maximum, torch's tie rule is its own)
            ref = val.double().sum(1)
            rel = 1e-2 if x.dtype == torch.bfloat16 else 1e-4  # (torch rounds the bfloat16 log-probabilities to bfloat16)
            assert bool(((score.double() - ref).abs() <= 1e-2 + rel * ref.abs()).all()), (score[:4], ref[:4])
            assert int(length.min()) > 0 and int(length.max()) < T
            yard = B * T * V * x.element_size() / HBM_PEAK * 1e6
            at_copy = B * T * V * x.element_size() / rate * 1e6
            lines.append(f"| {kind_name} | {what} | {np.median(td):.1f} ({td.min():.1f}) | {np.median(tt):.1f} ({tt.min():.1f}) | "
                         f"{np.median(td) / np.median(tt):.2f} | {yard:.1f} | {yard / np.median(td):.2f} | {at_copy:.1f} |")
            if wrt == 0:
                worst[(kind_name, what)] = (np.median(td), np.median(tt))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    for key, (d, t) in worst.items():
        assert d <= t, f"{key}: the decoding call ({d:.1f} us) is slower than the torch composition ({t:.1f} us)"


if __name__ == "__main__":
    main()
