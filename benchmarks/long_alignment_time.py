"""Time of the tiled long-form alignment call (ctc_amd_long_best_path), in the manner of benchmarks/alignment_time.py.

Warm calls timed with device events (one pair of events around each call: K + J - 1 tile launches, the trace and the per-label
kernel), float32 logits.  Every row is one (B, T, U, frames_per_tile); with --compare and U <= 1024 the whole-utterance call
(ctc_amd_best_path) runs on the same buffers, alternating.  "tile time" is the call's time divided by the K + J - 1 diagonals: if
time grows with the diagonals and not with the K * J tiles, it stays put as the shape grows.  No gate: numbers for
profiles/long_alignment_time.md and DESIGN.md section 5.18.  Needs a GPU (there is no CPU path).

    python benchmarks/long_alignment_time.py --shape 1,30000,8192,0 --shape 8,30000,8192,0 --shape 1,8192,1024,0 --compare \\
        --out profiles/long_alignment_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="B,T,U,frames_per_tile (0: the default); may be given several times")
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--kind", default="classic", choices=list(ops.KINDS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compare", action="store_true", help="also time ctc_amd_best_path where U <= 1024")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_alignment_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192, 0)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    kind, V = ops.KINDS[a.kind], a.V
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Tiled long-form alignment: {a.kind} lattice, V={V}, float32 logits, full-length utterances, label_length = U", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call; "
             "microseconds, median (minimum)", "",
             "| B | T | U | frames_per_tile | K x J | launches | tiled call | per diagonal | whole-utterance call | ratio |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U, tf in shapes:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn((B, T, V), generator=g).to(dev)
        labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(dev)
        ll = torch.full((B,), U, dtype=torch.int32, device=dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        score, score0 = torch.empty(B, device=dev), torch.empty(B, device=dev)
        tokens, index, tokens0, index0 = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(4))
        first, last = (torch.empty((B, U), dtype=torch.int32, device=dev) for _ in range(2))
        ws = torch.empty(max(_lib.long_best_path_workspace_bytes(kind, B, T, V, U, tf), 1), dtype=torch.uint8, device=dev)
        common_ex = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0, B, T, V, U)
        TF = tf or _lib.LONG_FRAMES_DEFAULT
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))

        def tiled():
            rc = lib.ctc_amd_long_best_path(*common_ex, tf, score.data_ptr(), tokens.data_ptr(), index.data_ptr(), first.data_ptr(),
                                            last.data_ptr(), ws.data_ptr(), ws.numel(), st)
            assert rc == 0, lib.ctc_amd_last_error()

        whole = None
        if a.compare and U <= 1024:
            ws0 = torch.empty(max(_lib.best_path_workspace_bytes(kind, B, T, V, U), 1), dtype=torch.uint8, device=dev)

            def whole():
                rc = lib.ctc_amd_best_path(*common_ex, score0.data_ptr(), tokens0.data_ptr(), index0.data_ptr(), ws0.data_ptr(), ws0.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

        for _ in range(a.warmup):
            tiled()
            if whole:
                whole()
        torch.cuda.synchronize()
        tt, tw = [], []
        for _ in range(a.steps):
            tt.append(timed(tiled))
            if whole:
                tw.append(timed(whole))
        tt = np.asarray(tt)
        assert torch.isfinite(score).all()
        cmp_text, ratio = "-", "-"
        if whole:
            tw = np.asarray(tw)
            assert torch.equal(tokens, tokens0) and torch.equal(index, index0), "the two calls disagree on the path"
            cmp_text, ratio = f"{np.median(tw):.0f} ({tw.min():.0f})", f"{np.median(tt) / np.median(tw):.2f}"
        lines.append(f"| {B} | {T} | {U} | {TF} | {K} x {J} | {K + J - 1} + 2 | {np.median(tt):.0f} ({tt.min():.0f}) | "
                     f"{np.median(tt) / (K + J - 1):.1f} | {cmp_text} | {ratio} |")
        print(lines[-1], flush=True)
        del x, ws
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
