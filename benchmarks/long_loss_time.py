"""Time of the tiled long-form CTC loss and gradient (ctc_amd_long_wildcard_loss_grad), in the manner of
benchmarks/long_wildcard_alignment_time.py.

Warm calls timed with device events (one pair of events around each call), float32 logits, full-length utterances.  Labels: random
tokens with a wildcard at both ends and one in the middle of every label block.  Every row is one (lattice, B, T, U) at the default
frames_per_tile and shows
  forward        the call with grad = NULL: the alpha tiles and the finish kernel;
  with gradient  the call with a gradient: the same, the beta tiles and the row stage;
  best path      ctc_amd_long_wildcard_best_path without per-label outputs on the same inputs (the max-plus tile on the same grid);
  one wavefront  at U <= 1024, ctc_amd_wildcard_loss_grad on the same inputs, forward and with a gradient,
the calls alternating; median and (minimum - maximum) of the repeats.  No gate: numbers for profiles/long_loss_time.md and DESIGN.md
section 5.20.  Needs a GPU.

    python benchmarks/long_loss_time.py --shape 1,30000,8192 --shape 8,30000,8192 --shape 1,8192,1024 --out profiles/long_loss_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

EXPECTATION = """Expectations, written before the numbers (none of them had been measured):
(a) the forward time grows with the K + J - 1 diagonals, not with the K x J tiles; per diagonal it is above the 134 us per 128
    frames of the best-path tile, because the sum-product step has two exp2 and one log2 per source where the max-plus step has a
    compare -- by how much is not known;
(b) at U = 1024 the tiled forward costs about what ctc_amd_wildcard_loss_grad's does (the tiled alignment paid 1.06 x); for the
    gradient nobody knows;
(c) B = 8 costs about what B = 1 does while a diagonal is short of workgroups."""


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
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "long_loss_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192), (8, 30000, 8192), (1, 8192, 1024)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, tf = a.V, 0
    TF = _lib.LONG_FRAMES_DEFAULT
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Tiled long-form CTC loss and gradient: V={V}, float32 logits, frames_per_tile={TF}, full-length utterances", "",
             EXPECTATION, "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call; "
             "microseconds, median (minimum - maximum)", "",
             "| lattice | B | T | U | K x J | workspace with gradient, bytes | forward | per diagonal | with gradient | beta tiles + row stage "
             "(difference) | best path | forward / best path | one wavefront forward | tiled / one wavefront | one wavefront with gradient | "
             "tiled / one wavefront |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in shapes:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn((B, T, V), generator=g).to(dev)
        lab = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
        wild = sorted({0, U - 1} | {k * 1024 + 512 for k in range(-(-U // 1024)) if k * 1024 + 512 < U})
        lab[:, wild] = _lib.WILDCARD
        labels = lab.to(dev)
        ll = torch.full((B,), U, dtype=torch.int32, device=dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        for kind_name, kind in ops.KINDS.items():
            loss, loss_g, loss1, loss1_g, score = (torch.empty(B, device=dev) for _ in range(5))
            grad = torch.empty((B, T, V), device=dev)
            tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
            n = _lib.long_wildcard_loss_workspace_bytes(kind, B, T, V, U, tf, True)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            wsa = torch.empty(max(_lib.long_wildcard_best_path_workspace_bytes(kind, B, T, V, U, tf), 1), dtype=torch.uint8, device=dev)
            head = (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), labels.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)

            def tiled(out, gr):
                def fn():
                    rc = lib.ctc_amd_long_wildcard_loss_grad(*head, 0.0, B, T, V, U, tf, None, out.data_ptr(), gr.data_ptr() if gr is not None else None,
                                                             _lib.F32, T * V, V, ws.data_ptr(), ws.numel(), st)
                    assert rc == 0, lib.ctc_amd_last_error()
                return fn

            def best_path():
                rc = lib.ctc_amd_long_wildcard_best_path(*head, B, T, V, U, tf, score.data_ptr(), tokens.data_ptr(), None, None, None, None,
                                                         wsa.data_ptr(), wsa.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            calls = {"fwd": tiled(loss, None), "grad": tiled(loss_g, grad), "path": best_path}
            if U <= 1024:
                grad1 = torch.empty((B, T, V), device=dev)
                ws1 = torch.empty(max(_lib.wildcard_loss_workspace_bytes(kind, B, T, V, U, True), 1), dtype=torch.uint8, device=dev)

                def one(out, gr):
                    def fn():
                        rc = lib.ctc_amd_wildcard_loss_grad(*head, 0.0, B, T, V, U, None, out.data_ptr(), gr.data_ptr() if gr is not None else None,
                                                            _lib.F32, T * V, V, ws1.data_ptr(), ws1.numel(), st)
                        assert rc == 0, lib.ctc_amd_last_error()
                    return fn
                calls["one_fwd"], calls["one_grad"] = one(loss1, None), one(loss1_g, grad1)
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in calls}
            for _ in range(a.steps):
                for name, fn in calls.items():
                    times[name].append(timed(fn))
            torch.cuda.synchronize()
            assert torch.isfinite(loss).all() and torch.equal(loss, loss_g) and torch.isfinite(grad).all()
            if "one_fwd" in calls:
                assert float((loss - loss1).abs().max()) <= 1e-4 + 1e-6 * float(loss.abs().max()), "the two calls disagree"
                assert float((grad - grad1).abs().max()) <= 1e-4, "the two gradients disagree"
            t = {name: np.asarray(v) for name, v in times.items()}
            med = {name: float(np.median(v)) for name, v in t.items()}
            cell = {name: f"{med[name]:.0f} ({t[name].min():.0f} - {t[name].max():.0f})" for name in t}
            ratio = {k: f"{med[k2] / med[k]:.3f}" if k in med else "-" for k, k2 in (("one_fwd", "fwd"), ("one_grad", "grad"))}
            lines.append(f"| {kind_name} | {B} | {T} | {U} | {K} x {J} | {n} | {cell['fwd']} | {med['fwd'] / (K + J - 1):.1f} | {cell['grad']} | "
                         f"{med['grad'] - med['fwd']:.0f} | {cell['path']} | {med['fwd'] / med['path']:.3f} | {cell.get('one_fwd', '-')} | "
                         f"{ratio['one_fwd']} | {cell.get('one_grad', '-')} | {ratio['one_grad']} |")
            print(lines[-1], flush=True)
            del ws, wsa, grad
        del x
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
