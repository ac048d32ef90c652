"""What the exclusion of the following label costs (ctc_amd_star_* beside ctc_amd_wildcard_loss_grad, ctc_amd_label_posterior and
ctc_amd_wildcard_best_path): exclude_next_label off and on, alternating in one process.

Warm launches timed with device events (one pair of events around each measured item, the items alternating in a fixed order), at
B=256 T=1000 U=128 V=256 unless told otherwise, on the inputs of benchmarks/wildcard_loss_time.py (wildcards at both ends of every
label and one in the middle: with the keyword on, the first and the middle one exclude their successor), both lattices, float32 and
bfloat16 logits.  Items: loss only, loss + gradient, label posteriors (with the statistics), alignment.  The whole measurement is
repeated `--repeats` times; the spread between the repeats' medians is printed beside the figures.  The script asserts nothing
about time: numbers for profiles/star_exclusion_time.md and DESIGN.md section 5.29.  Needs a GPU (there is no CPU path)."""
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
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "star_exclusion_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    wild = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    for b in range(B):
        L = int(ll[b])
        wild[b, 0] = wild[b, L - 1] = wild[b, L // 2] = _lib.WILDCARD
    wild, ll = wild.to(dev), ll.to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    f32 = lambda *s: torch.empty(s, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    loss = {k: f32(B) for k in ("off", "on")}
    post = (f32(B, T, U), f32(B, T), f32(B, U), f32(B, U))
    path = (f32(B), i32(B, T), i32(B, T), i32(B, U), i32(B, U), f32(B, U))

    rows = {}  # (lattice, input, item, off / on) -> [median of every repeat], [minimum of every repeat]
    for kind_name, kind in ops.KINDS.items():
        for what, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
            dt = ops._DTYPES[x.dtype]
            n = _lib.wildcard_loss_workspace_bytes(kind, B, T, V, U)
            na = max(_lib.wildcard_best_path_workspace_bytes(kind, B, T, V, U), _lib.star_best_path_workspace_bytes(kind, B, T, V, U))
            ws, wa = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(na, dtype=torch.uint8, device=dev)
            grad = torch.empty_like(x)
            head = (kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), wild.data_ptr(), U, ll.data_ptr(), tl.data_ptr(), 0)

            def loss_call(on, with_grad):
                fn, extra = (lib.ctc_amd_star_loss_grad, (0,)) if on else (lib.ctc_amd_wildcard_loss_grad, ())
                rc = fn(*head, *extra, 0.0, B, T, V, U, None, loss["on" if on else "off"].data_ptr(),
                        grad.data_ptr() if with_grad else None, dt, T * V, V, ws.data_ptr() if with_grad else None,
                        n if with_grad else 0, st)
                assert rc == 0, lib.ctc_amd_last_error()

            def post_call(on):
                fn, extra = (lib.ctc_amd_star_label_posterior, (0,)) if on else (lib.ctc_amd_label_posterior, ())
                rc = fn(*head, *extra, 0.0, B, T, V, U, loss["on" if on else "off"].data_ptr(), *(t.data_ptr() for t in post),
                        ws.data_ptr(), n, st)
                assert rc == 0, lib.ctc_amd_last_error()

            def path_call(on):
                fn, extra = (lib.ctc_amd_star_best_path, (0,)) if on else (lib.ctc_amd_wildcard_best_path, ())
                rc = fn(*head, *extra, B, T, V, U, *(t.data_ptr() for t in path), wa.data_ptr(), na, st)
                assert rc == 0, lib.ctc_amd_last_error()

            items = []
            for name, fn in (("loss only", lambda on: loss_call(on, False)), ("loss + gradient", lambda on: loss_call(on, True)),
                             ("label posteriors", post_call), ("alignment", path_call)):
                for on in (False, True):
                    items.append(((name, "on" if on else "off"), (lambda fn=fn, on=on: fn(on))))
            for _ in range(a.warmup):
                for _, fn in items:
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                t = {key: [] for key, _ in items}
                for _ in range(a.steps):
                    for key, fn in items:
                        t[key].append(timed(fn))
                for key, v in t.items():
                    med, mn = rows.setdefault((kind_name, what) + key, ([], []))
                    med.append(float(np.median(v))); mn.append(float(np.min(v)))
            assert torch.isfinite(loss["off"]).all() and torch.isfinite(loss["on"]).all() and bool((loss["on"] > loss["off"]).all())
            del ws, wa, grad

    lines = [f"# exclude_next_label off and on: B={B} T={T} U={U} V={V}, full-length utterances, label_length in [{U // 2}, {U}], "
             "wildcards at both ends and one in the middle", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every item, the items alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| lattice | logits | item | off | on | on / off |", "|---|---|---|---|---|---|"]
    cell = lambda med, mn: f"{float(np.median(med)):.1f} ({min(med):.1f} .. {max(med):.1f}; {min(mn):.1f})"
    for (kind_name, what, name, state), (med, mn) in rows.items():
        if state == "off":
            med1, mn1 = rows[(kind_name, what, name, "on")]
            lines.append(f"| {kind_name} | {what} | {name} | {cell(med, mn)} | {cell(med1, mn1)} | "
                         f"{float(np.median(med1)) / float(np.median(med)):.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
