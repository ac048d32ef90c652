"""Time of the optional-wildcard calls (ctc_amd_optional_wildcard_loss_grad / _label_posterior) beside the mandatory-wildcard calls
they extend, in the manner of wildcard_loss_time.py.

Warm launches timed with device events (one pair of events around each measured item, the items alternating in a fixed order), at
the north-star shape B=256 T=1000 U=128 V=256 unless told otherwise, both lattices, float32 and bfloat16 logits.  Per item the
loss alone, the loss with its gradient and the label posteriors:
  existing   the existing calls, mandatory wildcards at both ends of every label and one in the middle
  optional   the new calls on the same labels with those three made optional
  stc        the new calls on the STC pattern: an optional wildcard at every even position
The whole measurement is repeated `--repeats` times in the same process; the spread between the repeats' medians is printed beside
the figures.  The script asserts nothing about time: numbers for profiles/optional_wildcard_time.md and DESIGN.md section 5.26.
Needs a GPU (there is no CPU path)."""
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
    assert torch.cuda.is_available(), "optional_wildcard_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    plain = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    wild, opt, stc = plain.clone(), plain.clone(), plain.clone()
    stc[:, 0::2] = _lib.OPTIONAL_WILDCARD
    for b in range(B):
        L = int(ll[b])
        for i in (0, L - 1, L // 2):
            wild[b, i] = _lib.WILDCARD
            opt[b, i] = _lib.OPTIONAL_WILDCARD
    labels = {"existing": wild.to(dev), "optional": opt.to(dev), "stc": stc.to(dev)}
    ll = ll.to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    loss = {k: torch.empty(B, device=dev) for k in labels}
    post, blk = torch.empty((B, T, U), device=dev), torch.empty((B, T), device=dev)
    dur, exf = torch.empty((B, U), device=dev), torch.empty((B, U), device=dev)

    rows = {}  # (lattice, input, labels, item) -> [median of every repeat], [minimum of every repeat]
    for kind_name, kind in ops.KINDS.items():
        for what, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
            dt = ops._DTYPES[x.dtype]
            n = _lib.wildcard_loss_workspace_bytes(kind, B, T, V, U)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            grad = torch.empty_like(x)

            def loss_call(which, with_grad):
                fn = lib.ctc_amd_wildcard_loss_grad if which == "existing" else lib.ctc_amd_optional_wildcard_loss_grad
                rc = fn(kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), labels[which].data_ptr(), U, ll.data_ptr(),
                        tl.data_ptr(), 0, 0.0, B, T, V, U, None, loss[which].data_ptr(), grad.data_ptr() if with_grad else None, dt,
                        T * V, V, ws.data_ptr() if with_grad else None, n if with_grad else 0, st)
                assert rc == 0, lib.ctc_amd_last_error()

            def post_call(which):
                fn = lib.ctc_amd_label_posterior if which == "existing" else lib.ctc_amd_optional_wildcard_label_posterior
                rc = fn(kind, _lib.WRT_LOGITS, x.data_ptr(), dt, x.stride(0), x.stride(1), labels[which].data_ptr(), U, ll.data_ptr(),
                        tl.data_ptr(), 0, 0.0, B, T, V, U, loss[which].data_ptr(), post.data_ptr(), blk.data_ptr(), dur.data_ptr(),
                        exf.data_ptr(), ws.data_ptr(), n, st)
                assert rc == 0, lib.ctc_amd_last_error()

            items = []
            for which in labels:
                items += [((which, "loss only"), lambda w=which: loss_call(w, False)),
                          ((which, "loss + gradient"), lambda w=which: loss_call(w, True)),
                          ((which, "label posteriors"), lambda w=which: post_call(w))]
            for _ in range(a.warmup):
                for _, fn in items:
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                t = {name: [] for name, _ in items}
                for _ in range(a.steps):
                    for name, fn in items:
                        t[name].append(timed(fn))
                for name, v in t.items():
                    med, mn = rows.setdefault((kind_name, what) + name, ([], []))
                    med.append(float(np.median(v))); mn.append(float(np.min(v)))
            assert all(bool(torch.isfinite(v).all()) for v in loss.values())
            del ws, grad

    lines = [f"# Optional wildcards beside the mandatory-wildcard calls: B={B} T={T} U={U} V={V}, full-length utterances, "
             f"label_length in [{U // 2}, {U}]", "",
             "existing: the existing calls, wildcards at both ends and one in the middle; optional: the new calls, those three made "
             "optional; stc: the new calls, an optional wildcard at every even position", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every item, the items alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| lattice | logits | labels | item | time | against the existing call |", "|---|---|---|---|---|---|"]
    for (kind_name, what, which, item), (med, mn) in rows.items():
        ref = float(np.median(rows[(kind_name, what, "existing", item)][0]))
        m = float(np.median(med))
        lines.append(f"| {kind_name} | {what} | {which} | {item} | {m:.1f} ({min(med):.1f} .. {max(med):.1f}; {min(mn):.1f}) | {m / ref:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
