"""Time of the wildcard alignment call (ctc_amd_wildcard_best_path) beside the caller-side route it replaces and beside the plain
alignment call (ctc_amd_best_path) on the same logits.

Warm launches timed with device events (one pair of events around each measured item, the items alternating in a fixed order), at
the north-star shape B=256 T=1000 U=128 V=256 unless told otherwise, wildcards at both ends of every label and one in the middle.
  new call           float32 and bfloat16 logits, both lattices
  caller-side route  log_softmax + max + cat + the existing alignment on the float32 [B, T, V + 1] copy with the wildcard mapped to
                     token V: classic and float32 only, because that is all the route can do
  plain alignment    ctc_amd_best_path on the same logits, the wildcards replaced by ordinary labels
The whole measurement is repeated `--repeats` times in the same process; the spread between the repeats' medians is printed beside
the figures.  The script asserts nothing about time: numbers for profiles/wildcard_alignment_time.md and DESIGN.md section 5.15.
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wildcard_alignment_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U, V = a.B, a.T, a.U, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    x32 = torch.randn((B, T, V), generator=g).to(dev)
    plain = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
    ll = torch.randint(U // 2, U + 1, (B,), generator=g, dtype=torch.int32)
    wild = plain.clone()
    for b in range(B):
        L = int(ll[b])
        wild[b, 0] = wild[b, L - 1] = wild[b, L // 2] = _lib.WILDCARD
    mapped = torch.where(wild == _lib.WILDCARD, torch.full_like(wild, V), wild)
    plain, wild, mapped, ll = plain.to(dev), wild.to(dev), mapped.to(dev), ll.to(dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    score, score_r, score_p = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    tokens, index = torch.empty((B, T), **i32), torch.empty((B, T), **i32)
    first, last, lscore = torch.empty((B, U), **i32), torch.empty((B, U), **i32), torch.empty((B, U), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def ws(n):
        return torch.empty(max(n, 1), dtype=torch.uint8, device=dev)

    rows = {}  # (lattice, input, item) -> [median of every repeat], [minimum of every repeat]
    for kind_name, kind in ops.KINDS.items():
        for what, x in (("float32", x32), ("bfloat16", x32.to(torch.bfloat16))):
            dt = ops._DTYPES[x.dtype]
            ws_w = ws(_lib.wildcard_best_path_workspace_bytes(kind, B, T, V, U))
            ws_p = ws(_lib.best_path_workspace_bytes(kind, B, T, V, U))
            ws_r = ws(_lib.best_path_workspace_bytes(kind, B, T, V + 1, U))

            def ex(xx, lab, v):
                return (kind, xx.data_ptr(), ops._DTYPES[xx.dtype], xx.stride(0), xx.stride(1), lab.data_ptr(), U, ll.data_ptr(),
                        tl.data_ptr(), 0, B, T, v, U)

            def new_call():
                k, *rest = ex(x, wild, V)
                rc = lib.ctc_amd_wildcard_best_path(k, _lib.WRT_LOGITS, *rest, score.data_ptr(), tokens.data_ptr(), index.data_ptr(),
                                                    first.data_ptr(), last.data_ptr(), lscore.data_ptr(), ws_w.data_ptr(), ws_w.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            def plain_call():
                k, *rest = ex(x, plain, V)
                rc = lib.ctc_amd_best_path(k, _lib.WRT_LOGITS, *rest, score_p.data_ptr(), tokens.data_ptr(), index.data_ptr(),
                                           ws_p.data_ptr(), ws_p.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            def route():
                lp = torch.log_softmax(x, 2)
                e = torch.cat([lp, lp.max(-1, keepdim=True).values], -1)
                k, *rest = ex(e, mapped, V + 1)
                rc = lib.ctc_amd_best_path(k, _lib.WRT_LOGPROBS, *rest, score_r.data_ptr(), tokens.data_ptr(), index.data_ptr(),
                                           ws_r.data_ptr(), ws_r.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            items = [("new call", new_call), ("plain alignment", plain_call)]
            if kind_name == "classic" and dt == _lib.F32:
                items.insert(1, ("caller-side route", route))
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
                    med, mn = rows.setdefault((kind_name, what, name), ([], []))
                    med.append(float(np.median(v))); mn.append(float(np.min(v)))
            assert torch.isfinite(score).all() and torch.isfinite(score_p).all()
            if kind_name == "classic" and dt == _lib.F32:  # the two routes agree (no adjacent wildcards here)
                assert bool(((score - score_r).abs() <= 2e-4 + 2e-6 * score.abs()).all())

    lines = [f"# Wildcard alignment beside the caller-side route and the plain alignment: B={B} T={T} U={U} V={V}, full-length "
             f"utterances, label_length in [{U // 2}, {U}], wildcards at both ends and one in the middle", "",
             f"device: {torch.cuda.get_device_name(0)}; {a.repeats} repeats of {a.steps} warm launches each after {a.warmup}, device "
             "events around every item, the items alternating; microseconds: median of the repeats' medians (lowest .. highest "
             "repeat median; minimum)", "",
             "| lattice | logits | item | time | against the new call |", "|---|---|---|---|---|"]
    for (kind_name, what, name), (med, mn) in rows.items():
        ref = float(np.median(rows[(kind_name, what, "new call")][0]))
        m = float(np.median(med))
        lines.append(f"| {kind_name} | {what} | {name} | {m:.1f} ({min(med):.1f} .. {max(med):.1f}; {min(mn):.1f}) | {m / ref:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
