"""Time of the tiled long-form alignment with wildcard labels (ctc_amd_long_wildcard_best_path), in the manner of
benchmarks/long_alignment_time.py.

Warm calls timed with device events (one pair of events around each call), float32 logits, full-length utterances.  Labels:
random tokens with a wildcard at both ends and one in the middle of every label block.  Every row is one (lattice, B, T, U) at the
default frames_per_tile and shows
  all outputs      the call with label_index, first_frame, last_frame and label_score;
  no label_score   the same without label_score (one launch less);
  path only        without any per-label output (two launches less);
  plain tiled      ctc_amd_long_best_path on the same logits with the same labels minus the wildcards;
  whole-utterance  at U <= 1024, ctc_amd_wildcard_best_path on the same inputs,
the calls alternating.  No gate: numbers for profiles/long_wildcard_alignment_time.md and DESIGN.md section 5.19.  Needs a GPU.

    python benchmarks/long_wildcard_alignment_time.py --shape 1,30000,8192 --shape 8,30000,8192 --shape 1,8192,1024 \\
        --out profiles/long_wildcard_alignment_time.md"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tf_seq2seq_losses_amd import _lib, ops  # noqa: E402

EXPECTATION = """Expectation, written before the numbers.  The tile's chain step is unchanged and the extra row statistics (row maximum, its
index) live in label block 0's producers, which have slack: the time per diagonal should stay close to the plain tiled call's
133-135 us, so `path only` should cost about what `plain tiled` does.  What the call adds should be the back-trace's per-frame
gather (a_t, the token's logit, the frame's log-sum-exp) and the two per-label launches; the whole-utterance wildcard call was
1.42-1.53 x its plain counterpart without saying which part carried that, so `all outputs` against `no label_score` against
`path only` is the split to look at."""


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
    assert torch.cuda.is_available(), "long_wildcard_alignment_time.py needs a GPU"
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] or [(1, 30000, 8192), (8, 30000, 8192), (1, 8192, 1024)]
    lib = _lib.load()
    dev = torch.device("cuda:0")
    V, tf = a.V, 0
    TF = _lib.LONG_FRAMES_DEFAULT
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# Tiled long-form alignment with wildcard labels: V={V}, float32 logits, frames_per_tile={TF}, full-length utterances", "",
             EXPECTATION, "",
             f"device: {torch.cuda.get_device_name(0)}; {a.steps} warm calls each after {a.warmup}, device events around every call; "
             "microseconds, median (minimum)", "",
             "| lattice | B | T | U | K x J | wildcards | all outputs | no label_score | path only | per diagonal (path only) | plain tiled | "
             "path only / plain | all / plain | whole-utterance wildcard call |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B, T, U in shapes:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn((B, T, V), generator=g).to(dev)
        lab = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32)
        wild = sorted({0, U - 1} | {k * 1024 + 512 for k in range(-(-U // 1024)) if k * 1024 + 512 < U})
        keep = torch.ones(U, dtype=torch.bool)
        keep[wild] = False
        plain_lab = lab[:, keep].contiguous().to(dev)  # the same labels minus the wildcards
        lab[:, wild] = _lib.WILDCARD
        labels = lab.to(dev)
        U0 = int(plain_lab.shape[1])
        ll = torch.full((B,), U, dtype=torch.int32, device=dev)
        ll0 = torch.full((B,), U0, dtype=torch.int32, device=dev)
        tl = torch.full((B,), T, dtype=torch.int32, device=dev)
        K, J = max(1, -(-U // 1024)), max(1, -(-T // TF))
        for kind_name, kind in ops.KINDS.items():
            score, score0, score1 = (torch.empty(B, device=dev) for _ in range(3))
            tokens, index, tokens0, index0, tokens1, index1 = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(6))
            first, last, first0, last0, first1, last1 = (torch.empty((B, U), dtype=torch.int32, device=dev) for _ in range(6))
            ls, ls1 = (torch.empty((B, U), device=dev) for _ in range(2))
            ws = torch.empty(max(_lib.long_wildcard_best_path_workspace_bytes(kind, B, T, V, U, tf), 1), dtype=torch.uint8, device=dev)
            ws0 = torch.empty(max(_lib.long_best_path_workspace_bytes(kind, B, T, V, U0, tf), 1), dtype=torch.uint8, device=dev)

            def head(lb, width, lengths):
                return (kind, 0, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), lb.data_ptr(), width, lengths.data_ptr(), tl.data_ptr(),
                        0, B, T, V, width)

            def wild_call(fr, sc):
                def fn():
                    rc = lib.ctc_amd_long_wildcard_best_path(*head(labels, U, ll), tf, score.data_ptr(), tokens.data_ptr(), index.data_ptr(),
                                                             first.data_ptr() if fr else None, last.data_ptr() if fr else None,
                                                             ls.data_ptr() if sc else None, ws.data_ptr(), ws.numel(), st)
                    assert rc == 0, lib.ctc_amd_last_error()
                return fn

            def plain():
                rc = lib.ctc_amd_long_best_path(*head(plain_lab, U0, ll0), tf, score0.data_ptr(), tokens0.data_ptr(), index0.data_ptr(),
                                                first0.data_ptr(), last0.data_ptr(), ws0.data_ptr(), ws0.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            calls = {"all": wild_call(True, True), "no_score": wild_call(True, False), "path": wild_call(False, False), "plain": plain}
            if U <= 1024:
                ws1 = torch.empty(max(_lib.wildcard_best_path_workspace_bytes(kind, B, T, V, U), 1), dtype=torch.uint8, device=dev)

                def whole():
                    rc = lib.ctc_amd_wildcard_best_path(*head(labels, U, ll), score1.data_ptr(), tokens1.data_ptr(), index1.data_ptr(),
                                                        first1.data_ptr(), last1.data_ptr(), ls1.data_ptr(), ws1.data_ptr(), ws1.numel(), st)
                    assert rc == 0, lib.ctc_amd_last_error()
                calls["whole"] = whole
            for _ in range(a.warmup):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in calls}
            for _ in range(a.steps):
                for name, fn in calls.items():
                    times[name].append(timed(fn))
            calls["all"]()  # (the last wildcard call above was "path": leave every output of one call in place)
            torch.cuda.synchronize()
            assert torch.isfinite(score).all() and torch.isfinite(score0).all()
            if "whole" in calls:
                assert torch.equal(tokens, tokens1) and torch.equal(index, index1) and torch.equal(first, first1), "the two calls disagree"
            t = {name: np.asarray(v) for name, v in times.items()}
            med = {name: float(np.median(v)) for name, v in t.items()}
            cell = {name: f"{med[name]:.0f} ({t[name].min():.0f})" for name in t}
            lines.append(f"| {kind_name} | {B} | {T} | {U} | {K} x {J} | {len(wild)} | {cell['all']} | {cell['no_score']} | {cell['path']} | "
                         f"{med['path'] / (K + J - 1):.1f} | {cell['plain']} | {med['path'] / med['plain']:.3f} | "
                         f"{med['all'] / med['plain']:.3f} | {cell.get('whole', '-')} |")
            print(lines[-1], flush=True)
            del ws, ws0
        del x
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
