"""Time of the edit-distance call (ctc_amd_edit_distance: one launch) beside the two routes a user has without it, and of one
MWER step (classic_ctc_mwer_loss forward + backward) beside the sum of its parts, in the manner of nbest_loss_time.py.

    edit_distance_time.py --out profiles/edit_distance_time.md        on the GPU (there is no CPU path)

Edit distance: B=256, N in {1, 8, 32}, hypothesis and reference lengths near 128 (96..128, tensors 128 wide) and near 32 (24..32,
tensors 32 wide), tokens from 30 symbols with every hypothesis a corrupted copy of its reference (about 15% edits).
  route (a)  hypotheses and lengths .cpu(), the dynamic programme of tests/tools/edit_oracle.py on the host (its row-at-a-time NumPy
             form, the faster of the two), the result back .to(device): host wall time, end to end, the copies included;
  route (b)  the same recurrence in torch on the device: one row step per hypothesis token for all pairs at once, the in-row
             dependence resolved with torch.cummin (cur[j] = j + min_{k <= j} (c[k] - k)); device events around the whole loop
             (its launches are issued back to back, so this is also its host time when the host is the slower side).
MWER: B=256 T=1000 V=256, labels of 64..128 tokens, logits peaked (+8) along an alignment of the labels over N(0, 1) noise, so that
the beam's hypotheses are near the labels as a trained model's are; beam_width = 16, top_k = 16, nbest = 8; max_label_length = the
longest hypothesis (looked up once, outside the timed region).  Parts: the beam search, the edit distance, the N-best loss forward,
its gradient call.
Device time: events around every call on a warm device (around `--reps` back-to-back calls of the new one, per call), `--steps`
timings after `--warmup`; median, minimum and spread.  No threshold is asserted: the table is the result."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (1, 8, 32)
LENGTHS = ((128, 96), (32, 24))  # (width = longest, shortest)


def stats(us):
    us = np.asarray(us)
    return float(np.median(us)), float(us.min()), float((us.max() - us.min()) / np.median(us))


def cell(us):
    med, lo, spread = stats(us)
    return f"{med:.0f} ({lo:.0f}, {100 * spread:.0f}%)"


def corrupted(rng, ref, rl, N, width, alphabet):
    """[B, N, width] hypotheses: every reference with about 5% each of substitutions, deletions and insertions; their lengths."""
    B = ref.shape[0]
    hyp = np.full((B, N, width), -1, np.int32)
    hl = np.zeros((B, N), np.int32)
    u = rng.random((B, N, width))
    other = rng.integers(0, alphabet, (2, B, N, width)).astype(np.int32)
    for b in range(B):
        for n in range(N):
            r = int(rl[b])
            kept = np.nonzero(u[b, n, :r] >= 0.05)[0]
            base = np.where(u[b, n, kept] < 0.10, other[0, b, n, kept], ref[b, kept])
            grow = u[b, n, kept] > 0.95
            out = np.insert(base, np.nonzero(grow)[0] + 1, other[1, b, n, kept][grow])[:width]
            hyp[b, n, :len(out)] = out
            hl[b, n] = len(out)
    return hyp, hl


def torch_route(hyp, hl, ref, rl):
    """Route (b): distance[B, N] by one row step per hypothesis token, all pairs at once."""
    import torch
    B, N, W = hyp.shape
    R = ref.shape[1]
    P = B * N
    hyp, hl = hyp.reshape(P, W), hl.reshape(P)
    refp = ref.repeat_interleave(N, 0)
    rlp = rl.repeat_interleave(N, 0).long()
    j = torch.arange(R + 1, device=hyp.device, dtype=torch.int32)
    prev = j.repeat(P, 1)
    for i in range(W):
        c = torch.empty_like(prev)
        c[:, 0] = i + 1
        c[:, 1:] = torch.minimum(prev[:, 1:] + 1, prev[:, :-1] + (refp != hyp[:, i:i + 1]).to(torch.int32))
        cur = torch.cummin(c - j, dim=1).values + j
        prev = torch.where((hl > i)[:, None], cur, prev)
    return prev.gather(1, rlp.clamp(0, R)[:, None]).reshape(B, N)


def measure_edit(a, dev):
    import torch
    from tests.tools import edit_oracle as E
    from tf_seq2seq_losses_amd import ops

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # microseconds per call

    rng = np.random.default_rng(0)
    rows = []
    for width, low in LENGTHS:
        ref_h = rng.integers(0, 30, (a.B, width)).astype(np.int32)
        rl_h = rng.integers(low, width + 1, a.B).astype(np.int32)
        for N in NS:
            hyp_h, hl_h = corrupted(rng, ref_h, rl_h, N, width, 30)
            hyp, hl, ref, rl = (torch.tensor(t, device=dev) for t in (hyp_h, hl_h, ref_h, rl_h))
            out = {}

            def new():
                out["new"] = ops.edit_distance(hyp, hl, ref, rl)

            def route_b():
                out["b"] = torch_route(hyp, hl, ref, rl)

            def route_a():
                t0 = time.perf_counter()
                d = E.edit_distances(hyp.cpu().numpy(), hl.cpu().numpy(), ref.cpu().numpy(), rl.cpu().numpy(), one=E.edit_distance_rows)
                out["a"] = torch.from_numpy(d).to(dev)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e6

            for _ in range(a.warmup):
                new(); route_b()
            torch.cuda.synchronize()
            t_new, t_b = [], []
            for _ in range(a.steps):
                t_new.append(timed(new, a.reps)); t_b.append(timed(route_b))
            t_a = [route_a() for _ in range(a.host_steps)]
            assert torch.equal(out["new"], out["a"]) and torch.equal(out["new"], out["b"].to(torch.int32))
            rows.append(dict(width=width, N=N, new=t_new, a=t_a, b=t_b, mean=float(out["new"].float().mean())))
            print(f"lengths {low}..{width} N={N}: new {cell(t_new)} us, route a {cell(t_a)} us, route b {cell(t_b)} us", flush=True)
    return rows


def measure_mwer(a, dev):
    import torch
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib, ops

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    B, T, V, U, N = a.B, a.T, a.V, a.U, 8
    rng = np.random.default_rng(1)
    labels_h = rng.integers(1, V, (B, U)).astype(np.int32)
    ll_h = rng.integers(U // 2, U + 1, B).astype(np.int32)
    path = np.zeros((B, T), np.int64)
    for b in range(B):
        stride = T // int(ll_h[b])
        at = np.arange(int(ll_h[b])) * stride
        path[b, at] = labels_h[b, :ll_h[b]]
        path[b, at + 1] = labels_h[b, :ll_h[b]]
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn((B, T, V), generator=g)
    x.scatter_add_(2, torch.from_numpy(path)[:, :, None], torch.full((B, T, 1), 8.0))
    x = x.to(dev).requires_grad_(True)
    labels, ll = torch.tensor(labels_h, device=dev), torch.tensor(ll_h, device=dev)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    kw = dict(beam_width=16, top_k=16, nbest=N)
    beam = ctc.classic_ctc_beam_search(x, tl, 0, **kw)
    longest = int(beam.label_length.max())
    risk0 = ops.edit_distance(beam.labels, beam.label_length, labels, ll)
    weight = torch.randn((B, N), device=dev)
    k = ops.KINDS["classic"]

    def whole():
        x.grad = None
        ctc.classic_ctc_mwer_loss(labels, x, ll, tl, 0, max_label_length=longest, **kw).loss.sum().backward()

    parts = {
        "beam search": lambda: ctc.classic_ctc_beam_search(x, tl, 0, **kw),
        "edit distance": lambda: ops.edit_distance(beam.labels, beam.label_length, labels, ll),
        "N-best loss forward": lambda: ops.nbest_loss(k, _lib.WRT_LOGITS, beam.labels, x.detach(), beam.label_length, tl, 0, longest),
        "N-best loss gradient": lambda: ops.nbest_loss_grad(k, _lib.WRT_LOGITS, beam.labels, x.detach(), beam.label_length, tl, 0, weight, longest),
    }
    for _ in range(a.warmup):
        whole()
        for fn in parts.values():
            fn()
    torch.cuda.synchronize()
    t_whole, t_parts = [], {name: [] for name in parts}
    for _ in range(a.steps):
        t_whole.append(timed(whole))
        for name, fn in parts.items():
            t_parts[name].append(timed(fn))
    print(f"MWER step: {cell(t_whole)} us; parts " + ", ".join(f"{n} {cell(t)}" for n, t in t_parts.items()), flush=True)
    return dict(whole=t_whole, parts=t_parts, longest=longest, mean_risk=float(risk0.float().mean()),
                mean_len=float(beam.label_length.float().mean()))


def table(a, dev_name, rows, mwer):
    lines = [f"# Edit distance of N-best lists and one MWER step: B={a.B}", "",
             f"device: {dev_name}; {a.steps} warm calls each after {a.warmup}, the calls of a line alternating; microseconds: median (minimum, "
             f"spread = (max - min) / median).  `ctc_amd_edit_distance` by device events around {a.reps} calls issued back to back (time per call: a single call of a few tens of "
             f"microseconds is timed no better than the events themselves), route (b) by device events around one call, route (a) by the host's "
             f"clock around copy out + dynamic programme + copy back ({a.host_steps} call each).  The three agree on every distance "
             "(asserted).  Expectation before measuring: one launch of h + 63 short steps beats both routes.", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| lengths | N | mean distance | ctc_amd_edit_distance | (a) .cpu() + host DP | (b) torch row steps + cummin | new / (a) | new / (b) | expectation |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        n, ta, tb = stats(r["new"])[0], stats(r["a"])[0], stats(r["b"])[0]
        held = "held" if n < ta and n < tb else "did NOT hold"
        lines.append(f"| near {r['width']} | {r['N']} | {r['mean']:.1f} | {cell(r['new'])} | {cell(r['a'])} | {cell(r['b'])} | {n / ta:.5f} | {n / tb:.4f} | {held} |")
    if mwer is not None:
        total = sum(stats(t)[0] for t in mwer["parts"].values())
        w = stats(mwer["whole"])[0]
        lines += ["", f"## One MWER step: classic_ctc_mwer_loss forward + backward, B={a.B} T={a.T} V={a.V}, labels of {a.U // 2}..{a.U} tokens, nbest 8", "",
                  f"Hypotheses of the function's own beam search: mean length {mwer['mean_len']:.1f}, longest {mwer['longest']} (passed as "
                  f"max_label_length), mean edit distance to the labels {mwer['mean_risk']:.2f}.", "",
                  "| what | time |", "|---|---|",
                  f"| classic_ctc_mwer_loss(...).loss.sum().backward() | {cell(mwer['whole'])} |"]
        lines += [f"| part: {name} | {cell(t)} |" for name, t in mwer["parts"].items()]
        lines += [f"| sum of the parts' medians | {total:.0f} |", f"| whole / sum of parts | {w / total:.3f} |", "",
                  f"The edit distance is {100 * stats(mwer['parts']['edit distance'])[0] / w:.2f}% of the step.  Beside its parts the whole holds "
                  "the torch operations of the posterior and the estimator, and their backward."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="calls of ctc_amd_edit_distance between one pair of events")
    ap.add_argument("--host-steps", type=int, default=1, help="calls of route (a), which takes seconds")
    ap.add_argument("--no-mwer", action="store_true")
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "edit_distance_time.py needs a GPU"
    dev = torch.device("cuda:0")
    rows = measure_edit(a, dev)
    mwer = None if a.no_mwer else measure_mwer(a, dev)
    text = table(a, torch.cuda.get_device_name(0), rows, mwer)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
