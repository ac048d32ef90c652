"""Time of the prefix beam search call (ctc_amd_beam_search: both launches) beside the greedy decoding call on the same buffers,
in the manner of decode_time.py, and how it divides between its row stage and its search stage.

Three steps, because a kernel's own time comes from a kernel trace and a call's time must be taken with the profiler off:
  1. `beam_search_time.py --calls CALLS.json`                       on the GPU: warm calls, device events around every call, the
     beam search and the greedy decoding alternating; B=256 T=1000 V=256, blank-biased logits, (W, K) in {(4, 4), (16, 16),
     (64, 32)}, float32 and bfloat16 logits, classic lattice (the lattices differ in one multiply per candidate); and V=1024 with
     (16, 16), where the row stage reads a row once per counting pass (reported, outside the requirement below).
  2. `rocprofv3 --kernel-trace --output-format csv -d DIR -- python beam_search_time.py --calls /dev/null`   the same sequence of
     launches under the profiler: one line per kernel dispatch with its start and end.
  3. `beam_search_time.py --compose CALLS.json TRACE.csv --out profiles/beam_search_time.md`   anywhere: the table.  The
     dispatches are matched to the configurations by their order (every configuration launches warmup + steps times the four
     kernels beam_rows, beam_search, decode_rows, decode_collapse).
One requirement (asserted in step 3): the row stage reads the bytes decode_rows_kernel reads, so it takes at most 1.5 times that
kernel's time in the same run, in every configuration at V=256.  Steps 1 and 2 need a GPU (there is no CPU path).
As measured on the MI355X (profiles/beam_search_time.md) the requirement is NOT met and the assertion fails: 3.8 to 4.5 times at
V=256 (198-257 us against 49-57 us); the table is written before the assertion."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(4, 4), (16, 16), (64, 32)]  # (W, K) at the vocabulary of --V
WIDE_V, WIDE_CONFIG = 1024, (16, 16)     # one more line: a row wider than the 256 tokens the row stage keeps in registers
DTYPES = ["float32", "bfloat16"]
KERNELS = ("beam_rows_kernel", "beam_search_kernel", "decode_rows_kernel", "decode_collapse_kernel")
ROW_STAGE_BOUND = 1.5


def measure(a):
    import torch
    from tf_seq2seq_losses_amd import _lib, ops
    assert torch.cuda.is_available(), "beam_search_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, V = a.B, a.T, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    g_score = torch.empty(B, device=dev)
    g_tokens, g_labels, g_frames = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(3))
    g_length = torch.empty(B, dtype=torch.int32, device=dev)
    g_lscore = torch.empty((B, T), device=dev)
    g_ws = torch.empty(max(_lib.greedy_decode_workspace_bytes(B, T), 1), dtype=torch.uint8, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    rows = []
    for V, name, configs in [(a.V, n, CONFIGS) for n in DTYPES] + [(WIDE_V, n, [WIDE_CONFIG]) for n in DTYPES]:  # (V: of this line)
        x = torch.randn((B, T, V), generator=g).to(dev)
        x[..., 0] += 3.0  # blank-biased, as a trained model's output is
        if name == "bfloat16":
            x = x.to(torch.bfloat16)
        dt = ops._DTYPES[x.dtype]
        for W, K in configs:
            score = torch.empty((B, 1), device=dev)
            labels = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
            length = torch.empty((B, 1), dtype=torch.int32, device=dev)
            ws = torch.empty(_lib.beam_search_workspace_bytes(B, T, V, W, K), dtype=torch.uint8, device=dev)

            def beam():
                rc = lib.ctc_amd_beam_search(0, 0, x.data_ptr(), dt, x.stride(0), x.stride(1), tl.data_ptr(), 0, B, T, V, W, K, 1,
                                             score.data_ptr(), labels.data_ptr(), length.data_ptr(), ws.data_ptr(), ws.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            def greedy():
                rc = lib.ctc_amd_greedy_decode(0, 0, x.data_ptr(), dt, x.stride(0), x.stride(1), tl.data_ptr(), 0, B, T, V,
                                               g_score.data_ptr(), g_tokens.data_ptr(), g_labels.data_ptr(), g_length.data_ptr(),
                                               g_frames.data_ptr(), g_lscore.data_ptr(), g_ws.data_ptr(), g_ws.numel(), st)
                assert rc == 0, lib.ctc_amd_last_error()

            for _ in range(a.warmup):
                beam(); greedy()
            torch.cuda.synchronize()
            tb, tg = [], []
            for _ in range(a.steps):
                tb.append(timed(beam)); tg.append(timed(greedy))
            assert bool(torch.isfinite(score).all()) and int(length.min()) > 0 and int(length.max()) < T  # (both calls did their work)
            rows.append(dict(dtype=name, V=V, W=W, K=K, beam_us=tb, greedy_us=tg))
            del ws
        del x
    return dict(B=B, T=T, V=a.V, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), rows=rows)


def kernel_times(trace_csv):
    """[(kernel, microseconds)] in dispatch order, for the four kernels of the two calls."""
    out = []
    with open(trace_csv, newline="") as f:
        recs = [r for r in csv.DictReader(f)]
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in recs:
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                out.append((k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    return out


def compose(a):
    calls = json.load(open(a.compose[0]))
    disp = kernel_times(a.compose[1])
    B, T, V, steps, warmup = (calls[k] for k in ("B", "T", "V", "steps", "warmup"))
    per = warmup + steps
    assert len(disp) == len(calls["rows"]) * per * 4, (len(disp), len(calls["rows"]), per)
    lines = [f"# Prefix beam search call beside the greedy decoding call: B={B} T={T}, full-length utterances, classic lattice, nbest = 1",
             "", f"device: {calls['device']}; {steps} warm calls each after {warmup}, the two calls alternating on the same logits.  Call times: "
             "device events around every call, profiler off.  Kernel times: a kernel trace of the same sequence of launches in a run of "
             "its own.  Microseconds, median (minimum).  Row stage bound: beam_rows_kernel at most "
             f"{ROW_STAGE_BOUND} x decode_rows_kernel of the same run (asserted for the lines with V={V}; V={WIDE_V} is reported only: rows beyond 256 "
             "tokens are read once per counting pass)."]
    if a.note:
        lines.append(a.note)
    lines += ["", "| input | V | W | K | beam search call | per frame | greedy call | ratio | beam_rows_kernel | decode_rows_kernel | row stage ratio | "
              "beam_search_kernel | search stage per frame |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    worst = []
    for i, row in enumerate(calls["rows"]):
        seg = disp[i * per * 4:(i + 1) * per * 4]
        assert [k for k, _ in seg[:4]] == list(KERNELS), seg[:4]
        t = {k: np.asarray([us for kk, us in seg[warmup * 4:] if kk == k]) for k in KERNELS}
        tb, tg = np.asarray(row["beam_us"]), np.asarray(row["greedy_us"])
        ratio = np.median(t["beam_rows_kernel"]) / np.median(t["decode_rows_kernel"])
        if row["V"] == V:
            worst.append((row["dtype"], row["W"], row["K"], ratio))
        lines.append(f"| {row['dtype']} | {row['V']} | {row['W']} | {row['K']} | {np.median(tb):.0f} ({tb.min():.0f}) | {np.median(tb) / T:.2f} | "
                     f"{np.median(tg):.0f} ({tg.min():.0f}) | {np.median(tb) / np.median(tg):.1f} | "
                     f"{np.median(t['beam_rows_kernel']):.0f} ({t['beam_rows_kernel'].min():.0f}) | "
                     f"{np.median(t['decode_rows_kernel']):.0f} ({t['decode_rows_kernel'].min():.0f}) | {ratio:.2f} | "
                     f"{np.median(t['beam_search_kernel']):.0f} ({t['beam_search_kernel'].min():.0f}) | "
                     f"{np.median(t['beam_search_kernel']) / T:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    for dtype, W, K, ratio in worst:
        assert ratio <= ROW_STAGE_BOUND, f"{dtype} W={W} K={K}: the row stage takes {ratio:.2f} x decode_rows_kernel's time (bound {ROW_STAGE_BOUND})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", default=None, help="measure on the GPU and write the call times to this JSON file")
    ap.add_argument("--compose", nargs=2, metavar=("CALLS.json", "TRACE.csv"), default=None, help="write the table from the two runs")
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.compose:
        return compose(a)
    assert a.calls, "give --calls FILE (on the GPU) or --compose CALLS.json TRACE.csv"
    res = measure(a)
    with open(a.calls, "w") as f:
        json.dump(res, f)
    for row in res["rows"]:
        print(f"{row['dtype']} V={row['V']} W={row['W']} K={row['K']}: beam search {np.median(row['beam_us']):.0f} us, greedy {np.median(row['greedy_us']):.0f} us", flush=True)


if __name__ == "__main__":
    main()
