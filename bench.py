#!/usr/bin/env python3
"""Benchmark of the CTC loss+gradient hot path on MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it is launched by
torch.distributed.run with one rank per GPU.  One "step" = one loss+gradient call (loss[B] and
grad[B,T,V] w.r.t. logits) over one batch of synthetic logits that already sits in HBM.
Workload = BASELINE.json configs[1]: classic_ctc_loss B=256 T=1000 U=128 V=256 fp32 per GPU
(`--kind simplified` gives configs[2]; `--ragged` the ragged-length variant; `--hessian` configs[4]).
The batch axis shards across ranks with no data-path collective (weak scaling: 256 utterances per GPU);
the only collective is the all-reduce of the scalar sum of losses (RCCL), issued every step.

Rank 0 prints ONE JSON line with the fields the driver reads plus
  "roofline":     HBM roofline of the loss+grad pipeline (algorithmic bytes 2*T*V*4 per utterance), from the event pairs
                  of the timed region itself.
A plain run does only what that line needs: set-up, warm-up, the --steps timed steps, the line.  `--full` adds what takes
runs of its own, after the timed region:
  "kernel_us_after_timed_region": 100 more launches, an event pair around each;
  "box":          a 1 GiB device copy (tells a slow box from a slow kernel);
  "cpu_baseline": the C restatement of the reference (oracle/ctc_oracle.c) timed on the host cores on a bounded sample of
                  the same workload (--no-cpu-baseline leaves it out);
  "secondary":    the other configurations and callers of the path (--no-secondary leaves it out);
and the check that the in-kernel [sum(loss), count] pair of the last step equals a reduction of its losses.
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (see dump_outputs).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling


def make_inputs(B, T, U, V, seed, ragged, device, scale=1.0):
    """BASELINE.md 'Inputs (configs 2/3)': numpy default_rng(seed); logits N(0,1), labels uniform non-blank,
    full lengths (ragged variant: logit_length ~ U{T/2..T-1}, label_length ~ U{U/2..U}).  scale != 1: logits N(0, scale^2)
    (the sharp-logit entries of `secondary`; the headline keeps the reference's N(0,1), tests/common.py:74-76)."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, V), dtype=np.float32)
    if scale != 1.0:
        logits *= np.float32(scale)
    labels = rng.integers(1, V, (B, U), dtype=np.int32)
    if ragged:
        logit_length = rng.integers(T // 2, T, B, dtype=np.int32)
        label_length = rng.integers(U // 2, U + 1, B, dtype=np.int32)
    else:
        logit_length = np.full(B, T, dtype=np.int32)
        label_length = np.full(B, U, dtype=np.int32)
    host = dict(logits=logits, labels=labels, label_length=label_length, logit_length=logit_length)
    dev = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
    return host, dev


DUMP_SAMPLE = 1 << 22  # elements kept of an output larger than this by --dump-outputs (16 MB of float32)
DUMP_LIMIT = 64 << 20  # bytes written by --dump-outputs in all


def output_sample(t, n=DUMP_SAMPLE, seed=0):
    """Tensor t as a float32 array: all of it if it has at most n elements, else the elements at n seeded-random flat
    indices (row-major order of t's shape, sorted, repeats dropped) -- the same positions in every run with the same shape."""
    t = t.detach()
    if t.numel() <= n:
        return t.float().cpu().numpy()
    idx = np.unique(np.random.default_rng(seed).integers(0, t.numel(), n, dtype=np.int64))
    return t.reshape(-1)[torch.from_numpy(idx).to(t.device)].float().cpu().numpy()


def dump_outputs(path, arrays):
    """--dump-outputs: writes {name: float32 / float64 array} as path/<name>.npy (at most DUMP_LIMIT bytes in all)."""
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, total
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_baseline(kind, host, budget_s=15.0):
    """Times the C restatement of the reference's algorithm (oracle/ctc_oracle.c, float32 like the reference,
    OpenMP over the batch) on the host cores, on a bounded sample of the same workload."""
    from oracle import c_oracle as C
    cores = os.cpu_count() or 1
    threads = min(cores, C.num_threads())
    B = host["logits"].shape[0]
    n = min(B, max(threads, 8))

    def run(m):
        t0 = time.perf_counter()
        C.loss_grad(kind, host["labels"][:m], host["logits"][:m], host["label_length"][:m], host["logit_length"][:m], 0,
                    precision="f32", want_grad=True, n_threads=threads)
        return time.perf_counter() - t0

    dt = run(n)  # warm-up + calibration
    n = int(min(B, max(n, n * 2.0 / max(dt, 1e-3))))
    reps, dt = 0, 0.0
    while dt < budget_s and reps < 200:  # repeat the bounded sample until ~budget_s of CPU time has been measured
        dt += run(n)
        reps += 1
    dt /= reps
    out = dict(value=n / dt, unit="utterances/s", cores=threads, kind="port",
               sample=f"oracle/ctc_oracle.c (C restatement of the reference's log-space alpha/beta + gradient, float32, "
                      f"OpenMP {threads} threads of {cores} host cores) loss+grad on the first {n} utterances of the workload, mean of {reps} runs of {dt:.2f} s")
    # beside it: the same port on ONE thread, and an independent, widely used CPU implementation
    # (torch.nn.functional.ctc_loss forward + backward incl. log_softmax, float32, all host threads; classic lattice only)
    m1 = min(B, 4)
    t0 = time.perf_counter()
    C.loss_grad(kind, host["labels"][:m1], host["logits"][:m1], host["label_length"][:m1], host["logit_length"][:m1], 0,
                precision="f32", want_grad=True, n_threads=1)
    out["single_thread"] = dict(value=m1 / (time.perf_counter() - t0), unit="utterances/s", sample=f"{m1} utterances, 1 thread")
    if kind == "classic":
        mt = min(B, 64)
        old_threads = torch.get_num_threads()
        torch.set_num_threads(threads)
        x = torch.from_numpy(host["logits"][:mt]).requires_grad_(True)
        lab = torch.from_numpy(host["labels"][:mt]).long()
        il = torch.from_numpy(host["logit_length"][:mt]).long()
        tl = torch.from_numpy(host["label_length"][:mt]).long()

        def torch_run():
            t0 = time.perf_counter()
            lp = torch.log_softmax(x, dim=2).transpose(0, 1)
            loss = torch.nn.functional.ctc_loss(lp, lab, il, tl, blank=0, reduction="sum", zero_infinity=False)
            torch.autograd.grad(loss, x)
            return time.perf_counter() - t0
        torch_run()
        dtt = min(torch_run() for _ in range(3))
        out["torch_ctc_cpu"] = dict(value=mt / dtt, unit="utterances/s",
                                    sample=f"torch.nn.functional.ctc_loss + log_softmax forward+backward, float32, "
                                           f"{torch.get_num_threads()} threads, {mt} utterances, best of 3")
        torch.set_num_threads(old_threads)
    return out


def _events_ms(fn, steps, warmup, dist=None, run=4):
    """Mean device time of fn() over `steps` calls (HIP events on torch's current stream = the launch stream; one pair around
    every run of `run` consecutive calls, see main) and the wall time per call of the same loop; `dist`, if a dict, receives
    the distribution of the per-call times of the runs."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    steps = max(run, steps // run * run)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps // run)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        for _ in range(run):
            fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    ts = [a.elapsed_time(b) / run for a, b in ev]
    if dist is not None:
        dist.update(_dist([t * 1e3 for t in ts]))
    return sum(ts) / len(ts), wall * 1e3


def _dist(us):
    """min / median / p90 / max of a list of per-launch times in microseconds"""
    v = sorted(us)
    return dict(n=len(v), min=round(v[0], 2), median=round(v[len(v) // 2], 2), p90=round(v[min(len(v) - 1, int(len(v) * 0.9))], 2),
                max=round(v[-1], 2))


def prewarm(fn, min_ms=100.0, max_calls=4000):
    """Runs fn() until at least min_ms of device time has passed on the current stream (clocks, caches and the HBM power state
    in their steady state whatever --warmup says) AND the launch time has settled -- the last three runs of 16 calls within 3 % of
    the fastest run seen -- or 4 x min_ms have passed; returns the number of calls made.  (r04, rocprofv3 trace of the headline on
    one box: 140 us per launch for the first 12 launches after an idle period, 160-183 us for the next 40, 139 us from then on --
    a timed region of 20 steps that starts inside such an excursion reads 5 % high.)"""
    n, spent, per = 0, 0.0, []
    while n < max_calls:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(16):
            fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b)
        spent += t
        per.append(t)
        n += 16
        if spent >= min_ms and ((len(per) >= 3 and max(per[-3:]) <= 1.03 * min(per)) or spent >= 4 * min_ms):
            break
    return n


def box_probe(lib, device):
    """One-off probe of the box the bench runs on: a 1 GiB float4 copy (ctc_amd_probe_copy: 16 B per lane, non-temporal
    stores), best and median of 8 -> GB/s of read + written bytes.  Lets a reader tell a slow box from a slow kernel."""
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=device).zero_()
    dst = torch.empty(n, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream().cuda_stream
    ts = []
    for i in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.ctc_amd_probe_copy(dst.data_ptr(), src.data_ptr(), n, st)
        b.record()
        b.synchronize()
        assert rc == 0
        if i >= 2:
            ts.append(a.elapsed_time(b))
    ts.sort()
    del src, dst
    return dict(box_copy_GBps=round(2 * n / ts[len(ts) // 2] / 1e6, 1), box_copy_best_GBps=round(2 * n / ts[0] / 1e6, 1),
                what="1 GiB device-to-device float4 copy, read + written bytes per second, median / best of 8")


class EmulatedAllReduce:
    """Stand-in for dist.all_reduce(buf, async_op=True) on ONE GPU: what ProcessGroupNCCL does around the collective -- its
    own stream waits for the compute stream, runs the collective kernel, and work.wait() makes the compute stream wait for
    that -- with a one-workgroup kernel of RCCL's footprint in place of the collective (512 threads, 4 KB of LDS, polling the
    device clock for `us` microseconds: a two-number all-reduce over xGMI is latency-bound, ~10-20 us)."""

    class _Work:
        def __init__(self, ev):
            self.ev = ev

        def wait(self):
            torch.cuda.current_stream().wait_event(self.ev)

    def __init__(self, lib, device, us=12.0, threads=512, lds=4096, priority=0):
        self.lib, self.us, self.threads, self.lds = lib, us, threads, lds
        self.side = torch.cuda.Stream(device=device, priority=priority)

    def __call__(self, buf):
        ready = torch.cuda.Event()
        ready.record()                       # the pair of this step exists once the compute stream gets here
        self.side.wait_event(ready)
        rc = self.lib.ctc_amd_probe_spin(self.threads, self.lds, self.us, self.side.cuda_stream)
        assert rc == 0
        done = torch.cuda.Event()
        done.record(self.side)
        return EmulatedAllReduce._Work(done)


def emulated_collective_table(lib, step_sum_factory, device, steps=120):
    """Step time of the bench loop with no collective, and with the emulated one at pipeline depth 1 and 2 (VERDICT r02
    item 5): does a kernel of RCCL's footprint run beside 256 workgroups that hold 159 000 of 163 840 bytes of LDS each?"""
    from tf_seq2seq_losses_amd import dist as cdist
    out = {}
    for name, depth, emu_kw, every in (("no_collective", 1, None, 1), ("emulated_depth1", 1, {}, 1), ("emulated_depth2", 2, {}, 1),
                                       ("emulated_depth1_one_wave_no_lds", 1, dict(threads=64, lds=0), 1),
                                       ("emulated_depth2_every4", 2, {}, 4), ("emulated_depth2_every8", 2, {}, 8)):
        step = step_sum_factory((depth + 2) * every)
        kw = dict(every=every, group_view=step.view) if every > 1 else {}
        emu = EmulatedAllReduce(lib, device, **emu_kw) if emu_kw is not None else None
        prewarm(lambda: cdist.pipelined_steps(step, 4 * every, reduced=True, depth=depth, all_reduce=emu, **kw), 40.0)
        step.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cdist.pipelined_steps(step, steps, reduced=True, depth=depth, all_reduce=emu, **kw)
        b.record()
        torch.cuda.synchronize()
        out[name] = dict(wall_us_per_step=round((time.perf_counter() - t0) / steps * 1e6, 2), device_us_per_step=round(a.elapsed_time(b) / steps * 1e3, 2))
    out["what"] = ("loss+gradient step (ctc_amd_loss_grad_sum) in dist.pipelined_steps on one GPU; emulated = a 512-thread, 4 KB-LDS kernel polling "
                   "for 12 us on a second stream per step (every4 / every8: per 4 / 8 steps, their pairs in one collective -- bench.py --reduce-every), "
                   "ordered like RCCL's all-reduce (tf_seq2seq_losses_amd/dist.py)")
    return out


def _lossgrad_callable(lib, _lib, ops, kind, dev, B, T, U, V):
    prep = ops.Prepared(dev["labels"], dev["logits"], dev["label_length"], dev["logit_length"], 0, U=U)
    ws = torch.empty(_lib.workspace_bytes(_lib.WS_LOSS_GRAD_LOGITS, kind, B, T, V, U), dtype=torch.uint8, device=prep.device)
    loss = torch.empty(B, dtype=torch.float32, device=prep.device)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=prep.device)
    args_c = prep.common(kind, _lib.WRT_LOGITS) + (loss.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), ws.numel())

    def step():
        rc = lib.ctc_amd_loss_grad(*args_c, torch.cuda.current_stream().cuda_stream)
        if rc:
            _lib.check(rc, "ctc_amd_loss_grad")
        return loss
    step.keep = (prep, ws, loss, grad)
    return step


def _sum_step_factory(lib, _lib, ops, device, rank, nbuf, B=256, T=1000, U=128, V=256):
    """step() of the headline workload in its one-launch form with the in-launch loss sum, over `nbuf` rotating int64[2] buffers"""
    host, dev = make_inputs(B, T, U, V, seed=rank, ragged=False, device=device)
    prep = ops.Prepared(dev["labels"], dev["logits"], dev["label_length"], dev["logit_length"], 0, U=U)
    ws = torch.empty(_lib.workspace_bytes(_lib.WS_LOSS_GRAD_LOGITS, 0, B, T, V, U), dtype=torch.uint8, device=device)
    loss = torch.empty(B, dtype=torch.float32, device=device)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=device)
    sums = torch.zeros((nbuf, 2), dtype=torch.int64, device=device)
    rows = [sums[k] for k in range(nbuf)]
    ptrs = [r.data_ptr() for r in rows]
    x = dev["logits"]
    args = (0, _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, x.stride(0), x.stride(1), prep.labels.data_ptr(), prep.stride,
            prep.label_length.data_ptr(), prep.logit_length.data_ptr(), 0, B, T, V, U, loss.data_ptr(), grad.data_ptr(),
            _lib.F32, grad.stride(0), grad.stride(1), None)
    state = {"i": 0, "keep": (prep, ws, loss, grad, dev)}

    def step():
        k = state["i"] % nbuf
        state["i"] += 1
        rc = lib.ctc_amd_loss_grad_sum(*args, ptrs[k], ptrs[(k + 1) % nbuf], ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return rows[k]

    def reset():  # (a new loop starts at row 0 with every row clear)
        state["i"] = 0
        sums.zero_()
    step.view = lambda first, n: sums[first % nbuf:first % nbuf + n]
    step.reset = reset
    return step


def _roof(alg_bytes, kernel_ms, **extra):
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
    return dict(bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS,
                algorithmic_bytes_per_launch=alg_bytes, kernel_ms_per_launch=kernel_ms, **extra)


def secondary(device, rank):
    """The other configurations of BASELINE.json and the callers around the path, timed in the same process after the
    headline (each entry: device time per call by HIP events, its HBM-roofline fraction, utterances/s from the wall time)."""
    from tf_seq2seq_losses_amd import _lib, ops
    import tf_seq2seq_losses_amd as ctc
    lib = _lib.load()
    out = {}
    B, T, U, V = 256, 1000, 128, 256
    alg = B * 2 * T * V * 4

    def lossgrad(name, kind_name, ragged, seed, B=B, T=T, U=U, V=V, steps=50, scale=1.0, rotate=1, warm_ms=40.0):
        """rotate > 1: that many distinct logits / gradient buffer sets taken in turn -- what a training loop presents (fresh logits
        every step: phase 1 cannot hit lines the previous step left in the 256 MiB Infinity Cache); 1: the same buffers every call,
        the reference harness's protocol (tests/benchmark.py:110-162) and the headline's."""
        sets = [make_inputs(B, T, U, V, seed=seed + 17 * r, ragged=ragged, device=device, scale=scale) for r in range(rotate)]
        host = sets[0][0]
        steps_ = [_lossgrad_callable(lib, _lib, ops, ops.KINDS[kind_name], dev, B, T, U, V) for _, dev in sets]
        state = {"i": 0}

        def step():
            state["i"] += 1
            return steps_[state["i"] % rotate]()
        d = {}
        prewarm(step, warm_ms)  # (the GPU idled through the CPU baseline: every entry gets its own warm start)
        kms, wms = _events_ms(step, steps, 10, d, run=(3 if rotate == 3 else 4))
        frames = int(host["logit_length"].sum())
        out[name] = dict(workload=f"{kind_name}_ctc_loss loss+grad B={B} T={T} U={U} V={V} fp32 {'ragged' if ragged else 'full-length'}"
                                  + (f", logits N(0, {scale:g}^2)" if scale != 1.0 else "")
                                  + (f", {rotate} logits/gradient buffer sets in rotation" if rotate > 1 else ""),
                         value=B / (wms * 1e-3), unit="utterances/s", ms_per_step=wms,
                         pipeline=_lib.pipeline_name(ops.KINDS[kind_name], 0, B, T, V, U, True),
                         roofline=_roof(frames * 2 * V * 4, kms, traffic=None, kernel_us=d))
        del sets, steps_

    # the headline workload as a training loop presents it: fresh logits every step (three buffer sets in rotation), and a batch
    # four times the chip's CU count (1 GB of logits: nothing of the previous step survives in the caches)
    # (the first entry after the CPU baseline's 15-30 s of GPU idleness: warmed as long as the headline -- with 40 ms it once read
    # 0.285 ms on a box where the next run read 0.160)
    lossgrad("classic_rotating_buffers", "classic", False, rank, rotate=3, steps=60, warm_ms=150.0)
    lossgrad("classic_B1024", "classic", False, rank, B=1024, steps=20)
    # sharp logits, N(0, 3^2) -- closer to a trained acoustic model's posteriors than the reference's N(0,1)
    lossgrad("classic_sharp_logits_sigma3", "classic", False, rank, scale=3.0)
    lossgrad("config3_simplified", "simplified", False, rank)
    lossgrad("classic_ragged", "classic", True, 1)
    # shapes off the north star: long labels (eight label positions per lane) and a BPE-sized vocabulary (three-kernel pipeline)
    lossgrad("classic_long_labels_U512", "classic", False, rank, U=512, steps=20)
    lossgrad("classic_wide_vocabulary_V4096", "classic", False, rank, B=32, V=4096, steps=20)

    # the drop-in Python call: classic_ctc_loss + autograd.grad(mean(loss)) (tests/benchmark.py:195-201 of the reference)
    host, dev = make_inputs(B, T, U, V, seed=rank, ragged=False, device=device)
    x = dev["logits"].clone().requires_grad_(True)

    def dropin():
        loss = ctc.classic_ctc_loss(dev["labels"], x, dev["label_length"], dev["logit_length"], 0)
        return torch.autograd.grad(loss.mean(), x)[0]
    prewarm(dropin, 40.0)
    kms, wms = _events_ms(dropin, 50, 10)
    out["dropin_autograd"] = dict(workload=f"classic_ctc_loss(...) + autograd.grad(loss.mean(), logits) through the Python mirror, B={B} T={T} U={U} V={V}",
                                  value=B / (wms * 1e-3), unit="utterances/s", ms_per_step=wms,
                                  roofline=_roof(alg, kms, traffic=None, note="device time of forward (loss) + backward (gradient) incl. the mean and its backward"))

    # the same two-call path on sharp logits N(0, 3^2) (the headline distribution never shows what the loss-only guard costs)
    hosts, devs = make_inputs(B, T, U, V, seed=rank, ragged=False, device=device, scale=3.0)
    xs = devs["logits"].clone().requires_grad_(True)

    def dropin_sharp():
        loss = ctc.classic_ctc_loss(devs["labels"], xs, devs["label_length"], devs["logit_length"], 0)
        return torch.autograd.grad(loss.mean(), xs)[0]
    prewarm(dropin_sharp, 40.0)
    kms, wms = _events_ms(dropin_sharp, 50, 10)
    out["dropin_autograd_sharp_logits_sigma3"] = dict(workload=f"the same with logits N(0, 3^2), B={B} T={T} U={U} V={V}",
                                                      value=B / (wms * 1e-3), unit="utterances/s", ms_per_step=wms,
                                                      roofline=_roof(alg, kms, traffic=None))
    del xs, devs, hosts

    # Hessian-vector product (second-order backward), north-star shape
    prep = ops.Prepared(dev["labels"], dev["logits"], dev["label_length"], dev["logit_length"], 0, U=U)
    vec = torch.randn((B, T, V), device=device, generator=torch.Generator(device=device).manual_seed(0))
    # (r04: warmed like the headline and timed over 40 calls -- 12 calls after 3 cold ones read 0.39-0.41 ms for a kernel that
    # scripts/hvp_time.py measured at 0.32)
    hvp_fn = lambda: ops.hvp(ops.KINDS["classic"], _lib.WRT_LOGITS, prep, vec)
    prewarm(hvp_fn, 60.0)
    kms, wms = _events_ms(hvp_fn, 40, 4)
    hvp_traffic = None
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r04_hvp_fused_pmc_traffic.json")) as f:
            hvp_traffic = json.load(f).get("_total_bytes_per_call")
    except Exception:
        pass
    out["hvp"] = dict(workload=f"ctc_amd_hvp (Hessian-vector product, no [B,T,V,T,V] tensor) B={B} T={T} U={U} V={V}",
                      value=B / (wms * 1e-3), unit="utterances/s", ms_per_step=wms,
                      roofline=_roof(B * 3 * T * V * 4, kms, traffic=hvp_traffic, note="algorithmic bytes: logits + vector read, product written; "
                                     "traffic: profiles/r04_hvp_fused_pmc_traffic.json"))
    del vec, x

    # configs[4]: dense Hessian B=32 T=200 U=32 V=64
    Bh, Th, Uh, Vh = 32, 200, 32, 64
    hostb, devb = make_inputs(Bh, Th, Uh, Vh, seed=rank, ragged=False, device=device)
    prep = ops.Prepared(devb["labels"], devb["logits"], devb["label_length"], devb["logit_length"], 0, U=Uh)
    kindc = ops.KINDS["classic"]
    ws = torch.empty(_lib.workspace_bytes(_lib.WS_HESSIAN, kindc, Bh, Th, Vh, Uh), dtype=torch.uint8, device=device)
    loss = torch.empty(Bh, dtype=torch.float32, device=device)
    hess = torch.empty((Bh, Th, Vh, Th, Vh), dtype=torch.float32, device=device)

    def hstep():
        rc = lib.ctc_amd_hessian(*prep.common(kindc, _lib.WRT_LOGITS), loss.data_ptr(), None, hess.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "ctc_amd_hessian")
    d = {}
    kms, wms = _events_ms(hstep, 8, 3, d, run=2)
    out["config5_hessian"] = dict(workload=f"classic_ctc_loss dense Hessian B={Bh} T={Th} U={Uh} V={Vh} fp32 (one ctc_amd_hessian call)",
                                  value=Bh / (wms * 1e-3), unit="utterances/s", ms_per_step=wms,
                                  roofline=_roof(Bh * ((Th * Vh) ** 2 * 4 + Th * Vh * 4), kms, traffic=None, kernel_us=d))
    del hess, ws
    out["reference_table"] = reference_table(device)
    out["emulated_collective"] = emulated_collective_table(lib, lambda nbuf: _sum_step_factory(lib, _lib, ops, device, rank, nbuf), device)
    # the headline workload once more, after everything else: tells a warm-up transient of a cold process from a slow box
    lossgrad("classic_full_length_again", "classic", False, rank, steps=100)
    return out


def reference_table(device):
    """The reference's only published experiment (README.md:16-24, tests/benchmark.py:41-43,110-162,182-237) on this GPU:
    batch 256, 32 tokens, 255 frames, ragged lengths in the distribution of tests/common.py:77-94 with the label tensor as
    wide as T, forward and forward + gradient through the public Python functions (wall clock per call incl. Python, as the
    reference measures), next to torch's own CTC on the same GPU.  SURVEY.md section 8 (f4)."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V = 256, 255, 32
    rng = np.random.default_rng(0)
    logits = torch.from_numpy(rng.standard_normal((B, T, V), dtype=np.float32)).to(device)
    tl = torch.from_numpy(rng.integers(T // 2, T, B, dtype=np.int32)).to(device)
    ll_h = rng.integers(T // 4, T // 2, B, dtype=np.int32)
    ll = torch.from_numpy(ll_h).to(device)
    labels = torch.from_numpy(rng.integers(1, V, (B, T), dtype=np.int32)).to(device)

    def torch_ctc(labels, x, ll, tl, blank=0):
        lp = torch.log_softmax(x, dim=2).transpose(0, 1)
        return torch.nn.functional.ctc_loss(lp, labels.long(), tl.long(), ll.long(), blank=blank, reduction="none")

    def wall(fn, steps=100, warmup=5):
        for _ in range(warmup):
            fn()
        prewarm(fn, 20.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    rows = {}
    for name, fn in (("classic_ctc_loss", ctc.classic_ctc_loss), ("simple_ctc_loss", ctc.simple_ctc_loss), ("torch.nn.functional.ctc_loss", torch_ctc)):
        def forward():
            with torch.no_grad():
                return fn(labels, logits, ll, tl, 0)

        def gradient():
            x = logits.detach().requires_grad_(True)
            loss = fn(labels, x, ll, tl, 0)
            return torch.autograd.grad(loss.sum(), x)[0]
        # (best of three passes: a pass now and then runs twice as long -- allocator / clock state after the previous workload)
        rows[name] = dict(forward_ms=round(min(wall(forward) for _ in range(3)), 4), forward_gradient_ms=round(min(wall(gradient) for _ in range(3)), 4))
    return dict(workload=f"reference README table: B={B} T={T} V={V}, ragged lengths, label tensor {T} wide (labels <= {int(ll_h.max())}), "
                         "wall clock per call incl. Python, best of three passes of 100 calls after a 20 ms warm start", rows=rows)


def launcher_command(n, argv, port=None):
    """The command `bench.py --gpus N` runs as a CHILD process when it was not started by torch.distributed.run itself: one rank
    per GPU of this node, rendezvous on 127.0.0.1 (the driver's own form: `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`); every bench argument passes through."""
    if port is None:
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__), *argv]


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` with N > 1 and no RANK in the environment: start the N ranks as a child process (never exec: the
    parent has not touched the GPU and does not, the child owns it), relay its output, return its exit code."""
    import subprocess
    if args.backend == "nccl" and torch.cuda.device_count() < args.gpus:  # (device_count does not initialise the GPU)
        print(f"bench.py: --gpus {args.gpus} needs {args.gpus} GPUs, this node shows {torch.cuda.device_count()} "
              "(--backend gloo rehearses ranks that share one GPU)", file=sys.stderr, flush=True)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    proc = subprocess.Popen(launcher_command(args.gpus, argv), env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:  # rank 0's JSON line (and anything else the ranks print) goes to our stdout unchanged
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kind", default="classic", choices=["classic", "simplified"])
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=128)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--hessian", action="store_true", help="time the dense Hessian at B=32 T=200 U=32 V=64 (configs[4])")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the per-launch distribution, the box probe, the CPU baseline, the secondary "
                         "configurations and the check of the in-kernel loss sum (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy: loss, the [sum(loss), count] "
                         "pair, and a fixed seeded sample of 2^22 elements of the gradient (--hessian: of the Hessian)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full without the secondary configurations (simplified, ragged, drop-in autograd, HVP, Hessian)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="element type of logits and gradient (producer format)")
    ap.add_argument("--time-major", action="store_true", help="logits stored [T,B,V] (producer format), passed as a strided view")
    ap.add_argument("--reduce-every", type=int, default=8,
                    help="the [sum(loss), count] pairs of this many consecutive steps go out in ONE all-reduce (fewer, larger collectives: "
                         "what a collective costs the loss kernels is the event / stream-wait pair around it, secondary.emulated_collective); "
                         "1 = one all-reduce per step")
    ap.add_argument("--pipeline-depth", type=int, default=2,
                    help="steps the all-reduce of sum(loss) may lag behind the loss kernel (dist.pipelined_steps depth)")
    ap.add_argument("--emulate-collective", action="store_true",
                    help="N = 1 only: stand in for RCCL's all-reduce with a kernel of its footprint on a second stream (ctc_amd_probe_spin), "
                         "ordered as the real one is")
    ap.add_argument("--prewarm-ms", type=float, default=150.0,
                    help="after the --warmup steps, keep launching the timed kernel until this much device time has passed (untimed; 0 = off)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend for N > 1 (nccl = RCCL over xGMI; gloo only to rehearse ranks that share one GPU)")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    # BEFORE anything touches the GPU: a bare `python bench.py --gpus N` starts its own N ranks (one process per GPU) as a child
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"bench.py --gpus {args.gpus} is running with WORLD_SIZE={world}: launch it with one rank per GPU"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    if args.backend == "gloo":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    from tf_seq2seq_losses_amd import _lib, ops

    if args.hessian:
        args.B, args.T, args.U, args.V = 32, 200, 32, 64
        NBUF = 3
    B, T, U, V = args.B, args.T, args.U, args.V
    kind = ops.KINDS[args.kind]
    host, dev = make_inputs(B, T, U, V, seed=rank, ragged=args.ragged, device=device)
    prep = ops.Prepared(dev["labels"], dev["logits"], dev["label_length"], dev["logit_length"], 0, U=U)
    total = torch.zeros((), dtype=torch.float32, device=device)

    if args.hessian:
        ws = torch.empty(_lib.workspace_bytes(_lib.WS_HESSIAN, kind, B, T, V, U), dtype=torch.uint8, device=device)
        loss = torch.empty(B, dtype=torch.float32, device=device)
        hess = torch.empty((B, T, V, T, V), dtype=torch.float32, device=device)
        lib = _lib.load()

        def step():
            rc = lib.ctc_amd_hessian(*prep.common(kind, _lib.WRT_LOGITS), loss.data_ptr(), None, hess.data_ptr(),
                                     ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "ctc_amd_hessian")
            return loss
        alg_bytes = B * ((T * V) ** 2 * 4 + T * V * 4)
    else:
        # outputs and workspace are allocated once (the C ABI never allocates); one step = one ctc_amd_loss_grad call
        ws = torch.empty(_lib.workspace_bytes(_lib.WS_LOSS_GRAD_LOGITS, kind, B, T, V, U), dtype=torch.uint8, device=device)
        loss = torch.empty(B, dtype=torch.float32, device=device)
        grad = torch.empty((B, T, V), dtype=torch.float32, device=device)
        lib = _lib.load()
        # sum(loss) and the finite count of a step, accumulated by the loss kernel itself in fixed point: three int64[2] buffers
        # in rotation (step i fills i mod 3 and clears (i+1) mod 3; the collective of step i-1 may still be reading (i-1) mod 3)
        # (--reduce-every R: the pairs of R consecutive steps go out in one all-reduce -- R rows per group, depth + 2 groups)
        NBUF = (args.pipeline_depth + 2) * args.reduce_every
        sums = torch.zeros((NBUF, 2), dtype=torch.int64, device=device)
        # row addresses and group views made HERE: the first tensor-indexing operation of a process costs ~150 us of dispatch set-up,
        # and inside the timed region that was idle time between the first event and the first launch (first run of four launches
        # read 172-183 us per launch instead of 137)
        sum_rows = [sums[k] for k in range(NBUF)]
        sum_ptr = [r.data_ptr() for r in sum_rows]
        stream_h, ws_ptr, ws_n = torch.cuda.current_stream().cuda_stream, ws.data_ptr(), ws.numel()
        group_views = [sums[g * args.reduce_every:(g + 1) * args.reduce_every] for g in range(args.pipeline_depth + 2)]
        native = args.dtype != "f32" or args.time_major
        if native:  # producer formats through ctc_amd_loss_grad_ex: no conversion pass anywhere
            xf = dev["logits"].to(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
            if args.time_major:
                xf = xf.transpose(0, 1).contiguous().transpose(0, 1)
            grad = torch.empty_strided(xf.shape, xf.stride(), dtype=xf.dtype, device=device)
            dt = _lib.BF16 if args.dtype == "bf16" else _lib.F32
            ex_args = (kind, _lib.WRT_LOGITS, xf.data_ptr(), dt, xf.stride(0), xf.stride(1), prep.labels.data_ptr(), prep.stride,
                       prep.label_length.data_ptr(), prep.logit_length.data_ptr(), 0, B, T, V, U, loss.data_ptr(),
                       grad.data_ptr(), dt, xf.stride(0), xf.stride(1), None, ws.data_ptr(), ws.numel())

            def step():
                rc = lib.ctc_amd_loss_grad_ex(*ex_args, torch.cuda.current_stream().cuda_stream)
                if rc:
                    _lib.check(rc, "ctc_amd_loss_grad_ex")
                return loss

            def step_sum(k):  # the same call + sum(loss) accumulated inside the launch (ctc_amd_loss_grad_sum)
                a = ex_args
                rc = lib.ctc_amd_loss_grad_sum(*a[:21], sum_ptr[k], sum_ptr[(k + 1) % NBUF], a[21], a[22], stream_h)
                if rc:
                    _lib.check(rc, "ctc_amd_loss_grad_sum")
                return sum_rows[k]
        else:
            args_c = prep.common(kind, _lib.WRT_LOGITS) + (loss.data_ptr(), grad.data_ptr(), None, ws.data_ptr(), ws.numel())

            def step():
                rc = lib.ctc_amd_loss_grad(*args_c, torch.cuda.current_stream().cuda_stream)
                if rc:
                    _lib.check(rc, "ctc_amd_loss_grad")
                return loss
            x_ = dev["logits"]
            sum_args = (kind, _lib.WRT_LOGITS, x_.data_ptr(), _lib.F32, x_.stride(0), x_.stride(1), prep.labels.data_ptr(), prep.stride,
                        prep.label_length.data_ptr(), prep.logit_length.data_ptr(), 0, B, T, V, U, loss.data_ptr(), grad.data_ptr(),
                        _lib.F32, grad.stride(0), grad.stride(1), None)

            def step_sum(k):  # the same call + sum(loss) accumulated inside the launch (ctc_amd_loss_grad_sum)
                rc = lib.ctc_amd_loss_grad_sum(*sum_args, sum_ptr[k], sum_ptr[(k + 1) % NBUF], ws_ptr, ws_n, stream_h)
                if rc:
                    _lib.check(rc, "ctc_amd_loss_grad_sum")
                return sum_rows[k]
        alg_bytes = B * 2 * T * V * (2 if args.dtype == "bf16" else 4)

    # The reduced scalars are read one step later (a training loop logs them), so the all-reduce of step i is issued
    # asynchronously and runs on RCCL's stream beside the kernel of step i+1; every collective still completes inside the
    # timed region (tf_seq2seq_losses_amd/dist.py: pipelined_steps, covered at world size 2 by tests/test_dist_gloo.py).
    from tf_seq2seq_losses_amd import dist as cdist

    def full_step():
        return cdist.all_reduce_pair(step(), async_op=False)[0]

    for _ in range(args.warmup):
        full_step()
    # ... and, whatever --warmup says, at least 100 ms of the timed launch: a cold process ran its first ~25 launches 10 %
    # slow (r02: driver 174 us at --warmup 5 against 152-157 us at --warmup 20 on the same commit)
    extra_warm = prewarm(step, args.prewarm_ms) if args.prewarm_ms > 0 else 0
    if world > 1 and not args.hessian:
        # the collective of the timed region once before it, on the (still all-zero) rows it will carry: RCCL sets up a datatype /
        # message-size combination on first use, and the warm-up steps above reduce a float32 pair, not int64[R, 2]
        import torch.distributed as dist
        for gv in group_views:
            dist.all_reduce(gv, op=dist.ReduceOp.SUM)
    emu = EmulatedAllReduce(lib, device) if (args.emulate_collective and world == 1) else None
    if emu is not None:  # (its stream, events and kernel exist before the timed region)
        for _ in range(8):
            emu(None).wait()
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # the dominant kernel is timed live inside the timed region: HIP event pairs on the launch stream (torch's current stream),
    # each around a run of KEV consecutive launches (a pair around every single launch adds the 5-8 us the stream needs to
    # process the two event packets to the kernel it brackets and serialises its dispatch behind them: 158 against 150 us
    # here) -- launch duration = bracketed time / KEV, averaged over the K steps; the number the roofline fraction is priced on
    # (8 launches per pair since the end of r04: the two event packets between two runs cost the stream ~10 us of idle time -- the
    # rocprofv3 trace shows it as a 10 us gap before every run -- which is outside the brackets but inside the wall clock `value`
    # comes from: 2.5 us per step with runs of four, 1.25 with runs of eight)
    KEV = 8
    ngrp = (args.steps + KEV - 1) // KEV
    kev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ngrp)]
    in_kernel_sum = not args.hessian

    def timed_step():
        i = timed_step.i
        if i % KEV == 0:
            kev[i // KEV][0].record()
        loss_t = step_sum(i % NBUF) if in_kernel_sum else step()
        if i % KEV == KEV - 1 or i == args.steps - 1:
            kev[i // KEV][1].record()
        timed_step.i += 1
        return loss_t
    timed_step.i = 0
    t0 = time.perf_counter()
    ev0.record()
    # per step: ONE launch (loss + gradient + the [sum(loss), #finite] pair, ctc_amd_loss_grad_sum) + (N > 1) one asynchronous
    # all-reduce of the pair; the Hessian workload keeps the separate ctc_amd_reduce_loss launch
    seen = []
    grouped = in_kernel_sum and args.reduce_every > 1
    pairs = cdist.pipelined_steps(timed_step, args.steps, reduced=in_kernel_sum, depth=args.pipeline_depth, all_reduce=emu,
                                  consume=(lambda i, pair: seen.append(pair.reshape(-1, 2)[-1]) if i == args.steps - 1 else None) if in_kernel_sum else None,
                                  **(dict(every=args.reduce_every, group_view=lambda first, n: (group_views[(first % NBUF) // args.reduce_every] if n == args.reduce_every
                                                                                                    else group_views[(first % NBUF) // args.reduce_every][:n])) if grouped else {}))
    ev1.record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev_ms = ev0.elapsed_time(ev1)
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller: the losses, the [sum(loss), count] pair (all-reduced when N > 1; the
        # kernel's fixed-point sum taken back to float, or the pair of ctc_amd_reduce_loss for the Hessian) and a fixed sample
        # of the gradient / Hessian (positions in [B,T,V] / [B,T,V,T,V] order, a time-major gradient included)
        if in_kernel_sum:
            pair = seen[0].double().cpu().numpy() / np.array([1048576.0, 1.0])
        else:
            pair = pairs[-1].double().cpu().numpy()
        dump_outputs(args.dump_outputs, {"loss": output_sample(loss), "loss_sum_count": pair,
                                         ("hessian_sample" if args.hessian else "grad_sample"): output_sample(hess if args.hessian else grad)})
    if args.full and in_kernel_sum and world == 1 and seen:  # (outside the timed region) the pair the kernel accumulated is the sum of its losses
        fin = torch.isfinite(loss)
        want = float(loss[fin].double().sum())
        got, cnt = float(seen[0][0]) / 1048576.0, int(seen[0][1])
        assert cnt == int(fin.sum()) and abs(got - want) <= 1e-6 * max(1.0, abs(want)) + B * 1e-6, (got, want, cnt)
    reduced_check = None
    if args.full and in_kernel_sum and world > 1 and seen:
        # (outside the timed region) the pair of the last step as the collective left it on this rank against an independent
        # reduction of the ranks' own losses: the same count, the same sum in fixed point -- on every rank
        fin = torch.isfinite(loss)
        own = torch.stack([torch.round(loss[fin].double() * 1048576.0).sum().to(torch.int64), fin.sum().to(torch.int64)])
        dist.all_reduce(own, op=dist.ReduceOp.SUM)
        got = seen[0].to(torch.int64)
        assert int(got[1]) == int(own[1]) and abs(int(got[0]) - int(own[0])) <= 2 * B * world, (got.tolist(), own.tolist())
        reduced_check = dict(finite_utterances_all_ranks=int(got[1]), sum_loss_all_ranks=float(got[0]) / 1048576.0,
                             what="the all-reduced [sum(loss), count] pair of the last timed step, equal to an independent reduction of the ranks' losses")
    tmax = torch.tensor([wall], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    wall = float(tmax.item())
    kernel_ts = [a.elapsed_time(b) / min(KEV, args.steps - KEV * g) for g, (a, b) in enumerate(kev)]  # per launch, by group
    kernel_ms = sum(a.elapsed_time(b) for a, b in kev) / args.steps
    # (--full) after the timed region: the same launch 100 more times with an event pair around each, for the per-launch distribution
    post = []
    if args.full and not args.hessian:
        for _ in range(100):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            post.append((a, b))
        torch.cuda.synchronize()
        post = [a.elapsed_time(b) * 1e3 for a, b in post]

    if rank == 0:
        ms_per_step = wall * 1e3 / args.steps
        value = B * world * args.steps / wall
        dev_ms_per_step = dev_ms / args.steps
        achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
        if args.hessian:
            kernel_name = "emit_kernel + scan_kernel + grad_kernel (x2) + hess_slab_kernel (one ctc_amd_hessian call; hess_slab_kernel is >99 % of it)"
            traffic = traffic_src = None
        else:
            pipeline = _lib.pipeline_name(kind, _lib.WRT_LOGITS, B, T, V, U, True)
            kernel_name = {"fused6": "fused6_kernel (one launch: linear-domain chains + recompute chains + helpers; flagged utterances are redone in the log domain inside it, none here)",
                           "fused5": "fused5_kernel (one launch: chains + recompute chains + helpers)",
                           "v1": "emit_kernel + scan_kernel + grad_kernel"}[pipeline] + " = one ctc_amd_loss_grad call"
            # HBM bytes per launch from committed rocprofv3 PMC passes of this configuration (FETCH_SIZE x2 + WRITE_SIZE, see the
            # file's note).  Only quoted when the profiled kernel is the one this run launches (name with template arguments).
            traffic, traffic_src = None, None
            tfile = os.path.join(ROOT, "profiles", "r04_fused6_pmc_traffic.json")
            north_star = args.kind == "classic" and (B, T, U, V) == (256, 1000, 128, 256) and not args.ragged and args.dtype == "f32" and not args.time_major
            if north_star and os.path.exists(tfile):
                prof = json.load(open(tfile))
                running = f"ctc::{pipeline}::{pipeline}_kernel<0, 2, 4, 12, 1, 0>"
                if prof.get("_kernel") == running:
                    traffic = prof.get("_total_bytes_per_call")
                    traffic_src = f"{os.path.basename(tfile)} (kernel {prof.get('_kernel')}, commit {prof.get('_commit')})"
        out = {
            "metric": "utterances/sec (loss+grad) at B=256 T=1000 U=128 V=256; HBM roofline %" if not args.hessian
            else "utterances/sec (dense Hessian) at B=32 T=200 U=32 V=64",
            "value": value, "unit": "utterances/s", "n_gpus": world, "rccl_ranks": world if args.backend == "nccl" else 0,
            "collective_backend": (args.backend if world > 1 else None), "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if args.dtype == "f32" else "f32 arithmetic, bf16 logits/gradient in HBM", "data": "synthetic",
            "config": {"workload": f"{args.kind}_ctc_loss {'hessian' if args.hessian else 'loss+grad'} B={B} T={T} U={U} V={V} {'fp32' if args.dtype == 'f32' else 'bf16 logits/gradient, fp32 arithmetic'} per GPU"
                                   + (" ragged" if args.ragged else " full-length") + (" time-major [T,B,V]" if args.time_major else ""),
                       "global_batch": B * world,
                       "parallelism": (f"batch-sharded x{world}, every step's sum(loss) pair all-reduced, {args.reduce_every} steps' pairs per collective, "
                                       f"waited for {args.pipeline_depth} collective(s) later"
                                       if args.reduce_every > 1 and not args.hessian else
                                       f"batch-sharded x{world}, all-reduce of sum(loss) {args.pipeline_depth} step(s) behind")
                                      + (" (EMULATED on one GPU: ctc_amd_probe_spin on a second stream)" if emu is not None else ""),
                       "reduce_every": args.reduce_every},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src if not args.hessian else None,
                         "kernel": kernel_name, "algorithmic_bytes_per_launch": alg_bytes,
                         "kernel_ms_per_launch": kernel_ms, "device_ms_per_step_incl_reduction": dev_ms_per_step,
                         "kernel_us_in_timed_region": dict(_dist([t * 1e3 for t in kernel_ts]), in_order=[round(t * 1e3, 1) for t in kernel_ts],
                                                           what=f"per launch, event pairs around runs of {KEV} launches"),
                         "kernel_us_after_timed_region": dict(_dist(post), what="100 more launches, an event pair around EACH (adds the event packets' own time)") if post else None},
            "warmup_effective": args.warmup + extra_warm,
            "box": box_probe(lib, device) if world == 1 and args.full else None,
            "reduced_check": reduced_check,
        }
        if args.full and not args.no_cpu_baseline and not args.hessian and world == 1:  # reported at N = 1 only (rank 0's host cores)
            out["cpu_baseline"] = cpu_baseline(args.kind, host)
        else:
            out["cpu_baseline"] = None
        if args.full and world == 1 and not args.no_secondary and not args.hessian and (B, T, U, V) == (256, 1000, 128, 256):
            out["secondary"] = secondary(device, rank)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
