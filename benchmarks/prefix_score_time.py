"""Time of the CTC prefix scorer's two step calls (ctc_amd_prefix_score, ctc_amd_prefix_extend: one launch each) and of one whole
decoding step (score, top-k over N * V, extend), protocol of nbest_loss_time.py, beside
  (a) the same mathematics in torch on the device, written here: for the score a logsumexp over the [B, T, V] broadcast of one
      hypothesis at a time (the [B, N, T, V] temporary in N chunks), float32, on log-probabilities made beforehand; for the
      extension the recurrences in closed form with cumsum / logcumsumexp over T, float64;
  (b) for the score, one read of the logits at the device's copy rate (ctc_amd_probe_copy over a buffer of the logits' size).

    prefix_score_time.py --out profiles/prefix_score_time.md        on the GPU (there is no CPU path)

B=256 T=1000 V=256, full-length utterances, N in {1, 8, 16}; N(0, 1) logits and blank-biased N(0, 3^2) logits; both lattices; the
beam timed is three random extensions deep with every slot alive.  Device events around every call on a warm device, `--steps`
calls after `--warmup`, the calls of a line alternating; median, minimum and spread (max - min) / median.  The two sides are
compared once per line (1e-3 on finite entries; a disagreement is reported under the table).  No threshold is asserted: the table is the result."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (1, 8, 16)
INPUTS = (("N(0, 1)", 1.0, 0.0), ("blank-biased N(0, 3^2)", 3.0, 6.0))  # name, sigma, what the blank's logit gets on top
KINDS = ("classic", "simplified")


def stats(us):
    us = np.asarray(us)
    return float(np.median(us)), float(us.min()), float((us.max() - us.min()) / np.median(us))


def cell(us):
    med, lo, spread = stats(us)
    return f"{med:.0f} ({lo:.0f}, {100 * spread:.0f}%)"


def measure(a):
    import torch
    import tf_seq2seq_losses_amd as ctc
    from tf_seq2seq_losses_amd import _lib
    assert torch.cuda.is_available(), "prefix_score_time.py needs a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, V = a.B, a.T, a.V
    g = torch.Generator(device="cpu").manual_seed(0)
    NINF = -math.inf

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3  # microseconds

    src = torch.empty(B * T * V, device=dev).normal_()
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream

    def probe():
        assert lib.ctc_amd_probe_copy(dst.data_ptr(), src.data_ptr(), src.numel() * 4, st) == 0

    for _ in range(a.warmup):
        probe()
    copy_us = [timed(probe) for _ in range(a.steps)]
    copy_rate = 2 * src.numel() * 4 / (np.median(copy_us) * 1e-6) / 1e12  # TB/s, read + write
    read_us = float(np.median(copy_us)) / 2  # one read of the logits at that rate
    del src, dst

    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows = []
    for name, sigma, bias in INPUTS:
        x = (sigma * torch.randn((B, T, V), generator=g)).to(dev)
        x[..., 0] += bias
        lp64 = torch.log_softmax(x.double(), 2)
        lp32 = lp64.float()
        for kind in KINDS:
            classic = kind == "classic"
            scorer = (ctc.classic_ctc_prefix_scorer if classic else ctc.simplified_ctc_prefix_scorer)(x, tl, 0)
            for N in NS:
                state = scorer.initial_state(N)
                for step in range(3):
                    parent = torch.zeros((B, N), dtype=torch.int32, device=dev) if step == 0 else torch.arange(N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
                    state = scorer.extend(state, parent, torch.randint(1, V, (B, N), generator=g, dtype=torch.int32).to(dev))
                ident = torch.arange(N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
                token = torch.randint(1, V, (B, N), generator=g, dtype=torch.int32).to(dev)
                token[:, 0] = state.last_token[:, 0]  # one immediate repeat per utterance
                ln2 = math.log(2.0)
                s64, rb64 = state.state[:, :, :T] * ln2, state.state[:, :, T:2 * T] * ln2  # the torch side's state, natural logarithms
                s32, rb32 = s64.float(), rb64.float()
                last = state.last_token.long()
                out = {}

                def shifted(v):
                    return torch.cat([torch.full_like(v[:, :, :1], NINF), v[:, :, :-1]], 2)

                def torch_score():
                    phi = shifted(s32)
                    sc = torch.empty((B, N, V), dtype=torch.float32, device=dev)
                    for n in range(N):
                        sc[:, n] = torch.logsumexp(phi[:, n, :, None] + lp32, dim=1)
                    if classic:
                        col = lp32.gather(2, last[:, None, :].expand(B, T, N)).transpose(1, 2)
                        sc.scatter_(2, last[:, :, None], torch.logsumexp(shifted(rb32) + col, 2)[:, :, None])
                    sc[:, :, 0] = NINF
                    out["tscore"] = sc

                def torch_extend(par=ident, tok=token):
                    p = par.long()[:, :, None].expand(B, N, T)
                    sp, rbp = s64.gather(1, p), rb64.gather(1, p)
                    e = lp64.gather(2, tok.long()[:, None, :].expand(B, T, N)).transpose(1, 2)
                    eb = lp64[:, :, 0][:, None, :].expand(B, N, T)
                    phi = shifted(sp)
                    if classic:
                        phi = torch.where((tok.long() == last.gather(1, par.long()))[:, :, None], shifted(rbp), phi)
                        c = torch.cumsum(e, 2)
                        rn = c + torch.logcumsumexp(phi - (c - e), 2)
                    else:
                        rn = phi + e
                    cb = torch.cumsum(eb, 2)
                    rb = cb + torch.logcumsumexp(shifted(rn) - (cb - eb), 2)
                    out["tfull"] = torch.logaddexp(rn, rb)[:, :, -1]

                def new_score():
                    out["score"] = scorer.score(state)

                def new_extend():
                    out["ext"] = scorer.extend(state, ident, token)

                def pick(sc):
                    top, idx = sc.reshape(B, N * V).topk(N, dim=1)
                    return (idx // V).to(torch.int32), (idx % V).to(torch.int32)

                def new_step():
                    scorer.extend(state, *pick(scorer.score(state)))

                def torch_step():
                    torch_score()
                    torch_extend(*pick(out["tscore"]))

                cols = dict(score=new_score, tscore=torch_score, ext=new_extend, text=torch_extend, step=new_step, tstep=torch_step)
                for _ in range(a.warmup):
                    for fn in cols.values():
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in cols}
                for _ in range(a.steps):
                    for k, fn in cols.items():
                        t[k].append(timed(fn))
                new_score(); torch_score(); new_extend(); torch_extend()
                fin = torch.isfinite(out["tscore"])
                same_inf = bool((torch.isfinite(out["score"]) == fin).all())
                d_sc = float((out["score"][fin] - out["tscore"][fin]).abs().max())
                d_full = float((out["ext"].full_score - out["tfull"].float()).abs().max())
                agree = same_inf and d_sc <= 1e-3 * max(1.0, float(out["tscore"][fin].abs().max())) and d_full <= 1e-3 * max(1.0, float(out["tfull"].abs().max()))
                print(f"  both sides: score differs by {d_sc:.3g}, full score by {d_full:.3g}" + ("" if agree else "  ** DISAGREE **"), flush=True)
                rows.append(dict(input=name, N=N, kind=kind, agree=agree, **t))
                print(f"{name} {kind} N={N}: score {cell(t['score'])} / torch {cell(t['tscore'])}; extend {cell(t['ext'])} / torch {cell(t['text'])}; "
                      f"step {cell(t['step'])} / torch {cell(t['tstep'])} us", flush=True)
                del state, s64, rb64, s32, rb32
        del x, lp64, lp32
    return dict(device=torch.cuda.get_device_name(0), copy_us=float(np.median(copy_us)), copy_rate=copy_rate, read_us=read_us, rows=rows)


def table(a, res):
    B, T, V = a.B, a.T, a.V
    mb = B * T * V * 4 / 1e6
    lines = [f"# CTC prefix scorer, one decoding step beside the same mathematics in torch: B={B} T={T} V={V}", "",
             f"device: {res['device']}; {a.steps} warm calls each after {a.warmup}, the calls of a line alternating.  Device events around "
             "every call, microseconds: median (minimum, spread = (max - min) / median).  Logits: "
             f"{mb:.0f} MB; a copy of them (read + write) takes {res['copy_us']:.0f} us here: {res['copy_rate']:.2f} TB/s, so one read "
             f"at that rate is {res['read_us']:.0f} us.  `torch`: logsumexp over the [B, T, V] broadcast of one hypothesis at a time "
             "(float32, log-probabilities made beforehand) for the score, cumsum / logcumsumexp over T (float64) for the extension.  "
             "`met`: the new call's median is below torch's by more than torch's own spread (max - min).", ""]
    if a.note:
        lines += [a.note, ""]
    lines += ["| logits | lattice | N | score | torch score | met | score / one read | extend | torch extend | met | step | torch step | met |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def met(new, old):
        n, o = stats(new)[0], np.asarray(old)
        return "yes" if n < np.median(o) - (o.max() - o.min()) else "NO"

    for r in res["rows"]:
        lines.append(f"| {r['input']} | {r['kind']} | {r['N']} | {cell(r['score'])} | {cell(r['tscore'])} | {met(r['score'], r['tscore'])} | "
                     f"{stats(r['score'])[0] / res['read_us']:.1f} | {cell(r['ext'])} | {cell(r['text'])} | {met(r['ext'], r['text'])} | "
                     f"{cell(r['step'])} | {cell(r['tstep'])} | {met(r['step'], r['tstep'])} |")
    bad = [f"{r['input']} {r['kind']} N={r['N']}" for r in res["rows"] if not r["agree"]]
    lines += ["", "The two sides agree to 1e-3 on every line." if not bad else "The two sides DISAGREE beyond 1e-3 on: " + "; ".join(bad) + "."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default="", help="a line for the table's head (which build was timed)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    text = table(a, measure(a))
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
