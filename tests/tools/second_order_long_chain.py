"""Where the log-domain Hessian-vector pipeline's error sits on long chains, and whether it follows T or the lane tiling NL
(profiles/second_order_axes.md, "Finding").  Needs a GPU:  python -m tests.tools.second_order_long_chain

Inputs as tests/test_gpu_second_order_axes.py::test_label_axis (V = 8, two utterances per call, the second of 100 labels over T - 37
frames).  Per utterance: the largest error relative to max|Hv| and its frame, the median / 90 % / 99 % of the per-frame maxima, the
number of frames above 1e-4, and the maximum in every tenth of the utterance."""
import numpy as np
import torch

from tests.tools import second_order_reference as R


def run(U, T, kind, label_length=None, seed=None):
    from tf_seq2seq_losses_amd import ops, _lib
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    c = R.label_case(U)._replace(name=f"U={U} T={T}", T=T, label_length=(label_length or U, 100), logit_length=(T, T - 37),
                                 plant=511 if U > 515 else -1)
    if seed is not None:
        c = c._replace(seed=seed)
    inp, ref = R.inputs(c), R.hv_reference(c, kind)
    p = ops.Prepared(t(inp["labels"]), t(inp["logits"]), t(inp["label_length"]), t(inp["logit_length"]), 0)
    out = ops.hvp(ops.KINDS[kind], _lib.WRT_LOGITS, p, t(inp["v"]))[2].cpu().numpy().astype(np.float64)
    for b in range(2):
        e, top, n = np.abs(out[b] - ref[b]), np.abs(ref[b]).max(), c.logit_length[b]
        pf = e.max(1) / top
        fr, tk = np.unravel_index(e.argmax(), e.shape)
        q = [float(np.quantile(pf[:n], x)) for x in (0.5, 0.9, 0.99)]
        tenths = " ".join(f"{pf[i * n // 10:(i + 1) * n // 10].max():.1e}" for i in range(10))
        print(f"LONG-CHAIN {kind} call U={p.U} seed={c.seed}, utterance of {c.label_length[b]} labels over {n} frames: max {pf.max():.2e} at "
              f"frame {fr} token {tk}; per-frame median/90%/99% {q[0]:.1e}/{q[1]:.1e}/{q[2]:.1e}; frames over 1e-4: {(pf > 1e-4).sum()}; "
              f"max per tenth of T: {tenths}", flush=True)


if __name__ == "__main__":
    for kind in R.KINDS:
        run(1024, 1300, kind)                      # the test's case
        run(1024, 1300, kind, seed=77)             # another draw
        run(513, 1300, kind)                       # NL = 16, half the label
        run(260, 1300, kind)                       # NL = 8
        run(1024, 1300, kind, label_length=1000)   # lane 63's last slots empty
