"""Float64 references of the second-order kernels, and the inputs of tests/test_gpu_second_order_axes.py.

The reference of a Hessian-vector product is the directional derivative of the float64 NumPy oracle's gradient (oracle/ctc_oracle.py),
by central differences at eps and 2 eps with Richardson extrapolation (error O(eps^4)).  tests/test_second_order_reference.py pins,
without a GPU, that it has converged at every shape below (eps = 2e-3 against 1e-3: 1e-5 of max|Hv| per utterance) and that its
log-probability form equals the contraction of the oracle's own Hessian.

Inputs (`inputs`): logits N(0, 3^2) with +6 on the blank and on the label tokens, label tokens spread over the vocabulary (token 1, one
token in every further stretch of the vocabulary, V - 1 or V - 2), direction N(0, 1).  Everything is deterministic in the case and cached
per case, and the cached arrays are read-only.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import ctc_oracle as O

KINDS = ("classic", "simplified")
LOGITS, LOGPROBS = "logits", "logprobs"
BLOCK = 1024  # tokens per block of the input condition (input_condition)


def fd64_exact(kind, inp, v, eps=2e-3, blank=0):
    """Directional derivative of the float64 NumPy oracle's gradient along v, by central differences at eps and 2 eps with
    Richardson extrapolation (error O(eps^4)); logits and direction are taken in float64 exactly as the GPU sees them."""
    x = inp["logits"].astype(np.float64)
    vv = v.astype(np.float64)

    def grad(z):
        d = O.ctc_loss(kind, inp["labels"], z, inp["label_length"], inp["logit_length"], blank)
        return O.logits_gradient(d, z)
    d1 = (grad(x + eps * vv) - grad(x - eps * vv)) / (2 * eps)
    d2 = (grad(x + 2 * eps * vv) - grad(x - 2 * eps * vv)) / (4 * eps)
    return (4.0 * d1 - d2) / 3.0


def fd64_exact_logprobs(kind, inp, v, eps=2e-3, blank=0):
    """The same difference for log-probability input: inp["logprobs"] are free variables (base_loss.py:71-99: nothing renormalises
    them), perturbed along v; the gradient is loss_data.gradient."""
    x = inp["logprobs"].astype(np.float64)
    vv = v.astype(np.float64)

    def grad(z):
        return O.LOSS_DATA[kind](inp["labels"], z, inp["label_length"], inp["logit_length"], blank).gradient
    d1 = (grad(x + eps * vv) - grad(x - eps * vv)) / (2 * eps)
    d2 = (grad(x + 2 * eps * vv) - grad(x - 2 * eps * vv)) / (4 * eps)
    return (4.0 * d1 - d2) / 3.0


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
# label_length / logit_length: one entry per utterance; plant: first position of a run of four equal labels (-1: none);
# draw: (V, U, tokens) the logits and the direction are drawn V wide, the labels U wide from the tokens below `tokens`, and columns
# [:V] / [:U] are kept, so that cases of one draw and seed share their numbers; bf16: the logits are rounded to bfloat16 (the
# reference reads the rounded values)
Case = namedtuple("Case", "name V T U blank label_length logit_length seed plant draw bf16")


def _case(name, V, T, U, blank, label_length, logit_length, seed, plant=-1, draw=None, bf16=False):
    return Case(name, V, T, U, blank, tuple(label_length), tuple(logit_length), seed, plant, draw or (V, U, V), bf16)


def mid_blank(V):
    """A blank inside a later pass of the row loops (64 tokens per pass element-wise, 256 with 16 bytes per lane)."""
    return 4097 if V >= 4100 else V // 2 + 97


VOCABULARIES = (257, 260, 1028, 1030, 4096, 4100, 8192, 8196, 16380, 16377)


def vocabulary_case(V, which):
    """B = 2, T = 6..12, U = 3..5.  which = "first": blank 0, one full and one ragged utterance; "last": blank V - 1, the second
    utterance ragged with an empty label; "mid": blank inside a later pass, the first utterance ragged, the second infeasible."""
    i = VOCABULARIES.index(V)
    T, U = 6 + (3 * i) % 7, 3 + i % 3
    if which == "first":
        return _case(f"V={V} blank=0", V, T, U, 0, (U, U - 1), (T, T - 2), 100 + i)
    if which == "last":
        return _case(f"V={V} blank={V - 1}", V, T, U, V - 1, (U, 0), (T, T - 1), 200 + i)
    return _case(f"V={V} blank={mid_blank(V)}", V, T, U, mid_blank(V), (U - 1, U), (T - 1, U - 1), 300 + i)


def logprob_vocabulary_case(V):
    """For log-probability input only the blank and the label tokens have a non-zero row entry, so both utterances carry all U = 5
    labels (one per 1024-token block at V = 4100) and differ in their frames.  Sharp logits pin most label tokens to their frames,
    where the posterior does not move with the input: the seeds are ones at which the float64 reference meets the input condition
    (input_condition; found on the reference alone by scan_logprob_seeds below, seeds 400..439: 12 of 40 qualify at V = 4100)."""
    blank = 0 if V < 4100 else mid_blank(V)
    return _case(f"V={V} blank={blank} U=5", V, 12, 5, blank, (5, 5), (12, 10), 412 if V < 4100 else 417)


def label_case(U):
    """V = 8, B = 2: one utterance at full length, one with 100 labels (the upper lanes hold padding); a run of equal labels across
    positions 511..514."""
    T = 1300 if U > 520 else 700
    return _case(f"U={U} T={T}", 8, T, U, 0, (U, 100), (T, T - 37), 500 + U % 11, plant=511)


def boundary_case(V, U):
    """T = 150, U = 100 (129), one draw (260 columns, 129 labels below token 254) of which every case keeps its part."""
    return _case(f"boundary V={V} U={U}", V, 150, U, 0, (U, U - 30), (150, 131), 600, draw=(260, 129, 254))


def public_case(bf16):
    return _case("public V=1028 U=20 T=40" + (" bf16" if bf16 else ""), 1028, 40, 20, 0, (20, 13, 7), (40, 33, 40), 700, bf16=bf16)


PUBLIC_WEIGHTS = (1.0, 2.0, -0.5)

HESSIAN_SHAPES = ((2, 3, 909, 4), (2, 3, 912, 4), (1, 2, 4100, 2), (1, 1, 8192, 1))  # (B, T, V, U)


HESSIAN_SEEDS = {909: 899, 912: 877, 4100: 840}  # from scan_hessian_seeds, below


def hessian_case(B, T, V, U):
    """The labels tensor is U wide.  Every utterance has one frame more than labels, so that several alignments exist: the blocks
    between different frames are then non-zero and the two lattices differ (with as many labels as frames there is one path, all
    posteriors are 0 or 1 and every cross-frame block vanishes).  T = 1 leaves no choice: one label in one frame."""
    if T == 1:
        return _case(f"hessian B={B} T={T} V={V} U={U}", V, T, U, 0, (1,) * B, (1,) * B, 802)
    return _case(f"hessian B={B} T={T} V={V} U={U}", V, T, U, 0, (T - 1, T - 2)[:B], (T, T - 1)[:B], HESSIAN_SEEDS[V])


def hvp_cases():
    """Every (case, space) whose Hessian-vector reference a GPU test uses: the convergence pin walks this list."""
    out = [(vocabulary_case(V, w), LOGITS) for V in VOCABULARIES for w in ("first", "last", "mid")]
    out += [(label_case(U), LOGITS) for U in (513, 520, 1024)]
    out += [(logprob_vocabulary_case(V), space) for V in (1030, 4100) for space in (LOGPROBS, LOGITS)] + [(label_case(520), LOGPROBS)]
    out += [(boundary_case(V, U), LOGITS) for V, U in ((256, 100), (254, 100), (260, 100), (256, 129))]
    out += [(public_case(False), LOGITS), (public_case(True), LOGITS)]
    out += [(hessian_case(1, 1, 8192, 1), LOGITS)]
    return out


def label_tokens(V, U, blank):
    """U distinct tokens: 1, V - 1 (V - 2 where the blank is V - 1) and U - 2 tokens at even spacing in between, none the blank."""
    hi = V - 2 if blank == V - 1 else V - 1
    toks = [1] + [min(hi - 1, (j + 1) * V // max(1, U - 1) + 5) for j in range(U - 2)] + [hi]
    toks = toks[:U] if U >= 2 else [hi]
    out = []
    for k in toks:
        while k == blank or k in out:
            k -= 1
        out.append(k)
    assert len(set(out)) == len(out) and all(0 < k < V for k in out) and blank not in out, (V, U, blank, out)
    return out


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(logits float32 [B,T,V], logprobs float32 (log-softmax of the logits, rounded once), labels int32 [B,U], label_length,
    logit_length int32 [B], v float32 [B,T,V]), all read-only."""
    c = case
    B = len(c.label_length)
    rng = np.random.default_rng(c.seed)
    draw_V, draw_U, draw_tokens = c.draw
    x = 3.0 * rng.standard_normal((B, c.T, draw_V))
    v = rng.standard_normal((B, c.T, draw_V))
    labels = np.zeros((B, c.U), np.int32)
    if c.U <= 8:  # vocabulary axis: the spread tokens
        toks = label_tokens(c.V, c.U, c.blank)
        for b in range(B):  # (token 1 and the last token stay in front: a shorter label_length drops a token in between)
            labels[b] = [toks[0], toks[-1]] + list(np.roll(toks[1:-1], b)) if c.U >= 2 else toks
    else:  # long labels: the first, the last and the last but one token of the draw, then random ones
        tok = np.array([k for k in range(draw_tokens) if k != c.blank])
        labels[:] = tok[rng.integers(0, len(tok), (B, draw_U))][:, : c.U]
        labels[:, :3] = (tok[0], tok[-1], tok[-2])
        if c.plant >= 0:
            labels[:, c.plant: c.plant + 4] = labels[0, c.plant]
    x, v = x[:, :, : c.V], v[:, :, : c.V]
    for b in range(B):
        x[b][:, c.blank] += 6.0
        x[b][:, np.unique(labels[b, : c.label_length[b]])] += 6.0
    x = x.astype(np.float32)
    if c.bf16:  # round to nearest even to 8 significant bits: what torch's .to(bfloat16) gives
        u = x.view(np.uint32).astype(np.uint64)
        x = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    lp = O.logit_to_logproba(x.astype(np.float64), 2).astype(np.float32)
    return dict(logits=_frozen(np.ascontiguousarray(x)), logprobs=_frozen(lp), labels=_frozen(labels),
                label_length=_frozen(np.array(c.label_length, np.int32)), logit_length=_frozen(np.array(c.logit_length, np.int32)),
                v=_frozen(np.ascontiguousarray(v.astype(np.float32))))


def _per_utterance(case, fn):
    """fn(inp_b, v_b) -> [1, len, V] on each utterance cut to its own frames and labels (the oracle's tables are dense in
    max(label_length) and T: an utterance of 100 labels beside one of 1024 would cost as much as the long one); zeros beyond."""
    inp = inputs(case)
    B = len(case.label_length)
    out = np.zeros((B, case.T, case.V))
    for b in range(B):
        n, ll = case.logit_length[b], case.label_length[b]
        one = dict(labels=inp["labels"][b: b + 1, : max(ll, 1)], label_length=inp["label_length"][b: b + 1],
                   logit_length=inp["logit_length"][b: b + 1], logits=inp["logits"][b: b + 1, :n], logprobs=inp["logprobs"][b: b + 1, :n])
        out[b, :n] = fn(one, inp["v"][b: b + 1, :n])[0]
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def hv_reference(case, kind, space=LOGITS, eps=2e-3):
    """[B,T,V] float64: H v of every utterance (zero rows beyond logit_length, zeros for an infeasible utterance)."""
    fd = fd64_exact if space == LOGITS else fd64_exact_logprobs
    return _per_utterance(case, lambda one, v: fd(kind, one, v, eps, case.blank))


@functools.lru_cache(maxsize=None)
def grad_reference(case, kind, space=LOGITS):
    """(loss [B], gradient [B,T,V]) of the float64 oracle."""
    inp = inputs(case)
    if space == LOGITS:
        d = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], case.blank)
        return _frozen(d.loss), _frozen(O.logits_gradient(d, inp["logits"]))
    d = O.LOSS_DATA[kind](inp["labels"], inp["logprobs"], inp["label_length"], inp["logit_length"], case.blank)
    return _frozen(d.loss), _frozen(d.gradient)


def hessian_reference(case, kind):
    """[B,T,V,T,V] float64, O.logits_hessian (not cached: up to 0.5 GB)."""
    inp = inputs(case)
    d = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], case.blank)
    return O.logits_hessian(d, inp["logits"])


def input_condition(case, ref):
    """The smallest, over feasible utterances with a non-zero product and over the blocks of 1024 consecutive tokens, of
    max_{t, k in block} |Hv_ref| / max|Hv_ref|: the tests require >= 1e-2, so that no column pass of a row loop can be dropped
    unseen by a comparison relative to max|Hv|."""
    worst = 1.0
    for b in range(ref.shape[0]):
        top = np.abs(ref[b]).max()
        if top == 0.0:
            continue
        for k0 in range(0, case.V, BLOCK):
            worst = min(worst, np.abs(ref[b][:, k0: k0 + BLOCK]).max() / top)
    return worst


def scan_logprob_seeds(seeds=range(400, 440)):
    """How the seeds of logprob_vocabulary_case were found: the seeds at which the float64 reference of both lattices meets the input
    condition in log-probability space.  `python -m tests.tools.second_order_reference` prints them."""
    for V in (1030, 4100):
        c0 = logprob_vocabulary_case(V)
        good = []
        for seed in seeds:
            c = c0._replace(seed=seed)
            worst = min(input_condition(c, hv_reference(c, kind, LOGPROBS)) for kind in KINDS)
            if worst >= 1e-2:
                good.append((seed, round(float(worst), 3)))
        print(f"V={V}: used seed {c0.seed}; seeds meeting the input condition (seed, smallest block maximum / max|Hv|): {good}")


def cross_frame_strength(case, kind):
    """Per utterance, the largest |H| between two different frames.  There the logits-space Hessian is the log-probability one (the
    rows of the latter sum to zero, so the softmax Jacobian leaves them alone), and that one depends on the blank's and the labels'
    columns only: a lattice over those few columns gives it without the [T V, T V] tensor."""
    inp = inputs(case)
    out = []
    for b, (ll, n) in enumerate(zip(case.label_length, case.logit_length)):
        cols = [case.blank] + [int(k) for k in inp["labels"][b, :ll]]
        lp = inp["logprobs"][b: b + 1, :n][:, :, cols].astype(np.float64)
        H = O.LOSS_DATA[kind](np.arange(1, ll + 1)[None, :], lp, np.array([ll]), np.array([n]), 0).hessian[0]
        out.append(max(np.abs(H[t, :, u, :]).max() for t in range(n) for u in range(n) if t != u))
    return out


def scan_hessian_seeds(seeds=range(800, 900)):
    """How the seeds of hessian_case were found: N(0, 3^2) logits with +6 on the labels mostly leave one dominant alignment, whose
    cross-frame blocks are far below the 1e-4 the kernel is held to; these seeds give every utterance a cross-frame entry >= 0.05
    (max|H| is ~0.2) in both lattices."""
    for shape in HESSIAN_SHAPES[:3]:
        c0 = hessian_case(*shape)
        good = []
        for seed in seeds:
            c = c0._replace(seed=seed)
            worst = min(min(cross_frame_strength(c, kind)) for kind in KINDS)
            if worst >= 0.05:
                good.append((seed, round(float(worst), 3)))
        print(f"{c0.name}: used seed {c0.seed}; seeds with every utterance's cross-frame maximum >= 0.05: {good}")


if __name__ == "__main__":
    scan_logprob_seeds()
    scan_hessian_seeds()
