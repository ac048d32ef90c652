"""N-best rescoring (ctc_amd_nbest_loss) against the float64 loss oracle, one hypothesis at a time:
    oracle.ctc_oracle.ctc_loss(kind, labels[:, n], x, label_length[:, n], logit_length, blank).

Tolerance (derived, not measured): |loss - oracle| <= 1e-4 + 1e-6 * |loss|, the bound of tests/test_gpu_alignment.py and
tests/test_gpu_beam_search.py for the same float32 row log-sum-exps plus one float32 rounding.  Where the oracle is +inf the result
is +inf exactly.  Every worst-case figure is printed before it is asserted."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from oracle import ctc_oracle as O
from tests import _ownership as OW

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KINDS = ("classic", "simplified")
KIND_ID = {"classic": 0, "simplified": 1}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tol(loss):
    return 1e-4 + 1e-6 * np.abs(loss)


def data_cls(kind):
    import tf_seq2seq_losses_amd as ctc
    return ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData


def run(kind, wrt, labels, x, ll, tl, blank, U=None, mask=None, both=False):
    """The public functions.  x: a NumPy array or a device tensor (taken as it stands).  Returns loss[B, N] as a NumPy array."""
    import tf_seq2seq_losses_amd as ctc
    xt = x if isinstance(x, torch.Tensor) else torch.tensor(x, device=DEV)
    args = (torch.tensor(np.asarray(labels, np.int32), device=DEV), xt, torch.tensor(np.asarray(ll, np.int32), device=DEV),
            torch.tensor(np.asarray(tl, np.int32), device=DEV), blank)
    kw = dict(max_label_length=U, hypothesis_mask=None if mask is None else torch.tensor(mask, device=DEV))
    if wrt:
        out = ctc.ctc_nbest_loss_from_logproba(*args, data_cls(kind), **kw)
    else:
        out = (ctc.classic_ctc_nbest_loss if kind == "classic" else ctc.simplified_ctc_nbest_loss)(*args, **kw)
    torch.cuda.synchronize()
    assert isinstance(out, ctc.CtcNbestLoss)
    shape = tuple(np.asarray(ll).shape)
    assert out.loss.shape == shape == out.log_posterior.shape and out.loss.dtype == out.log_posterior.dtype == torch.float32
    assert not out.loss.requires_grad and not out.log_posterior.requires_grad
    if both:
        return out.loss.cpu().numpy(), out.log_posterior.cpu().numpy()
    return out.loss.cpu().numpy()


def oracle(kind, wrt, labels, x, ll, tl, blank):
    """loss[B, N] in float64, one hypothesis at a time.  (The oracle indexes a row with every label position, padding included:
    padding is replaced by a valid token, which it does not read into the result.)"""
    labels, ll = np.asarray(labels), np.asarray(ll)
    V = x.shape[2]
    safe = np.where((labels < 0) | (labels >= V), (blank + 1) % V, labels)
    x64 = np.asarray(x, np.float64)
    cols = []
    for n in range(labels.shape[1]):
        if wrt:
            cols.append(np.asarray(O.LOSS_DATA[kind](safe[:, n], x64, ll[:, n], tl, blank, np.float64).loss))
        else:
            cols.append(np.asarray(O.ctc_loss(kind, safe[:, n], x64, ll[:, n], tl, blank).loss))
    return np.stack(cols, axis=1)


def check(got, want, what):
    inf = np.isposinf(want)
    assert not np.isnan(want).any(), (what, "the oracle has no answer here")
    assert np.array_equal(np.isposinf(got), inf), (what, "+inf where and only where the oracle is", got, want)
    err = np.abs(got[~inf] - want[~inf])
    worst = float(err.max()) if err.size else 0.0
    bound = tol(got[~inf])
    print(f"NBEST-MEASURE {what}: worst |loss - oracle| {worst:.3e}, smallest bound {bound.min() if err.size else 0.0:.3e}, "
          f"worst error / bound {float((err / bound).max()) if err.size else 0.0:.3f}, {int(inf.sum())} of {inf.size} infeasible, "
          f"largest loss {float(np.abs(want[~inf]).max()) if err.size else 0.0:.4g}", flush=True)
    assert np.all(err <= bound), (what, worst)


def draw_labels(rng, shape, V, blank):
    lab = rng.integers(0, V - 1, shape).astype(np.int32)
    return lab + (lab >= blank)


def same(a, b):
    return OW.same_bits(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@functools.lru_cache(maxsize=None)
def small(blank=0, V=6, seed=3):
    """The shape of the parity test: B=3, T=40, N=5, ragged lengths with 0 and 1, hypotheses of 0..12 labels; read-only."""
    rng = np.random.default_rng(seed + 10 * blank + V)
    B, T, N, W = 3, 40, 5, 12
    x = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([33, 0, 1], np.int32)
    labels = draw_labels(rng, (B, N, W), V, blank)
    ll = rng.integers(0, W + 1, (B, N)).astype(np.int32)
    ll[0, 0], ll[0, 1], ll[1, 0], ll[2, 0], ll[2, 1] = W, 0, 0, 1, 0
    for a in (x, tl, labels, ll):
        a.setflags(write=False)
    return x, tl, labels, ll


# ---- 1. parity ----
@pytest.mark.parametrize("blank", [0, 1, 5])
@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(kind, wrt, blank):
    x, tl, labels, ll = small(blank)
    if wrt:
        x = O.logit_to_logproba(np.asarray(x, np.float64), 2).astype(np.float32)
    want = oracle(kind, wrt, labels, x, ll, tl, blank)
    got = run(kind, wrt, labels, x, ll, tl, blank)
    check(got, want, f"parity {kind} wrt={wrt} blank={blank}")
    assert got[1, 0] == 0.0 and np.all(np.isposinf(got[1][ll[1] > 0]))  # no frames: 0 for the empty hypothesis, +inf otherwise


# ---- 2. label tiers ----
def needing(frames, U):
    """A label of at most U - 1 tokens (1 and 2 alternating behind a run of 1s) that needs exactly `frames` frames on the classic lattice."""
    L = U - 1
    r = frames - L
    assert 0 <= r and r + 1 <= L, (frames, U)
    lab = np.asarray([1] * (r + 1) + [2 - (i % 2) for i in range(L - r - 1)], np.int32)
    assert OW.frames_needed("classic", lab) == frames
    return lab


@functools.lru_cache(maxsize=None)
def tier_case(U):
    rng = np.random.default_rng(U)
    B, N, V = 2, 3, 8
    labels = np.ones((B, N, U), np.int32)
    labels[:, 0] = rng.integers(1, V, (B, U))
    labels[:, 1] = rng.integers(1, V, (B, U))
    ll = np.asarray([[U, U - 1, 0]] * B, np.int32)
    need = max(OW.frames_needed("classic", labels[b, n, :ll[b, n]]) for b in range(B) for n in range(2))
    T = need + 8
    tl = np.asarray([T, T - 3], np.int32)
    for b in range(B):
        lab = needing(int(tl[b]) + 1, U)
        labels[b, 2, :len(lab)] = lab
        ll[b, 2] = len(lab)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    return x, tl, labels, ll


@pytest.mark.parametrize("U", [64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_label_tiers(U):
    x, tl, labels, ll = tier_case(U)
    for kind in KINDS:
        want = oracle(kind, 0, labels, x, ll, tl, 0)
        got = run(kind, 0, labels, x, ll, tl, 0, U=U)
        check(got, want, f"tier U={U} T={x.shape[1]} {kind}")
        assert np.all(np.isfinite(got[:, :2])), "the hypotheses of U and U - 1 labels fit"
        if kind == "classic":
            assert np.all(np.isposinf(got[:, 2])), "one frame short"


# ---- 3. hypothesis counts ----
def test_hypothesis_counts():
    from tf_seq2seq_losses_amd import _lib
    G = _lib.NBEST_GROUP
    assert G >= 8
    rng = np.random.default_rng(11)
    B, T, V, W = 2, 30, 8, 10
    x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([T, 19], np.int32)
    labels = draw_labels(rng, (B, 64, W), V, 0)
    ll = rng.integers(0, W + 1, (B, 64)).astype(np.int32)
    for kind in KINDS:
        want = oracle(kind, 0, labels, x, ll, tl, 0)
        full = None
        for N in (1, 2, G - 1, G, G + 1, 2 * G + 1, 64):
            got = run(kind, 0, labels[:, :N], x, ll[:, :N], tl, 0)
            check(got, want[:, :N], f"counts {kind} N={N}")
            full = got if N == 64 else full
        for N in (1, G + 1):  # the same hypotheses in a shorter list: the same bits
            assert same(run(kind, 0, labels[:, :N], x, ll[:, :N], tl, 0), full[:, :N])


# ---- 4. isolation, bit for bit ----
@pytest.mark.parametrize("kind", KINDS)
def test_isolation(kind):
    rng = np.random.default_rng(5)
    B, T, V, N, W, U = 2, 30, 8, 7, 13, 12
    x = (1.5 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([T, 21], np.int32)
    labels = draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(1, U + 1, (B, N)).astype(np.int32)
    base = run(kind, 0, labels, x, ll, tl, 0, U=U)
    check(base, oracle(kind, 0, labels, x, ll, tl, 0), f"isolation {kind}")
    alone = np.concatenate([run(kind, 0, labels[:, n:n + 1], x, ll[:, n:n + 1], tl, 0, U=U) for n in range(N)], axis=1)
    assert same(alone, base), "scored alone"
    for s in range(1, N):  # every hypothesis at every position
        got = run(kind, 0, np.roll(labels, s, axis=1), x, np.roll(ll, s, axis=1), tl, 0, U=U)
        assert same(got, np.roll(base, s, axis=1)), s
    perm = rng.permutation(N)
    assert same(run(kind, 0, labels[:, perm], x, ll[:, perm], tl, 0, U=U), base[:, perm])
    # one malformed hypothesis: its own result is the contract's, the other six keep their bits
    empty = run(kind, 0, labels[:, :1], x, np.zeros((B, 1), np.int32), tl, 0, U=U)
    k = 3
    others = [n for n in range(N) if n != k]
    for name, tok, length in (("blank", 0, None), ("minus one", -1, None), ("V", V, None), ("too long", None, U + 1), ("negative", None, -2)):
        lab2, ll2 = labels.copy(), ll.copy()
        if tok is not None:
            lab2[:, k, 0] = tok
        if length is not None:
            ll2[:, k] = length
        got = run(kind, 0, lab2, x, ll2, tl, 0, U=U)
        assert same(got[:, others], base[:, others]), name
        if name == "negative":
            assert same(got[:, k:k + 1], empty) and np.all(np.isfinite(got[:, k])), name
        else:
            assert np.all(np.isposinf(got[:, k])), (name, got[:, k])


# ---- 5. formats ----
@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    for V in (6, 8):
        x, tl, labels, ll = small(0, V)
        B, T, _ = x.shape
        xt = torch.tensor(x, device=DEV)
        ref32 = run(kind, 0, labels, xt, ll, tl, 0)
        for dt in (torch.bfloat16, torch.float16):
            xh = xt.to(dt)
            want = oracle(kind, 0, labels, xh.float().cpu().numpy(), ll, tl, 0)  # on the values the element type converts to
            check(run(kind, 0, labels, xh, ll, tl, 0), want, f"formats {kind} V={V} {dt}")
            odd = torch.zeros(B * T * V + 1, dtype=dt, device=DEV)[1:].view(B, T, V)  # 2 bytes off: no 8-byte rows
            odd.copy_(xh)
            assert same(run(kind, 0, labels, odd, ll, tl, 0), run(kind, 0, labels, xh, ll, tl, 0)), (V, dt, "odd base")
        x_tm = xt.transpose(0, 1).contiguous()
        assert same(run(kind, 0, labels, x_tm.transpose(0, 1), ll, tl, 0), ref32), (V, "time-major")
        for sb, st in ((T * (V + 3) + 5, V + 3), (T * (V + 4), V + 4)):  # padded rows: element-wise, and (V = 8) vector accesses
            _, view, _ = OW.strided_storage(xt, sb, st, 0xFF)
            assert same(run(kind, 0, labels, view, ll, tl, 0), ref32), (V, sb, st)
        odd = torch.zeros(B * T * V + 1, device=DEV)[1:].view(B, T, V)  # 4 bytes off a 16-byte boundary: the element-wise path
        odd.copy_(xt)
        assert odd.data_ptr() % 16 != 0 and xt.data_ptr() % 16 == 0
        assert same(run(kind, 0, labels, odd, ll, tl, 0), ref32), (V, "odd base")
        check(ref32, oracle(kind, 0, labels, x, ll, tl, 0), f"formats {kind} V={V} float32")


# ---- 6. sharp and extreme inputs ----
@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits(kind):
    rng = np.random.default_rng(17)
    B, T, V, N, U = 2, 300, 32, 4, 40
    x = (6.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    tl = np.asarray([T, 211], np.int32)
    labels = draw_labels(rng, (B, N, U), V, 0)
    ll = np.asarray([[40, 17, 3, 0], [25, 40, 1, 8]], np.int32)
    check(run(kind, 0, labels, x, ll, tl, 0, U=U), oracle(kind, 0, labels, x, ll, tl, 0), f"sharp N(0, 6^2) {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_minus_infinity_and_huge_logits(kind):
    rng = np.random.default_rng(23)
    B, T, V, N, W = 3, 24, 6, 4, 8
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tl = np.asarray([T, T, 15], np.int32)
    labels = draw_labels(rng, (B, N, W), V, 0)
    ll = rng.integers(0, 7, (B, N)).astype(np.int32)
    xi = x.copy()
    xi[0, 3, 2] = -np.inf                 # single elements: no trouble
    xi[0, 9, 0] = -np.inf                 # ... the blank's among them
    xi[2, :, 4] = -np.inf                 # a token that is never possible: +inf for the hypotheses that use it
    xi[1, 7, :] = -np.inf                 # a frame that is -inf everywhere: +inf for every hypothesis of the utterance
    got = run(kind, 0, labels, xi, ll, tl, 0)
    assert not np.isnan(got).any()
    assert np.all(np.isposinf(got[1])), got[1]
    rows = [0, 2]
    with np.errstate(all="ignore"):
        want = oracle(kind, 0, labels[rows], xi[rows], ll[rows], tl[rows], 0)
    check(got[rows], want, f"-inf {kind}")
    uses4 = np.asarray([(labels[2, n, :ll[2, n]] == 4).any() for n in range(N)])
    assert np.array_equal(np.isposinf(got[2]), uses4 | np.isposinf(want[1]))
    xh = x.copy()
    xh[0] = 1e10                          # a uniform row of 1e10
    xh[1, :, 2] += 1e10                   # one token 1e10 above the rest
    xh[2] += 1e10                         # (float32: multiples of 1024 around 1e10)
    check(run(kind, 0, labels, xh, ll, tl, 0), oracle(kind, 0, labels, xh, ll, tl, 0), f"1e10 {kind}")


HARD = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "r04_case_*.npz")) + glob.glob(os.path.join(GOLDEN, "soak_case_*.npz")))


@pytest.mark.parametrize("name", HARD)
def test_committed_hard_cases(name):
    """The cases on which the float32 linear-domain sweeps lost mass, as hypothesis 0 of N = 4 beside three random relabelings of
    the same length.  (Read with np.load as tests/test_gpu_round3.py and test_gpu_round4.py read them: OW.case serves the generated
    cases of tests/_ownership.py, not these files.)"""
    d = np.load(os.path.join(GOLDEN, name), allow_pickle=True)
    x, lab0, L, tl = d["x"], d["labels"], int(d["ll"][0]), d["tl"]
    assert x.shape[0] == lab0.shape[0] == d["ll"].shape[0] == tl.shape[0] == 1, "every recorded case is one utterance"
    V = x.shape[2]
    rng = np.random.default_rng(len(name))
    labels = np.concatenate([lab0[:, None, :L], rng.integers(1, V, (1, 3, L)).astype(np.int32)], axis=1)
    ll = np.full((1, 4), L, np.int32)
    for kind in KINDS:
        check(run(kind, 0, labels, x, ll, tl, 0, U=L), oracle(kind, 0, labels, x, ll, tl, 0), f"{name} {kind} T_b={int(tl[0])} V={V} L={L}")


def test_every_hard_case_is_there():
    assert len(HARD) == 6, HARD


# ---- 7. beam round trip ----
def lp_numpy(loss):
    with np.errstate(all="ignore"):
        a = -loss.astype(np.float64)
        m = a.max(axis=1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        lse = m + np.log(np.exp(a - m).sum(axis=1, keepdims=True))
        return np.where(np.isposinf(loss), -np.inf, a - lse)


def check_log_posterior(loss, lp, what):
    assert not np.isnan(lp).any(), what
    want = lp_numpy(loss)
    assert np.array_equal(np.isneginf(lp), np.isneginf(want)), what
    fin = np.isfinite(want)
    # float32 arithmetic on the losses: a few units in the last place of the largest |loss| of the list
    bound = 8 * np.finfo(np.float32).eps * max(1.0, float(np.abs(loss[np.isfinite(loss)]).max()) if np.isfinite(loss).any() else 1.0)
    err = np.abs(lp[fin] - want[fin])
    print(f"NBEST-MEASURE {what}: worst |log_posterior - NumPy| {float(err.max()) if err.size else 0.0:.3e} (bound {bound:.3e})", flush=True)
    assert np.all(err <= bound), what


@pytest.mark.parametrize("kind", KINDS)
def test_beam_round_trip_exhaustive(kind):
    """T=5, V=3, W=64, K=2: nothing is pruned, so every finite beam score is -loss of its hypothesis."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, W, K = 6, 5, 3, 64, 2
    x = torch.tensor((2.0 * np.random.default_rng(7).standard_normal((B, T, V))).astype(np.float32), device=DEV)
    tl = torch.arange(B, dtype=torch.int32, device=DEV)
    search, rescore = ((ctc.classic_ctc_beam_search, ctc.classic_ctc_nbest_loss) if kind == "classic" else
                       (ctc.simplified_ctc_beam_search, ctc.simplified_ctc_nbest_loss))
    dec = search(x, tl, 0, beam_width=W, top_k=K, nbest=W)
    assert dec.labels.shape == (B, W, T)
    mask = torch.isfinite(dec.score)
    out = rescore(dec.labels, x, dec.label_length, tl, 0, hypothesis_mask=mask)
    torch.cuda.synchronize()
    score, loss, lp, m = dec.score.cpu().numpy(), out.loss.cpu().numpy(), out.log_posterior.cpu().numpy(), mask.cpu().numpy()
    assert np.all(np.isposinf(loss[~m])) and np.all(np.isfinite(loss[m])) and m.sum() >= 2 * B
    err = np.abs(score[m] + loss[m])
    print(f"NBEST-MEASURE beam exhaustive {kind}: {int(m.sum())} hypotheses, worst |score + loss| {err.max():.3e} "
          f"(bound {2 * tol(loss[m]).min():.3e})", flush=True)
    assert np.all(err <= 2 * tol(loss[m]))
    check(loss, np.where(m, oracle(kind, 0, dec.labels.cpu().numpy(), x.cpu().numpy(), dec.label_length.cpu().numpy(), tl.cpu().numpy(), 0),
                         np.inf), f"beam exhaustive {kind} against the oracle")
    check_log_posterior(loss, lp, f"beam exhaustive {kind}")
    assert np.all(np.abs(np.exp(lp.astype(np.float64)).sum(axis=1) - 1.0) < 1e-5)
    none = rescore(dec.labels, x, dec.label_length, tl, 0, hypothesis_mask=mask & (torch.arange(B, device=DEV)[:, None] != 2))
    torch.cuda.synchronize()
    assert np.all(np.isposinf(none.loss[2].cpu().numpy())) and np.all(np.isneginf(none.log_posterior[2].cpu().numpy()))
    assert not np.isnan(none.log_posterior.cpu().numpy()).any()
    assert same(none.loss[3:].cpu().numpy(), loss[3:])


@pytest.mark.parametrize("kind", KINDS)
def test_beam_round_trip_pruned(kind):
    """T=60, V=16, W=8, K=4: the beam sums a subset of the alignments, so its score is a lower bound of -loss."""
    import tf_seq2seq_losses_amd as ctc
    B, T, V, W, K = 3, 60, 16, 8, 4
    rng = np.random.default_rng(31)
    xn = (2.0 * rng.standard_normal((B, T, V))).astype(np.float32)
    xn[..., 0] += 3.0
    x = torch.tensor(xn, device=DEV, requires_grad=True)  # logits that require grad are accepted; the result is detached
    tl = torch.tensor([T, 41, 1], dtype=torch.int32, device=DEV)
    search, rescore = ((ctc.classic_ctc_beam_search, ctc.classic_ctc_nbest_loss) if kind == "classic" else
                       (ctc.simplified_ctc_beam_search, ctc.simplified_ctc_nbest_loss))
    dec = search(x, tl, 0, beam_width=W, top_k=K, nbest=W)
    mask = torch.isfinite(dec.score)
    out = rescore(dec.labels, x, dec.label_length, tl, 0, hypothesis_mask=mask)
    torch.cuda.synchronize()
    assert not out.loss.requires_grad
    score, loss, lp, m = dec.score.cpu().numpy(), out.loss.cpu().numpy(), out.log_posterior.cpu().numpy(), mask.cpu().numpy()
    assert np.all(np.isposinf(loss[~m])) and np.all(np.isfinite(loss[m]))
    gap = -loss[m] - score[m]
    print(f"NBEST-MEASURE beam pruned {kind}: -loss - score between {gap.min():.3e} and {gap.max():.3e}", flush=True)
    assert np.all(score[m] <= -loss[m] + tol(loss[m]))
    check(loss, np.where(m, oracle(kind, 0, dec.labels.cpu().numpy(), xn, dec.label_length.cpu().numpy(), tl.cpu().numpy(), 0), np.inf),
          f"beam pruned {kind} against the oracle")
    check_log_posterior(loss, lp, f"beam pruned {kind}")


# ---- 8. ownership ----
GUARD = 64


def raw_call(kind, x, labels, ll, tl, blank, U, fill=0xA5, ws_pattern=0x00, ws_bytes=4096, wrt=0):
    """The C ABI with every buffer under the test's control: the losses between two guard regions, a workspace it has no use for."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = x.shape
    N, W = labels.shape[1], labels.shape[2]
    buf = OW.filled((GUARD + B * N + GUARD,), torch.float32, fill, DEV)
    ws = OW.workspace(ws_bytes, ws_pattern)
    rc = lib.ctc_amd_nbest_loss(KIND_ID[kind], wrt, x.data_ptr(), OW._dt(x), x.stride(0), x.stride(1), labels.data_ptr(), W, ll.data_ptr(),
                                tl.data_ptr(), blank, B, T, V, U, N, buf[GUARD:].data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ctc_amd_last_error()
    torch.cuda.synchronize()
    assert bool(OW.keeps_prefill(buf[:GUARD], fill).all()) and bool(OW.keeps_prefill(buf[GUARD + B * N:], fill).all()), "guards"
    assert bool((ws == ws_pattern).all()), "the workspace is not written"
    return buf[GUARD:GUARD + B * N].clone().view(B, N)


@pytest.mark.parametrize("kind", KINDS)
def test_unowned_memory_changes_no_bit(kind):
    x, tl, labels, ll = small(0, 8)
    B, T, V = x.shape
    N, W = labels.shape[1], labels.shape[2]
    xt, lab, llt, tlt = (torch.tensor(np.array(a), device=DEV) for a in (x, labels, ll, tl))
    clean = raw_call(kind, xt, lab, llt, tlt, 0, W, fill=0x00)
    check(clean.cpu().numpy(), oracle(kind, 0, labels, x, ll, tl, 0), f"ownership {kind}")
    for value in OW.poison_values(torch.float32):
        assert OW.same_bits(raw_call(kind, OW.poison_padding(xt, tl, value), lab, llt, tlt, 0, W), clean), value
    poisoned = OW.poison_labels(lab.view(B * N, W), ll.reshape(-1), OW.label_poison_cycle(V, 0)).view(B, N, W)
    assert OW.same_bits(raw_call(kind, xt, poisoned, llt, tlt, 0, W), clean), "label tails"
    for sb, st in ((T * (V + 3) + 5, V + 3), (V + 4, B * (V + 4))):  # padded rows; time-major with padded rows
        storage, view, owned = OW.strided_storage(xt, sb, st)
        for value in OW.poison_values(torch.float32):
            gaps = OW.poison_gaps(storage, owned, value).as_strided((B, T, V), (sb, st, 1))
            assert OW.same_bits(raw_call(kind, gaps, lab, llt, tlt, 0, W), clean), (sb, st, value)
    for pattern in OW.BYTE_PATTERNS:  # the outputs' contents on entry and every workspace prefill
        assert OW.same_bits(raw_call(kind, xt, lab, llt, tlt, 0, W, fill=pattern, ws_pattern=pattern), clean), pattern
    # a null workspace is accepted
    from tf_seq2seq_losses_amd import _lib
    out = OW.filled((B, N), torch.float32, 0xA5, DEV)
    rc = _lib.load().ctc_amd_nbest_loss(KIND_ID[kind], 0, xt.data_ptr(), 0, T * V, V, lab.data_ptr(), W, llt.data_ptr(), tlt.data_ptr(), 0,
                                        B, T, V, W, N, out.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and OW.same_bits(out, clean)


# ---- 9. graph capture ----
@pytest.mark.parametrize("kind", KINDS)
def test_nbest_loss_in_a_hip_graph(kind):
    """One launch on one stream: captured once and replayed on new inputs in the same buffers, the same bits as the eager call."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    src = small(0, 8)
    B, T, V = src[0].shape
    N, W = src[2].shape[1], src[2].shape[2]
    x = torch.zeros((B, T, V), device=DEV)
    tl = torch.zeros(B, dtype=torch.int32, device=DEV)
    labels = torch.ones((B, N, W), dtype=torch.int32, device=DEV)
    ll = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    loss = torch.zeros((B, N), device=DEV)

    def call():
        rc = lib.ctc_amd_nbest_loss(KIND_ID[kind], _lib.WRT_LOGITS, x.data_ptr(), _lib.F32, T * V, V, labels.data_ptr(), W, ll.data_ptr(),
                                    tl.data_ptr(), 0, B, T, V, W, N, loss.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ctc_amd_last_error()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for dst, a in zip((x, tl, labels, ll), src):
        dst.copy_(torch.from_numpy(np.array(a)))
    loss.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = loss.cpu().numpy().copy()
    loss.zero_()
    call()
    torch.cuda.synchronize()
    assert same(got, loss.cpu().numpy())
    check(got, oracle(kind, 0, src[2], src[0], src[3], src[1], 0), f"graph replay {kind}")
