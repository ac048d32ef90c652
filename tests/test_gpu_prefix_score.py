"""CTC prefix scores on the device (ctc_amd_prefix_rows / _extend / _score and the label-synchronous beam search on top of them)
against the float64 oracle tests/tools/prefix_oracle.py.  Small shapes at which the kernels take every path: T around the extend
kernel's blocks of 64 frames and the score kernel's chunks of 8, V around its tiles of 64 columns, N around its groups of 8.
The bound is that of tests/test_gpu_nbest_loss.py: 1e-4 + 1e-6 |oracle| where finite, -inf exactly, no NaN."""
import itertools

import numpy as np
import pytest
import torch

from tests.tools import prefix_oracle as PO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("classic", "simplified")


def tol(ref):
    return 1e-4 + 1e-6 * np.abs(ref)


def make_scorer(kind, x, tl, blank, logproba=False):
    import tf_seq2seq_losses_amd as ctc
    tl = torch.as_tensor(tl, dtype=torch.int32, device=DEV)
    if logproba:
        return ctc.ctc_prefix_scorer_from_logproba(x, tl, blank, simplified=kind == "simplified")
    return (ctc.classic_ctc_prefix_scorer if kind == "classic" else ctc.simplified_ctc_prefix_scorer)(x, tl, blank)


def check(got, want, what, factor=1.0):
    got = np.asarray(got, dtype=np.float64)
    assert not np.isnan(got).any(), f"{what}: NaN"
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: -inf pattern differs at {np.argwhere(np.isfinite(got) != fin)[:5].tolist()}"
    assert (got[~fin] == -np.inf).all(), what
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        worst = (err / tol(want[fin])).max()
        print(f"{what}: worst error / bound = {worst:.3f} (max abs {err.max():.3g})")
        assert (err <= factor * tol(want[fin])).all(), f"{what}: {worst:.3f} x the bound"


def token_plan(V, blank, N, steps, rng):
    """[steps][N] tokens: immediate repeats, a token returning after one other, and in slots 2 and 3 a blank and a token outside
    the vocabulary (both kill the slot from there on)."""
    toks = [c for c in range(V) if c != blank]
    a, b, c = toks[0], toks[len(toks) // 2], toks[-1]
    base = [[a, a, b, a, b, b], [b, c, b, b, a, c], [c, a, blank, a, b, c], [a, V + 3, b, c, a, a], [c, c, c, a, c, b]]
    plan = np.zeros((steps, N), dtype=np.int32)
    for n in range(N):
        seq = base[n] if n < len(base) else [int(rng.choice(toks)) for _ in range(6)]
        plan[:, n] = seq[:steps]
    return plan


def run_plan(kind, x, tl, blank, N, plan, xf=None, logproba=False, check_at=(0, 1, 2, 6), what=""):
    """Drives the device scorer and the oracle along `plan` (slot n extends the empty prefix by plan[:, n]) and compares scores
    and full scores after the steps in check_at.  xf: the float64 values the oracle sees (default: x as float64)."""
    B, T, V = x.shape
    scorer = make_scorer(kind, x, tl, blank, logproba)
    xf = x.detach().cpu().double().numpy() if xf is None else xf
    lps = [xf[b] if logproba else PO.log_softmax(xf[b]) for b in range(B)]
    state = scorer.initial_state(N)
    ref = [[PO.empty_state(lps[b], int(tl[b]), blank) if n == 0 else None for n in range(N)] for b in range(B)]
    out = {}
    for step in range(len(plan) + 1):
        if step in check_at:
            sc = scorer.score(state).cpu().numpy()
            want = np.array([[PO.scores(kind, lps[b], int(tl[b]), blank, ref[b][n]) for n in range(N)] for b in range(B)])
            check(sc, want, f"{what} scores after {step} steps")
            wfull = np.array([[PO.full_score(ref[b][n]) for n in range(N)] for b in range(B)])
            check(state.full_score.cpu().numpy(), wfull, f"{what} full_score after {step} steps")
            alive = np.array([[ref[b][n] is not None for n in range(N)] for b in range(B)])
            assert np.array_equal(state.length.cpu().numpy() >= 0, alive)
            out[step] = (sc, state.full_score.cpu().numpy())
        if step == len(plan):
            break
        parent = torch.full((B, N), 0 if step == 0 else -1, dtype=torch.int32, device=DEV)
        if step > 0:
            parent[:] = torch.arange(N, dtype=torch.int32, device=DEV)
        token = torch.as_tensor(plan[step], device=DEV).expand(B, N).contiguous()
        state = scorer.extend(state, parent, token)
        ref = [[PO.extend(kind, lps[b], int(tl[b]), blank, ref[b][0 if step == 0 else n], int(plan[step, n])) for n in range(N)]
               for b in range(B)]
    return out


def lengths(T):
    return np.array([T, 0, min(1, T), max(T - 3, 0)], dtype=np.int32)


SHAPES = [(1, 2, 1), (2, 3, 8), (3, 64, 9), (64, 65, 8), (65, 257, 9), (130, 3, 1), (130, 65, 9)]


@pytest.mark.parametrize("last_blank", [False, True])
@pytest.mark.parametrize("T,V,N", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_scores_against_oracle(kind, T, V, N, last_blank):
    rng = np.random.default_rng(T * 1000 + V)
    blank = V - 1 if last_blank else 0
    x = torch.tensor(rng.standard_normal((4, T, V), dtype=np.float32), device=DEV)
    run_plan(kind, x, lengths(T), blank, N, token_plan(V, blank, N, 6, rng), what=f"{kind} T={T} V={V} N={N}")


@pytest.mark.parametrize("kind", KINDS)
def test_sharp_logits_long_utterance(kind):
    rng = np.random.default_rng(7)
    T, V, N = 300, 65, 8
    x = torch.tensor((6.0 * rng.standard_normal((2, T, V))).astype(np.float32), device=DEV)
    run_plan(kind, x, np.array([T, T - 37], dtype=np.int32), 0, N, token_plan(V, 0, N, 6, rng), what=f"{kind} sharp")


@pytest.mark.parametrize("kind", KINDS)
def test_minus_infinity_and_huge_logits(kind):
    rng = np.random.default_rng(11)
    T, V, N = 65, 65, 9
    x = rng.standard_normal((4, T, V), dtype=np.float32)
    x[0][rng.random((T, V)) < 0.2] = -np.inf              # scattered impossible tokens
    x[1, 5, :] = -np.inf                                  # a frame that is -inf everywhere: nothing survives it
    x[2] = 1e10 - 1024.0 * rng.integers(0, 4, (T, V))     # rows of 1e10
    x[3, ::2] += 1e10
    x[3, :, 0] = -np.inf                                  # ... and a blank that never happens
    run_plan(kind, torch.tensor(x, device=DEV), np.array([T, T, T, T - 1], dtype=np.int32), 0, N, token_plan(V, 0, N, 6, rng),
             what=f"{kind} -inf / 1e10")


@pytest.mark.parametrize("kind", KINDS)
def test_full_score_is_minus_nbest_loss(kind):
    import tf_seq2seq_losses_amd as ctc
    rng = np.random.default_rng(5)
    B, T, V, N = 3, 65, 17, 9
    x = torch.tensor(rng.standard_normal((B, T, V), dtype=np.float32), device=DEV)
    tl = torch.tensor([T, 40, 9], dtype=torch.int32, device=DEV)
    plan = rng.integers(1, V, (6, N)).astype(np.int32)
    plan[1] = plan[0]  # an immediate repeat in every hypothesis
    scorer = make_scorer(kind, x, tl, 0)
    state = scorer.initial_state(N)
    for step in range(6):
        parent = torch.zeros((B, N), dtype=torch.int32, device=DEV) if step == 0 else torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N)
        state = scorer.extend(state, parent.contiguous(), torch.as_tensor(plan[step], device=DEV).expand(B, N).contiguous())
    labels = torch.as_tensor(plan.T.copy(), device=DEV).expand(B, N, 6).contiguous()
    fn = ctc.classic_ctc_nbest_loss if kind == "classic" else ctc.simplified_ctc_nbest_loss
    loss = fn(labels, x, torch.full((B, N), 6, dtype=torch.int32, device=DEV), tl, 0).loss
    check(state.full_score.cpu().numpy(), -loss.cpu().double().numpy(), f"{kind} full_score against -nbest_loss", factor=2.0)


@pytest.mark.parametrize("kind", KINDS)
def test_identity_on_device_outputs(kind):
    """psi(g) = P(g) + sum_c psi(g . c), every term from the device; each side is within the bound of its exact value and a
    log-sum-exp moves by no more than its largest argument does: twice the bound."""
    rng = np.random.default_rng(9)
    B, T, V, N = 3, 66, 65, 9
    x = torch.tensor(rng.standard_normal((B, T, V), dtype=np.float32), device=DEV)
    scorer = make_scorer(kind, x, [T, 10, 1], V - 1)
    state = scorer.initial_state(N)
    sc = scorer.score(state)
    one = torch.logsumexp(torch.cat([state.full_score[:, :1].double(), sc[:, 0].double()], 1), 1).cpu().numpy()
    check(one, np.zeros(B), f"{kind} 1 = P(empty) + sum psi(c)", factor=2.0)
    for step in range(4):
        parent = torch.as_tensor(rng.integers(0, 1 if step == 0 else N, (B, N)).astype(np.int32), device=DEV)
        token = torch.as_tensor(rng.integers(0, V - 1, (B, N)).astype(np.int32), device=DEV)
        if step > 0:
            token[:, 0] = state.last_token[:, 0].clamp(min=0)
            parent[:, 0] = 0  # an immediate repeat
        psi_g = sc.gather(1, parent.long()[:, :, None].expand(-1, -1, V)).gather(2, token.long()[:, :, None])[:, :, 0]
        state = scorer.extend(state, parent, token)
        sc = scorer.score(state)
        rhs = torch.logsumexp(torch.cat([state.full_score[:, :, None].double(), sc.double()], 2), 2)
        check(rhs.cpu().numpy(), psi_g.cpu().double().numpy(), f"{kind} identity at step {step + 1}", factor=2.0)


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_isolation_and_determinism(kind):
    rng = np.random.default_rng(13)
    B, T, V = 2, 70, 130
    x = torch.tensor(rng.standard_normal((B, T, V), dtype=np.float32), device=DEV)
    scorer = make_scorer(kind, x, [T, 33], 0)
    seq = [5, 5, 9, 5]

    def run(N, slot, others):
        """The hypothesis `seq` in `slot` of a beam of N; the other slots extend by others(step, n) (a token, or None: dead)."""
        state = scorer.initial_state(N)
        for step, c in enumerate(seq):
            parent = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
            token = torch.zeros((B, N), dtype=torch.int32, device=DEV)
            for n in range(N):
                o = c if n == slot else others(step, n)
                if o is not None:
                    parent[:, n] = 0 if step == 0 else n
                    token[:, n] = o
            state = scorer.extend(state, parent, token)
        return scorer.score(state)[:, slot], state.full_score[:, slot]

    sc0, f0 = run(1, 0, None)
    sc_again, f_again = run(1, 0, None)
    assert np.array_equal(bits(sc0), bits(sc_again)) and np.array_equal(bits(f0), bits(f_again)), "two runs differ"
    neighbours = {"dead": lambda step, n: None, "alive": lambda step, n: 1 + (n * 7 + step) % (V - 1),
                  "malformed": lambda step, n: (0, V, -5, 3)[(n + step) % 4]}
    for N, slot in ((8, 0), (8, 7), (9, 8), (9, 3)):
        for name, others in neighbours.items():
            sc, f = run(N, slot, others)
            assert np.array_equal(bits(sc), bits(sc0)) and np.array_equal(bits(f), bits(f0)), (N, slot, name)

    # permuted and repeated parents: the permuted / repeated results, bit for bit
    N = 9
    state = scorer.initial_state(N)
    state = scorer.extend(state, torch.zeros((B, N), dtype=torch.int32, device=DEV),
                          torch.arange(1, N + 1, dtype=torch.int32, device=DEV).expand(B, N).contiguous())
    token = torch.as_tensor(rng.integers(1, V, (B, N)).astype(np.int32), device=DEV)
    ident = torch.arange(N, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    base = scorer.extend(state, ident, token)
    base_sc = scorer.score(base)
    perm = torch.as_tensor(np.array([[3, 3, 0, 8, 1, 1, 1, 7, 2], [8, 7, 6, 5, 4, 3, 2, 1, 0]], dtype=np.int32), device=DEV)
    tok_p = token.gather(1, perm.long())
    got = scorer.extend(state, perm, tok_p)
    got_sc = scorer.score(got)
    # (b, n) of `got` is parent perm[b, n] with token[b, perm[b, n]]: slot perm[b, n] of `base`
    assert np.array_equal(bits(got.full_score), bits(base.full_score.gather(1, perm.long())))
    assert np.array_equal(bits(got_sc), bits(base_sc.gather(1, perm.long()[:, :, None].expand(-1, -1, V))))
    assert torch.equal(got.last_token, base.last_token.gather(1, perm.long())) and torch.equal(got.length, base.length.gather(1, perm.long()))


@pytest.mark.parametrize("kind", KINDS)
def test_formats(kind):
    rng = np.random.default_rng(17)
    B, T, V, N = 3, 66, 67, 9
    x32 = torch.tensor(rng.standard_normal((B, T, V), dtype=np.float32), device=DEV)
    tl = np.array([T, 31, 2], dtype=np.int32)
    plan = token_plan(V, 0, N, 2, rng)
    for dt in (torch.bfloat16, torch.float16):
        xh = x32.to(dt)
        run_plan(kind, xh, tl, 0, N, plan, xf=xh.float().cpu().double().numpy(), check_at=(0, 2), what=f"{kind} {dt}")
    tm = x32.transpose(0, 1).contiguous().transpose(0, 1)  # time-major memory behind a batch-major view
    assert not tm.is_contiguous()
    a = run_plan(kind, tm, tl, 0, N, plan, check_at=(0, 2), what=f"{kind} time-major")
    b = run_plan(kind, x32, tl, 0, N, plan, check_at=(0, 2), what=f"{kind} contiguous")
    assert np.array_equal(a[2][0], b[2][0], equal_nan=True)
    # log-probabilities as they stand: the oracle's result on them, and the logits form within twice the bound
    lp = torch.log_softmax(x32.double(), 2).float()
    c = run_plan(kind, lp, tl, 0, N, plan, logproba=True, check_at=(0, 2), what=f"{kind} from logproba")
    fin = np.isfinite(b[2][0])
    assert np.array_equal(np.isfinite(c[2][0]), fin)
    assert (np.abs(c[2][0][fin] - b[2][0][fin]) <= 2 * tol(b[2][0][fin])).all()


@pytest.mark.parametrize("kind", KINDS)
def test_label_sync_beam_search_is_exhaustive_when_wide_enough(kind):
    """V = 4, T = 6, at most 3 labels: 3 + 9 + 27 prefixes, none pruned at beam_width = 32, so the result is the enumeration's."""
    import tf_seq2seq_losses_amd as ctc
    rng = np.random.default_rng(21)
    B, T, V, W, L = 3, 6, 4, 32, 3
    xn = rng.standard_normal((B, T, V), dtype=np.float32) * 2
    xn[..., 0] += 1.0
    scorer = make_scorer(kind, torch.tensor(xn, device=DEV), [T, T, 4], 0)
    res = ctc.ctc_label_sync_beam_search(scorer, W, L)
    banned = 2
    res_b = ctc.ctc_label_sync_beam_search(scorer, W, L, extra_score=lambda st: torch.where(
        torch.arange(V, device=DEV) == banned, -torch.inf, 0.0).expand(B, W, V))
    for b, Tb in enumerate([T, T, 4]):
        seqs = {s: w for s, w in PO.enumerate_sequences(kind, PO.log_softmax(xn[b].astype(np.float64)), Tb, 0).items() if len(s) <= L}
        for r, allowed in ((res, seqs), (res_b, {s: w for s, w in seqs.items() if banned not in s})):
            best = max(allowed, key=allowed.get)
            n = int(r.label_length[b, 0])
            assert tuple(r.labels[b, 0, :n].tolist()) == best, (b, r.labels[b, 0].tolist(), best)
            assert abs(float(r.score[b, 0]) - np.log(allowed[best])) <= tol(np.log(allowed[best]))
            assert (r.score[b, :-1] >= r.score[b, 1:]).all()
        assert not (res_b.labels[b] == banned).any()
        # every sequence of the enumeration is in the result with its probability (40 candidates, the 32 best are kept)
        ranked = sorted(seqs.values(), reverse=True)[:W]
        check(res.score[b].cpu().numpy(), np.log(np.array(ranked)), f"{kind} ranked probabilities of utterance {b}")


@pytest.mark.parametrize("kind", KINDS)
def test_one_step_in_a_hip_graph(kind):
    rng = np.random.default_rng(23)
    B, T, V, N = 3, 70, 65, 9
    x = torch.tensor(rng.standard_normal((B, T, V), dtype=np.float32), device=DEV)
    scorer = make_scorer(kind, x, [T, 20, 64], 0)
    state = scorer.initial_state(N)
    parent = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    token = torch.arange(1, N + 1, dtype=torch.int32, device=DEV).expand(B, N).contiguous()
    eager = scorer.extend(state, parent, token)
    eager_sc = scorer.score(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        scorer.score(scorer.extend(state, parent, token))
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = scorer.extend(state, parent, token)
        sc = scorer.score(st)
    for _ in range(2):
        sc.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(sc), bits(eager_sc)) and np.array_equal(bits(st.full_score), bits(eager.full_score))
