"""Pins the float64 reference of the label posteriors (tests/tools/label_posterior_oracle.py) that the GPU tests compare against:
all five outputs against brute-force enumeration of every state sequence of the header's lattices, the plain CTC oracle where
there is no wildcard, and the closed forms of the definition.  No GPU."""
import itertools

import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import label_posterior_oracle as LP

W = LP.WILDCARD

# labels of at most three positions over tokens 1..3 (blank 0): a wildcard first, in the middle and last, adjacent wildcards, a
# repeated label with and without a wildcard between, no label at all
LABELS = [[], [W], [1], [W, W], [W, 1], [1, W], [1, 1], [1, 2], [W, 1, W], [1, W, 1], [2, W, 2], [W, W, 1], [1, W, W], [W, W, W],
          [1, 1, W], [W, 2, 2], [1, 2, 3], [2, 2, 2], [3, W, 1]]


def brute_force(kind, label, x, blank, wrt, weight):
    """(Z, label mass [T, L], blank mass [T]) by enumeration: every sequence of states, one per frame, weighs the product of its
    emissions; the mass of a path goes, frame by frame, to the position or to the blank that the header assigns the frame to."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    L = len(label)
    lse = np.log(np.exp(x).sum(axis=1))
    lp = x if wrt else x - lse[:, None]
    e = np.exp(np.concatenate([lp, (weight + (lse if wrt else 0.0 * lse))[:, None]], axis=1))
    wild = [k == W for k in label]
    col = [V if w else k for k, w in zip(label, wild)]
    z, lab, blk = 0.0, np.zeros((T, L)), np.zeros(T)
    if kind == "classic":
        S = 2 * L + 1
        ends = {S - 1, S - 2} if L else {0}

        def step_ok(a, b):  # from state a (-1: before the first frame) to state b
            if a < 0:
                return b in (0, 1)
            if b == a or b == a + 1:
                return True
            if b == a + 2 and b % 2 == 1:
                i = (b - 1) // 2
                return label[i] != label[i - 1] or wild[i] or wild[i - 1]
            return False
        for seq in itertools.product(range(S), repeat=T):
            if not all(step_ok(a, b) for a, b in zip((-1,) + seq[:-1], seq)) or seq[-1] not in ends:
                continue
            p = float(np.prod([e[t, col[(s - 1) // 2] if s % 2 else blank] for t, s in enumerate(seq)]))
            z += p
            for t, s in enumerate(seq):
                if s % 2:
                    lab[t, (s - 1) // 2] += p
                else:
                    blk[t] += p
        return z, lab, blk
    for moves in itertools.product((0, 1), repeat=T):  # simplified: a frame enters the next position or stays
        if sum(moves) != L:
            continue
        owner, l, p = [], 0, 1.0
        for t, m in enumerate(moves):
            if m:
                p *= e[t, col[l]]
                owner.append(l)
                l += 1
            elif l > 0 and wild[l - 1]:
                p *= e[t, V]
                owner.append(l - 1)
            else:
                p *= e[t, blank]
                owner.append(-1)
        z += p
        for t, i in enumerate(owner):
            if i < 0:
                blk[t] += p
            else:
                lab[t, i] += p
    return z, lab, blk


@pytest.mark.parametrize("wrt", [0, 1])
@pytest.mark.parametrize("kind", LP.KINDS)
def test_all_five_outputs_equal_the_enumeration_of_every_state_sequence(kind, wrt):
    rng = np.random.default_rng(17)
    V, worst, feasible, infeasible = 4, 0.0, 0, 0
    for label in LABELS:
        L = len(label)
        for T in range(1, 7):
            for weight in (0.0, -0.5):
                x = rng.standard_normal((T, V)) * 2.0
                if wrt:
                    x = x - 0.3  # log-"probabilities" that do not sum to one: e_w carries their log-sum-exp
                z, lab, blk = brute_force(kind, label, x, 0, wrt, weight)
                loss, post, bpost, dur, exf = LP.posterior_one(kind, label, x, 0, wrt, weight)
                assert post.shape == (T, L) and bpost.shape == (T,) and dur.shape == (L,) and exf.shape == (L,)
                if z == 0.0:
                    assert loss == np.inf and not post.any() and not bpost.any() and not dur.any() and np.all(exf == -1.0), (label, T)
                    infeasible += 1
                    continue
                feasible += 1
                rdur = (lab / z).sum(axis=0)
                rexf = (np.arange(T)[:, None] * lab / z).sum(axis=0) / rdur
                err = max([abs(np.exp(-loss) - z) / z, np.abs(post - lab / z).max(initial=0.0), np.abs(bpost - blk / z).max(),
                           np.abs(dur - rdur).max(initial=0.0), np.abs(exf - rexf).max(initial=0.0)])
                worst = max(worst, err)
                assert err <= 1e-12, (kind, label, T, weight, err)
                assert np.abs(post.sum(axis=1) + bpost - 1.0).max() <= 1e-12, "a frame's posteriors sum to 1"
                assert np.all(dur >= 1.0 - 1e-12), "every position holds at least one frame on every path"
                if kind == "simplified":
                    ordinary = np.asarray([k != W for k in label], dtype=bool)
                    assert np.abs(dur[ordinary] - 1.0).max(initial=0.0) <= 1e-12, "an ordinary label is entered exactly once"
    print(f"LABEL-POSTERIOR-ORACLE {kind} wrt={wrt}: worst |oracle - brute force| {worst:.3e} over {feasible} cases, {infeasible} infeasible")
    assert feasible > 100 and infeasible > 10


@pytest.mark.parametrize("blank", [0, 5])
@pytest.mark.parametrize("kind", LP.KINDS)
def test_without_a_wildcard_the_scatter_by_token_is_softmax_minus_the_ctc_gradient(kind, blank):
    inp = O.generate_ctc_loss_inputs(5, 14, 1, 6, max_label_length=5)
    labels, x, ll, tl = (np.asarray(inp[k]) for k in ("labels", "logits", "label_length", "logit_length"))
    if blank:  # tokens 1..5 become 0..4 around the blank 5
        labels = np.where(labels > 0, labels - 1, labels)
    ref = O.ctc_loss(kind, labels, x, ll, tl, blank)
    gref = O.logits_gradient(ref, x)
    sm = np.exp(O.logit_to_logproba(np.asarray(x, np.float64), 2))
    fin = np.isfinite(ref.loss)
    assert fin.any()
    for weight in (0.0, -1.5):  # nothing reads the weight
        loss, post, bpost, dur, exf = LP.label_posterior(kind, 0, labels, x, ll, tl, blank, weight)
        assert np.array_equal(np.isfinite(loss), fin)
        assert np.abs(loss[fin] - ref.loss[fin]).max() < 1e-10
        B, T, V = x.shape
        gamma = np.zeros((B, T, V))
        for b in range(B):
            for i in range(int(ll[b])):
                gamma[b, :, labels[b, i]] += post[b, :, i]
            gamma[b, :, blank] += bpost[b]
        live = (np.arange(T)[None, :] < np.asarray(tl)[:, None]) & fin[:, None]
        want = np.where(live[:, :, None], sm - gref, 0.0)
        assert np.abs(gamma - want).max() < 1e-10
        assert np.abs((post.sum(axis=2) + bpost)[live] - 1.0).max() < 1e-12
        assert not (post.sum(axis=2) + bpost)[~live].any()


@pytest.mark.parametrize("kind", LP.KINDS)
def test_padding_infeasible_and_empty_cases_follow_the_contract(kind):
    rng = np.random.default_rng(0)
    B, T, V, U = 8, 5, 6, 3
    x = rng.standard_normal((B, T, V))
    x[7, 2] = -np.inf
    #          feasible   ragged   no label   no frame   no frame+labels  too few frames  label > U   a dead row
    labels = [[W, 1, 2], [3, W, 0], [1, 1, 1], [1, 1, 1], [1, 2, 3],       [W, W, W],     [1, 2, 3], [W, 1, 0]]
    ll = [3, 2, 0, 0, 2, 3, 4, 2]
    tl = [5, 4, 3, 0, 0, 2, 5, 5]
    loss, post, bpost, dur, exf = LP.label_posterior(kind, 0, labels, x, ll, tl, 0, 0.0)
    assert post.shape == (B, T, U) and bpost.shape == (B, T) and dur.shape == (B, U) and exf.shape == (B, U)
    assert np.isfinite(loss[:4]).all() and np.all(loss[4:] == np.inf) and loss[3] == 0.0
    for b in range(B):
        Tb, Lb = (tl[b], ll[b]) if np.isfinite(loss[b]) else (0, 0)
        assert not post[b, Tb:].any() and not bpost[b, Tb:].any() and not post[b, :, Lb:].any()
        assert not dur[b, Lb:].any() and np.all(exf[b, Lb:] == -1.0)
        assert np.abs(post[b, :Tb].sum(axis=1) + bpost[b, :Tb] - 1.0).max(initial=0.0) < 1e-12
        assert np.all(dur[b, :Lb] >= 1.0 - 1e-12) and np.all((exf[b, :Lb] >= 0.0) & (exf[b, :Lb] <= Tb - 1))
    assert np.abs(bpost[2, :3] - 1.0).max() < 1e-12, "no label: every frame is blank"
    lsm = O.logit_to_logproba(x, 2)
    assert abs(loss[2] + lsm[2, :3, 0].sum()) < 1e-12
    # a label equal to the blank, beyond V, a negative value other than the wildcard
    for bad in (0, 6, -3, -1):
        out = LP.label_posterior(kind, 0, [[1, bad, 2]] * B, x, [2] * B, [5] * B, 0, 0.0)
        assert np.all(out[0] == np.inf) and not out[1].any() and not out[2].any() and not out[3].any() and np.all(out[4] == -1.0), bad
    # a smaller bound U cuts the outputs and makes the longer transcripts infeasible
    out = LP.label_posterior(kind, 0, labels, x, ll, tl, 0, 0.0, U=2)
    assert out[1].shape == (B, T, 2) and out[0][0] == np.inf and out[0][1] == loss[1] and np.array_equal(out[1][1], post[1, :, :2])
    # a lone wildcard on one frame owns it on both lattices, and the loss is -w whatever the logits
    out = LP.label_posterior(kind, 0, [[W, 0, 0]], x[:1], [1], [1], 0, -0.5)
    assert out[0][0] == 0.5 and out[1][0, 0, 0] == 1.0 and out[2][0, 0] == 0.0 and out[3][0, 0] == 1.0 and out[4][0, 0] == 0.0
    assert not out[1][0, 1:].any() and not out[2][0, 1:].any()
