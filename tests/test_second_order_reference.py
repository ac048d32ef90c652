"""The float64 references of tests/test_gpu_second_order_axes.py (tests/tools/second_order_reference.py), pinned without a GPU:

  * convergence: at every shape the GPU module uses, the Richardson-extrapolated central difference of the oracle's gradient at
    eps = 2e-3 and at eps = 1e-3 agree to 1e-5 of max|Hv| per utterance, a tenth of the bar the kernels are held to;
  * log-probability space: the same difference of loss_data.gradient, the log-probabilities perturbed as free variables, is the
    contraction of the oracle's own Hessian (base_loss.py:186-260) with the direction;
  * the dense-Hessian cases have several alignments: cross-frame blocks comparable to max|H|, and the two lattices differ;
  * the inputs: label tokens at both ends and across the vocabulary, none the blank, and the input condition of the GPU module.
"""
import numpy as np
import pytest

from oracle import ctc_oracle as O
from tests.tools import second_order_reference as R

CASES = R.hvp_cases()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case,space", CASES, ids=[f"{c.name} {s}" for c, s in CASES])
def test_reference_has_converged(kind, case, space):
    a, b = R.hv_reference(case, kind, space, 2e-3), R.hv_reference(case, kind, space, 1e-3)
    loss = R.grad_reference(case, kind, space)[0]
    for u in range(a.shape[0]):
        top = np.abs(a[u]).max()
        if not np.isfinite(loss[u]):
            assert top == 0.0 and np.abs(b[u]).max() == 0.0
            continue
        assert top > 0.0
        assert np.abs(a[u] - b[u]).max() < 1e-5 * top, (u, np.abs(a[u] - b[u]).max() / top, top)
        assert np.all(a[u, case.logit_length[u]:] == 0.0)
    assert R.input_condition(case, a) >= 1e-2, R.input_condition(case, a)


@pytest.mark.parametrize("kind", R.KINDS)
def test_log_probability_reference_is_the_oracle_hessian_contracted(kind):
    B, T, V = 3, 12, 5
    inp = O.generate_ctc_loss_inputs(B, T, 2, V)
    lp = O.logit_to_logproba(inp["logits"].astype(np.float64), 2).astype(np.float32)
    v = np.random.default_rng(102).standard_normal((B, T, V)).astype(np.float32)
    refd = O.LOSS_DATA[kind](inp["labels"], lp, inp["label_length"], inp["logit_length"], 0)
    want = np.einsum("btkuj,buj->btk", refd.hessian, v.astype(np.float64))
    got = R.fd64_exact_logprobs(kind, dict(inp, logprobs=lp), v)
    assert np.abs(want).max() > 0.1
    for u in range(B):
        assert np.abs(got[u] - want[u]).max() < 1e-5 * np.abs(want[u]).max(), u
    # and in logits space: the chain rule through the log-softmax (oracle.logits_hessian) against the logits difference
    ref = O.ctc_loss(kind, inp["labels"], inp["logits"], inp["label_length"], inp["logit_length"], 0)
    want_x = np.einsum("btkuj,buj->btk", O.logits_hessian(ref, inp["logits"]), v.astype(np.float64))
    got_x = R.fd64_exact(kind, inp, v)
    for u in range(B):
        assert np.abs(got_x[u] - want_x[u]).max() < 1e-5 * np.abs(want_x[u]).max(), u


@pytest.mark.parametrize("B,T,V,U", R.HESSIAN_SHAPES[:3])
def test_hessian_cases_have_cross_frame_blocks_and_tell_the_lattices_apart(B, T, V, U):
    """A case with as many labels as frames has one alignment: every block between two frames is zero and classic = simplified.  Here
    every utterance's largest cross-frame entry is at least a quarter of max|H| in both lattices, and the lattices differ by more than
    ten times the 1e-4 the kernel is held to (V = 909, 912: a hundred times).  At V = 909 and 912 this is read off O.logits_hessian itself, which also pins
    cross_frame_strength (the same blocks from a lattice over the blank's and the labels' columns alone); at V = 4100, where the
    oracle tensor takes 7-15 s, off cross_frame_strength alone."""
    case = R.hessian_case(B, T, V, U)
    n = case.logit_length
    strength = {kind: R.cross_frame_strength(case, kind) for kind in R.KINDS}
    if V < 1000:
        H = {kind: R.hessian_reference(case, kind) for kind in R.KINDS}
        for kind in R.KINDS:
            full = [max(np.abs(H[kind][b, t, :, u, :]).max() for t in range(n[b]) for u in range(n[b]) if t != u) for b in range(B)]
            assert np.allclose(full, strength[kind], rtol=1e-6, atol=0)  # (the float32 log-probabilities sum to 1 within 1e-7), (kind, full, strength[kind])
            top = [np.abs(H[kind][b]).max() for b in range(B)]
            assert all(f >= 0.25 * m for f, m in zip(full, top)), (kind, full, top)
            assert all(np.all(H[kind][b, n[b]:] == 0) and np.all(H[kind][b, :, :, n[b]:] == 0) for b in range(B))
        assert np.abs(H["classic"] - H["simplified"]).max() > 1e-2
    else:
        assert all(min(strength[kind]) >= 0.1 for kind in R.KINDS), strength  # (max|H| <= 0.25: a variance of an indicator)
        assert abs(strength["classic"][0] - strength["simplified"][0]) > 1e-3, strength


def test_label_tokens_span_the_vocabulary():
    for V in R.VOCABULARIES:
        for which in ("first", "last", "mid"):
            c = R.vocabulary_case(V, which)
            toks = R.label_tokens(c.V, c.U, c.blank)
            assert 1 in toks and (V - 1 in toks or (c.blank == V - 1 and V - 2 in toks))
            assert any(V // 4 < k < 3 * V // 4 for k in toks)
            inp = R.inputs(c)
            assert inp["logits"].shape == (2, c.T, V) and inp["labels"].shape == (2, c.U)
            assert not (inp["labels"] == c.blank).any()
    c = R.logprob_vocabulary_case(4100)
    assert sorted(set(k // R.BLOCK for k in R.label_tokens(c.V, c.U, c.blank)) | {c.blank // R.BLOCK}) == [0, 1, 2, 3, 4]
    for U in (513, 520, 1024):
        lab = R.inputs(R.label_case(U))["labels"]
        assert len(set(lab[0, 511:515])) == 1 and lab.shape == (2, U)
    x = [R.inputs(R.boundary_case(V, U)) for V, U in ((256, 100), (254, 100), (260, 100), (256, 129))]
    assert np.array_equal(x[0]["v"][:, :, :254], x[1]["v"]) and np.array_equal(x[2]["v"][:, :, :256], x[3]["v"])
    assert np.array_equal(x[0]["labels"], x[3]["labels"][:, :100]) and np.array_equal(x[0]["labels"], x[2]["labels"])
