"""The helpers of tests/_ownership.py on their own (no GPU): what they call unowned is exactly the complement of what the utterances
own, owned elements keep their bits, every unowned element changes, and the shared cases reach the oracles unchanged."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from tests import _ownership as W

B, T, V, U = 4, 7, 5, 6
TL = np.array([7, 0, 3, 9], np.int32)   # 9: beyond T, counts as T
LL = np.array([6, -2, 0, 3], np.int32)  # -2: counts as 0


def _x(dtype=torch.float32):
    return (torch.arange(B * T * V, dtype=torch.float32).reshape(B, T, V) / 8 - 3).to(dtype)


def _owned_frames():
    m = torch.zeros((B, T), dtype=torch.bool)
    for b, n in enumerate([7, 0, 3, 7]):
        m[b, :n] = True
    return m


def _layouts(x):
    """the same values as a batch-major tensor, as a [B, T, V] view of time-major storage and as a strided view with gaps"""
    tm = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert tm.stride() == (V, B * V, 1)
    _, gapped, _ = W.strided_storage(x, T * (V + 5) + 11, V + 5, 0xA5)
    return {"batch-major": x, "time-major": tm, "strided": gapped}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_poison_padding_changes_the_padding_frames_and_nothing_else(dtype):
    own = _owned_frames()
    for name, x in _layouts(_x(dtype)).items():
        before = x.clone()
        for value in W.poison_values(dtype):
            y = W.poison_padding(x, TL, value)
            assert y.stride() == x.stride() and y.data_ptr() != x.data_ptr(), name
            assert W.same_bits(x.contiguous(), before.contiguous()), name  # (the argument is left alone)
            assert W.same_bits(y[own], x[own]), (name, value)
            changed = W.bits(y.contiguous()) != W.bits(x.contiguous())
            assert bool(changed[~own].all()) and not bool(changed[own].any()), (name, value)
            pad = y[~own].float()
            assert bool(torch.isnan(pad).all()) if value != value else bool((pad == torch.tensor(value, dtype=dtype).float()).all())
    assert len(W.poison_values(torch.float32)) == 4 and len(W.poison_values(torch.bfloat16)) == 2
    assert W.poison_values(torch.float16)[1] == 65504.0


def test_poison_labels_changes_the_tails_and_nothing_else():
    labels = torch.from_numpy(np.random.default_rng(0).integers(1, V, (B, U)).astype(np.int32))
    labels[0, 0] = V + 100  # (a position that already holds a value of the cycle -- row 0 owns all six, so this one is owned)
    labels[2, 0] = -7       # unowned and equal to the value the cycle would put there
    values = W.label_poison_cycle(V, 0)
    assert values == (-7, V + 100, 0, -2 ** 31, 2 ** 31 - 1)
    y = W.poison_labels(labels, LL, values)
    own = torch.arange(U)[None, :] < torch.tensor([6, 0, 0, 3])[:, None]
    assert y.dtype == torch.int32 and torch.equal(y[own], labels[own])
    assert bool((y != labels)[~own].all())
    assert set(y[~own].tolist()) == set(values)  # every value occurs


def test_poison_gaps_strided_and_packed():
    x = _x()
    sb, st = T * (V + 5) + 11, V + 5
    storage, view, owned = W.strided_storage(x, sb, st, 0xA5)
    assert torch.equal(view, x) and int(owned.sum()) == B * T * V and storage.numel() == (B - 1) * sb + (T - 1) * st + V
    assert bool(W.keeps_prefill(storage, 0xA5)[~owned].all())
    y = W.poison_gaps(storage, owned, float("nan"))
    assert W.same_bits(y[owned], storage[owned]) and bool(torch.isnan(y[~owned]).all())
    assert torch.equal(y.as_strided((B, T, V), (sb, st, 1)), x)
    # packed: an unowned row in front, between and behind; utterance 1 has no rows
    offsets, rs, rows = [1, 9, 9, 13], V + 3, 22
    pk, pown = W.packed_storage(x, TL, offsets, rs, rows, 0xFF)
    assert int(pown.sum()) == (7 + 0 + 3 + 7) * V and not bool(pown[0].any()) and not bool(pown[8].any()) and not bool(pown[20:].any())
    assert torch.equal(pk[9:12, :V], x[2, :3]) and torch.equal(pk[13:20, :V], x[3])
    assert bool(W.keeps_prefill(pk, 0xFF)[~pown].all())
    z = W.poison_gaps(pk, pown, float("nan"))
    assert W.same_bits(z[pown], pk[pown]) and bool(torch.isnan(z[~pown]).all())
    with pytest.raises(AssertionError):
        W.packed_storage(x, TL, [0, 9, 9, 5], rs, rows)  # utterances 0 and 3 would share rows


def test_byte_patterns():
    assert W.BYTE_PATTERNS == (0x00, 0xFF, 0xA5)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert bool(torch.isnan(W.filled((3, 2), dtype, 0xFF, "cpu")).all())
    assert W.filled((2,), torch.int32, 0xFF, "cpu").tolist() == [-1, -1]
    assert W.filled((2,), torch.int64, 0xA5, "cpu").view(torch.uint8).tolist() == [0xA5] * 16
    t = W.filled((4,), torch.float32, 0xA5, "cpu")
    t[1] = 0.0
    assert W.keeps_prefill(t, 0xA5).tolist() == [True, False, True, True]
    a = torch.tensor([0.0, float("nan"), 1.0])
    b = torch.tensor([-0.0, float("nan"), 1.0])
    assert W.count_diff(a, b) == 1 and W.same_bits(a[1:], b[1:])


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_cases_are_read_only_and_have_the_rows_they_promise(name):
    c = W.case(name)
    Bc, Tc, Vc, Uc = c.shape
    for a in (c.logits, c.labels, c.ll, c.tl):
        assert not a.flags.writeable
    assert c.logits.shape == (Bc, Tc, Vc) and c.labels.shape == (Bc, Uc) and np.isfinite(c.logits).all()
    assert c.labels.min() >= 1 and c.labels.max() < Vc and c.tl.max() == Tc
    if name.startswith("lg_") or name.startswith("hvp") or name in ("small", "align_a", "align_b"):
        feas = [W.feasible_rows(c, k) for k in W.KINDS]
        assert all(f[0] for f in feas) and c.ll[0] > 0
        assert (c.ll == 0).any() or any((~f).any() for f in feas)
    if W.CASES[name][4]:  # drawn without replacement
        assert all(len(set(c.labels[b].tolist())) == Uc for b in range(Bc))


@pytest.mark.parametrize("kind", W.KINDS)
def test_the_oracle_sees_the_clean_arrays_only(kind):
    """Poisoning works on copies: the case's arrays, and what the oracle makes of them, are the same before and after; infeasible
    rows are +inf with a zero gradient, the others finite -- what the GPU tests compare their clean runs with."""
    c = W.case("lg_nl1")
    before = (c.logits.copy(), c.labels.copy())
    loss0, grad0 = C.loss_grad(kind, c.labels, c.logits, c.ll, c.tl, 0)
    x, lab = torch.tensor(c.logits), torch.tensor(c.labels)
    for value in W.POISON_F32:
        px = W.poison_padding(x, c.tl, value)
        assert px.data_ptr() != x.data_ptr()
    pl = W.poison_labels(lab, c.ll, W.label_poison_cycle(c.shape[2], 0))
    assert pl.data_ptr() != lab.data_ptr()
    assert np.array_equal(c.logits, before[0]) and np.array_equal(c.labels, before[1])
    loss1, grad1 = C.loss_grad(kind, c.labels, c.logits, c.ll, c.tl, 0)
    assert np.array_equal(loss0, loss1) and np.array_equal(grad0, grad1)
    feas = W.feasible_rows(c, kind)
    assert np.array_equal(np.isfinite(loss0), feas) and np.all(loss0[~feas] == np.inf) and np.all(grad0[~feas] == 0)
    pad = W.padding_mask(c.tl, c.shape[1]).numpy()
    assert np.all(grad0[pad] == 0)
