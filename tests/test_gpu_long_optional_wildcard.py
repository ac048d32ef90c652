"""Optional wildcards above 1024 labels on the GPU: the long-form loss and gradient (both workspaces) and the long-form label
posteriors with labels equal to OPTIONAL_WILDCARD (-3), against tests/tools/optional_wildcard_oracle.py (float64, no limit on U),
and the properties include/ctc_amd.h promises for them.  V = 8 throughout; the optional positions sit on both sides of the label
block boundary (1022, 1023, 1024), where a skip, an end state or an adjacent pair crosses it.

Bars: 1e-4 + 1e-6 |loss| on the loss, 1e-4 per float32 gradient or posterior element (16-bit gradients: plus 2^-8 |oracle|),
duration within 1e-4 max(1, oracle).  Every oracle result is computed once per input and shared."""
import ctypes

import numpy as np
import pytest
import torch

from tests.tools import optional_wildcard_oracle as OO

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = OO.KINDS
W, O = OO.WILDCARD, OO.OPTIONAL
V = 8
WEIGHT = -0.25
FIELDS = ("loss", "label_posterior", "blank_posterior", "duration", "expected_frame", "peak_posterior", "peak_frame")


def tol(s):
    return 1e-4 + 1e-6 * np.abs(s)


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        u, v = a[k].contiguous().reshape(-1), b[k].contiguous().reshape(-1)
        assert u.dtype == v.dtype and u.shape == v.shape, k
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), k


def row(out, b):
    return {k: v[b] for k, v in out.items()}


def fns(kind, wrt):
    """(long loss, long posterior with optional wildcards, long posterior without) for a lattice and an input kind."""
    import tf_seq2seq_losses_amd as ctc
    cls = ctc.ClassicCtcLossData if kind == "classic" else ctc.SimplifiedCtcLossData
    if wrt:
        return tuple((lambda *a, _f=f, **k: _f(*a[:4], a[4], cls, **k)) for f in (
            ctc.ctc_long_loss_from_logproba, ctc.ctc_long_optional_wildcard_label_posterior_from_logproba,
            ctc.ctc_long_label_posterior_from_logproba))
    c = kind == "classic"
    return (ctc.classic_ctc_long_loss if c else ctc.simplified_ctc_long_loss,
            ctc.classic_ctc_long_optional_wildcard_label_posterior if c else ctc.simplified_ctc_long_optional_wildcard_label_posterior,
            ctc.classic_ctc_long_label_posterior if c else ctc.simplified_ctc_long_label_posterior)


def short_fns(kind):
    import tf_seq2seq_losses_amd as ctc
    c = kind == "classic"
    return (ctc.classic_ctc_wildcard_loss if c else ctc.simplified_ctc_wildcard_loss,
            ctc.classic_ctc_label_posterior if c else ctc.simplified_ctc_label_posterior)


def run(kind, wrt, x, labels, ll, tl, opt=True, weight=WEIGHT, checkpoint=False, dense=True, post=True, short=False, blank=0,
        d_loss=None, **kw):
    """The long-form loss + gradient (one `checkpoint` setting) and, with `post`, the label posteriors, as a dict of CPU tensors.
    opt=False: the existing calls, without the keyword.  short: the short-form calls with optional_wildcards=True."""
    if short:
        loss_fn, post_fn = short_fns(kind)
        lk, pk = {"optional_wildcards": True}, {"optional_wildcards": True}
    else:
        loss_fn, opt_post, plain_post = fns(kind, wrt)
        post_fn = opt_post if opt else plain_post
        lk = {"checkpoint": checkpoint, **({"optional_wildcards": True} if opt else {})}
        pk = {"dense": dense}
    lab, l1, l2 = dev(labels), dev(ll), dev(tl)
    xt = dev(x).clone().requires_grad_(True)
    loss = loss_fn(lab, xt, l1, l2, blank, wildcard_log_weight=weight, **lk, **kw)
    (grad,) = torch.autograd.grad(loss.sum(), xt) if d_loss is None else torch.autograd.grad(loss, xt, dev(d_loss))
    out = dict(loss=loss.detach(), grad=grad)
    if post:
        p = post_fn(lab, dev(x), l1, l2, blank, wildcard_log_weight=weight, **pk, **kw)
        out.update({"p_" + k: v for k, v in p._asdict().items() if v is not None})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


_ORACLE = {}


def oracle(key, kind, wrt, x64, labels, ll, tl, weight=WEIGHT, blank=0, d_loss=None):
    """The float64 results for an input, computed once per `key` and not changed by anybody."""
    k = (key, kind, wrt, weight, blank, None if d_loss is None else tuple(np.asarray(d_loss, np.float64).tolist()))
    if k not in _ORACLE:
        loss, grad = OO.loss_and_grad(kind, wrt, labels, x64, ll, tl, blank, weight, d_loss)
        loss2, post, blk, dur, exf = OO.label_posterior(kind, wrt, labels, x64, ll, tl, blank, weight)
        assert np.array_equal(loss, loss2)
        res = dict(loss=loss, grad=grad, post=post, blk=blk, dur=dur, exf=exf)
        for a in res.values():
            a.setflags(write=False)
        _ORACLE[k] = res
    return _ORACLE[k]


def check(ref, got, tl, what, grad_rel=0.0):
    """What `got` holds of loss, gradient and posteriors against the oracle at the bars; every frame of a feasible utterance sums to
    1, an infeasible one is +inf with zeros and expected_frame -1."""
    o_loss = ref["loss"]
    loss = got["loss"].numpy().astype(np.float64)
    fin = np.isfinite(o_loss)
    assert np.array_equal(np.isfinite(loss), fin) and np.all(loss[~fin] == np.inf), (what, o_loss, loss)
    e_loss = np.abs(loss[fin] - o_loss[fin])
    g = got["grad"].float().numpy().astype(np.float64)
    e_grad = np.abs(g - ref["grad"])
    print(f"{what}: oracle loss {o_loss}, loss err {e_loss.max(initial=0.0):.3g} grad err {e_grad.max():.3g}")
    assert np.all(e_loss <= tol(o_loss[fin])), (what, loss, o_loss)
    assert np.all(e_grad <= 1e-4 + grad_rel * np.abs(ref["grad"])), (what, e_grad.max())
    assert np.all(g[~fin] == 0.0), what
    if "p_loss" not in got:
        return
    same_bits({"p_loss": got["loss"]}, got, ["p_loss"])  # the posterior call's loss is the loss call's
    e_blk = np.abs(got["p_blank_posterior"].numpy() - ref["blk"]).max()
    dur = got["p_duration"].numpy()
    e_dur = np.abs(dur - ref["dur"])
    exf = got["p_expected_frame"].numpy()
    print(f"{what}: blank err {e_blk:.3g} duration err {e_dur.max():.3g}")
    assert e_blk <= 1e-4, (what, e_blk)
    assert np.all(e_dur <= 1e-4 * np.maximum(1.0, ref["dur"])), what
    assert np.all(dur[~fin] == 0.0) and np.all(exf[~fin] == -1.0), what
    sure = ref["dur"] > 1e-3  # (a soft timestamp is a quotient: compared where the divisor is not tiny)
    assert np.all(np.abs(exf[sure] - ref["exf"][sure]) <= 1e-4 * np.maximum(1.0, ref["exf"][sure]) / np.minimum(1.0, ref["dur"][sure])), what
    if "p_label_posterior" not in got:
        return
    post = got["p_label_posterior"].numpy()
    e_post = np.abs(post - ref["post"]).max()
    print(f"{what}: posterior err {e_post:.3g}")
    assert e_post <= 1e-4, (what, e_post)
    assert np.all(post[~fin] == 0.0), what
    assert np.all(np.abs(got["p_peak_posterior"].numpy() - ref["post"].max(axis=1, initial=0.0)) <= 1e-4), what
    # peak_frame: the oracle column's argmax wherever its maximum leads the runner-up by more than twice the posterior bar
    pf = got["p_peak_frame"].numpy()
    compared = 0
    for b in np.nonzero(fin)[0]:
        col = ref["post"][b, :tl[b]]
        if col.shape[0] < 2 or col.shape[1] == 0:
            continue
        top = np.sort(col, axis=0)[-2:]
        clear = (top[1] - top[0]) > 2e-4
        compared += int(clear.sum())
        assert np.array_equal(pf[b][clear], col.argmax(axis=0)[clear]), (what, b)
    assert compared > 0, what
    assert np.all(pf[~fin] == -1), what
    total = post.sum(axis=2, dtype=np.float64) + got["p_blank_posterior"].numpy()
    for b in np.nonzero(fin)[0]:
        assert np.all(np.abs(total[b, :tl[b]] - 1.0) <= 1e-4), (what, b)


def draw(B, T, U, seed, ll=None, tl=None, p_wild=0.08, p_opt=0.08, scale=1.0, V=V, blank=0):
    """Random logits and labels with wildcards of both kinds, no two optional ones adjacent.  A blank other than 0: the labels
    drawn equal to it become 0."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    labels[labels == blank] = 0
    labels[rng.random((B, U)) < p_wild] = W
    for b in range(B):
        for i in np.nonzero(rng.random(U) < p_opt)[0]:
            if (i == 0 or labels[b, i - 1] != O) and (i + 1 >= U or labels[b, i + 1] != O):
                labels[b, i] = O
    ll = np.full(B, U, np.int32) if ll is None else np.asarray(ll, np.int32)
    tl = np.full(B, T, np.int32) if tl is None else np.asarray(tl, np.int32)
    return x, labels, ll, tl


def put(labels, b, at, V=V, blank=0):
    """Optional wildcards at the positions `at` of utterance b, ordinary labels around them."""
    for i in at:
        for j in (i - 1, i + 1):
            if 0 <= j < labels.shape[1] and labels[b, j] == O:
                labels[b, j] = 1 + (j % (V - 1))
                if labels[b, j] == blank:
                    labels[b, j] = 0
        labels[b, i] = O


_MAIN = {}


def main_input():
    """B = 3, T = 1400, U = 1030: -3 at 1023 (the skip into block 1 reaches two back), at 1024 (position 1025 reaches back over the
    boundary), at 1022 and 1024; random wildcards of both kinds elsewhere."""
    if not _MAIN:
        x, labels, ll, tl = draw(3, 1400, 1030, seed=71)
        put(labels, 0, [1023])
        put(labels, 1, [1024])
        put(labels, 2, [1022, 1024])
        tl[1] = 1333
        _MAIN["v"] = (x, labels, ll, tl)
    return _MAIN["v"]


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_oracle_at_the_block_boundary(kind):
    x, labels, ll, tl = main_input()
    d_loss = np.random.default_rng(17).standard_normal(3).astype(np.float32)
    ref = oracle("main", kind, 0, x.astype(np.float64), labels, ll, tl, d_loss=d_loss)
    got = run(kind, 0, x, labels, ll, tl, d_loss=d_loss)
    check(ref, got, tl, f"{kind} main")
    ck = run(kind, 0, x, labels, ll, tl, d_loss=d_loss, checkpoint=True, post=False)
    same_bits(ck, got, ["loss", "grad"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 2600, 2100, 64), (2, 169, 129, None), (2, 1300, 1024, None)])
def test_against_the_oracle_further_shapes(kind, shape):
    B, T, U, tf = shape
    x, labels, ll, tl = draw(B, T, U, seed=T)
    if U > 2048:  # three label blocks, the ring wraps: -3 on both sides of both boundaries
        put(labels, 0, [1022, 1024, 2047, 2049])
        put(labels, 1, [1023, 1025, 2046, 2048])
    else:
        put(labels, 0, [U - 1])
        put(labels, 1, [0, U - 2])
    ref = oracle(f"shape{shape}", kind, 0, x.astype(np.float64), labels, ll, tl)
    kw = {} if tf is None else {"frames_per_tile": tf}
    check(ref, run(kind, 0, x, labels, ll, tl, **kw), tl, f"{kind} {shape}")
    ck = run(kind, 0, x, labels, ll, tl, checkpoint=True, post=False, **kw)
    check(ref, ck, tl, f"{kind} {shape} checkpoint=True")


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_oracle_on_log_probabilities(kind):
    x, labels, ll, tl = (a[2:3] for a in main_input())
    x = torch.log_softmax(torch.from_numpy(x).double() * 1.5, -1).float().numpy()
    ref = oracle("main[2] logproba", kind, 1, x.astype(np.float64), labels, ll, tl, weight=-0.7)
    for ck in (False, True):
        check(ref, run(kind, 1, x, labels, ll, tl, weight=-0.7, checkpoint=ck, post=not ck), tl, f"{kind} logproba checkpoint={ck}")


def stc_input():
    """-3 before, between and after 514 labels (no two neighbours equal): L = 1029; the same transcript with 600 and with 500
    frames, the second below the 514 it needs."""
    rng = np.random.default_rng(5)
    real = np.zeros(514, np.int32)
    for i in range(514):
        real[i] = rng.choice([k for k in range(1, V) if i == 0 or k != real[i - 1]])
    lab = np.full(1029, O, np.int32)
    lab[1::2] = real
    labels = np.stack([lab, lab])
    x = (rng.standard_normal((1, 600, V)) * 2.0).astype(np.float32).repeat(2, axis=0)
    return x, labels, np.array([1029, 1029], np.int32), np.array([600, 500], np.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_star_between_every_pair_of_labels_in_fewer_frames_than_positions(kind):
    x, labels, ll, tl = stc_input()
    ref = oracle("stc", kind, 0, x.astype(np.float64), labels, ll, tl)
    assert np.isfinite(ref["loss"][0]) and np.isinf(ref["loss"][1])
    assert ref["post"][0, :, 1024:].sum() > 1.0  # the second label block carries mass although T_b < 1024
    base = None
    for tf in (128, 64):
        for ck in (False, True):
            got = run(kind, 0, x, labels, ll, tl, checkpoint=ck, post=not ck, frames_per_tile=tf)
            check(ref, got, tl, f"{kind} STC frames_per_tile={tf} checkpoint={ck}")
            base = base or got
            same_bits(got, base, got.keys())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", [1025, 1026])
def test_end_states_across_the_block_boundary(kind, L):
    """-3 last: position L - 2 ends the utterance too (L = 1025: it lives in block 0).  A wildcard frame costs e^-8.  Utterance 0:
    the last frames are sure of the blank, and the star is skipped; utterance 1: they are sure of a token that no label near the end
    is, and the star takes them."""
    T, weight = L + 300, -8.0
    x, labels, ll, tl = draw(2, T, L, seed=L, p_opt=0.0)
    tail = labels[:, L - 30:L - 1]  # no wildcard and no token 7 near the end
    tail[(tail == W) | (tail == 7)] = 2
    labels[:, L - 1] = O
    x[0, T - 12:, :] = -6.0
    x[0, T - 12:, 0] = 6.0
    x[1, T - 12:, :] = -10.0
    x[1, T - 12:, 7] = 10.0
    ref = oracle(f"end{L}", kind, 0, x.astype(np.float64), labels, ll, tl, weight=weight)
    assert ref["dur"][0, L - 1] < 0.05 and ref["dur"][1, L - 1] >= 1.0, ref["dur"][:, L - 1]
    got = run(kind, 0, x, labels, ll, tl, weight=weight)
    check(ref, got, tl, f"{kind} L={L}")
    dur = got["p_duration"].numpy()[:, L - 1]
    assert dur[0] < 0.05 and dur[1] >= 1.0, dur


@pytest.mark.parametrize("kind", KINDS)
def test_adjacent_pair_on_the_block_boundary_is_infeasible(kind):
    x, labels, ll, tl = (a.copy() for a in main_input())
    labels[1, 1023] = labels[1, 1024] = O
    labels[1, 1022] = labels[1, 1025] = 2
    for ck in (False, True):
        got = run(kind, 0, x, labels, ll, tl, checkpoint=ck)
        assert np.isinf(got["loss"].numpy()[1]) and got["loss"].numpy()[1] > 0
        assert torch.all(got["grad"][1] == 0) and torch.all(got["p_label_posterior"][1] == 0) and torch.all(got["p_blank_posterior"][1] == 0)
        assert torch.all(got["p_duration"][1] == 0) and torch.all(got["p_expected_frame"][1] == -1)
        assert torch.all(got["p_peak_posterior"][1] == 0) and torch.all(got["p_peak_frame"][1] == -1)
        for b in (0, 2):
            alone = run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], checkpoint=ck)
            assert np.isfinite(alone["loss"].numpy()).all()
            same_bits(row(alone, 0), row(got, b), alone.keys())


@pytest.mark.parametrize("kind", KINDS)
def test_subset_equivalence_on_the_device(kind):
    """Z is the sum of Z over the transcripts with every subset of the optional positions deleted and the rest made mandatory: the
    eight existing long-form losses against the new one."""
    x, labels, ll, tl = draw(1, 1400, 1030, seed=3, p_opt=0.0)
    at = [400, 1022, 1024]
    put(labels, 0, at)
    new = run(kind, 0, x, labels, ll, tl, post=False)["loss"].double().numpy()[0]
    terms = []
    for mask in range(8):
        keep = [i for i in range(1030) if not (i in at and (mask >> at.index(i)) & 1)]
        lab = labels[0, keep].copy()
        lab[lab == O] = W
        padded = np.zeros((1, 1030), np.int32)
        padded[0, :len(lab)] = lab
        terms.append(run(kind, 0, x, padded, np.array([len(lab)], np.int32), tl, opt=False, post=False)["loss"].double().numpy()[0])
    total = -np.logaddexp.reduce(-np.array(terms))
    print(f"{kind}: new {new}, eight terms {terms}, their sum {total}")
    assert abs(new - total) <= tol(total)


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_for_both_workspaces_every_tile_height_and_batch(kind):
    x, labels, ll, tl = main_input()
    U = labels.shape[1]
    base = run(kind, 0, x, labels, ll, tl)
    assert np.isfinite(base["loss"].numpy()).all()
    same_bits({"p_loss": base["loss"]}, base, ["p_loss"])
    for tf in (64, 128, 4):
        for ck in (False, True):
            got = run(kind, 0, x, labels, ll, tl, checkpoint=ck, post=ck, frames_per_tile=tf)
            same_bits(got, base, got.keys())
    sparse = run(kind, 0, x, labels, ll, tl, dense=False)
    assert "p_label_posterior" not in sparse
    same_bits(sparse, base, sparse.keys())
    for b in (0, 2):
        alone = run(kind, 0, x[b:b + 1], labels[b:b + 1], ll[b:b + 1], tl[b:b + 1], checkpoint=b == 2, max_label_length=U)
        same_bits(row(alone, 0), row(base, b), alone.keys())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("U", [1030, 2100])
def test_without_an_optional_wildcard_the_bits_of_the_existing_calls(kind, U):
    T = U + 300
    x, labels, ll, tl = draw(3, T, U, seed=U, p_opt=0.0)
    ll[1] = U - 7
    tl[2] = U // 2  # an infeasible utterance
    for ck in (False, True):
        old = run(kind, 0, x, labels, ll, tl, opt=False, checkpoint=ck, post=ck)
        assert np.isinf(old["loss"].numpy()[2]) and np.isfinite(old["loss"].numpy()[:2]).all()
        same_bits(run(kind, 0, x, labels, ll, tl, checkpoint=ck, post=ck), old)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(169, 129), (1300, 1024)])
def test_one_label_block_is_the_short_form(kind, shape):
    T, U = shape
    x, labels, ll, tl = draw(2, T, U, seed=U)
    put(labels, 0, [U - 1])
    ll[1] = U - 3
    long = run(kind, 0, x, labels, ll, tl)
    short = run(kind, 0, x, labels, ll, tl, short=True)
    same_bits(short, long, ["loss", "grad", "p_label_posterior", "p_duration", "p_expected_frame"])
    assert (long["p_blank_posterior"] - short["p_blank_posterior"]).abs().max() <= 1e-4


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_off_and_windows(kind):
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = draw(2, 1200, 1030, seed=9, p_opt=0.0)
    labels[0, 1024] = O
    off = run(kind, 0, x, labels, ll, tl, opt=False)
    assert np.isinf(off["loss"].numpy()[0]) and np.isfinite(off["loss"].numpy()[1])  # -3 is a bad label
    assert torch.all(off["grad"][0] == 0)
    spelled = fns(kind, 0)[0](dev(labels), dev(x), dev(ll), dev(tl), 0, wildcard_log_weight=WEIGHT, optional_wildcards=False)
    same_bits({"loss": spelled.cpu()}, off, ["loss"])
    on = run(kind, 0, x, labels, ll, tl, post=False)
    assert np.isfinite(on["loss"].numpy()).all()
    window = torch.zeros((2, 1030, 2), dtype=torch.int32, device=DEV)
    window[..., 1] = 1199
    with pytest.raises(ValueError):
        fns(kind, 0)[0](dev(labels), dev(x), dev(ll), dev(tl), 0, optional_wildcards=True, frame_window=window)
    with pytest.raises(ValueError):
        ctc.ops.check_labels(dev(labels), dev(ll), V, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_formats_strides_and_blank(kind):
    B, T, U = 2, 1200, 1030
    x, labels, ll, tl = draw(B, T, U, seed=21)
    put(labels, 0, [1023])
    put(labels, 1, [1022, 1024])
    big = torch.zeros((T, B, V + 8), device=DEV)
    big[:, :, :V] = dev(x).transpose(0, 1)
    for ck in (False, True):
        base = run(kind, 0, x, labels, ll, tl, checkpoint=ck)
        same_bits(run(kind, 0, big[:, :, :V].transpose(0, 1), labels, ll, tl, checkpoint=ck), base)
    for dt in (torch.bfloat16, torch.float16):
        xh = torch.from_numpy(x).to(dt)
        ref = oracle(f"formats {dt}", kind, 0, xh.double().numpy(), labels, ll, tl)
        for ck in (False, True):
            got = run(kind, 0, xh.to(DEV), labels, ll, tl, checkpoint=ck, post=not ck)
            assert got["grad"].dtype == dt
            check(ref, got, tl, f"{kind} {dt} checkpoint={ck}", grad_rel=2.0 ** -8)
    # a blank that is not 0: the labels avoid it
    blank = 5
    lab5 = labels.copy()
    lab5[lab5 == blank] = 0
    ref = oracle("blank 5", kind, 0, x.astype(np.float64), lab5, ll, tl, blank=blank)
    check(ref, run(kind, 0, x, lab5, ll, tl, blank=blank), tl, f"{kind} blank={blank}")


def _raw_calls(kind, x, labels, ll, tl, fill, tf=64, blank=0, d_loss=None, like_x=False):
    """The three C entry points themselves on outputs and an exact-size workspace prefilled with the byte `fill`.  x: numpy, or a
    device tensor of any of the three element types and any strides with a contiguous token axis.  like_x: the gradients have the
    type and strides of x, and their whole buffers are returned too (grad_storage, ckpt_grad_storage)."""
    from tf_seq2seq_losses_amd import _lib
    lib = _lib.load()
    B, T, V = x.shape
    U = labels.shape[1]
    k = KINDS.index(kind)
    t = {n: dev(a) for n, a in dict(x=x, labels=labels, ll=ll, tl=tl).items()}
    xt = t["x"]
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
    lead = (k, 0, xt.data_ptr(), code[xt.dtype], xt.stride(0), xt.stride(1), t["labels"].data_ptr(), U, t["ll"].data_ptr(),
            t["tl"].data_ptr(), blank, ctypes.c_float(WEIGHT), B, T, V, U, tf)
    dl = None if d_loss is None else dev(np.asarray(d_loss, np.float32))

    def buf(shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=DEV)[:n].view(dtype).reshape(shape)

    out = {}
    for name, call, size in (("", lib.ctc_amd_long_optional_wildcard_loss_grad, _lib.long_optional_wildcard_loss_workspace_bytes),
                             ("ckpt_", lib.ctc_amd_long_optional_wildcard_loss_grad_ckpt,
                              _lib.long_optional_wildcard_loss_ckpt_workspace_bytes)):
        lg = {name + "loss": buf((B,), torch.float32), name + "grad": buf((B, T, V), torch.float32)}
        if like_x:
            n = (B - 1) * xt.stride(0) + (T - 1) * xt.stride(1) + V
            out[name + "grad_storage"] = buf((n,), xt.dtype)
            lg[name + "grad"] = out[name + "grad_storage"].as_strided((B, T, V), xt.stride())
        g = lg[name + "grad"]
        w = torch.full((size(k, B, T, V, U, tf, True),), fill, dtype=torch.uint8, device=DEV)
        rc = call(*lead, None if dl is None else dl.data_ptr(), *(v.data_ptr() for v in lg.values()), code[g.dtype], g.stride(0),
                  g.stride(1), w.data_ptr(), w.numel(), None)
        assert rc == 0, lib.ctc_amd_last_error()
        out.update(lg)
    po = dict(p_loss=buf((B,), torch.float32), post=buf((B, T, U), torch.float32), blk=buf((B, T), torch.float32),
              dur=buf((B, U), torch.float32), exf=buf((B, U), torch.float32), peak=buf((B, U), torch.float32),
              peak_frame=buf((B, U), torch.int32))
    w = torch.full((_lib.long_optional_wildcard_label_posterior_workspace_bytes(k, B, T, V, U, tf),), fill, dtype=torch.uint8, device=DEV)
    rc = lib.ctc_amd_long_optional_wildcard_label_posterior(*lead, *(v.data_ptr() for v in po.values()), w.data_ptr(), w.numel(), None)
    assert rc == 0, lib.ctc_amd_last_error()
    out.update(po)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_prefilled_outputs_and_workspace_do_not_show(kind):
    """Every element of every output has a writer and nothing unwritten is read: 0x00 and 0xFF in the outputs and an exact-size
    workspace give the same bits, an infeasible utterance's and a short one's (T_b < L, few tiles run) included."""
    x, labels, ll, tl = (a.copy() for a in main_input())
    labels[0, 1022] = O
    labels[0, 1021] = 4  # (1022 and 1023: an adjacent pair)
    xs, ls, lls, tls = stc_input()
    x[2, :600], labels[2, :1029], ll[2], tl[2] = xs[0], ls[0], 1029, 600
    a = _raw_calls(kind, x, labels, ll, tl, 0x00)
    b = _raw_calls(kind, x, labels, ll, tl, 0xFF)
    same_bits(a, b)
    assert np.isinf(a["loss"].numpy()[0]) and np.isfinite(a["loss"].numpy()[1:]).all()
    same_bits({"loss": a["loss"], "grad": a["grad"]}, {"loss": a["ckpt_loss"], "grad": a["ckpt_grad"]})
    same_bits({"loss": a["loss"]}, {"loss": a["p_loss"]})
    pub = run(kind, 0, x, labels, ll, tl, checkpoint=True, frames_per_tile=64)
    same_bits({n: a[m] for n, m in (("loss", "loss"), ("grad", "grad"), ("p_label_posterior", "post"), ("p_peak_frame", "peak_frame"))}, pub,
              ["loss", "grad", "p_label_posterior", "p_peak_frame"])


def test_graph_capture_replays():
    """The calls neither synchronise nor allocate outside the graph's pool: one capture, one replay, the eager bits."""
    import tf_seq2seq_losses_amd as ctc
    x, labels, ll, tl = (a[2:3] for a in main_input())
    U = labels.shape[1]
    eager = run("classic", 0, x, labels, ll, tl, checkpoint=True, max_label_length=U)
    xs, lab, l1, l2 = dev(x), dev(labels), dev(ll), dev(tl)

    def work():
        xg = xs.clone().requires_grad_(True)
        loss = ctc.classic_ctc_long_loss(lab, xg, l1, l2, 0, wildcard_log_weight=WEIGHT, max_label_length=U, checkpoint=True,
                                         optional_wildcards=True)
        (g,) = torch.autograd.grad(loss.sum(), xg)
        p = ctc.classic_ctc_long_optional_wildcard_label_posterior(lab, xs, l1, l2, 0, wildcard_log_weight=WEIGHT, max_label_length=U)
        return dict(loss=loss.detach(), grad=g, **{"p_" + k: v for k, v in p._asdict().items()})

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = work()
    graph.replay()
    torch.cuda.synchronize()
    same_bits(eager, {k: v.cpu() for k, v in out.items()})


@pytest.mark.parametrize("kind", KINDS)
def test_autograd(kind):
    from tf_seq2seq_losses_amd import ops
    x, labels, ll, tl = (a[:2] for a in main_input())
    U = labels.shape[1]
    xt = dev(x).clone().requires_grad_(True)
    loss = fns(kind, 0)[0](dev(labels), xt, dev(ll), dev(tl), 0, wildcard_log_weight=WEIGHT, optional_wildcards=True)
    (g,) = torch.autograd.grad(loss.sum(), xt, create_graph=True)
    l2, g2 = ops.long_optional_wildcard_loss_grad(KINDS.index(kind), 0, dev(labels), dev(x), dev(ll), dev(tl), 0, None, U, None, WEIGHT,
                                                  True, 0, False)
    torch.cuda.synchronize()
    same_bits({"loss": loss.detach().cpu(), "grad": g.detach().cpu()}, {"loss": l2.cpu(), "grad": g2.cpu()})
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xt)
