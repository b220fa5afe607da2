"""The construction of tests/saturation_cases.py, checked on the CPU before the GPU sees its bounds
(tests/test_gpu_saturation.py): the logits are exact in fp32 whatever the summation order, the fp64 reference of every
checked quantity is finite, every rung of the gap ladder is some column's label gap, and a plain fp32 numpy
restatement of the stable formulas -- not the project's code -- is within the bounds the GPU kernels are held to.
The torch backend of MlpEngine, which restates the HIP step, reports the finite loss too."""
import numpy as np
import pytest
import torch

from cme213_sp18_amd.parallel import MlpEngine

from . import saturation_cases as sc

HEAD_SHAPES = [(2, 16, 37), (10, 100, 37), (11, 130, 37), (16, 100, 37), (16, 1024, 37), (17, 16, 37), (47, 100, 37),
               (64, 100, 37), (16, 100, 1), (47, 16, 1)]


@pytest.mark.parametrize("shift", [1, 0])
@pytest.mark.parametrize("C,H,n", HEAD_SHAPES)
def test_logits_are_exact_in_fp32_in_any_order(C, H, n, shift):
    W2, b2, a1, lab, z2, gap = sc.head_operands(C, H, n, shift, p0=12 if n == 1 else 0)
    f = np.float32
    for t in (W2, b2, a1):
        assert (t.astype(f).astype(np.float64) == t).all()
    assert set(np.unique(a1)) <= {0.0, 0.5, 1.0}
    fwd, rev = np.zeros((C, n), f), np.zeros((C, n), f)
    for h in range(H):
        fwd += W2[:, h:h + 1].astype(f) * a1[h:h + 1].astype(f)
    for h in reversed(range(H)):
        rev += W2[:, h:h + 1].astype(f) * a1[h:h + 1].astype(f)
    assert ((fwd + b2[:, None].astype(f)).astype(np.float64) == z2).all()
    assert ((b2[:, None].astype(f) + rev).astype(np.float64) == z2).all()
    assert (W2 @ a1 + b2[:, None] == z2).all()
    # every column has a class at gap 0 and its logit is top - gap; unshifted, every logit stays inside [-80, 80]
    assert (gap.min(0) == 0).all() and (z2.max(0)[None] - z2 == gap).all()
    if not shift:
        assert np.abs(z2).max() <= 80.0
    if n > 1:
        assert ((gap == 0).sum(0) == 2).any()  # an exact tie for the maximum


@pytest.mark.parametrize("C", [2, 10, 11, 16, 17, 47, 64])
def test_labels_reach_every_rung(C):
    """n = 37, shifted: the label's gap takes every rung of the ladder, from the winner to gap 200; the tie patterns
    put the second maximum in the last live class, in the next class and 16 (or 4) classes up."""
    _, _, _, lab, _, gap = sc.head_operands(C, 100, 37, 1)
    assert set(gap[lab, np.arange(37)]) == set(sc.G)
    _, g16 = sc.pattern_logits(C, 1)
    tied = [tuple(np.flatnonzero(g16[:, p] == 0)) for p in range(sc.S)]
    assert all(len(t) == 2 for p, t in enumerate(tied) if p == 15 or (p % 4 == 3 and C > 2))
    assert any(t[1] == C - 1 for t in tied if len(t) == 2)
    if C > 16:
        assert any(t[0] // 16 != t[1] // 16 for t in tied if len(t) == 2)


@pytest.mark.parametrize("shift", [1, 0])
@pytest.mark.parametrize("C,H,n", HEAD_SHAPES)
def test_fp32_restatement_is_within_the_bounds(C, H, n, shift):
    """The bounds of tests/test_gpu_saturation.py against an evaluation that is not the project's: fp64 reference
    finite everywhere, fp32 numpy within (gap + 8) 2^-23 |ref| + 2^-126 on yhat and D / scale, within the sum of
    (l + 4) 2^-22 on the loss partials, dZ1 finite and exactly 0 where a1 is 0 or 1."""
    scale = 1.0 / (3 * n)
    W2, b2, a1, lab, z2, gap = sc.head_operands(C, H, n, shift, p0=12 if n == 1 else 0)
    yh, dref, D, dZ1, loss, _ = sc.head_reference(W2, b2, a1, lab, z2, scale)
    for t in (yh, dref, D, dZ1, loss):
        assert np.isfinite(t).all()
    assert loss.max() <= 200.0 + np.log(C) and (loss.max() >= 150.0 or not shift or n == 1)
    y32, D32, dZ32, l32 = sc.head_f32(W2, b2, a1, lab, scale, shift)
    onehot = (dref != yh).astype(np.float64)
    assert sc.worst_ratio(y32, yh, sc.prob_bound(gap, yh)) <= 1.0
    assert sc.worst_ratio(D32.astype(np.float64) / scale, dref, sc.grad_bound(gap, yh, onehot)) <= 1.0
    assert sc.worst_ratio(sc.block_sums32(l32), sc.block_sums(loss), sc.loss_bound(loss)) <= 1.0
    assert np.isfinite(dZ32).all() and (dZ32[(a1 == 0) | (a1 == 1)] == 0).all()
    assert float(np.abs(dZ32 - dZ1).max()) <= 1e-5 * float(np.abs(dZ1).max())


@pytest.mark.parametrize("C,H", [(2, 100), (16, 100), (16, 512), (47, 100)])
def test_step_operands_give_the_stated_activations(C, H):
    """z1 = W1 x is a multiple of 8192 (exact in fp32 in any order: W1 = 0 wherever the pixels are arbitrary) and
    the sigmoid of it is the stated a1 in {0, 1/2, 1}; z2 is then the stated ladder."""
    N = 96
    x, lab, W1, b1, W2, b2, a1, z2, gap = sc.step_operands(784, H, C, N)
    assert set(np.unique(W1)) <= {-sc.BIG, 0.0, sc.BIG} and not b1.any()
    assert (W1[:, [i for i in range(784) if i not in sc.SEL + sc.BIT]] == 0).all()
    z1 = W1 @ x.T.astype(np.float64)
    assert (z1 % sc.BIG == 0).all()
    f = np.float32
    assert ((W1.astype(f) @ x.T.astype(f)).astype(np.float64) == z1).all()
    assert (W1.astype(f).astype(np.float64) == W1).all()
    assert (torch.tensor(W1).to(torch.bfloat16).double().numpy() == W1).all()  # one bf16 plane holds it
    with np.errstate(over="ignore"):
        for t in (np.float32, np.float64):
            assert ((1 / (1 + np.exp(-z1.astype(t)))).astype(np.float64) == a1).all()
    assert {0.0, 0.5, 1.0} == set(np.unique(a1))
    assert (W2 @ a1 + b2[:, None] == z2).all()
    assert set(gap[lab, np.arange(N)]) == set(sc.G)


def test_sigmoid_ladder_reference():
    b1 = sc.sigmoid_ladder(100)
    assert {abs(v) for v in b1} == set(sc.SIG_LADDER) and (np.float32(b1).astype(np.float64) != 0).sum() == 96
    ref = sc.sigmoid_reference(np.float32(b1).astype(np.float64))
    assert np.isfinite(ref).all() and ref[b1 >= 128].min() == 1.0 and ref[b1 <= -8192].max() == 0.0
    # a plain fp32 restatement, 1 / (1 + exp(-x)), within the bound the kernels are held to
    with np.errstate(over="ignore"):
        got = (np.float32(1) / (np.float32(1) + np.exp(-np.float32(b1)))).astype(np.float64)
    bound = (np.abs(b1) + 8.0) * sc.EPS32 * ref + sc.TINY32
    assert (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_torch_backend_step_loss_is_finite_at_underflowed_labels(dt):
    """MlpEngine's torch backend (the restatement of the HIP step that the CPU runs) forms the loss as
    log(sum) - (z_label - m): finite at a label gap of 200, where -log(yhat[label]) is +inf in fp32, and equal to
    the fp64 reference within the loss bound."""
    H, C, n = 100, 16, 96
    x, lab, W1, b1, W2, b2, a1, z2, gap = sc.step_operands(784, H, C, n)
    e = MlpEngine((784, H, C), dtype=dt, max_cols=n, device="cpu", backend="torch")
    e.set_params(W1, b1, W2, b2)
    e.load_dataset(x, lab)
    e.run(0, n, 1.0 / n, 1e-4, 0.0, sgd=False, with_loss=True)
    _, loss, _ = sc.softmax_reference(z2, lab)
    assert gap[lab, np.arange(n)].max() == 200.0
    assert np.isfinite(e.loss_sum()) and abs(e.loss_sum() - loss.sum()) <= sc.loss_bound(loss).sum()
    assert torch.isfinite(e.grads).all()
    assert (e.a1[:, :n].double().numpy() == a1).all()
