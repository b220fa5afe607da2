"""More than 16 output classes on the GPU: the many-class MFMA head (csrc/mlp/head_mc.hip) alone against torch fp64,
whole steps against the torch backend, SGD, determinism, predict and a data-parallel epoch.

Tolerances are those of tests/test_gpu_mlp.py (its ``TOL``: f32 paths vs a reference with another accumulation order
2e-5, f64 1e-11, bf16 3e-2 relative max-norm; test_fused_sgd_matches_torch / test_dp_grads_then_sgd_matches_fused for
the parameter updates), copied here because a test module does not import another."""
import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import hip
from cme213_sp18_amd.models import mlp as cpu_mlp
from cme213_sp18_amd.parallel import DataParallelTrainer, MlpEngine
from cme213_sp18_amd.utils.data import synthetic_mnist

pytestmark = pytest.mark.gpu

# tests/test_gpu_mlp.py TOL
TOL = {("f64", "mfma"): 1e-11, ("f32", "split3"): 2e-5, ("f32", "mfma"): 2e-5, ("bf16", "split1"): 3e-2,
       ("bf16", "mfma"): 3e-2}
DT = {"f32": (0, torch.float32), "f64": (1, torch.float64)}
TRAIN, PREDICT, PROBS = 0, 1, 2
# distinct pitches for a1, D, dZ1 and probs (a mixed-up pitch shows), each >= the largest n = 37
LDA, LDD, LDZ, LDP = 48, 64, 80, 56
FILL = 7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _head_inputs(C, H, n, tdt, seed):
    """Random, non-symmetric operands (a transposed C/D map passes on symmetric data)."""
    g = torch.Generator().manual_seed(seed)
    W2 = (torch.randn(C, H, generator=g, dtype=torch.float64) * 0.3).to(tdt)
    b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).to(tdt)
    a1 = torch.full((H, LDA), FILL, dtype=torch.float64)
    a1[:, :n] = torch.rand(H, n, generator=g, dtype=torch.float64) * 0.9 + 0.05
    lab = torch.randint(0, C, (n,), generator=g, dtype=torch.int32)
    lab[0] = C - 1  # (the last class, in the class tail of the last tile)
    return W2.cuda(), b2.cuda(), a1.to(tdt).cuda(), lab.cuda()


def _head_reference(W2, b2, a1, lab, n, scale, shift):
    """fp64 torch: z2, yhat, D, dZ1 and the loss partial of every 16-column block."""
    W, b, A = W2.double(), b2.double(), a1[:, :n].double()
    z2 = W @ A + b[:, None]
    zs = z2 - z2.max(0, keepdim=True).values if shift else z2
    e = torch.exp(zs)
    yh = e / e.sum(0, keepdim=True)
    onehot = torch.zeros_like(yh)
    onehot[lab.long(), torch.arange(n, device=yh.device)] = 1.0
    D = (yh - onehot) * scale
    dZ1 = (W.t() @ D) * A * (1 - A)
    lcol = -torch.log(yh[lab.long(), torch.arange(n, device=yh.device)])
    nblk = (n + 15) // 16
    loss = torch.stack([lcol[16 * k: 16 * k + 16].sum() for k in range(nblk)])
    return z2, yh, D, dZ1, loss


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 16, 37])
@pytest.mark.parametrize("H", [16, 100, 130])
@pytest.mark.parametrize("C", [17, 32, 33, 64])
def test_head_alone_matches_torch_fp64(C, H, n, dt):
    """mlp_head at C > 16 in every mode: class, row and column tails, a tile edge, a single column."""
    code, tdt = DT[dt]
    tol = TOL[(dt, "mfma")]
    m = hip()
    W2, b2, a1, lab = _head_inputs(C, H, n, tdt, seed=1000 * C + 10 * H + n)
    scale = 1.0 / (3 * n)
    nblk = (n + 15) // 16
    for shift in (1, 0):
        z2, yh, Dr, dZr, lossr = _head_reference(W2, b2, a1, lab, n, scale, shift)
        D = torch.full((C, LDD), FILL, dtype=tdt, device="cuda")
        dZ1 = torch.full((H, LDZ), FILL, dtype=tdt, device="cuda")
        loss = torch.full((nblk + 1,), FILL, dtype=torch.float32, device="cuda")
        # the bf16 shadow (the bf16 mode's dW1 operand) and the split path's exact planes, where requested: f32
        lo = torch.zeros(H, LDZ, dtype=torch.bfloat16, device="cuda") if dt == "f32" and shift else None
        planes = torch.zeros(3, H, LDZ, dtype=torch.bfloat16, device="cuda") if dt == "f32" and not shift else None
        m.mlp_head(code, TRAIN, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), labels=lab.data_ptr(), H=H, C=C,
                   n=n, scale=scale, D=D.data_ptr(), ldd=LDD, dZ1=dZ1.data_ptr(), ldz=LDZ,
                   dZ1_bf16=lo.data_ptr() if lo is not None else 0, loss=loss.data_ptr(), shift=shift,
                   stream=_stream(), dZ1_planes=planes.data_ptr() if planes is not None else 0,
                   npz=3 if planes is not None else 0)
        torch.cuda.synchronize()
        assert _rel(D[:, :n], Dr) < tol, ("D", shift)
        assert _rel(dZ1[:, :n], dZr) < tol, ("dZ1", shift)
        assert _rel(loss[:nblk], lossr) < max(tol, 1e-6), ("loss", shift)  # (fp32 partials in both dtypes)
        # nothing past the n columns, nothing past the last block's partial
        assert bool((D[:, n:] == FILL).all()) and bool((dZ1[:, n:] == FILL).all()) and float(loss[nblk]) == FILL
        if lo is not None:
            assert torch.equal(lo[:, :n], dZ1[:, :n].to(torch.bfloat16))
            assert bool((lo[:, n:] == 0).all())
        if planes is not None:  # an exact 3-way split of the fp32 dZ1, the first plane its rounding
            assert torch.equal(planes[:, :, :n].float().sum(0), dZ1[:, :n])
            assert torch.equal(planes[0, :, :n], dZ1[:, :n].to(torch.bfloat16))
            assert bool((planes[:, :, n:] == 0).all())
        # planes only (a null fp32 dZ1 is skipped)
        if planes is not None:
            p2 = torch.zeros_like(planes)
            m.mlp_head(code, TRAIN, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), labels=lab.data_ptr(), H=H,
                       C=C, n=n, scale=scale, D=D.data_ptr(), ldd=LDD, dZ1=0, ldz=LDZ, shift=shift,
                       stream=_stream(), dZ1_planes=p2.data_ptr(), npz=3)
            torch.cuda.synchronize()
            assert torch.equal(p2, planes)

        probs = torch.full((C, LDP), FILL, dtype=tdt, device="cuda")
        m.mlp_head(code, PROBS, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
                   probs=probs.data_ptr(), ldp=LDP, shift=shift, stream=_stream())
        torch.cuda.synchronize()
        assert _rel(probs[:, :n], yh) < tol, ("probs", shift)
        assert bool((probs[:, n:] == FILL).all())

    pred = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    m.mlp_head(code, PREDICT, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
               pred=pred.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    p = pred[:n].long()
    assert int(p.min()) >= 0 and int(p.max()) < C and int(pred[n]) == -5
    chosen = z2[p, torch.arange(n, device="cuda")]
    assert bool((z2.max(0).values - chosen <= tol * z2.abs().max()).all())


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("C", [17, 47, 64])
def test_head_predict_returns_the_first_maximum(C, dt):
    """Equal rows of W2 give bit-equal logits in every class tile: the lowest class wins; with classes 0..2 pushed
    down it is class 3, and with only the last class raised it is the last."""
    code, tdt = DT[dt]
    H, n = 100, 37
    W2, b2, a1, _ = _head_inputs(C, H, n, tdt, seed=C)
    W2[:] = W2[0].clone()
    m = hip()
    for b2v, want in ((torch.zeros(C), 0), (torch.tensor([-1.0] * 3 + [0.0] * (C - 3)), 3),
                      (torch.tensor([0.0] * (C - 1) + [1.0]), C - 1)):
        b = b2v.to(tdt).cuda()
        pred = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        m.mlp_head(code, PREDICT, a1.data_ptr(), LDA, W2.data_ptr(), b.data_ptr(), H=H, C=C, n=n,
                   pred=pred.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        assert bool((pred == want).all()), (want, pred.tolist())


def _engine_pair(dt, path, H, C, n, N):
    x, y = synthetic_mnist(N, seed=3, num_classes=C)
    nn = NeuralNetwork([784, H, C])
    engines = []
    for backend in ("hip", "torch"):
        e = MlpEngine(nn.H, dtype=dt, max_cols=n, device="cuda", backend=backend, path=path)
        e.set_params(*nn.params)
        e.load_dataset(x, y)
        engines.append(e)
    return engines


STEP_CFGS = [("f32", "split3"), ("bf16", "split1"), ("f32", "mfma"), ("f64", "mfma")]


@pytest.mark.parametrize("dt,path", STEP_CFGS)
@pytest.mark.parametrize("H,C,n", [(100, 47, 37), (100, 47, 96), (512, 26, 96)])
def test_step_gradients_match_torch(dt, path, H, C, n):
    """test_gpu_mlp.test_step_gradients_match_torch above 16 classes (512: the wide engines' dW1 launch)."""
    hipe, te = _engine_pair(dt, path, H, C, n, N=64 + 96)
    assert hipe.path == path
    scale, reg = 1.0 / n, 1e-4
    for e in (hipe, te):
        e.run(64, n, scale, reg, 0.0, sgd=False, with_loss=True)
    torch.cuda.synchronize()
    tol = TOL[(dt, path)]
    for name in ("gW1", "gb1", "gW2", "gb2"):
        err = _rel(getattr(hipe, name), getattr(te, name))
        print(f"{dt} {path} {H}-{C} n={n} {name}: {err:.3e} (tol {tol:g})")
        assert err < tol, name
    assert abs(hipe.loss_sum() - te.loss_sum()) / te.loss_sum() < 1e-4
    for name in ("a1", "dZ1", "D"):
        a = (hipe.dz1() if name == "dZ1" else getattr(hipe, name))[:, :n]
        b = getattr(te, name)[:, :n]
        err = _rel(a, b)
        print(f"{dt} {path} {H}-{C} n={n} {name}: {err:.3e} (tol {max(tol, 1e-5):g})")
        assert err < max(tol, 1e-5), name


@pytest.mark.parametrize("dt,path", STEP_CFGS)
def test_fused_sgd_matches_torch(dt, path):
    hipe, te = _engine_pair(dt, path, 100, 47, 96, N=192)
    for it in range(3):
        for e in (hipe, te):
            e.run(96 * (it % 2), 96, 1 / 96, 1e-4, 0.01, sgd=True)
    torch.cuda.synchronize()
    tol = {"f64": 1e-11, "f32": 1e-5, "bf16": 1e-2}[dt]
    assert _rel(hipe.params, te.params) < tol
    assert _rel(hipe.W2, te.W2) < tol and _rel(hipe.b2, te.b2) < max(tol, 1e-5)
    if hipe.W1p is not None:
        if not hipe.w1_planes_maintained():
            hipe.refresh_w1_planes()
        recon = hipe.W1p.float().sum(0)
        assert torch.equal(recon, hipe.W1 if path == "split3" else hipe.W1.to(torch.bfloat16).float())


@pytest.mark.parametrize("dt,path", STEP_CFGS)
def test_grads_then_sgd_matches_fused(dt, path):
    """sgd=0 (gradient bucket) + the flat SGD kernel == the fused in-place update."""
    a, _ = _engine_pair(dt, path, 100, 47, 96, N=192)
    b, _ = _engine_pair(dt, path, 100, 47, 96, N=192)
    a.run(0, 96, 1 / 96, 1e-4, 0.01, sgd=True)
    b.run(0, 96, 1 / 96, 1e-4, 0.0, sgd=False)
    b.sgd(0.01)
    torch.cuda.synchronize()
    assert _rel(a.params, b.params) < (1e-13 if dt == "f64" else 1e-6)
    if a.W1p is not None and a.w1_planes_maintained():
        assert torch.equal(a.W1p, b.W1p)


@pytest.mark.parametrize("H", [100, 512])
def test_bucketed_weight_gradients_equal_the_whole_step(H):
    """The overlapped all-reduce's pieces (forward + head, then the [b1|W2|b2] bucket, then dW1 row chunks) leave
    the gradients of the whole step: the output-layer part bitwise (the same launch), dW1 within the step's TOL."""
    n, C = 96, 47
    a, _ = _engine_pair("f32", "split3", H, C, n, N=192)
    b, _ = _engine_pair("f32", "split3", H, C, n, N=192)
    a.run(64, n, 1.0 / n, 1e-4, 0.0, sgd=False)
    assert b.supports_bucketed_wgrad
    b.run_forward_head(64, n, 1.0 / n)
    b.run_wgrad(64, n, 1.0 / n, 1e-4, parts=2)
    half = (H // 2 + 15) // 16 * 16
    b.run_wgrad(64, n, 1.0 / n, 1e-4, parts=1, row0=0, rows=half)
    b.run_wgrad(64, n, 1.0 / n, 1e-4, parts=1, row0=half, rows=H - half)
    torch.cuda.synchronize()
    assert torch.equal(a.gW2, b.gW2) and torch.equal(a.gb2, b.gb2)
    assert _rel(b.gW1, a.gW1) < TOL[("f32", "split3")] and _rel(b.gb1, a.gb1) < TOL[("f32", "split3")]


@pytest.mark.parametrize("dt,path", [("f32", "split3"), ("f64", "mfma")])
@pytest.mark.parametrize("H,n", [(100, 96), (512, 37)])
def test_step_is_deterministic_on_fresh_engines(dt, path, H, n):
    """No atomics, no arrival-order sums: the same step on two freshly created engines is bitwise equal (the head's
    row blocks each redo pass 1 -- H = 512 spreads pass 2 over 8 of them)."""
    x, y = synthetic_mnist(64 + 96, seed=3, num_classes=47)
    nn = NeuralNetwork([784, H, 47])
    ref = None
    for _ in range(2):
        e = MlpEngine(nn.H, dtype=dt, max_cols=n, device="cuda", path=path)
        e.set_params(*nn.params)
        e.load_dataset(x, y)
        e.run(64, n, 1.0 / n, 1e-4, 0.0, sgd=False, with_loss=True)
        torch.cuda.synchronize()
        got = [e.a1[:, :n].clone(), e.D[:, :n].clone(), e.dz1()[:, :n].clone(), e.grads.clone(), e.loss_buf.clone()]
        if ref is None:
            ref = got
        for name, a, b in zip(("a1", "D", "dZ1", "grads", "loss"), got, ref):
            assert torch.equal(a, b), (name, int((a != b).sum()))
        del e


@pytest.mark.parametrize("dt,path", STEP_CFGS)
def test_predict_is_within_tolerance_of_the_oracle_best(dt, path):
    """For every one of 512 samples the fp64 oracle's logit of the GPU's class is within TOL . max|z2| of the
    oracle's best logit (no sample excluded)."""
    x, _ = synthetic_mnist(512, seed=5, num_classes=47)
    nn = NeuralNetwork([784, 100, 47])
    e = MlpEngine(nn.H, dtype=dt, max_cols=512, device="cuda", path=path)
    e.set_params(*nn.params)
    pg = e.predict(x).astype(np.int64)
    assert pg.shape == (512,) and pg.min() >= 0 and pg.max() < 47
    W1, b1, W2, b2 = (np.asarray(p, np.float64) for p in nn.params)
    a1 = 1.0 / (1.0 + np.exp(-(x.astype(np.float64) @ W1.T + b1.reshape(1, -1))))
    z2 = a1 @ W2.T + b2.reshape(1, -1)
    gap = z2.max(1) - z2[np.arange(512), pg]
    bound = TOL[(dt, path)] * np.abs(z2).max()
    print(f"{dt} {path}: worst gap {gap.max():.3e}, bound {bound:.3e}, agree {np.mean(pg == z2.argmax(1)):.4f}")
    assert (gap <= bound).all()


def test_data_parallel_trainer_26_classes():
    C, N = 26, 1600
    x, y = synthetic_mnist(N, seed=7, num_classes=C)
    nn = NeuralNetwork([784, 100, C])
    loss0 = cpu_mlp.loss(nn, cpu_mlp.feedforward(nn, x).yc, y, 1e-4)
    tr = DataParallelTrainer(nn, dtype="f32", batch_size=800)
    tr.load(x, y)
    st = tr.train(1, 0.01, 1e-4)
    assert st.steps == 2
    loss1 = cpu_mlp.loss(nn, cpu_mlp.feedforward(nn, x).yc, y, 1e-4)
    print(f"loss {loss0:.6f} -> {loss1:.6f}")
    assert np.isfinite(loss1) and loss1 < loss0
    p = tr.predict(x)
    assert p.shape == (N,) and p.min() >= 0 and p.max() < C
