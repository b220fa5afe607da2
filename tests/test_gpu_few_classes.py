"""The <= 16-class output layer at class counts other than 10, against plain torch fp64 written here (never the
engine's torch backend, except for bf16 where input rounding dominates and the torch-backend bf16 engine is the
convention of tests/test_gpu_mlp.py).

What each group reaches (csrc/mlp):

* test_head_alone_matches_torch_fp64 -- ``mlp_head`` through its binding: ``head32_kernel`` (f32 TRAIN, H <= 128, the
  ``cls < C`` masks of head32 / head32_stage at C = 1, 2, 9, 11, 15, 16), ``launch_head<float,16>`` and
  ``launch_head<double,16>`` -> ``head_kernel<.,16,true>`` (every C != 10; PROBS / PREDICT in f32, all modes in f64 and at
  H = 130 > kH32MaxH), ``launch_head<.,10>`` -> ``head_kernel<.,10,true>`` at C = 10, ``head_stage``'s ``c < C``.
* test_head_predict_returns_the_first_maximum -- the PREDICT argmax of ``head_kernel<.,16,true>``.
* test_head_without_lds_and_at_the_lds_threshold -- ``head_kernel<double,16,false>``, ``head_kernel<double,10,false>``,
  ``head_kernel<float,16,false>`` (W2 read from global memory, ``c < C`` guards in ``w2``), and the largest LDS forms.
* test_*_step_matches_fp64 -- whole steps with the form asserted first: ``fwd1_head_ag_kernel`` / fha_body (allgather, with
  and without the head's dW2 partials), ``fwd1_head_kernel`` + head32<true> (last_arriver), ``fwd1_split_kernel`` +
  ``head_kernel<float,16,true>`` + ``wgrad_split_kernel``'s dW2 / db2 roles (separate, H = 300), the fused wide heads on
  the 64 x 64 (wide64) and 128 x 128 (wide128) tilings, ``fwd1_glds_kernel`` + ``head_wide_kernel`` + ``wgrad_glds_kernel``
  (the wide separate form: z2 partials, the dW2-partial stores), and the plain ``fwd1_kernel`` / ``head32_kernel`` or
  ``head_kernel`` / ``wgrad_kernel`` of the mfma paths.
* test_xstep_pipeline_few_classes -- the XCD-local pipeline (xstep.hip role workgroups) at C = 2 and 16.
* test_predict_is_within_tolerance_of_the_oracle_best -- MlpStep.predict and, on the mfma path, ``mlp_forward1`` + the
  PREDICT head with NC = 16.

Tolerances: f64 1e-11 relative max-norm; f32 against fp64 1e-5 per gradient (tests/test_gpu_mlp.py
test_f32_gradients_are_fp32_class_vs_fp64) or, where a shape's own fp32 rounding is larger, 4x the error of a plain
fp32 torch evaluation of the same step against the fp64 one (both are logged); 1e-4 on the loss; bf16 3e-2 against the
torch-backend bf16 engine.  The head-alone cases use tests/test_gpu_mlp.py's TOL, copied because a test module does not
import another.  The loss partials are fp32 in every dtype, so the f64 loss is compared at 1e-6 (fp32 epsilon 6e-8 times
the 16-term sum and its log).  Measured worst errors: profiles/numerics_classes_widths.jsonl."""
import functools
import json

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import hip
from cme213_sp18_amd.parallel import MlpEngine
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
LR, REG = 0.01, 1e-4  # (the learning rate of test_fused_sgd_matches_torch: raw pixels at 0.05 amplify rounding over steps)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _log(**kw):
    print("NUMERICS " + json.dumps(kw))


# ------------------------------------------------------------------------------------------------ the head alone
def _head_inputs(C, H, n, tdt, seed):
    """Random, non-symmetric operands; every class among the labels (n permitting), class C - 1 in the first and the
    last column."""
    g = torch.Generator().manual_seed(seed)
    W2 = (torch.randn(C, H, generator=g, dtype=torch.float64) * 0.3).to(tdt)
    b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.1).to(tdt)
    a1 = torch.full((H, LDA), FILL, dtype=torch.float64)
    a1[:, :n] = torch.rand(H, n, generator=g, dtype=torch.float64) * 0.9 + 0.05
    lab = ((torch.arange(n) * 7 + 3) % C).to(torch.int32)  # (7 is coprime to every C used: C consecutive columns hold all)
    lab[0] = lab[n - 1] = C - 1
    if n >= 32:
        assert set(lab.tolist()) == set(range(C))
    return W2.cuda(), b2.cuda(), a1.to(tdt).cuda(), lab.cuda()


def _head_reference(W2, b2, a1, lab, n, scale, shift):
    """fp64 torch: z2, yhat, D, dZ1 and the loss partial of every 16-column block."""
    W, b, A = W2.double(), b2.double(), a1[:, :n].double()
    z2 = W @ A + b[:, None]
    zs = z2 - z2.max(0, keepdim=True).values if shift else z2
    e = torch.exp(zs)
    yh = e / e.sum(0, keepdim=True)
    cols = torch.arange(n, device=yh.device)
    onehot = torch.zeros_like(yh)
    onehot[lab.long(), cols] = 1.0
    D = (yh - onehot) * scale
    dZ1 = (W.t() @ D) * A * (1 - A)
    lcol = -torch.log(yh[lab.long(), cols])
    loss = torch.stack([lcol[16 * k: 16 * k + 16].sum() for k in range((n + 15) // 16)])
    return z2, yh, D, dZ1, loss


def _check_head(C, H, n, dt):
    """Every mode of mlp_head at one (C, H, n, dtype): values against fp64, sentinels past column n, past row C and
    past the last loss partial."""
    code, tdt = DT[dt]
    tol = TOL[(dt, "mfma")]
    m = hip()
    W2, b2, a1, lab = _head_inputs(C, H, n, tdt, seed=1000 * C + 10 * H + n)
    scale = 1.0 / (3 * n)
    nblk = (n + 15) // 16
    worst = {}

    def close(name, got, want, bound, absolute=None):
        # C = 1: D, dZ1 and the loss are zero in exact arithmetic -- compared absolutely
        err = float(got.double().abs().max()) / absolute if absolute else _rel(got, want)
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= bound, (name, err, bound)

    for shift in (1, 0):
        z2, yh, Dr, dZr, lossr = _head_reference(W2, b2, a1, lab, n, scale, shift)
        D = torch.full((16, LDD), FILL, dtype=tdt, device="cuda")
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
        if C == 1:
            close("D", D[:C, :n], Dr, tol, absolute=scale)
            close("dZ1", dZ1[:, :n], dZr, tol, absolute=scale * float(W2.abs().max()))  # (|a (1 - a)| <= 1/4)
            close("loss", loss[:nblk], lossr, tol, absolute=1.0)
        else:
            close("D", D[:C, :n], Dr, tol)
            close("dZ1", dZ1[:, :n], dZr, tol)
            close("loss", loss[:nblk], lossr, max(tol, 1e-6))  # (fp32 partials in both dtypes)
        # nothing past the n columns, past the C rows, past the last block's partial
        assert bool((D[:, n:] == FILL).all()) and bool((D[C:] == FILL).all())
        assert bool((dZ1[:, n:] == FILL).all()) and float(loss[nblk]) == FILL
        if lo is not None:
            assert torch.equal(lo[:, :n], dZ1[:, :n].to(torch.bfloat16))
            assert bool((lo[:, n:] == 0).all())
        if planes is not None:  # an exact 3-way split of the fp32 dZ1, the first plane its rounding
            assert torch.equal(planes[:, :, :n].float().sum(0), dZ1[:, :n])
            assert torch.equal(planes[0, :, :n], dZ1[:, :n].to(torch.bfloat16))
            assert bool((planes[:, :, n:] == 0).all())
            # planes only (a null fp32 dZ1 is skipped)
            p2 = torch.zeros_like(planes)
            m.mlp_head(code, TRAIN, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), labels=lab.data_ptr(), H=H,
                       C=C, n=n, scale=scale, D=D.data_ptr(), ldd=LDD, dZ1=0, ldz=LDZ, shift=shift,
                       stream=_stream(), dZ1_planes=p2.data_ptr(), npz=3)
            torch.cuda.synchronize()
            assert torch.equal(p2, planes)

        probs = torch.full((16, LDP), FILL, dtype=tdt, device="cuda")
        m.mlp_head(code, PROBS, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
                   probs=probs.data_ptr(), ldp=LDP, shift=shift, stream=_stream())
        torch.cuda.synchronize()
        close("probs", probs[:C, :n], yh, tol)
        assert bool((probs[:, n:] == FILL).all()) and bool((probs[C:] == FILL).all())

    pred = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
    m.mlp_head(code, PREDICT, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
               pred=pred.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    p = pred[:n].long()
    assert int(p.min()) >= 0 and int(p.max()) < C and int(pred[n]) == -5
    chosen = z2[p, torch.arange(n, device="cuda")]
    assert bool((z2.max(0).values - chosen <= tol * z2.abs().max()).all())
    _log(test="head_alone", dt=dt, C=C, H=H, n=n, tol=tol, **worst)


# f32 H <= 128: head32_kernel in TRAIN, head_kernel<float, .> for PROBS / PREDICT; 130 is just past kH32MaxH
HEAD_CASES = [("f32", H) for H in (16, 100, 128, 130)] + [("f64", H) for H in (100, 130)]


@pytest.mark.parametrize("dt,H", HEAD_CASES)
@pytest.mark.parametrize("n", [1, 32, 37])
@pytest.mark.parametrize("C", [1, 2, 9, 10, 11, 15, 16])
def test_head_alone_matches_torch_fp64(C, H, n, dt):
    """mlp_head at C <= 16 in every mode: no class padding (16), a partly live last lane group (11, 15), whole lane
    groups dead (1, 2, 9), the NC = 10 instantiation (10); a single column, a whole 32-column tile, a column tail."""
    _check_head(C, H, n, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("C", [2, 11, 16])
def test_head_predict_returns_the_first_maximum(C, dt):
    """Equal rows of W2 give bit-equal logits: the lowest class wins; with the leading classes pushed down it is the
    first class that is not, and with only the last class raised it is the last."""
    code, tdt = DT[dt]
    H, n = 100, 37
    W2, b2, a1, _ = _head_inputs(C, H, n, tdt, seed=C)
    W2[:] = W2[0].clone()
    m = hip()
    k = min(3, C - 1)  # (classes 0..k-1 pushed down: class k is the first maximum)
    for b2v, want in ((torch.zeros(C), 0), (torch.tensor([-1.0] * k + [0.0] * (C - k)), k),
                      (torch.tensor([0.0] * (C - 1) + [1.0]), C - 1)):
        b = b2v.to(tdt).cuda()
        pred = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        m.mlp_head(code, PREDICT, a1.data_ptr(), LDA, W2.data_ptr(), b.data_ptr(), H=H, C=C, n=n,
                   pred=pred.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        assert bool((pred == want).all()), (want, pred.tolist())


@pytest.mark.parametrize("dt,C,H", [("f64", 16, 512), ("f64", 10, 819), ("f64", 16, 511), ("f64", 10, 818),
                                    ("f32", 16, 1024)])
def test_head_without_lds_and_at_the_lds_threshold(dt, C, H):
    """launch_head stages W2^T in (H NC + NC) elements of dynamic LDS up to 64 KB and reads W2 from global memory
    above: f64 (16, 512) -> 65664 B and (10, 819) -> 65600 B take head_kernel<double, NC, false>, f32 (16, 1024) ->
    65600 B head_kernel<float, 16, false>; f64 (16, 511) -> exactly 65536 B and (10, 818) -> 65520 B are the largest
    LDS forms, launched next to the kernel's static zred + lred (8192 + 16 B at NC = 16, 5120 + 16 B at NC = 10).
    launch_head compares only the dynamic size with 64 KB and sets no LDS limit attribute; measured on an MI355X:
    both largest forms (73744 B and 70656 B of LDS per workgroup in all) are accepted and compute the right values
    (gfx950 workgroups may use up to 160 KB), so the threshold needs no correction for the static arrays."""
    _check_head(C, H, 37, dt)


# ------------------------------------------------------------------------------------------------ whole steps
@functools.lru_cache(maxsize=None)
def _data(N, C, seed=3):
    return synthetic_mnist(N, seed=seed, num_classes=C)


def _params(H, C):
    """The network's initial weights with non-zero biases (the initial ones are zero: a dropped bias would not show)."""
    nn = NeuralNetwork([784, H, C])
    g = np.random.default_rng(H + C)
    W1, _, W2, _ = nn.params
    return W1, g.normal(0, 0.1, H), W2, g.normal(0, 0.1, C)


def _engine(dt, path, H, C, n, N, backend="hip", seed=3):
    e = MlpEngine((784, H, C), dtype=dt, max_cols=n, device="cuda", backend=backend, path=path)
    e.set_params(*_params(H, C))
    e.raw = _data(N, C, seed)
    e.load_dataset(*e.raw)
    return e


def _step_math(x, lab, W1, b1, W2, b2, scale, reg):
    """One step in plain torch, in the dtype of its arguments: x [n][P], lab [n] -> gradients, loss sum, D [C][n]."""
    z1 = x @ W1.t() + b1
    a1 = 1.0 / (1.0 + torch.exp(-z1))
    z2 = a1 @ W2.t() + b2
    z2 = z2 - z2.max(1, keepdim=True).values
    e = torch.exp(z2)
    yh = e / e.sum(1, keepdim=True)
    rows = torch.arange(x.shape[0], device=x.device)
    onehot = torch.zeros_like(yh)
    onehot[rows, lab] = 1.0
    D = (yh - onehot) * scale
    dZ1 = (D @ W2) * a1 * (1 - a1)
    return {"gW1": dZ1.t() @ x + reg * W1, "gb1": dZ1.sum(0), "gW2": D.t() @ a1 + reg * W2, "gb2": D.sum(0),
            "loss": -torch.log(yh[rows, lab]).sum(), "D": D.t()}


def _step_refs(e, off, n, scale, reg):
    """The step of engine `e` on samples [off, off + n) in fp64 and in fp32, from the engine's own parameters."""
    out = []
    for tdt in (torch.float64, torch.float32):
        x = e.X[off:off + n].to(tdt) * e.xscale  # (the split paths keep raw pixels; the others hold scaled values)
        lab = e.labels[off:off + n].long()
        out.append(_step_math(x, lab, *(t.to(tdt) for t in (e.W1, e.b1, e.W2, e.b2)), scale, reg))
    return out


def _check_step(e, dt, path, n, tag, off=64, names=("gW1", "gb1", "gW2", "gb2", "D", "loss")):
    """One gradient step of `e` against fp64 (f32, f64) or against the torch-backend bf16 engine (bf16)."""
    scale = 1.0 / n
    e.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
    torch.cuda.synchronize()
    assert not e.kernel_error()
    if dt == "bf16":
        te = MlpEngine((e.P, e.H, e.C), dtype=dt, max_cols=n, device="cuda", backend="torch", path=path)
        te.set_params(*(t.cpu().numpy() for t in (e.W1, e.b1, e.W2, e.b2)))
        te.load_dataset(*e.raw, normalize=e._normalize)
        te.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
        ref = {k: getattr(te, k) for k in ("gW1", "gb1", "gW2", "gb2")}
        ref["D"], ref["loss"] = te.D[:, :n], torch.tensor(te.loss_sum())
        r32 = None
    else:
        ref, r32 = _step_refs(e, off, n, scale, REG)
    for name in names:
        got = torch.tensor(e.loss_sum()) if name == "loss" else (e.D[:, :n] if name == "D" else getattr(e, name))
        err = _rel(got.cpu(), ref[name].cpu())
        if dt == "bf16":
            bound, e32 = TOL[(dt, path)], None
        elif dt == "f64":
            bound, e32 = (1e-6 if name == "loss" else 1e-11), None  # (the loss partials are fp32)
        else:
            e32 = _rel(r32[name].cpu(), ref[name].cpu())
            bound = 1e-4 if name == "loss" else max(1e-5, 4 * e32)
        _log(test="step", tag=tag, dt=dt, path=path, P=e.P, H=e.H, C=e.C, n=n, off=off, what=name, err=err,
             fp32_torch_err=e32, bound=bound)
        assert err < bound, (name, err, bound)


def _forced(e, **attrs):
    st = e._hip_step()
    for k, v in attrs.items():
        setattr(st, k, v)
    return st


CLASSES = [2, 11, 16]


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("head_dw2", [1, 0])
@pytest.mark.parametrize("H,n", [(100, 96), (128, 37)])
def test_allgather_step_matches_fp64(H, n, head_dw2, C):
    """fwd1_head_ag_kernel (fha_body): with the head's dW2 partials per 16 columns summed by the weight-gradient
    launch's role, and with that role forming D a1^T itself."""
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    st = _forced(e, head_dw2=head_dw2)
    plan = st.plan(64, n, 0, 3)
    assert plan["form"] == "allgather" and plan["dw2_cols"] == (16 if head_dw2 else 0)
    _check_step(e, "f32", "split3", n, f"allgather/dw2_{head_dw2}")


@pytest.mark.parametrize("C", CLASSES)
def test_last_arriver_step_matches_fp64(C):
    """fwd1_head_kernel: the last row-tile workgroup of a column tile runs head32<true>."""
    H, n = 100, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    e.set_fh_allgather(False)
    assert e._hip_step().plan(64, n, 0, 3)["form"] == "last_arriver"
    _check_step(e, "f32", "split3", n, "last_arriver")


@pytest.mark.parametrize("C", CLASSES)
def test_separate_step_matches_fp64(C):
    """H = 300: fwd1_split_kernel, then the column head (launch_head<float, 16>: no z2 partials below H = 512 and
    H > kH32MaxH), then wgrad_split_kernel with its dW2 / db2 roles."""
    H, n = 300, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "separate" and plan["dw2_cols"] == 0
    _check_step(e, "f32", "split3", n, "separate")


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("dt,path", [("f32", "split3"), ("bf16", "split1")])
def test_wide64_step_matches_fp64(dt, path, C):
    """The all-gather head fused into the 64 x 64 direct-to-LDS forward (taken when a1 is not stored)."""
    H, n = 512, 64
    e = _engine(dt, path, H, C, n, 64 + n + 16)
    e.set_store_a1(False)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "wide64" and plan["dw2_cols"] == 64
    _check_step(e, dt, path, n, "wide64")


@pytest.mark.parametrize("C", [2, 16])
def test_wide128_step_matches_fp64(C):
    """The all-gather head fused into the 128 x 128 A-in-registers forward (24 x 8 = 192 tiles: the smallest shape
    tests/test_gpu_step_plan.py records for it)."""
    H, n = 3072, 1024
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "wide128" and plan["dw2_cols"] == 128
    _check_step(e, "f32", "split3", n, "wide128")


@pytest.mark.parametrize("C", CLASSES)
def test_wide_separate_step_matches_fp64(C):
    """fwd1_glds_kernel leaving z2 partials, head_wide_kernel (its ``zc < C`` / ``c < C`` masks and the dW2-partial
    stores), then the wide weight-gradient launch summing the partials."""
    H, n = 512, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    e.set_fh_allgather(False)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "separate" and plan["dw2_cols"] == 32
    _check_step(e, "f32", "split3", n, "wide_separate")


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("H,n", [(100, 37), (300, 96)])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16"])
def test_plain_step_matches_fp64(dt, H, n, C):
    """The mfma paths (no plan: MlpStep.run_plain always runs mlp_forward1, mlp_head, mlp_wgrad): fwd1_kernel, head32_kernel
    (f32 / bf16 at H = 100) or head_kernel<., 16 | 10, true>, and wgrad_kernel's dW2 / bias roles."""
    e = _engine(dt, "mfma", H, C, n, 64 + n + 16)
    assert e.path == "mfma" and e._hip_step().split == 0
    _check_step(e, dt, "mfma", n, "plain")


# ------------------------------------------------------------------------------------------------ the pipeline
def _sgd_steps(x, lab, params, offs, n, scale, reg, lr, tdt):
    """Plain torch SGD over the batches starting at `offs`, in dtype `tdt`: the final (W1, b1, W2, b2)."""
    W1, b1, W2, b2 = (t.to(tdt).clone() for t in params)
    for off in offs:
        g = _step_math(x[off:off + n].to(tdt), lab[off:off + n].long(), W1, b1, W2, b2, scale, reg)
        W1, b1, W2, b2 = W1 - lr * g["gW1"], b1 - lr * g["gb1"], W2 - lr * g["gW2"], b2 - lr * g["gb2"]
    return W1, b1, W2, b2


def _flat(ts):
    return torch.cat([t.double().reshape(-1) for t in ts])


def _check_update(e, before, offs, n, tag):
    """params_after - params_before of engine `e` against the same steps in fp64; the bound is 4x the error of the
    same steps in plain fp32 torch (from the two references alone)."""
    after = [t.clone() for t in (e.W1, e.b1, e.W2, e.b2)]
    runs = [_sgd_steps(e.X.to(t) * e.xscale, e.labels, before, offs, n, 1.0 / n, REG, LR, t)
            for t in (torch.float64, torch.float32)]
    d64 = _flat(runs[0]) - _flat(before)
    e32 = _rel(_flat(runs[1]) - _flat(before), d64)
    err = _rel(_flat(after) - _flat(before), d64)
    _log(test="update", tag=tag, P=e.P, H=e.H, C=e.C, n=n, steps=len(offs), err=err, fp32_torch_err=e32, bound=4 * e32)
    assert err < 4 * e32, (err, e32)


@pytest.mark.parametrize("C", [2, 16])
def test_xstep_pipeline_few_classes(C):
    """Two epochs as ONE pipeline launch at C = 2 and 16 (tests/test_gpu_xstep.py pairs the forms at C = 10 only):
    parameters bitwise those of the two-launch step, whose update is then compared with the same steps in fp64 --
    both forms share fha_body, so the bitwise comparison alone cannot see a masking bug."""
    H, n = 100, 256
    N = 5 * n + 48
    engines = []
    for xs in (0, -1):
        e = _engine("f32", "split3", H, C, n, N, seed=H + n)
        e.set_store_a1(False)
        _forced(e, xstep=xs, head_dw2=1)
        engines.append(e)
    before = [t.clone() for t in (engines[0].W1, engines[0].b1, engines[0].W2, engines[0].b2)]
    count = 2 * (N // n)
    for e in engines:
        e._hip_step().run_steps(0, count, n, 0, n, N, 1.0 / n, REG, LR, 1, _stream())
    torch.cuda.synchronize()
    assert engines[1]._hip_step().xstep_used == 1, engines[1]._hip_step().xstep_reason
    assert engines[0]._hip_step().xstep_used == 0
    assert torch.equal(engines[0].params, engines[1].params)
    for e in engines:
        assert not e.kernel_error()
    offs = [n * (i % (N // n)) for i in range(count)]  # (the walk wraps before the partial batch at the end)
    _check_update(engines[0], before, offs, n, "xstep")


# ------------------------------------------------------------------------------------------------ predict
@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("dt,path", [("f32", "split3"), ("f64", "mfma"), ("bf16", "split1")])
def test_predict_is_within_tolerance_of_the_oracle_best(dt, path, C):
    """For every one of 256 samples the fp64 oracle's logit of the GPU's class is within TOL . max|z2| of the
    oracle's best logit (no sample excluded)."""
    x, _ = _data(256, C, 5)
    params = _params(100, C)
    e = MlpEngine((784, 100, C), dtype=dt, max_cols=256, device="cuda", path=path)
    e.set_params(*params)
    pg = e.predict(x).astype(np.int64)
    assert pg.shape == (256,) and pg.min() >= 0 and pg.max() < C
    W1, b1, W2, b2 = (np.asarray(p, np.float64) for p in params)
    a1 = 1.0 / (1.0 + np.exp(-(x.astype(np.float64) @ W1.T + b1.reshape(1, -1))))
    z2 = a1 @ W2.T + b2.reshape(1, -1)
    gap = z2.max(1) - z2[np.arange(256), pg]
    bound = TOL[(dt, path)] * np.abs(z2).max()
    _log(test="predict", dt=dt, path=path, C=C, worst_gap=float(gap.max()), bound=float(bound),
         agree=float(np.mean(pg == z2.argmax(1))))
    assert (gap <= bound).all()
