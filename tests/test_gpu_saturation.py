"""The output-layer heads, the evaluation head and the sigmoid epilogues at SATURATED logits and pre-activations,
per element against fp64 (the other GPU tests of these kernels run in the benign middle of the number line and compare
in the max norm, where an error in a small element never shows).

Operands: tests/saturation_cases.py -- logits top - gap that are exact in fp32 in any summation order, gaps from
G = {0, .5, 1, 3, 8, 16, 32, 64, 80, 86, 87, 88, 90, 104, 150, 200}, tops {0, +40, -75, +1000} (shifted softmax),
exact ties for the maximum, labels on every rung; tests/test_saturation.py checks that construction and the bounds on
the CPU.  What is compared, per element, no element left out:

* yhat / PROBS and D / scale: |got - ref| <= (gap + 8) 2^-23 |ref| + 2^-126 in fp32 (bf16 mode's head is fp32),
  (gap + 8) 2^-50 |ref| in fp64.  __expf is v_exp_f32(x log2 e): 1 ulp plus the argument's rounding, gap 2^-24
  relative; a few ulps for the sum, the reciprocal and the multiply; the floor is the flush of denormals.  At the
  label's element of D / scale, |ref| is max(yhat, 1 - yhat) (saturation_cases.grad_bound: yhat - 1 can be smaller than
  yhat's last bit, which no fp32 yhat can resolve).
* the loss partial of every 16-column block: sum over its columns of (l + 4) 2^-22 (fp32 partials in every dtype), and
  finite on every rung: the heads form log(sum) - (z_label - m) (head_math.h head_nll); -log(yhat[label]) was +inf
  from a label gap of 88 on.
* dZ1 and the gradients: finite, 1e-5 max-norm relative or 4x the error of a plain fp32 evaluation (both logged), f64
  1e-11, bf16 3e-2 against the torch-backend bf16 engine (tests/test_gpu_few_classes.py's rule); dZ1 exactly 0 where a1
  is 0 or 1.
* PREDICT / the evaluation head's pred: exactly the lowest class at gap 0.
* sentinels past n, past C and past the last loss partial.

Which test catches what: dropping a ``cls < C`` mask puts exp(0 - m) of a padded class into the sum -- with top = -75
that is e^75 against 1 and every yhat of the column fails (test_head_*, C = 2, 10, 11, 17, 47); dropping one fmaxf lane
exchange leaves a lane group with a smaller maximum -- e^(+gap) overflows or the sum differs between lane groups
(test_head_* at C = 16 / 47 / 64, where the winner walks over all lane groups); breaking a tie upward fails the exact
PREDICT / confusion comparison on the tie patterns; the old loss form fails ``finite`` on the rungs from 88 up in every
train-mode case and in test_step_loss_equals_evaluation_loss.

The engine forwards' sigmoid is checked at the shapes that select each forward (n = 96 / 1024); the untouched column
tail (n = 37) is checked on mlp_forward1, whose pitch the test owns -- the engine's padding columns are the kernels'
to use.  The unshifted softmax (shift = 0) runs with tops {0, +-4, 2}: saturation_cases.py says why.

Measured on an MI355X (profiles/numerics_saturation.jsonl: the NUMERICS lines of a run with -s, the worst ratio of
error to bound per case): yhat, D / scale and the sigmoid 0.515 in fp32 (0.06 in fp64), the loss partials 0.53, the
training heads' summed loss against the evaluation head's 0.15 of the sum of their bounds."""
import json

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import hip
from cme213_sp18_amd.parallel import DataParallelTrainer, MlpEngine

from . import saturation_cases as sc

pytestmark = pytest.mark.gpu

DT = {"f32": (0, torch.float32), "f64": (1, torch.float64), "bf16": (2, torch.bfloat16)}
TRAIN, PREDICT, PROBS = 0, 1, 2
LDA, LDD, LDZ, LDP = 48, 64, 80, 56  # distinct pitches, each >= the largest n = 37
FILL = 7.0
REG = 1e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _log(**kw):
    print("NUMERICS " + json.dumps(kw))


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _eps(dt):
    return (sc.EPS64, 0.0) if dt == "f64" else (sc.EPS32, sc.TINY32)


def _dev(a, tdt, pitch=None):
    """A host array on the device in dtype tdt; 2-D with `pitch`: FILL past its columns."""
    t = torch.as_tensor(np.asarray(a))
    if pitch is not None:
        full = torch.full((t.shape[0], pitch), FILL, dtype=torch.float64)
        full[:, :t.shape[1]] = t
        t = full
    return t.to(tdt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ the head alone
def _check_head(C, H, n, dt):
    """Every mode of mlp_head at one (C, H, n, dtype) and both shifts; returns {shift: loss partials} and the fp64
    per-column loss for the comparison with the evaluation head."""
    code, tdt = DT[dt]
    eps, floor = _eps(dt)
    m = hip()
    scale = 1.0 / (3 * n)
    nblk, CP = (n + 15) // 16, (C + 15) // 16 * 16
    worst, out = {}, {}

    def ratio(name, got, ref, bound):
        r = sc.worst_ratio(got, ref, bound)
        worst[name] = max(worst.get(name, 0.0), r)
        return r

    for shift in (1, 0):
        W2h, b2h, a1h, labh, z2, gap = sc.head_operands(C, H, n, shift, p0=12 if n == 1 else 0)
        yh, dref, Dr, dZr, lossr, predr = sc.head_reference(W2h, b2h, a1h, labh, z2, scale)
        onehot = (dref != yh).astype(np.float64)
        W2, b2, a1 = _dev(W2h, tdt), _dev(b2h, tdt), _dev(a1h, tdt, LDA)
        lab = torch.as_tensor(labh).cuda()
        D = torch.full((CP, LDD), FILL, dtype=tdt, device="cuda")
        dZ1 = torch.full((H, LDZ), FILL, dtype=tdt, device="cuda")
        loss = torch.full((nblk + 1,), FILL, dtype=torch.float32, device="cuda")
        m.mlp_head(code, TRAIN, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), labels=lab.data_ptr(), H=H, C=C,
                   n=n, scale=scale, D=D.data_ptr(), ldd=LDD, dZ1=dZ1.data_ptr(), ldz=LDZ, loss=loss.data_ptr(),
                   shift=shift, stream=_stream())
        probs = torch.full((CP, LDP), FILL, dtype=tdt, device="cuda")
        m.mlp_head(code, PROBS, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
                   probs=probs.data_ptr(), ldp=LDP, shift=shift, stream=_stream())
        pred = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
        m.mlp_head(code, PREDICT, a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), H=H, C=C, n=n,
                   pred=pred.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        tag = (C, H, n, dt, shift)
        r = ratio("probs", _np(probs[:C, :n]), yh, sc.prob_bound(gap, yh, eps, floor))
        assert r <= 1.0, ("probs", tag, r)
        r = ratio("D", _np(D[:C, :n]) / scale, dref, sc.grad_bound(gap, yh, onehot, eps, floor))
        assert r <= 1.0, ("D", tag, r)
        lg = _np(loss[:nblk])
        assert np.isfinite(lg).all(), ("loss", tag, lg.tolist())
        r = ratio("loss", lg, sc.block_sums(lossr), sc.loss_bound(lossr))
        assert r <= 1.0, ("loss", tag, r)
        dz = _np(dZ1[:, :n])
        assert np.isfinite(dz).all() and (dz[(a1h == 0) | (a1h == 1)] == 0).all(), ("dZ1", tag)
        err = _rel(dz, dZr)
        e32 = _rel(sc.head_f32(W2h, b2h, a1h, labh, scale, shift)[2], dZr)
        bound = 1e-11 if dt == "f64" else max(1e-5, 4 * e32)
        worst["dZ1_err"], worst["dZ1_fp32_numpy_err"] = max(worst.get("dZ1_err", 0.0), err), e32
        assert err <= bound, ("dZ1", tag, err, bound)
        # the lowest class at gap 0, exactly (the logits are exact): ties, the tie in the last live class, top +1000
        assert np.array_equal(pred[:n].cpu().numpy(), predr), ("pred", tag, pred[:n].tolist(), predr.tolist())
        # nothing past the n columns, past the C rows, past the last block's partial, past pred[n]
        assert bool((D[:, n:] == FILL).all()) and bool((D[C:] == FILL).all())
        assert bool((probs[:, n:] == FILL).all()) and bool((probs[C:] == FILL).all())
        assert bool((dZ1[:, n:] == FILL).all()) and float(loss[nblk]) == FILL and int(pred[n]) == -5
        out[shift] = (lg, lossr, (a1, W2, b2, lab, labh, z2))
    _log(test="head_alone", dt=dt, C=C, H=H, n=n, **worst)
    return out


# f32 H <= 128: head32_kernel in TRAIN, head_kernel<float, .> for PROBS / PREDICT and past kH32MaxH; f64: head_kernel
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("C", [2, 10, 11, 16])
@pytest.mark.parametrize("dt,H", [("f32", 16), ("f32", 100), ("f32", 130), ("f64", 100)])
def test_head_at_saturated_logits(dt, H, C, n):
    _check_head(C, H, n, dt)


def test_head_without_lds_at_saturated_logits():
    """f32 (16, 1024): head_kernel<float, 16, false>, W2 read from global memory."""
    _check_head(16, 1024, 37, "f32")


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("H", [16, 100])
@pytest.mark.parametrize("C", [17, 47, 64])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_many_class_head_at_saturated_logits(dt, C, H, n):
    """head_mc_kernel: the ladder wraps over the classes, the tie sits across two class tiles."""
    _check_head(C, H, n, dt)


# ------------------------------------------------------------------------------------------------ the evaluation head
@pytest.mark.parametrize("C", [2, 16, 47])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_eval_head_and_training_head_report_the_same_loss(dt, C):
    """mlp_eval_head on the training head's operands: loss_sum against fp64 at (l + 4) 2^-22 per sample (f32) / 1e-11
    (f64), the hit count and the confusion matrix exactly (ties -> the lower class), and the training head's summed
    loss partials within the sum of the two bounds of it."""
    H, n = 100, 37
    lg, lossr, (a1, W2, b2, lab, labh, z2) = _check_head(C, H, n, dt)[1]
    words = 3 + C * C
    stats = torch.full((words + 8,), 12345, dtype=torch.int64, device="cuda")
    partials = torch.zeros(256, dtype=torch.float64, device="cuda")
    hip().mlp_eval_head(DT[dt][0], a1.data_ptr(), LDA, W2.data_ptr(), b2.data_ptr(), lab.data_ptr(), H, C, n,
                        stats.data_ptr(), partials.data_ptr(), 1, _stream())
    torch.cuda.synchronize()
    w = stats.cpu()
    assert (w[words:] == 12345).all() and int(w[0]) == n
    got = float(w[2:3].view(torch.float64)[0])
    ebound = float(sc.loss_bound(lossr).sum()) if dt == "f32" else 1e-11 * float(lossr.sum())
    assert np.isfinite(got) and abs(got - lossr.sum()) <= ebound, (got, lossr.sum(), ebound)
    predr = z2.argmax(0)  # the first maximum
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (labh, predr), 1)
    assert np.array_equal(w[3:words].view(C, C).numpy(), want) and int(w[1]) == int((predr == labh).sum())
    tbound = float(sc.loss_bound(lossr).sum())
    assert abs(float(lg.sum()) - got) <= tbound + ebound, (float(lg.sum()), got)
    _log(test="eval_head", dt=dt, C=C, H=H, n=n, loss=abs(got - lossr.sum()) / ebound,
         train_vs_eval=abs(float(lg.sum()) - got) / (tbound + ebound))


# ------------------------------------------------------------------------------------------------ whole steps
def _engine(dt, path, H, C, n, N, backend="hip"):
    ops = sc.step_operands(784, H, C, N)
    e = MlpEngine((784, H, C), dtype=dt, max_cols=n, device="cuda", backend=backend, path=path)
    e.set_params(*ops[2:6])
    e.load_dataset(ops[0], ops[1])
    e.ops = ops
    return e


def _forced(e, **attrs):
    st = e._hip_step()
    for k, v in attrs.items():
        setattr(st, k, v)
    return st


def _step_math(x, lab, W1, b1, W2, b2, scale, reg):
    """One step in plain torch in the dtype of its arguments (x [n][P]); the loss in the stable form."""
    z1 = x @ W1.t() + b1
    a1 = 1.0 / (1.0 + torch.exp(-z1))
    z2 = a1 @ W2.t() + b2
    m = z2.max(1, keepdim=True).values
    e = torch.exp(z2 - m)
    s = e.sum(1, keepdim=True)
    yh = e / s
    rows = torch.arange(x.shape[0], device=x.device)
    onehot = torch.zeros_like(yh)
    onehot[rows, lab] = 1.0
    D = (yh - onehot) * scale
    dZ1 = (D @ W2) * a1 * (1 - a1)
    return {"gW1": dZ1.t() @ x + reg * W1, "gb1": dZ1.sum(0), "gW2": D.t() @ a1 + reg * W2, "gb2": D.sum(0),
            "loss_cols": torch.log(s[:, 0]) - (z2[rows, lab] - m[:, 0]), "yh": yh.t(), "dZ1": dZ1.t(), "a1": a1.t(),
            "z2": z2.t()}


def _check_step(e, dt, path, n, tag, off=64):
    """One gradient step with loss of `e` on samples [off, off + n)."""
    C, H = e.C, e.H
    eps, floor = _eps(dt)
    scale = 1.0 / n
    for t in (e.dZ1, e.dZ1s, e.dZ1p):  # (a finite sentinel: whichever form of dZ1 the step leaves shows)
        if t is not None:
            t.fill_(FILL)
    e.loss_buf.fill_(FILL)
    e.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
    torch.cuda.synchronize()
    assert not e.kernel_error()
    a1x, z2x, gap = (t[:, off:off + n] for t in e.ops[6:9])
    labh = e.ops[1][off:off + n]
    refs = []
    for tdt in (torch.float64, torch.float32):
        x = e.X[off:off + n].to(tdt) * e.xscale
        refs.append(_step_math(x, e.labels[off:off + n].long(), *(t.to(tdt) for t in (e.W1, e.b1, e.W2, e.b2)), scale,
                               REG))
    ref, r32 = refs
    # the operands are what the construction says (a1 exactly 0, 1/2, 1; the logits exactly top - gap)
    assert np.array_equal(_np(ref["a1"]), a1x) and np.array_equal(_np(ref["z2"]), z2x)
    assert gap[labh, np.arange(n)].max() == 200.0
    if e.store_a1:
        assert np.array_equal(_np(e.a1[:, :n]), a1x), "a1"
    yh = _np(ref["yh"])
    onehot = np.zeros_like(yh)
    onehot[labh, np.arange(n)] = 1.0
    worst = {}
    worst["D"] = sc.worst_ratio(_np(e.D[:C, :n]) / scale, yh - onehot, sc.grad_bound(gap, yh, onehot, eps, floor))
    assert worst["D"] <= 1.0, ("D", tag, worst["D"])
    nblk = (n + 15) // 16
    lossr = _np(ref["loss_cols"])
    lg = _np(e.loss_buf[:nblk])
    assert np.isfinite(lg).all(), ("loss", tag, lg.tolist())
    worst["loss"] = sc.worst_ratio(lg, sc.block_sums(lossr), sc.loss_bound(lossr))
    assert worst["loss"] <= 1.0, ("loss", tag, worst["loss"])
    if e.loss_buf.numel() > nblk:
        assert float(e.loss_buf[nblk]) == FILL
    # dZ1: the fp32 array (row-major or in the dW1 launch's fragment order), else the planes the step left instead
    dz = e.dz1()[:, :n]
    if bool((dz == FILL).all()) and e.dZ1p is not None:
        dz = e.dZ1p.float().sum(0)[:, :n]
    dz = _np(dz)
    assert np.isfinite(dz).all() and not (dz == FILL).all() and (dz[(a1x == 0) | (a1x == 1)] == 0).all(), ("dZ1", tag)
    bf = dt == "bf16"
    if bf:
        te = MlpEngine((e.P, H, C), dtype=dt, max_cols=n, device="cuda", backend="torch", path=path)
        te.set_params(*(t.cpu().numpy() for t in (e.W1, e.b1, e.W2, e.b2)))
        te.load_dataset(e.ops[0], e.ops[1])
        te.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
        assert np.isfinite(te.loss_sum())
    for name in ("dZ1", "gW1", "gb1", "gW2", "gb2"):
        got = dz if name == "dZ1" else _np(getattr(e, name))
        assert np.isfinite(got).all(), (name, tag)
        if bf:
            want = _np(te.dZ1[:, :n] if name == "dZ1" else getattr(te, name))
            e32, bound = None, 3e-2
        else:
            want = _np(ref[name])
            e32 = None if dt == "f64" else _rel(_np(r32[name]), want)
            bound = 1e-11 if dt == "f64" else max(1e-5, 4 * e32)
        err = _rel(got, want)
        worst[name + "_err"], worst[name + "_fp32_torch_err"] = err, e32
        assert err <= bound, (name, tag, err, bound)
    _log(test="step", tag=tag, dt=dt, path=path, H=H, C=C, n=n, **worst)
    return float(lg.sum()), lossr


@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("head_dw2", [1, 0])
def test_allgather_step_at_saturated_logits(head_dw2, C):
    """fwd1_head_ag_kernel (fha_body), with and without the head's dW2 partials."""
    H, n = 100, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    st = _forced(e, head_dw2=head_dw2)
    plan = st.plan(64, n, 0, 3)
    assert plan["form"] == "allgather" and plan["dw2_cols"] == (16 if head_dw2 else 0)
    _check_step(e, "f32", "split3", n, f"allgather/dw2_{head_dw2}")


@pytest.mark.parametrize("C", [2, 16])
def test_last_arriver_step_at_saturated_logits(C):
    """fwd1_head_kernel: head32<true>."""
    H, n = 100, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    e.set_fh_allgather(False)
    assert e._hip_step().plan(64, n, 0, 3)["form"] == "last_arriver"
    _check_step(e, "f32", "split3", n, "last_arriver")


@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("H,cols", [(300, 0), (512, 32)])
def test_separate_step_at_saturated_logits(H, cols, C):
    """H = 300: fwd1_split_kernel + head_kernel<float, 16, true>; H = 512 without the all-gather: fwd1_glds_kernel +
    head_wide_kernel on z2 partials."""
    n = 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    e.set_fh_allgather(False)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "separate" and plan["dw2_cols"] == cols
    _check_step(e, "f32", "split3", n, f"separate/H{H}")


@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("dt,path", [("f32", "split3"), ("bf16", "split1")])
def test_wide64_step_at_saturated_logits(dt, path, C):
    """The all-gather head fused into the 64 x 64 forward (mlp_split.hip wide_head_ag)."""
    H, n = 512, 64
    e = _engine(dt, path, H, C, n, 64 + n + 16)
    e.set_store_a1(False)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "wide64" and plan["dw2_cols"] == 64
    _check_step(e, dt, path, n, "wide64")


def test_wide128_step_at_saturated_logits():
    """The all-gather head fused into the 128 x 128 A-in-registers forward."""
    H, n, C = 3072, 1024, 16
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    plan = e._hip_step().plan(64, n, 0, 3)
    assert plan["form"] == "wide128" and plan["dw2_cols"] == 128
    _check_step(e, "f32", "split3", n, "wide128")


@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("dt", ["f32", "f64", "bf16"])
def test_plain_step_at_saturated_logits(dt, C):
    """The mfma paths: fwd1_kernel, head32_kernel (f32 / bf16) or head_kernel<double, .>, wgrad_kernel."""
    H, n = 100, 37
    e = _engine(dt, "mfma", H, C, n, 64 + n + 16)
    assert e.path == "mfma" and e._hip_step().split == 0
    _check_step(e, dt, "mfma", n, "plain")


def test_four_launch_step_at_saturated_logits():
    """C = 47 on the split path: forward GEMM, mlp_head_mc, dW1 launch, mlp_out_wgrad_mc."""
    H, C, n = 100, 47, 37
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    assert e.path == "split3" and e.C > 16
    _check_step(e, "f32", "split3", n, "four_launch")


def test_step_loss_equals_evaluation_loss():
    """The same weights, the same samples, label gaps up to 200: the step's loss partials and evaluate()'s loss_sum are
    both finite and agree within the sum of their bounds."""
    H, C, n = 100, 16, 96
    e = _engine("f32", "split3", H, C, n, 64 + n + 16)
    got, lossr = _check_step(e, "f32", "split3", n, "step_vs_eval")
    e.load_eval(e.ops[0][64:64 + n], e.ops[1][64:64 + n])
    ev = e.evaluate()
    bound = float(sc.loss_bound(lossr).sum())
    assert ev["n"] == n and np.isfinite(ev["loss_sum"])
    assert abs(ev["loss_sum"] - lossr.sum()) <= bound and abs(got - ev["loss_sum"]) <= 2 * bound
    _log(test="step_vs_eval", step=got, evaluate=ev["loss_sum"], fp64=float(lossr.sum()), bound=bound)


def test_train_loss_events_equal_the_evaluation_loss():
    """DataParallelTrainer.train(print_every=1, eval_every=1) at lr = 0, reg = 0 on these weights (label gaps up to
    200), the validation set being the training batch: the step's loss event and the evaluation's loss are the same
    finite mean within the sum of their bounds (the loss event was +inf before head_nll)."""
    H, C, n = 100, 16, 96
    x, lab, W1, b1, W2, b2, _, z2, gap = sc.step_operands(784, H, C, n)
    nn = NeuralNetwork([784, H, C])
    for dst, src in zip(nn.params, (W1, b1, W2, b2)):
        dst[...] = src
    tr = DataParallelTrainer(nn, dtype="f32", batch_size=n)
    tr.load(x, lab)
    tr.load_eval(x, lab)
    events = []
    st = tr.train(1, 0.0, 0.0, print_every=1, eval_every=1, on_event=events.append, log=lambda *a: None)
    losses = [ev["loss"] for ev in events if ev["event"] == "loss"]
    _, lossr, _ = sc.softmax_reference(z2, lab)
    want, bound = float(lossr.mean()), float(sc.loss_bound(lossr).sum()) / n
    assert gap[lab, np.arange(n)].max() == 200.0 and len(losses) == 1 and len(st.evals) == 1
    assert np.isfinite(losses[0]) and abs(losses[0] - want) <= bound, (losses, want, bound)
    assert st.evals[0]["n"] == n and abs(st.evals[0]["loss"] - want) <= bound, (st.evals[0]["loss"], want, bound)
    _log(test="train_vs_eval", loss_event=losses[0], evaluation=st.evals[0]["loss"], fp64=want, bound=bound)


# ------------------------------------------------------------------------------------------------ the pipeline
def _sgd_steps(x, lab, params, offs, n, scale, reg, lr, tdt):
    W1, b1, W2, b2 = (t.to(tdt).clone() for t in params)
    for off in offs:
        g = _step_math(x[off:off + n].to(tdt), lab[off:off + n].long(), W1, b1, W2, b2, scale, reg)
        W1, b1, W2, b2 = W1 - lr * g["gW1"], b1 - lr * g["gb1"], W2 - lr * g["gW2"], b2 - lr * g["gb2"]
    return W1, b1, W2, b2


def _flat(ts):
    return torch.cat([t.double().reshape(-1) for t in ts])


def test_xstep_pipeline_at_saturated_logits():
    """2 (N // n) fused SGD steps as ONE pipeline launch (xstep.hip), lr = 2^-10: parameters bitwise those of the
    two-launch step, all finite, and the update against the same steps in fp64 within 4x the error of the same steps in
    plain fp32 torch (tests/test_gpu_few_classes.py _check_update)."""
    H, n, C, lr = 100, 256, 16, 2.0 ** -10
    N = 5 * n + 48
    engines = []
    for xs in (0, -1):
        e = _engine("f32", "split3", H, C, n, N)
        e.set_store_a1(False)
        _forced(e, xstep=xs, head_dw2=1)
        engines.append(e)
    before = [t.clone() for t in (engines[0].W1, engines[0].b1, engines[0].W2, engines[0].b2)]
    count = 2 * (N // n)
    for e in engines:
        e._hip_step().run_steps(0, count, n, 0, n, N, 1.0 / n, REG, lr, 1, _stream())
    torch.cuda.synchronize()
    assert engines[1]._hip_step().xstep_used == 1, engines[1]._hip_step().xstep_reason
    assert engines[0]._hip_step().xstep_used == 0
    assert torch.equal(engines[0].params, engines[1].params)
    assert bool(torch.isfinite(engines[1].params).all())
    for e in engines:
        assert not e.kernel_error()
    offs = [n * (i % (N // n)) for i in range(count)]
    e = engines[0]
    runs = [_sgd_steps(e.X.to(t) * e.xscale, e.labels, before, offs, n, 1.0 / n, REG, lr, t)
            for t in (torch.float64, torch.float32)]
    d64 = _np(_flat(runs[0]) - _flat(before))
    e32 = _rel(_np(_flat(runs[1]) - _flat(before)), d64)
    err = _rel(_np(_flat([e.W1, e.b1, e.W2, e.b2]) - _flat(before)), d64)
    _log(test="xstep_update", H=H, C=C, n=n, steps=count, err=err, fp32_torch_err=e32, bound=4 * e32)
    assert err < 4 * e32, (err, e32)


# ------------------------------------------------------------------------------------------------ the sigmoid alone
def _check_sigmoid(got, b1, dt, tag):
    """a1 [H][n] of W1 = 0, b1 = the ladder: against the fp64 sigmoid of the b1 the kernel holds."""
    eps, floor = _eps(dt)
    x = _np(b1)
    ref = sc.sigmoid_reference(x)[:, None]
    got = _np(got)
    assert not np.isnan(got).any(), tag
    r = sc.worst_ratio(got, ref, (np.abs(x)[:, None] + 8.0) * eps * ref + floor)
    _log(test="sigmoid", tag=tag, dt=dt, H=int(got.shape[0]), n=int(got.shape[1]), a1=r)
    assert r <= 1.0, (tag, r)
    assert (got[x >= 128] == 1.0).all() and (got[x <= -8192] == 0.0).all(), tag


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16"])
def test_forward1_sigmoid_at_saturated_preactivations(dt):
    """mlp_forward1 (fwd1_kernel's EpiBiasAct), n = 37: the column tail untouched."""
    code, tdt = DT[dt]
    P, H, n, ld = 784, 100, 37, 48
    pdt = torch.float64 if dt == "f64" else torch.float32
    X = torch.randint(0, 256, (n, P), generator=torch.Generator().manual_seed(1)).to(tdt).cuda()
    W = torch.zeros(H, P, dtype=tdt, device="cuda")
    b = torch.as_tensor(sc.sigmoid_ladder(H)).to(pdt).cuda()
    a1 = torch.full((H, ld), FILL, dtype=pdt, device="cuda")
    hip().mlp_forward1(code, W.data_ptr(), b.data_ptr(), X.data_ptr(), P, H, n, a1.data_ptr(), ld, 1, _stream())
    torch.cuda.synchronize()
    _check_sigmoid(a1[:, :n], b, dt, "forward1")
    assert bool((a1[:, n:] == FILL).all())


@pytest.mark.parametrize("H,n,form,allgather", [(100, 96, "allgather", True), (100, 96, "last_arriver", False),
                                                (300, 96, "separate", False), (512, 96, "separate", False),
                                                (3072, 1024, "wide128", True)])
def test_engine_forward_sigmoid_at_saturated_preactivations(H, n, form, allgather):
    """The split (H <= 128 fused forms, fwd1_split_kernel), direct-to-LDS (fwd1_glds_kernel) and A-in-registers
    (wide128) forward epilogues through a step that stores a1: W1 = 0, b1 = the ladder."""
    C = 10
    g = np.random.default_rng(H)
    e = MlpEngine((784, H, C), dtype="f32", max_cols=n, device="cuda", path="split3")
    e.set_params(np.zeros((H, 784)), sc.sigmoid_ladder(H), g.normal(0, 0.3, (C, H)), g.normal(0, 0.1, C))
    e.load_dataset(g.integers(0, 256, (64 + n, 784)).astype(np.uint8), g.integers(0, C, 64 + n))
    e.set_fh_allgather(allgather)
    assert e._hip_step().plan(64, n, 0, 3)["form"] == form and e.store_a1
    e.run(64, n, 1.0 / n, REG, 0.0, sgd=False, with_loss=True)
    torch.cuda.synchronize()
    assert not e.kernel_error()
    _check_sigmoid(e.a1[:, :n], e.b1, "f32", f"engine/{form}/H{H}")
    assert bool(torch.isfinite(e.grads).all()) and np.isfinite(e.loss_sum())
