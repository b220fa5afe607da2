"""Input widths other than 784: whole steps against plain torch fp64 written here (bf16 against the torch-backend bf16
engine, the convention of tests/test_gpu_mlp.py), each case asserting first which form its plan takes.  The expected
plan fields are derived below from the predicates' documented conditions (csrc/mlp/mlp_kernels.hip fha_vec /
mlp_fwd_swz_ok, csrc/mlp/mlp_split.hip glds_fwd_ok / rega_fwd_ok / wide_ag_bm, csrc/mlp/mlp_step.hip plan), not from a run.

What each group reaches (csrc/mlp):

* test_small_layer_widths -- ``fwd1_head_ag_kernel<., VEC, .>`` with fha_vec 0 (P = 30, 780, 777: element pixel loads),
  1 (P = 776: 4-byte pixel loads) and 3 (P = 1024: 16-byte pairs, and the fragment-ordered W1 / pixel copies SWZ 1 / 3
  with four pairs per wave); P = 30 leaves seven of the eight K-split waves without work; ``wgrad_split_kernel`` at
  XT pitches and P + 1 bias columns that are not vector multiples; steps from sample 0 and 7 (aligned / unaligned
  pixel base).
* test_plain_kernel_widths -- ``mlp_forward1``'s ``P % V`` vector predicate (fwd1_kernel<., ., false>) and
  ``wgrad_kernel``'s tile tails at P = 30 and 777, f32 and f64.
* test_fused_sgd_widths -- three fused SGD steps at P = 776 and 1024 (the update's maintenance of the fragment-ordered
  W1 copy at P = 1024, bitwise against an engine that reads neither copy).
* test_wide_layer_widths -- H = 512: ``fwd1_glds_kernel`` / ``wgrad_glds_kernel`` with 25 stages and an 8-wide K tail
  (P = 776, also under the fused 64 x 64 head), ``fwd1_split_kernel`` + ``launch_head<float, 10 | 16>`` where
  glds_fwd_ok fails (P = 780, 777), ``wgrad_glds_kernel`` at P % 4 == 0 (780) and ``wgrad_split_kernel`` at P = 777.
* test_rega_layer_widths -- H = 4096, n = 768 (32 x 6 = 192 tiles, the smallest shape of rega_fwd_ok): the A-in-registers
  forward with the fused 128 x 128 head and dW1 on the runtime K loop, NKS = 0 (P = 752: 24 stages, P = 1000: 32
  stages with P % 16 != 0; n = 768 is 24 stages of the dW1 K loop) and on the unrolled 25-stage loop with a tail other
  than 784's (P = 776); fp32 (rega) and bf16 (g64) engines.

Pixels are uniform random bytes, normalised (xscale = 1/255 folded into the kernels' epilogues) as in
tests/test_gpu_mlp.py test_fragment_ordered_copies_are_bitwise_the_row_major_forward: raw random bytes under 0.01-randn
weights saturate every sigmoid at these widths and would leave gradients of rounding noise.

Tolerances: f64 1e-11; f32 against fp64 1e-5 per gradient or, where the shape's own fp32 rounding is larger, 4x the
error of a plain fp32 torch evaluation of the same step (both logged); 1e-4 on the loss; bf16 3e-2 against the
torch-backend bf16 engine; the update after three fused SGD steps within 4x the error of the same steps in plain fp32
torch.  Measured worst errors: profiles/numerics_classes_widths.jsonl."""
import json

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd.parallel import MlpEngine

pytestmark = pytest.mark.gpu

# tests/test_gpu_mlp.py TOL
TOL = {("f64", "mfma"): 1e-11, ("f32", "split3"): 2e-5, ("f32", "mfma"): 2e-5, ("bf16", "split1"): 3e-2,
       ("bf16", "mfma"): 3e-2}
LR, REG = 0.01, 1e-4
SPLIT = [("f32", "split3"), ("bf16", "split1")]
OFFS = (0, 7)  # the pixel base X + off * P: aligned, and as unaligned as P allows


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _log(**kw):
    print("NUMERICS " + json.dumps(kw))


def _cdiv(a, b):
    return (a + b - 1) // b


def _engine(dt, path, P, H, C, n, N, backend="hip"):
    g = torch.Generator().manual_seed(P + H + C)
    x = torch.randint(0, 256, (N, P), generator=g, dtype=torch.uint8).numpy()
    y = torch.randint(0, C, (N,), generator=g).numpy()
    W1, _, W2, _ = NeuralNetwork([P, H, C]).params
    rng = np.random.default_rng(P + H + C)  # (the initial biases are zero: a dropped bias would not show)
    e = MlpEngine((P, H, C), dtype=dt, max_cols=n, device="cuda", backend=backend, path=path)
    e.set_params(W1, rng.normal(0, 0.1, H), W2, rng.normal(0, 0.1, C))
    e.raw = (x, y)
    e.load_dataset(x, y, normalize=True)
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


def _check_step(e, dt, path, n, tag, off, te=None):
    """One gradient step of `e` against fp64 (f32, f64) or against the torch-backend bf16 engine `te` (bf16)."""
    scale = 1.0 / n
    e.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
    torch.cuda.synchronize()
    assert not e.kernel_error()
    if dt == "bf16":
        te.run(off, n, scale, REG, 0.0, sgd=False, with_loss=True)
        ref = {k: getattr(te, k) for k in ("gW1", "gb1", "gW2", "gb2")}
        ref["D"], ref["loss"] = te.D[:, :n], torch.tensor(te.loss_sum())
        r32 = None
    else:
        ref, r32 = _step_refs(e, off, n, scale, REG)
    for name in ("gW1", "gb1", "gW2", "gb2", "D", "loss"):
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


def _bf16_reference(e, dt, path, n):
    if dt != "bf16":
        return None
    te = MlpEngine((e.P, e.H, e.C), dtype=dt, max_cols=n, device="cuda", backend="torch", path=path)
    te.set_params(*(t.cpu().numpy() for t in (e.W1, e.b1, e.W2, e.b2)))
    te.load_dataset(*e.raw, normalize=True)
    return te


def _plan_fields(e, off, n):
    p = e._hip_step().plan(off, n, 0, 3)
    return {k: p[k] for k in ("form", "w1_swz", "x_swz", "wide_eng")}


# ------------------------------------------------------------------------------------------------ small layers
# (w1_swz, x_swz) of the split3 forward per (P, first sample), H <= 128.  The pixel base is X + off * P with X on an
# allocator (>= 256-byte) boundary and W1 at the start of the 256-byte aligned parameter arena.  fha_vec: 0 unless
# the base is 4-byte aligned and P % 8 == 0; 3 when also the base is 16-byte aligned and P % 16 == 0; else 1.
# mlp_fwd_swz_ok (w1_swz): fp32 W1 split in registers (split3 below H = 512), fha_vec == 3 and an even number of
# 32-k chunks per wave, cdiv(cdiv(P, 32), 8) % 2 == 0.  x_swz: w1_swz and the step starts a 16-sample tile.
SWZ = {
    (30, 0): (0, 0),    # 30 % 8 != 0: fha_vec 0 (one 32-k chunk: waves 1-7 of the K split have no work)
    (30, 7): (0, 0),
    (776, 0): (0, 0),   # 776 % 8 == 0 but 776 % 16 == 8: fha_vec 1, never 3
    (776, 7): (0, 0),   # base 7 * 776 = 5432 = 4 * 1358: still fha_vec 1
    (780, 0): (0, 0),   # 780 % 8 == 4: fha_vec 0
    (780, 7): (0, 0),
    (777, 0): (0, 0),   # odd: fha_vec 0
    (777, 7): (0, 0),
    (1024, 0): (1, 1),  # 1024 % 16 == 0, 32 chunks / 8 waves = 4 per wave (even): both copies from sample 0
    (1024, 7): (1, 0),  # base 7 * 1024 is 16-byte aligned: fha_vec 3, the W1 copy; sample 7 starts no 16-sample tile
}


def _small_expect(path, P, off):
    # split1 multiplies bf16 planes (mlp_split_fwd_fp32_w false): neither copy.  Both forms fit the device at these
    # sizes (at most 8 x 3 workgroups), so plan takes the all-gather forward + head.  wide_eng is the 128 x 128 wide
    # K loop's engine policy, carried by every plan: rega (0) for fp32 A, g64 (1) for bf16 A.
    w1, xs = SWZ[(P, off)] if path == "split3" else (0, 0)
    return {"form": "allgather", "w1_swz": w1, "x_swz": xs, "wide_eng": 0 if path == "split3" else 1}


@pytest.mark.parametrize("dt,path", SPLIT)
@pytest.mark.parametrize("H,n", [(100, 96), (37, 37)])
@pytest.mark.parametrize("P", [30, 776, 780, 777, 1024])
def test_small_layer_widths(P, H, n, dt, path):
    e = _engine(dt, path, P, H, 10, n, 112)
    te = _bf16_reference(e, dt, path, n)
    for off in OFFS:
        assert _plan_fields(e, off, n) == _small_expect(path, P, off), (P, off)
        _check_step(e, dt, path, n, "small", off, te)


def test_small_layer_width_and_class_tails_together():
    """P = 777 (nothing vectorised) with 16 classes (no class padding), 37 x 37."""
    e = _engine("f32", "split3", 777, 37, 16, 37, 112)
    for off in OFFS:
        assert _plan_fields(e, off, 37) == _small_expect("split3", 777, off)
        _check_step(e, "f32", "split3", 37, "small/C16", off)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("H,n", [(100, 96), (37, 37)])
@pytest.mark.parametrize("P", [30, 777])
def test_plain_kernel_widths(P, H, n, dt):
    """The mfma paths have no plan: MlpStep.run_plain always runs mlp_forward1, mlp_head, mlp_wgrad."""
    e = _engine(dt, "mfma", P, H, 10, n, 112)
    assert e.path == "mfma" and e._hip_step().split == 0
    for off in OFFS:
        _check_step(e, dt, "mfma", n, "plain", off)


def _sgd_steps(x, lab, params, offs, n, scale, reg, lr, tdt):
    """Plain torch SGD over the batches starting at `offs`, in dtype `tdt`: the final (W1, b1, W2, b2)."""
    W1, b1, W2, b2 = (t.to(tdt).clone() for t in params)
    for off in offs:
        g = _step_math(x[off:off + n].to(tdt), lab[off:off + n].long(), W1, b1, W2, b2, scale, reg)
        W1, b1, W2, b2 = W1 - lr * g["gW1"], b1 - lr * g["gb1"], W2 - lr * g["gW2"], b2 - lr * g["gb2"]
    return W1, b1, W2, b2


def _flat(ts):
    return torch.cat([t.double().reshape(-1) for t in ts])


@pytest.mark.parametrize("P", [776, 1024])
def test_fused_sgd_widths(P):
    """Three fused SGD steps (from samples 0, 7 and 16: at P = 1024 the pixel copy, the row-major pixels, the copy):
    params_after - params_before against the same steps in fp64, within 4x the error of the same steps in plain fp32
    torch; where the forward reads the fragment-ordered W1 copy, bitwise an engine that reads neither copy."""
    H, n, offs = 100, 96, (0, 7, 16)
    e = _engine("f32", "split3", P, H, 10, n, 112)
    swz = [_plan_fields(e, off, n)["w1_swz"] for off in offs]
    assert swz == [_small_expect("split3", P, 0)["w1_swz"]] * 3  # (P = 1024: sample 16's base is aligned like sample 0's)
    before = [t.clone() for t in (e.W1, e.b1, e.W2, e.b2)]
    engines = [e]
    if swz[0]:
        e2 = _engine("f32", "split3", P, H, 10, n, 112)
        e2._hip_step().w1_swz = e2._hip_step().x_swz = 0
        assert _plan_fields(e2, 0, n)["w1_swz"] == 0 and _plan_fields(e2, 0, n)["x_swz"] == 0
        engines.append(e2)
    for eng in engines:
        for off in offs:
            eng.run(off, n, 1.0 / n, REG, LR, sgd=True)
    torch.cuda.synchronize()
    for eng in engines:
        assert not eng.kernel_error()
    if swz[0]:
        assert torch.equal(engines[0].params, engines[1].params)
    after = [t.clone() for t in (e.W1, e.b1, e.W2, e.b2)]
    runs = [_sgd_steps(e.X.to(t) * e.xscale, e.labels, before, offs, n, 1.0 / n, REG, LR, t)
            for t in (torch.float64, torch.float32)]
    d64 = _flat(runs[0]) - _flat(before)
    e32 = _rel(_flat(runs[1]) - _flat(before), d64)
    err = _rel(_flat(after) - _flat(before), d64)
    _log(test="update", tag="fused_sgd", P=P, H=H, C=10, n=n, steps=3, err=err, fp32_torch_err=e32, bound=4 * e32)
    assert err < 4 * e32, (err, e32)


# ------------------------------------------------------------------------------------------------ wide layers
def _wide_expect(path, P, store_a1):
    # H = 512, n = 96.  glds_fwd_ok: the bf16 pixel rows are whole 16-byte chunks, P % 8 == 0 (then the base
    # Xw + off * P * 2 is 16-byte aligned for every off) -- true at 776, false at 780 and 777.  rega_fwd_ok needs
    # cdiv(H, 128) * cdiv(n, 128) = 4 >= 192: never.  The fused 64 x 64 head is taken (wide_ag_bm) only when a1 is not
    # stored and glds_fwd_ok holds; everything else is the separate forward, head and weight-gradient launches.
    # No fragment-ordered copies above H = 128.
    fused = P % 8 == 0 and not store_a1
    return {"form": "wide64" if fused else "separate", "w1_swz": 0, "x_swz": 0, "wide_eng": 0 if path == "split3" else 1}


@pytest.mark.parametrize("dt,path", SPLIT)
@pytest.mark.parametrize("store_a1", [True, False])
@pytest.mark.parametrize("P", [776, 780, 777])
def test_wide_layer_widths(P, store_a1, dt, path):
    H, n = 512, 96
    e = _engine(dt, path, P, H, 10, n, 112)
    e.set_store_a1(store_a1)
    te = _bf16_reference(e, dt, path, n)
    for off in OFFS:
        assert _plan_fields(e, off, n) == _wide_expect(path, P, store_a1), (P, off)
        _check_step(e, dt, path, n, f"wide512/a1_{int(store_a1)}", off, te)


def test_wide_layer_width_and_class_tails_together():
    """P = 776 (the direct-to-LDS engines' 8-wide K tail) with 16 classes: head_wide_kernel without class padding."""
    e = _engine("f32", "split3", 776, 512, 16, 96, 112)
    for off in OFFS:
        assert _plan_fields(e, off, 96) == _wide_expect("split3", 776, True)
        _check_step(e, "f32", "split3", 96, "wide512/C16", off)


def _rega_expect(path):
    # H = 4096, n = 768, P % 8 == 0: glds_fwd_ok holds and cdiv(4096, 128) * cdiv(768, 128) = 32 * 6 = 192 >= 192, so
    # rega_fwd_ok holds (P % 4 == 0, W1 16-byte aligned); 192 workgroups fit the device's CUs at once, so the head is
    # fused on the 128 x 128 tiling whether or not a1 is stored.  wide_eng: rega (0) for fp32 A, g64 (1) for bf16 A.
    return {"form": "wide128", "w1_swz": 0, "x_swz": 0, "wide_eng": 0 if path == "split3" else 1}


@pytest.mark.parametrize("dt,path", SPLIT)
@pytest.mark.parametrize("P", [752, 1000, 776])
def test_rega_layer_widths(P, dt, path):
    H, n = 4096, 768
    e = _engine(dt, path, P, H, 10, n, 784)
    te = _bf16_reference(e, dt, path, n)
    for off in OFFS:
        assert _plan_fields(e, off, n) == _rega_expect(path), (P, off)
        _check_step(e, dt, path, n, "rega", off, te)


def test_rega_layer_width_and_class_tails_together():
    """P = 752 (the runtime K loop) with 16 classes: the fused 128 x 128 head without class padding."""
    e = _engine("f32", "split3", 752, 4096, 16, 768, 784)
    for off in OFFS:
        assert _plan_fields(e, off, 768) == _rega_expect("split3")
        _check_step(e, "f32", "split3", 768, "rega/C16", off)
