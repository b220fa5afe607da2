"""The stateful optimizers on the CPU: the update rules (csrc/mlp/optim.h through _cpu.optim_step) against torch.optim,
the torch-backend trainer against the fp64 oracle (models.mlp.train(optimizer=...)), loopback and gloo ranks against one
process, train(2) + train(2) == train(4), checkpoints, the Optimizer's validation, and that plain SGD keeps no state."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.optim import Optimizer, new_state
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, TensorParallelTrainer
from cme213_sp18_amd.parallel.launcher import spawn
from cme213_sp18_amd.utils.checkpoint import load_checkpoint, load_optim_state, save_checkpoint
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.eval_oracle import TOL
from tests.optim_workers import (check_adam_drift, check_adam_first_update, dp_optim_worker, first_update_state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4
# the comparisons with the fp64 oracle hold a whole training run to the bound TOL sets for ONE gradient step: they run
# at the CLI's default rate (config.TrainConfig.learning_rate), where 8 steps move the parameters by a fraction of their
# scale and a rounding difference is carried, not amplified (at 0.05 with momentum 0.9 on raw 0..255 pixels the fp64
# torch backend and the fp64 oracle, which differ only in summation order, already part by 2e-11)
ORACLE_LR = 1e-3
KINDS = {"momentum": Optimizer.momentum(0.9, False), "nesterov": Optimizer.momentum(0.8, True),
         "adam": Optimizer.adam(0.9, 0.999, 1e-8)}
TORCH = {"momentum": lambda p, lr: torch.optim.SGD([p], lr=lr, momentum=0.9, dampening=0),
         "nesterov": lambda p, lr: torch.optim.SGD([p], lr=lr, momentum=0.8, dampening=0, nesterov=True),
         "adam": lambda p, lr: torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_update_rules_are_torch_optims(kind):
    """Both sides are fp64 evaluations of the same formulas, 5 consecutive steps (Adam's bias correction at t = 1 .. 5).
    The two evaluations round differently (torch multiplies and adds where the header fuses), an absolute error of a
    few ulps of the operands, and rtol measures it against |p|: |p| starts in [0.5, 2] and lr = 5e-3 moves an element
    by at most 5 lr max|d| < 0.25 (|d| <= ~10: five N(0, 1) gradients summed with momentum), so no element comes near
    zero, where rtol would measure cancellation instead.  The state buffers are sums of signed O(1) terms that may
    cancel, hence their atol of a few ulps of 1."""
    rng = np.random.default_rng(0)
    n, lr, opt = 4096, 5e-3, KINDS[kind]
    p = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    tp = torch.tensor(p.copy(), requires_grad=True)
    to = TORCH[kind](tp, lr)
    st = [np.zeros(n) for _ in range(opt.num_state)]
    t = 0
    for k in range(5):
        g = rng.standard_normal(n)
        tp.grad = torch.tensor(g)
        to.step()
        t, b1p, b2p = cpu().optim_step(opt.code, opt.hyper(lr), p, g, st[0], st[1] if len(st) > 1 else None, t)
        assert t == k + 1
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
    if kind == "adam":
        assert b1p == pytest.approx(0.9 ** 5, rel=1e-15) and b2p == pytest.approx(0.999 ** 5, rel=1e-15)
        np.testing.assert_allclose(st[0], to.state[tp]["exp_avg"].numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(st[1], to.state[tp]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-14)
    else:
        np.testing.assert_allclose(st[0], to.state[tp]["momentum_buffer"].numpy(), rtol=1e-12, atol=1e-14)


def test_optim_step_carries_the_products_and_checks_its_arrays():
    opt = KINDS["adam"]
    rng = np.random.default_rng(1)
    a = [rng.standard_normal(100).astype(np.float32) for _ in range(2)]
    runs = []
    for carried in (False, True):
        p, g = a[0].copy(), a[1].copy()
        m, s = np.zeros(100, np.float32), np.zeros(100, np.float32)
        t, b1p, b2p = 0, None, None
        for _ in range(4):
            t, b1p, b2p = cpu().optim_step(opt.code, opt.hyper(0.01), p, g, m, s, t, *((b1p, b2p) if carried else ()))
        runs.append((p, m, s, b1p, b2p))
    for u, v in zip(*runs):  # the products recomputed from t equal the carried ones: bitwise the same updates
        assert np.array_equal(u, v)
    p = np.zeros(4, np.float32)
    with pytest.raises(ValueError):
        cpu().optim_step(opt.code, opt.hyper(0.01), p, np.zeros(4, np.float64), p.copy(), p.copy(), 0)
    with pytest.raises(ValueError):
        cpu().optim_step(opt.code, opt.hyper(0.01), p, p.copy(), p.copy(), None, 0)  # adam needs s2
    with pytest.raises(ValueError):
        cpu().optim_step(7, opt.hyper(0.01), p, p.copy(), p.copy(), p.copy(), 0)


def test_adam_with_zero_gradient_and_zero_state_moves_nothing():
    opt = KINDS["adam"]
    for dt, den in ((np.float32, np.float32(1e-42)), (np.float64, 5e-320)):
        p = np.array([1.5, -0.0, 0.0, 3.0], dt)
        g = np.array([0.0, 0.0, 0.0, den], dt)
        m, s = np.zeros(4, dt), np.zeros(4, dt)
        p0 = p.copy()
        t = 0
        for _ in range(3):
            t, _, _ = cpu().optim_step(opt.code, opt.hyper(0.1), p, g, m, s, t)
        assert np.array_equal(p[:3].view(np.uint8), p0[:3].view(np.uint8)) and not m[:3].any() and not s[:3].any()
        assert np.isfinite(p[3]) and m[3] > 0  # the denormal gradient is kept, not flushed


def _torch_trainer(dtype, opt, x, y, comm=None, H=100, B=64):
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), comm=comm, device="cpu", dtype=dtype, batch_size=B,
                             backend="torch", use_graphs=False, optimizer=opt)
    tr.load(x, y)
    return tr


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# TOL bounds a gradient's error relative to max|g|: an element far below max|g| may be wrong by many times its own size.
# Momentum and Nesterov are linear in g, so that bound carries over to the parameters.  Adam divides by sqrt(s): every
# element moves by about lr whatever its gradient's size, so the elements TOL says nothing about move as far as the
# others (measured at the rate below: fp32 torch backend W1 3.3e-2 against 2e-5; two fp64 ranks against one process
# 1.0e-11 / 1.5e-11 against 1e-11).  Wherever two Adam runs see different roundings of the gradient they are held to
# the two bounds derived in tests/optim_workers.py instead: TOL on the first update's m and s, and the elementwise
# drift bound 2 lr sum_t c_t on the parameters.  The fp64 torch backend against the fp64 oracle keeps TOL as well.
ORACLE_CASES = [(d, key, k) for d, key in (("f64", ("f64", "mfma")), ("f32", ("f32", "split3"))) for k in KINDS]


def oracle_first_update(H, x, y, B, lr, reg, opt):
    """[m, s] (or [v]) of the fp64 oracle after ONE update on the first batch."""
    ref = NeuralNetwork(list(H))
    st = new_state(opt, ref.num_params())
    mlp.train(ref, x[:B], y[:B], lr, reg, 1, B, optimizer=opt, optim_state=st)
    assert st["t"] == 1
    return st["state"]


@pytest.mark.parametrize("dtype,key,kind", ORACLE_CASES)
def test_torch_trainer_matches_the_fp64_oracle(dtype, key, kind):
    x, y = synthetic_mnist(256, seed=3)
    opt = KINDS[kind]
    tr = _torch_trainer(dtype, opt, x, y)
    first = first_update_state(tr, ORACLE_LR, REG)
    tr.train(2, ORACLE_LR, REG)
    ref = NeuralNetwork([784, 100, 10])
    st = new_state(opt, ref.num_params())
    mlp.train(ref, x, y, ORACLE_LR, REG, 2, 64, optimizer=opt, optim_state=st)
    assert st["t"] == 8 and tr.engine.optim_state()["t"] == 8
    if kind == "adam":
        check_adam_first_update(ref.H, first, oracle_first_update(ref.H, x, y, 64, ORACLE_LR, REG, opt), TOL[key],
                                f"torch {dtype}")
        check_adam_drift(opt, ORACLE_LR, 8, np.concatenate([p.ravel() for p in tr.engine.get_params()]),
                         np.concatenate([p.ravel() for p in ref.params]), f"torch {dtype}")
    for name, got, want in zip(("W1", "b1", "W2", "b2"), tr.engine.get_params(), ref.params):
        rel = _rel(got, want)
        print(f"NUMERICS {dtype} {kind} {name} rel {rel:.3e} (bound {TOL[key]})")
        if kind != "adam" or dtype == "f64":
            assert rel < TOL[key], (name, rel)
    if dtype == "f64":  # ... and the state itself
        for got, want in zip(tr.engine.optim_state()["state"], st["state"]):
            assert _rel(got, want) < TOL[key]


def test_oracle_continues_its_state_one_epoch_at_a_time():
    x, y = synthetic_mnist(256, seed=3)
    for kind in ("nesterov", "adam"):
        opt = KINDS[kind]
        a, b = NeuralNetwork([784, 24, 10]), NeuralNetwork([784, 24, 10])
        mlp.train(a, x, y, LR, REG, 3, 64, optimizer=opt)
        st = new_state(opt, b.num_params())
        for ep in range(3):
            mlp.train(b, x, y, LR, REG, 1, 64, iter0=4 * ep, optimizer=opt, optim_state=st)
        assert st["t"] == 12
        for u, v in zip(a.params, b.params):
            np.testing.assert_array_equal(u, v)
        c = NeuralNetwork([784, 24, 10])  # the shuffled oracle goes one epoch at a time by itself
        mlp.train(c, x, y, LR, REG, 3, 64, shuffle_seed=5, optimizer=opt)
        assert _rel(c.W[0], a.W[0]) > 1e-9
    plain, sgd = NeuralNetwork([784, 24, 10]), NeuralNetwork([784, 24, 10])
    mlp.train(plain, x, y, LR, REG, 2, 64)
    mlp.train(sgd, x, y, LR, REG, 2, 64, optimizer=Optimizer.sgd())
    np.testing.assert_array_equal(plain.W[0], sgd.W[0])


@pytest.mark.parametrize("kind", ["nesterov", "adam"])
def test_loopback_world2_matches_single(kind):
    H, N, B = 24, 512, 128
    x, y = synthetic_mnist(N, seed=11)
    comms = LoopbackComm.create(2)
    out = [None, None]

    def work(r):
        torch.set_num_threads(1)
        tr = _torch_trainer("f64", KINDS[kind], x, y, comm=comms[r], H=H, B=B)
        first = first_update_state(tr, ORACLE_LR, REG)
        tr.train(2, ORACLE_LR, REG)
        out[r] = (tr.engine.params.clone(), [b.clone() for b in tr.engine.opt_bufs], tr.engine.optim_state()["t"],
                  first)

    ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    one = _torch_trainer("f64", KINDS[kind], x, y, H=H, B=B)
    first = first_update_state(one, ORACLE_LR, REG)
    one.train(2, ORACLE_LR, REG)
    assert out[0][2] == out[1][2] == 8
    assert torch.equal(out[0][0], out[1][0]) and all(torch.equal(u, v) for u, v in zip(out[0][1], out[1][1]))
    rel = _rel(out[0][0].numpy(), one.engine.params.numpy())
    print(f"NUMERICS loopback {kind} rel {rel:.3e}")
    if kind == "adam":  # (ORACLE_CASES: the bounds derived for Adam across summation orders)
        check_adam_first_update([784, H, 10], out[0][3], first, TOL[("f64", "mfma")], "loopback")
        check_adam_drift(KINDS[kind], ORACLE_LR, 8, out[0][0].numpy(), one.engine.params.numpy(), "loopback")
    else:
        assert rel < TOL[("f64", "mfma")]


def test_gloo_world2_matches_single(tmp_path):
    H, N, B, E = 24, 512, 128, 2
    spawn(dp_optim_worker, 2, args=(str(tmp_path), H, N, B, E, "f64"), backend="gloo")
    x, y = synthetic_mnist(N, seed=11)
    r0, r1 = (np.load(tmp_path / f"optim{r}.npz") for r in range(2))
    for kind in ("nesterov", "adam"):
        one = _torch_trainer("f64", KINDS[kind], x, y, H=H, B=B)
        first = first_update_state(one, ORACLE_LR, REG)
        one.train(E, ORACLE_LR, REG)
        ref = np.concatenate([p.ravel() for p in one.engine.get_params()])
        for k in (f"{kind}_params", f"{kind}_state"):
            np.testing.assert_array_equal(r0[k], r1[k])  # replicas stay bit-identical, state included
        assert int(r0[f"{kind}_t"]) == 8
        rel = _rel(r0[f"{kind}_params"], ref)
        print(f"NUMERICS gloo {kind} rel {rel:.3e}")
        np.testing.assert_array_equal(r0[f"{kind}_first"], r1[f"{kind}_first"])
        if kind == "adam":  # (ORACLE_CASES: the bounds derived for Adam across summation orders)
            n = one.nn.num_params()
            check_adam_first_update([784, H, 10], [r0["adam_first"][:n], r0["adam_first"][n:]], first,
                                    TOL[("f64", "mfma")], "gloo")
            check_adam_drift(KINDS[kind], ORACLE_LR, 8, r0["adam_params"], ref, "gloo")
        else:
            assert rel < TOL[("f64", "mfma")]


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_train_2_plus_2_equals_train_4(kind):
    x, y = synthetic_mnist(200, seed=3)
    a = _torch_trainer("f32", KINDS[kind], x, y, H=24)
    b = _torch_trainer("f32", KINDS[kind], x, y, H=24)
    a.train(2, LR, REG)
    a.train(2, LR, REG)
    b.train(4, LR, REG)
    assert torch.equal(a.engine.params, b.engine.params)
    assert all(torch.equal(u, v) for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs))
    assert a.engine.optim_state()["t"] == b.engine.optim_state()["t"] == 16
    # _snapshot / _restore carry the state and the counter (what a recovered epoch relies on)
    snap = a._snapshot()
    a.train(1, LR, REG)
    a._restore(snap)
    assert a.engine.optim_state()["t"] == 16 and torch.equal(a.engine.params, b.engine.params)
    assert all(torch.equal(u, v) for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs))


def test_status_element_skips_the_update_on_the_torch_backend():
    x, y = synthetic_mnist(128, seed=3)
    tr = _torch_trainer("f64", KINDS["adam"], x, y, H=24)
    e = tr.engine
    e.run(0, 64, 1 / 64, REG, LR, sgd=False)
    e.grads[e.status_index] = 1.0
    before = (e.params.clone(), [b.clone() for b in e.opt_bufs], e.opt_rec.clone())
    e.apply(LR)
    assert torch.equal(e.params, before[0]) and torch.equal(e.opt_rec, before[2])
    assert all(torch.equal(u, v) for u, v in zip(e.opt_bufs, before[1]))
    e.grads[e.status_index] = 0.0
    e.apply(LR)
    assert e.optim_state()["t"] == 1 and not torch.equal(e.params, before[0])


def test_checkpoint_and_resume_continue_the_state(tmp_path):
    x, y = synthetic_mnist(200, seed=3)
    opt = KINDS["adam"]
    whole = _torch_trainer("f64", opt, x, y, H=24)
    whole.train(4, LR, REG)
    half = _torch_trainer("f64", opt, x, y, H=24)
    half.train(2, LR, REG)
    save_checkpoint(half.nn, str(tmp_path / "ck"), meta={"iter": half.iter, "optimizer": opt.as_meta()},
                    optim_state=half.engine.optim_state())
    nn, meta = load_checkpoint(str(tmp_path / "ck"))
    assert meta["optim_kind"] == "adam" and meta["optim_t"] == 8 and Optimizer.from_meta(meta["optimizer"]) == opt
    st = load_optim_state(str(tmp_path / "ck"), meta)
    assert st["t"] == 8 and len(st["state"]) == 2 and st["state"][0].dtype == np.float64
    rest = DataParallelTrainer(nn, device="cpu", dtype="f64", batch_size=64, backend="torch", use_graphs=False,
                               optimizer=opt)
    rest.engine.set_optim_state(st)
    rest.iter = meta["iter"]
    rest.load(x, y)
    rest.train(2, LR, REG)
    assert torch.equal(rest.engine.params, whole.engine.params)
    assert rest.engine.optim_state()["t"] == 16
    # a plain-SGD checkpoint into the same directory leaves no stale state behind
    save_checkpoint(half.nn, str(tmp_path / "ck"), meta={"iter": 0})
    assert not (tmp_path / "ck" / "optim.npz").exists()
    assert load_optim_state(str(tmp_path / "ck"), load_checkpoint(str(tmp_path / "ck"))[1]) is None


def _cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "1600", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_optimizer_checkpoint_and_resume(tmp_path):
    """--optimizer on the sequential and the parallel run alike (the preset runs both: -s), resumed == unbroken."""
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--optimizer", "momentum", "--momentum", "0.8", "--nesterov")
    r = _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "-g", "0", "-d")
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert meta["optimizer"]["kind"] == "momentum" and meta["optimizer"]["nesterov"] is True
    assert meta["optim_t"] == meta["iter"] == 16
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["correct"] is True  # the fp64 parallel run against the sequential oracle with the same optimizer
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])
    a, b = np.load(tmp_path / "whole" / "optim.npz"), np.load(tmp_path / "rest" / "optim.npz")
    np.testing.assert_array_equal(a["s0"], b["s0"])
    assert json.loads((tmp_path / "rest" / "meta.json").read_text())["optim_t"] == 16
    other = _cli(tmp_path, "--optimizer", "adam", "-e", "1", "--resume", half, "--ckpt-dir", str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with optimizer" in other.stdout
    assert json.loads((tmp_path / "other" / "meta.json").read_text())["optim_t"] == 4


def test_optimizer_validation():
    assert Optimizer.sgd().stateful is False and Optimizer().kind == "sgd"
    m = Optimizer.momentum(0.5, True)
    assert (m.kind, m.momentum, m.nesterov) == ("momentum", 0.5, True) and m == Optimizer("momentum", 0.5, True)
    a = Optimizer.adam(0.8, 0.99, 1e-6)
    assert (a.kind, a.beta1, a.beta2, a.eps) == ("adam", 0.8, 0.99, 1e-6)
    assert Optimizer.momentum(0.0).momentum == 0.0 and Optimizer.adam(beta1=0.0, beta2=0.0).beta2 == 0.0
    for bad in (dict(kind="rmsprop"), dict(kind="momentum", momentum=1.0), dict(kind="momentum", momentum=-0.1),
                dict(kind="adam", beta1=1.0), dict(kind="adam", beta2=-1e-3), dict(kind="adam", eps=0.0),
                dict(kind="adam", eps=-1.0)):
        with pytest.raises(ValueError):
            Optimizer(**bad)
    with pytest.raises(Exception):
        m.momentum = 0.1  # frozen
    assert hash(m) == hash(Optimizer.momentum(0.5, True))
    # the field and the constructor helper share the name `momentum`: the dataclass machinery still sees the field
    import copy
    import dataclasses
    import pickle
    assert dataclasses.replace(m, momentum=0.25) == Optimizer.momentum(0.25, True)
    assert dataclasses.replace(m, nesterov=False).momentum == 0.5
    assert pickle.loads(pickle.dumps(m)) == m and copy.deepcopy(m) == m and pickle.loads(pickle.dumps(m)).momentum == 0.5
    assert dataclasses.asdict(m)["momentum"] == 0.5 and Optimizer.from_meta(m.as_meta()) == m
    with pytest.raises(TypeError):
        DataParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", optimizer="adam")


def test_plain_sgd_keeps_no_state_and_tensor_parallel_refuses():
    x, y = synthetic_mnist(128, seed=3)
    runs = []
    for opt in (None, Optimizer.sgd()):
        tr = _torch_trainer("f64", opt, x, y, H=24)
        e = tr.engine
        assert tr.optimizer is None and e.optimizer is None and e.opt_bufs == [] and e.opt_rec is None
        assert e.optim_state() is None
        assert len(tr._snapshot()) == 3
        tr.train(1, LR, REG)
        runs.append(e.params.clone())
    assert torch.equal(runs[0], runs[1])
    st = _torch_trainer("f64", KINDS["adam"], x, y, H=24).engine
    assert len(st.opt_bufs) == 2 and all(b.shape == st.params.shape and b.dtype == st.params.dtype for b in st.opt_bufs)
    assert len(_torch_trainer("f32", KINDS["momentum"], x, y, H=24).engine.opt_bufs) == 1
    with pytest.raises(ValueError, match="one value per parameter"):  # checked before anything is copied
        before = [b.clone() for b in st.opt_bufs]
        bad = st.optim_state()
        bad["state"] = [s_[:-1] for s_ in bad["state"]]
        st.set_optim_state(bad)
    assert all(torch.equal(u, v) for u, v in zip(before, st.opt_bufs))
    from cme213_sp18_amd.config import parse_config
    with pytest.raises(SystemExit):  # refused when the flags are parsed, before data or the sequential run
        parse_config(["--parallel", "tp", "--optimizer", "adam"])
    with pytest.raises(SystemExit):
        parse_config(["--optimizer", "momentum", "--momentum", "1.5"])
    assert parse_config(["--parallel", "tp"]).optim.stateful is False
    assert parse_config(["--optimizer", "adam", "--beta2", "0.99"]).optim == Optimizer.adam(beta2=0.99)
    with pytest.raises(ValueError, match="plain SGD only"):
        TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", optimizer=KINDS["adam"])
    TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", optimizer=Optimizer.sgd())
