"""An exponential moving average of the weights (csrc/mlp/ema.h), CPU side: the rule against exact rational arithmetic,
the engine API, the torch-backend trainer against the host recurrence over its twin's per-step parameters, the weights
evaluations read, loopback ranks, the fp64 oracle, the CLI with checkpoints, and the native driver."""
import json
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.optim import Ema, new_ema_state, new_state
from cme213_sp18_amd.parallel import LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer

from .best_oracle import data
from .ema_workers import (LR, OPT_LR, OPTS, REG, RULE, average, frac_update, live, make_trainer, py_decay, recurrence,
                          same, twin_steps)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("warmup", [False, True])
def test_rule_is_exact_rational_arithmetic_rounded_once(dtype, warmup):
    g = np.random.default_rng(5)
    e = g.standard_normal(512).astype(dtype)
    want = e.copy()
    t = 0
    for _ in range(5):
        p = (e + g.standard_normal(512) * 10.0 ** g.integers(-6, 1, 512)).astype(dtype)
        p[::17] = e[::17]  # some fixed points
        d = py_decay(0.999, warmup, t)
        want = np.array([frac_update(a, b, d, dtype) for a, b in zip(want, p)], dtype)
        t1 = cpu().ema_step(e, p, 0.999, warmup, t)
        assert t1 == t + 1 and same(e, want)
        assert same(e[::17], p[::17])
        t = t1


def test_fixed_point_and_decay_sequence():
    for dtype in (np.float32, np.float64):
        x = np.random.default_rng(1).standard_normal(300).astype(dtype)
        x[0], x[1] = 0.0, -0.0
        for warmup in (False, True):
            e = x.copy()
            for t in range(3):
                cpu().ema_step(e, x, 0.75, warmup, t)
            assert same(e, x)
    for decay in (0.0, 0.9, 0.999, 0.9999):
        last = 0.0
        for t in list(range(200)) + [8989, 8990, 8991, 10**6]:
            assert cpu().ema_decay(decay, False, t) == decay
            d = cpu().ema_decay(decay, True, t)
            assert d == py_decay(decay, True, t) == Ema(decay, True).decay_at(t)
            assert last <= d <= decay
            last = d
    assert cpu().ema_decay(0.999, True, 0) == 1.0 / 10.0 and cpu().ema_decay(0.999, True, 90) == 91.0 / 100.0
    assert cpu().ema_decay(0.999, True, 10**6) == 0.999
    with pytest.raises(ValueError):
        cpu().ema_decay(1.0, False, 0)
    with pytest.raises(ValueError):
        cpu().ema_step(np.zeros(2, np.float32), np.zeros(2, np.float64), 0.5, False, 0)
    with pytest.raises(ValueError):
        Ema(1.0)


# ------------------------------------------------------------------------------------------------ the engine
def test_engine_api_allocates_only_when_enabled():
    (x, y), (xv, yv) = data()
    e = MlpEngine((784, 16, 10), "f64", max_cols=128, device="cpu", backend="torch")
    assert e._ema is None
    e.ema_update()  # a no-op
    with pytest.raises(RuntimeError):
        e.ema_params()
    with pytest.raises(RuntimeError):
        e.evaluate(weights="ema")
    nn = NeuralNetwork([784, 16, 10])
    e.set_params(*nn.params)
    e.set_ema(Ema(0.5))
    assert e.ema_count() == 0 and all(same(a, b) for a, b in zip(e.ema_params(), e.get_params()))
    e.load_dataset(x, y)
    e.run(0, 128, 1.0 / 128, REG, LR, sgd=True)
    e.ema_update()
    st = e.ema_state()
    assert st == {"decay": 0.5, "warmup": False, "t": 1, "last_decay": 0.5}
    for a, p, p0 in zip(e.ema_params(), e.get_params(), nn.params):  # e = p0 + 0.5 (p - p0)
        assert same(a, np.where(p == p0, p0, p0 + 0.5 * (p - p0)))
    # a non-zero status element: the update was not applied, the launch changes nothing
    before = e.ema_params()
    e.grads[e.status_index] = 1.0
    e.ema_update(status=True)
    assert e.ema_count() == 1 and all(same(a, b) for a, b in zip(before, e.ema_params()))
    e.grads[e.status_index] = 0.0
    # set_params starts the average again; set_ema(None) releases it
    e.set_params(*nn.params)
    assert e.ema_count() == 0 and all(same(a, b) for a, b in zip(e.ema_params(), nn.params))
    e.set_ema_state(7, e.get_params())
    assert e.ema_count() == 7
    e.set_ema(None)
    assert e._ema is None
    with pytest.raises(TypeError):
        e.set_ema(0.5)


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("opt", list(OPTS))
def test_torch_trainer_average_is_the_host_recurrence_and_leaves_the_parameters_alone(opt):
    lr = OPT_LR[opt]
    tr = make_trainer(opt)
    plain = make_trainer(opt, ema=None)
    assert tr.native_plan(tr.epoch_plan()) is None and "averag" in tr.native_reason
    e0 = live(tr)
    assert same(average(tr), e0) and tr.engine.ema_count() == 0
    tr.train(4, lr, REG)
    plain.train(4, lr, REG)
    assert same(live(tr), live(plain))  # the parameters with the average are those without it
    seq = twin_steps(make_trainer(opt, ema=None), 4, lr)
    assert same(seq[-1], live(plain))
    want, t = recurrence(e0, seq, RULE)
    assert t == 16 == tr.engine.ema_count() and same(average(tr), want)
    assert not same(want, seq[-1])
    # train(2) twice equals train(4) in the average and the count
    two = make_trainer(opt)
    two.train(2, lr, REG)
    assert two.engine.ema_count() == 8
    two.train(2, lr, REG)
    assert two.engine.ema_count() == 16 and same(average(two), want) and same(live(two), live(plain))
    # the eager step() path folds the same average
    st = make_trainer(opt)
    twin_steps(st, 4, lr)
    assert st.engine.ema_count() == 16 and same(average(st), want)


def test_evaluations_keep_best_and_adopt_use_the_averaged_weights():
    (x, y), (xv, yv) = data()
    tr = make_trainer("momentum")
    evs = []
    st = tr.train(5, LR, REG, eval_every=1, keep_best="loss", on_event=evs.append)
    assert [e["weights"] for e in st.evals] == ["ema"] * 5
    assert all(e["weights"] == "ema" for e in evs if e["event"] == "eval")
    # a twin stopped after every epoch: evaluate() of a fresh engine that received the averaged weights
    twin = make_trainer("momentum")
    want, avgs = [], []
    for _ in range(5):
        twin.train(1, LR, REG)
        avgs.append(twin.ema_params())
        f = MlpEngine((784, 16, 10), "f64", max_cols=128, device="cpu", backend="torch")
        f.load_dataset(x, y)
        f.set_params(*avgs[-1])
        f.load_eval(xv, yv)
        want.append(f.evaluate())
        got = twin.evaluate(weights="ema")
        assert got["n"] == want[-1]["n"] and got["loss"] == want[-1]["loss_sum"] / want[-1]["n"]
        assert twin.evaluate()["loss"] != got["loss"]  # the current weights are other weights
    for a, b in zip(st.evals, want):
        assert a["loss"] == b["loss_sum"] / b["n"] and a["accuracy"] == b["correct"] / b["n"]
        np.testing.assert_array_equal(a["confusion"], b["confusion"])
    assert same(live(tr), live(twin)) and same(average(tr), average(twin))
    # keep_best stored the AVERAGED weights of the chosen epoch
    bi = tr.best_state()["best_index"]
    assert bi == int(np.argmin([w["loss_sum"] for w in want]))
    for a, b in zip(tr.engine.best_params(), avgs[bi]):
        assert same(a, b)
    # eval_weights="current" reads the live parameters, as a trainer without averaging does
    cur = make_trainer("momentum").train(2, LR, REG, eval_every=1, eval_weights="current")
    ref = make_trainer("momentum", ema=None).train(2, LR, REG, eval_every=1)
    assert [e["loss"] for e in cur.evals] == [e["loss"] for e in ref.evals]
    assert [e["weights"] for e in cur.evals] == ["current"] * 2 and "weights" not in ref.evals[0]
    # predict with the averaged weights, then adopt them: nn, the parameters and predict() become the average's
    pe = tr.predict(xv, weights="ema")
    f = MlpEngine((784, 16, 10), "f64", max_cols=128, device="cpu", backend="torch")
    f.set_params(*tr.ema_params())
    np.testing.assert_array_equal(pe, f.predict(xv))
    avg = tr.ema_params()
    tr.adopt_ema()
    for a, b, c in zip(tr.engine.get_params(), avg, tr.nn.params):
        assert same(a, b) and same(np.asarray(c, np.float64).reshape(a.shape), b)
    np.testing.assert_array_equal(tr.predict(xv), pe)
    assert tr.engine.ema_count() == 20 and all(same(a, b) for a, b in zip(tr.ema_params(), avg))


def test_snapshot_and_restore_carry_the_average():
    tr = make_trainer("momentum")
    tr.train(1, LR, REG)
    snap = tr._snapshot()
    avg, p, t = average(tr), live(tr), tr.engine.ema_count()
    tr.train(1, LR, REG)
    assert not same(average(tr), avg) and tr.engine.ema_count() == t + 4
    tr._restore(snap)
    assert same(average(tr), avg) and same(live(tr), p) and tr.engine.ema_count() == t


def test_refusals():
    with pytest.raises(ValueError, match="data parallelism"):
        TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", ema=Ema(0.9))
    with pytest.raises(TypeError):
        make_trainer("sgd", ema=0.9)
    tr = make_trainer("sgd", ema=None)
    with pytest.raises(ValueError, match="ema"):
        tr.train(1, LR, REG, eval_every=1, eval_weights="ema")
    with pytest.raises(ValueError):
        make_trainer("sgd").train(1, LR, REG, eval_every=1, eval_weights="best")
    assert tr.engine._ema is None and tr.native_reason == ""


# ------------------------------------------------------------------------------------------------ loopback ranks
def test_loopback_world3_uneven_shards_average_alike():
    R = 3
    comms = LoopbackComm.create(R)
    out = [None] * R

    def work(r):
        torch.set_num_threads(1)
        tr = make_trainer("momentum", comm=comms[r], batch=126, nval=256)
        st = tr.train(3, LR, REG, eval_every=1, keep_best="loss")
        out[r] = dict(shard=tr.engine.eval_samples, avg=average(tr), params=live(tr), t=tr.engine.ema_count(),
                      agree=tr.replicas_agree(), losses=[e["loss"] for e in st.evals],
                      best=tr.engine._best["arena"].clone())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert [o["shard"] for o in out] == [85, 85, 86]  # uneven validation shards
    for o in out:
        assert o["agree"] and o["t"] == out[0]["t"] == 3 * 5 and same(o["avg"], out[0]["avg"])
        assert same(o["params"], out[0]["params"]) and o["losses"] == out[0]["losses"]
        assert torch.equal(o["best"], out[0]["best"])
    assert not same(out[0]["avg"], out[0]["params"])


# ------------------------------------------------------------------------------------------------ the fp64 oracle
@pytest.mark.parametrize("opt", ["sgd", "momentum"])
def test_fp64_oracle_keeps_and_returns_the_average(opt):
    (x, y), _ = data()
    x = np.asarray(x, np.float64)
    kw = dict(optimizer=OPTS[opt].get("optimizer"))
    nn = NeuralNetwork([784, 16, 10])
    st = new_ema_state(nn)
    e0 = st["avg"].copy()
    mlp.train(nn, x, y, LR, REG, 2, 128, ema=RULE, ema_state=st, **kw)
    plain = NeuralNetwork([784, 16, 10])
    mlp.train(plain, x, y, LR, REG, 2, 128, **kw)
    assert all(same(a, b) for a, b in zip(nn.params, plain.params)) and st["t"] == 8
    # one epoch of one batch at a time: the parameters after every update
    twin, seq = NeuralNetwork([784, 16, 10]), []
    ost = None
    if opt != "sgd":
        ost = new_state(kw["optimizer"], twin.num_params())
    for _ in range(2):
        for s in range(0, 512, 128):
            mlp.train(twin, x[s:s + 128], y[s:s + 128], LR, REG, 1, 128, optim_state=ost, **kw)
            seq.append(np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in twin.params]))
    assert same(seq[-1], np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in nn.params]))
    want, t = recurrence(e0, seq, RULE)
    assert t == 8 and same(st["avg"], want)
    # two calls continue the state
    nn2 = NeuralNetwork([784, 16, 10])
    st2 = new_ema_state(nn2)
    ost2 = None
    if opt != "sgd":
        ost2 = new_state(kw["optimizer"], nn2.num_params())
    for _ in range(2):
        mlp.train(nn2, x, y, LR, REG, 1, 128, ema=RULE, ema_state=st2, optim_state=ost2, **kw)
    assert st2["t"] == 8 and same(st2["avg"], want)


# ------------------------------------------------------------------------------------------------ CLI
def _cli(tmp_path, *args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--backend", "torch", "--dtype", "f64", "-n",
                        "16", "-b", "128", "--num-train", "640", "--num-test", "64", "-l", "0.2", "--optimizer",
                        "momentum", "--outdir", str(tmp_path / "Outputs"), *args],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_ema_checkpoint_round_trips_through_resume(tmp_path):
    flags = ("--ema", "0.9", "--ema-warmup", "--eval-every", "1")
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    log = tmp_path / "run.jsonl"
    r = _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "--log-json", str(log))
    assert "Weight averaging: decay 0.9 with warmup" in r.stdout
    ev = [json.loads(line) for line in log.read_text().splitlines()]
    assert ev[0]["event"] == "config" and ev[0]["ema"] == {"decay": 0.9, "warmup": True}
    assert [e["weights"] for e in ev if e.get("event") == "eval"] == ["ema"] * 4
    assert [e for e in ev if e.get("event") == "ema"][0]["adopted"] is False
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with weight averaging" not in r.stdout
    a, b = (json.loads((tmp_path / d / "meta.json").read_text())["ema"] for d in ("whole", "rest"))
    assert a == b and a["decay"] == 0.9 and a["warmup"] is True and a["t"] > 0
    assert a["t"] == 2 * json.loads((tmp_path / "half" / "meta.json").read_text())["ema"]["t"]
    for n in ("W0", "W1", "b0", "b1"):  # the count and the average continue
        assert (tmp_path / "whole" / "ema" / f"{n}.mat").read_bytes() == (
            tmp_path / "rest" / "ema" / f"{n}.mat").read_bytes()
        assert (tmp_path / "whole" / "ema" / f"{n}.mat").read_bytes() != (
            tmp_path / "whole" / f"{n}.mat").read_bytes()
    other = _cli(tmp_path, "--ema", "0.5", "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with weight averaging" in other.stdout
    none = _cli(tmp_path, "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with weight averaging" in none.stdout
    # --use-ema: the final checkpoint's weights are the averaged ones
    used = str(tmp_path / "used")
    r = _cli(tmp_path, *flags, "-e", "2", "--use-ema", "--ckpt-dir", used)
    assert "-- adopted" in r.stdout
    from cme213_sp18_amd.utils.checkpoint import load_raw_ascii

    for n in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(load_raw_ascii(str(tmp_path / "used" / "ema" / f"{n}.mat")).ravel(),
                                      load_raw_ascii(str(tmp_path / "used" / f"{n}.mat")).ravel())
        assert (tmp_path / "used" / "ema" / f"{n}.mat").read_bytes() == (
            tmp_path / "half" / "ema" / f"{n}.mat").read_bytes()
    for bad in (("--ema", "0.9", "--parallel", "tp"), ("--ema-warmup",), ("--use-ema",), ("--ema", "1.0"),
                ("--eval-weights", "ema")):
        rr = _cli(tmp_path, *bad, "-e", "1", ok=False)
        assert rr.returncode == 2 and "Loaded" not in rr.stdout  # refused when the flags are parsed


# ------------------------------------------------------------------------------------------------ native driver
@pytest.mark.skipif(shutil.which("cmake") is None, reason="cmake not available")
def test_native_ema_tests_under_asan_ubsan(tmp_path):
    build = tmp_path / "build"
    env = dict(os.environ, TMPDIR=str(tmp_path), NO_COLOR="1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.run(["cmake", "-S", ROOT, "-B", str(build), *gen, "-DCME_SANITIZE=ON", "-DCMAKE_BUILD_TYPE=Debug"],
                   check=True, capture_output=True, env=env, timeout=300)
    subprocess.run(["cmake", "--build", str(build), "-j", "4", "--target", "native_ema_tests"], check=True,
                   capture_output=True, env=env, timeout=600)
    r = subprocess.run([str(build / "native_ema_tests")], capture_output=True, text=True, env=env, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert "0 failed" in r.stdout and "5 tests" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
