"""Learning-rate schedules and gradient-norm clipping on the CPU: optim.Schedule against its formulas, the summation
order of csrc/mlp/clip.h (_cpu.grad_sumsq) against numpy, _cpu.grad_clip and the kSgd rule against torch, the
torch-backend trainer against the fp64 oracle (models.mlp.train(schedule=, clip_norm=)), split runs, loopback ranks,
checkpoints, the refusals, and the native driver under the sanitizers."""
import json
import math
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
from cme213_sp18_amd.optim import Optimizer, Schedule, new_state
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, TensorParallelTrainer
from cme213_sp18_amd.utils.checkpoint import load_checkpoint, load_optim_state, save_checkpoint
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.eval_oracle import TOL
from tests.sched_workers import LR, ORACLE_CLIP, ORACLE_LR, REG, RULES, SCHED, padded_arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _torch_trainer(dtype, opt, x, y, comm=None, H=100, B=64, **kw):
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), comm=comm, device="cpu", dtype=dtype, batch_size=B,
                             backend="torch", use_graphs=False, optimizer=opt, **kw)
    tr.load(x, y)
    return tr


# ------------------------------------------------------------------------------------------------------- Schedule
def _formula(s: Schedule, t: int, spe: int) -> float:
    u = t if s.unit == "step" else t // spe
    if u < s.warmup:
        return s.warmup_start + (1 - s.warmup_start) * u / s.warmup
    v = u - s.warmup
    if s.kind == "constant":
        return 1.0
    if s.kind == "step":
        return s.gamma ** (v // s.size)
    if s.kind == "exponential":
        return s.gamma ** v
    if s.kind == "linear":
        return 1 + (s.end_factor - 1) * min(v, s.total) / s.total
    return s.min_factor + (1 - s.min_factor) * (1 + math.cos(math.pi * min(v, s.total) / s.total)) / 2


@pytest.mark.parametrize("unit", ["step", "epoch"])
def test_schedule_factor_is_the_documented_formula(unit):
    kw = dict(unit=unit, warmup=3, warmup_start=0.2)
    cases = [Schedule.constant(**kw), Schedule.step(2, 0.5, **kw), Schedule.exponential(0.9, **kw),
             Schedule.linear(5, 0.1, **kw), Schedule.cosine(5, 0.05, **kw), Schedule.cosine(4, unit=unit),
             Schedule.step(3, 0.1, unit=unit)]
    spe = 4
    for s in cases:
        for t in range(0, 60):
            assert s.factor(t, spe) == pytest.approx(_formula(s, t, spe), rel=1e-15, abs=1e-300), (s, t)
        assert isinstance(s.factor(0, spe), float)
        assert s == Schedule.from_meta(json.loads(json.dumps(s.as_meta()))) and s.key() == Schedule(**s.as_meta()).key()
        assert hash(s) == hash(Schedule(**s.as_meta()))
        np.testing.assert_array_equal(s.factors(7, 5, spe), [s.factor(7 + i, spe) for i in range(5)])
    per = spe if unit == "epoch" else 1  # updates per unit
    w = Schedule.step(2, 0.5, **kw)
    assert w.factor(0, spe) == 0.2                                       # the first unit
    assert w.factor(3 * per - 1, spe) == pytest.approx(0.2 + 0.8 * 2 / 3)  # u = warmup - 1
    assert w.factor(3 * per, spe) == 1.0                                 # u = warmup
    assert w.factor(5 * per, spe) == 0.5 and w.factor(7 * per, spe) == 0.25
    lin, cos = Schedule.linear(5, 0.1, **kw), Schedule.cosine(5, 0.05, **kw)
    for v in (5, 6, 50):  # v beyond total: the final factor, held
        assert lin.factor((3 + v) * per, spe) == pytest.approx(0.1) and cos.factor((3 + v) * per, spe) == pytest.approx(
            0.05)
    assert Schedule.cosine(4, unit=unit).factor(2 * per, spe) == pytest.approx(0.5)
    assert Schedule.from_meta(None) is None


def test_schedule_validation():
    for bad in (dict(kind="poly"), dict(unit="minute"), dict(kind="step", size=0), dict(kind="step", gamma=0.0),
                dict(kind="step", gamma=1.5), dict(kind="exponential", gamma=-0.1), dict(kind="linear", total=0),
                dict(kind="cosine", total=-2), dict(kind="linear", end_factor=-0.5), dict(kind="cosine", min_factor=-1e-3),
                dict(warmup=-1), dict(warmup_start=-0.1), dict(warmup=1.5), dict(kind="step", size=2.5),
                dict(warmup_start=float("nan"))):
        with pytest.raises(ValueError):
            Schedule(**bad)
    assert Schedule.step(1, 1.0).gamma == 1.0 and Schedule.linear(1, 0.0).end_factor == 0.0
    with pytest.raises(ValueError):
        Schedule.constant().factor(-1)
    with pytest.raises(ValueError):
        Schedule.constant(unit="epoch").factor(3, 0)
    with pytest.raises(Exception):
        Schedule.constant().warmup = 2  # frozen
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            DataParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", clip_norm=bad)
    with pytest.raises(TypeError):
        DataParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", schedule="cosine")


# ------------------------------------------------------------------------------------------- clip.h on the host
@pytest.mark.parametrize("count", [1, 255, 257, 1025, 2 ** 20 + 3])
@pytest.mark.parametrize("ndt", [np.float32, np.float64])
def test_grad_sumsq_against_numpy(ndt, count):
    """The bound for a sum of n non-negative fp64 terms, each product rounded once: (n + 2) 2^-53 relative.  Every
    padding slot and the status element hold NaN: a finite result shows they are excluded."""
    g, segs = padded_arena(count, ndt)
    parts, norm = cpu().grad_sumsq(g, segs)
    assert parts.dtype == np.float64 and len(parts) == cpu().clip_grid(count) and 1 <= len(parts) <= 64
    if count > 64 * 4096:
        assert len(parts) == 64  # the fixed grid's cap: threads wrap around
    ref = sum(float((g[o:o + s].astype(np.float64) ** 2).sum()) for o, s in segs)
    assert np.isfinite(norm)
    assert abs(float(np.sum(parts)) - ref) <= (count + 2) * 2.0 ** -53 * ref
    assert abs(norm - math.sqrt(ref)) <= (count + 2) * 2.0 ** -53 * math.sqrt(ref)
    with pytest.raises(Exception):
        cpu().grad_sumsq(g, [(0, g.size + 1)])
    with pytest.raises(Exception):
        cpu().grad_sumsq(g, [(0, 1)] * 5)


def test_grad_clip_is_torch_clip_grad_norm():
    rng = np.random.default_rng(0)
    sizes = [701, 13, 130, 10]
    g, segs, tens, o = [], [], [], 0
    for s in sizes:
        a = rng.standard_normal(s)
        tens.append(torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)))
        tens[-1].grad = torch.tensor(a.copy())
        segs.append((o, s))
        g.append(a)
        o += s
    g = np.concatenate(g)
    norm0 = float(np.sqrt((g ** 2).sum()))
    above = g.copy()
    n, c = cpu().grad_clip(above, segs, 2 * norm0)  # a threshold above the norm: bitwise unchanged
    assert c > 1.0 and n == pytest.approx(norm0, rel=1e-14) and np.array_equal(above.view(np.uint8), g.view(np.uint8))
    total = torch.nn.utils.clip_grad_norm_(tens, max_norm=2 * norm0, norm_type=2)
    assert float(total) == pytest.approx(n, rel=1e-12)
    np.testing.assert_array_equal(torch.cat([t.grad for t in tens]).numpy(), g)
    below = g.copy()
    n, c = cpu().grad_clip(below, segs, 0.5 * norm0)
    assert c == pytest.approx(0.5 * norm0 / (norm0 + 1e-6), rel=1e-14) and c < 1.0
    torch.nn.utils.clip_grad_norm_(tens, max_norm=0.5 * norm0, norm_type=2)
    np.testing.assert_allclose(below, torch.cat([t.grad for t in tens]).numpy(), rtol=1e-12, atol=0)
    f = g.astype(np.float32)  # one rounding in T: g * float32(coef)
    n32, c32 = cpu().grad_clip(f, segs, 0.5 * norm0)
    assert np.array_equal(f, g.astype(np.float32) * np.float32(c32))
    bad = g.copy()
    bad[3] = np.nan  # a non-finite norm propagates, as torch's default (error_if_nonfinite=False)
    n, c = cpu().grad_clip(bad, segs, 1.0)
    assert math.isnan(n) and math.isnan(c) and np.isnan(bad).all()
    with pytest.raises(Exception):
        cpu().grad_clip(g.copy(), segs, 0.0)


def test_ksgd_rule_is_torch_sgd():
    """test_update_rules_are_torch_optims (tests/test_optim.py) for the third rule: both sides fp64, 5 steps, |p| in
    [0.5, 2] so that rtol never measures a cancellation."""
    rng = np.random.default_rng(0)
    n, lr = 4096, 5e-3
    p = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    tp = torch.tensor(p.copy(), requires_grad=True)
    to = torch.optim.SGD([tp], lr=lr)
    t = 0
    for k in range(5):
        g = rng.standard_normal(n)
        tp.grad = torch.tensor(g)
        to.step()
        t, _, _ = cpu().optim_step(2, Optimizer.sgd().hyper(lr), p, g, None, None, t)
        assert t == k + 1
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
    with pytest.raises(Exception):
        cpu().optim_step(7, Optimizer.sgd().hyper(lr), p, g, None, None, 0)
    with pytest.raises(Exception):
        cpu().optim_step(0, Optimizer.sgd().hyper(lr), p, g, None, None, 0)  # momentum needs its state


def test_window_rate_clamps_into_the_window():
    f = np.array([0.5, 2.0, 0.125])
    assert [cpu().window_rate(0.1, 1, f, t) for t in range(6)] == [0.1 * v for v in (0.5, 0.5, 2.0, 0.125, 0.125, 0.125)]


# ------------------------------------------------------------------------------------- trainer against the oracle
@pytest.mark.parametrize("kind", ["momentum", "sgd"])
@pytest.mark.parametrize("dtype,key", [("f64", ("f64", "mfma")), ("f32", ("f32", "split3"))])
def test_torch_trainer_matches_the_fp64_oracle(dtype, key, kind):
    x, y = synthetic_mnist(256, seed=3)
    opt = Optimizer.momentum(0.9, False) if kind == "momentum" else Optimizer.sgd()
    ref, log = NeuralNetwork([784, 100, 10]), []
    st = new_state(opt, ref.num_params(), policy=True)
    mlp.train(ref, x, y, ORACLE_LR, REG, 2, 64, optimizer=opt, optim_state=st, schedule=SCHED, clip_norm=ORACLE_CLIP,
              update_log=log)
    assert st["t"] == 8 and [r[0] for r in log] == list(range(8))
    assert [r[1] for r in log] == [ORACLE_LR * SCHED.factor(t) for t in range(8)]
    coefs = [r[3] for r in log]
    print(f"NUMERICS oracle norms {[round(r[2], 4) for r in log]} coefficients {[round(c, 4) for c in coefs]}")
    assert any(c < 1.0 for c in coefs) and any(c >= 1.0 for c in coefs)  # clipped and unclipped updates
    events = []
    tr = _torch_trainer(dtype, opt, x, y, schedule=SCHED, clip_norm=ORACLE_CLIP)
    tr.train(2, ORACLE_LR, REG, print_every=1, on_event=events.append, log=lambda m: None)
    assert tr.engine.update_count() == 8
    losses = [e for e in events if e["event"] == "loss"]
    assert [e["lr"] for e in losses] == [r[1] for r in log]  # the loss events carry the update's rate and norm
    for e, r in zip(losses, log):
        assert e["grad_norm"] == pytest.approx(r[2], rel=10 * TOL[key])
    for name, got, want in zip(("W1", "b1", "W2", "b2"), tr.engine.get_params(), ref.params):
        rel = _rel(got, want)
        print(f"NUMERICS {dtype} {kind} {name} rel {rel:.3e} (bound {TOL[key]})")
        assert rel < TOL[key], (name, rel)
    if kind == "sgd":  # scheduled plain SGD: the kSgd rule with a counter and no state buffer
        assert tr.engine.opt_bufs == [] and tr.engine.optim_state()["kind"] == "sgd"


def test_oracle_continues_its_rates_one_epoch_at_a_time():
    x, y = synthetic_mnist(256, seed=3)
    sch = Schedule.cosine(total=3, unit="epoch", warmup=1)
    for opt in (Optimizer.sgd(), RULES["adam"]):
        a, b, c = (NeuralNetwork([784, 24, 10]) for _ in range(3))
        mlp.train(a, x, y, LR, REG, 3, 64, optimizer=opt, schedule=sch, clip_norm=50.0)
        st = new_state(opt, b.num_params(), policy=True)
        for ep in range(3):
            mlp.train(b, x, y, LR, REG, 1, 64, iter0=4 * ep, optimizer=opt, optim_state=st, schedule=sch, clip_norm=50.0)
        assert st["t"] == 12
        for u, v in zip(a.params, b.params):
            np.testing.assert_array_equal(u, v)
        mlp.train(c, x, y, LR, REG, 3, 64, shuffle_seed=5, optimizer=opt, schedule=sch, clip_norm=50.0)
        assert _rel(c.W[0], a.W[0]) > 1e-9
    plain, none = NeuralNetwork([784, 24, 10]), NeuralNetwork([784, 24, 10])
    mlp.train(plain, x, y, LR, REG, 2, 64)
    mlp.train(none, x, y, LR, REG, 2, 64, schedule=None, clip_norm=None)
    np.testing.assert_array_equal(plain.W[0], none.W[0])


# ------------------------------------------------------------------------------------------------- split runs
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_train_2_plus_2_equals_train_4(kind):
    x, y = synthetic_mnist(200, seed=3)
    sch = Schedule.cosine(total=4, unit="epoch", warmup=1)
    a, b, c = (_torch_trainer("f32", RULES[kind], x, y, H=24, schedule=sch, clip_norm=100.0) for _ in range(3))
    a.train(2, LR, REG)
    a.train(2, LR, REG)
    b.train(4, LR, REG)
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.opt_rec, b.engine.opt_rec)
    assert all(torch.equal(u, v) for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs))
    assert a.engine.update_count() == 16 and a.engine.last_update() == b.engine.last_update()
    assert b.engine.last_update()["lr"] == LR * sch.factor(15, 4)
    # a hand-driven loop of step() calls gets the same rates
    for _ in range(4):
        for s, n in c.epoch_plan().steps:
            c.step(s, n, LR, REG)
    assert torch.equal(c.engine.params, b.engine.params)
    # _snapshot / _restore carry the counter records of scheduled plain SGD too
    snap = a._snapshot()
    assert len(snap) == 5
    a.train(1, LR, REG)
    a._restore(snap)
    assert a.engine.update_count() == 16 and torch.equal(a.engine.params, b.engine.params)


def test_status_element_skips_the_update_and_the_last_record():
    x, y = synthetic_mnist(128, seed=3)
    tr = _torch_trainer("f64", None, x, y, H=24, schedule=SCHED, clip_norm=1.0)
    e = tr.engine
    assert e.last_update() is None
    e.run(0, 64, 1 / 64, REG, LR, sgd=False)
    e.grads[e.status_index] = 1.0
    before = (e.params.clone(), e.opt_rec.clone(), e.opt_last.clone())
    e.apply(LR)
    assert torch.equal(e.params, before[0]) and torch.equal(e.opt_rec, before[1])
    assert torch.equal(e.opt_last.view(torch.int64), before[2].view(torch.int64))
    e.grads[e.status_index] = 0.0
    g = e.grads.clone()
    e.apply(LR)
    assert e.update_count() == 1 and not torch.equal(e.params, before[0])
    assert torch.equal(e.grads, g)  # the bucket itself is left as the step wrote it
    up = e.last_update()
    assert up["t"] == 0 and up["lr"] == LR * SCHED.factor(0) and up["grad_norm"] > 0


def test_window_growth_reallocates_and_reports_it():
    x, y = synthetic_mnist(128, seed=3)
    e = _torch_trainer("f64", None, x, y, H=24, schedule=SCHED).engine
    cap = e.sched_win.numel() - 2
    ptr = e.sched_win.data_ptr()
    assert e.set_schedule_window(3, np.ones(cap)) is False and e.sched_win.data_ptr() == ptr
    assert e.set_schedule_window(3, np.ones(cap + 1)) is True and e.sched_win.numel() - 2 >= cap + 1
    for bad in ((-1, [1.0]), (0, []), (0, [-0.5])):
        with pytest.raises(ValueError):
            e.set_schedule_window(*bad)
    with pytest.raises(RuntimeError):
        _torch_trainer("f64", None, x, y, H=24, clip_norm=1.0).engine.set_schedule_window(0, [1.0])


# ------------------------------------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("kind", ["sgd", "nesterov"])
def test_loopback_world2_matches_single(kind):
    H, N, B = 24, 512, 128
    x, y = synthetic_mnist(N, seed=11)
    comms = LoopbackComm.create(2)
    out = [None, None]
    kw = dict(H=H, B=B, schedule=SCHED, clip_norm=ORACLE_CLIP / 2)  # (H = 24: norms near 1)

    def work(r):
        torch.set_num_threads(1)
        tr = _torch_trainer("f64", RULES[kind], x, y, comm=comms[r], **kw)
        tr.train(2, ORACLE_LR, REG)
        out[r] = (tr.engine.params.clone(), tr.engine.opt_rec.clone(), tr.engine.last_update())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    one = _torch_trainer("f64", RULES[kind], x, y, **kw)
    one.train(2, ORACLE_LR, REG)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    assert out[0][2]["t"] == 7 and out[0][2]["lr"] == one.engine.last_update()["lr"]
    rel = _rel(out[0][0].numpy(), one.engine.params.numpy())
    print(f"NUMERICS loopback {kind} rel {rel:.3e} last {out[0][2]} one {one.engine.last_update()}")
    assert rel < TOL[("f64", "mfma")]
    assert out[0][2]["grad_norm"] == pytest.approx(one.engine.last_update()["grad_norm"], rel=1e-9)


# -------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_and_resume_continue_the_rates(tmp_path):
    x, y = synthetic_mnist(200, seed=3)
    sch = Schedule.cosine(total=4, unit="epoch", warmup=1)
    kw = dict(H=24, schedule=sch, clip_norm=100.0)
    whole = _torch_trainer("f64", None, x, y, **kw)
    whole.train(4, LR, REG)
    half = _torch_trainer("f64", None, x, y, **kw)
    half.train(2, LR, REG)
    save_checkpoint(half.nn, str(tmp_path / "ck"), meta={"iter": half.iter, "schedule": sch.as_meta(), "clip_norm": 100.0},
                    optim_state=half.engine.optim_state())
    nn, meta = load_checkpoint(str(tmp_path / "ck"))
    assert meta["optim_kind"] == "sgd" and meta["optim_t"] == 8 and Schedule.from_meta(meta["schedule"]) == sch
    st = load_optim_state(str(tmp_path / "ck"), meta)
    assert st["t"] == 8 and st["state"] == []  # scheduled plain SGD: the count alone
    rest = DataParallelTrainer(nn, device="cpu", dtype="f64", batch_size=64, backend="torch", use_graphs=False,
                               schedule=Schedule.from_meta(meta["schedule"]), clip_norm=meta["clip_norm"])
    rest.engine.set_optim_state(st)
    rest.iter = meta["iter"]
    rest.load(x, y)
    rest.train(2, LR, REG)
    assert torch.equal(rest.engine.params, whole.engine.params) and rest.engine.update_count() == 16
    assert rest.engine.last_update() == whole.engine.last_update()


def _cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "1600", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_schedule_checkpoint_and_resume(tmp_path):
    """The flags on the sequential and the parallel run alike (the preset runs both: -s), resumed == unbroken, for
    scheduled plain SGD, which has no optim.npz state but keeps optim_t."""
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--lr-schedule", "cosine", "--lr-unit", "epoch", "--lr-total", "4", "--warmup", "1", "--warmup-start",
             "0.25", "--clip-norm", "1.5")
    r = _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "-g", "0", "-d")
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert meta["schedule"]["kind"] == "cosine" and meta["schedule"]["unit"] == "epoch" and meta["clip_norm"] == 1.5
    assert meta["optim_kind"] == "sgd" and meta["optim_t"] == meta["iter"] == 16
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["correct"] is True  # the fp64 parallel run against the sequential oracle with the same policy
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])
    assert json.loads((tmp_path / "rest" / "meta.json").read_text())["optim_t"] == 16
    other = _cli(tmp_path, "--lr-schedule", "exp", "--lr-gamma", "0.9", "-e", "1", "--resume", half, "--ckpt-dir",
                 str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with schedule" in other.stdout


# ---------------------------------------------------------------------------------------------------- refusals
def test_plain_sgd_with_nothing_set_allocates_no_record_and_tp_refuses():
    x, y = synthetic_mnist(128, seed=3)
    tr = _torch_trainer("f64", None, x, y, H=24, schedule=None, clip_norm=None)
    e = tr.engine
    assert e.opt_rec is None and e.opt_bufs == [] and e.sched_win is None and e.clip_partials is None
    assert e.opt_last is None and not e.uses_apply_launch and len(tr._snapshot()) == 3 and e.optim_state() is None
    with pytest.raises(RuntimeError):
        e.update_count()
    on = _torch_trainer("f64", None, x, y, H=24, clip_norm=1.0)
    assert on.engine.opt_rec is not None and on.engine.opt_bufs == [] and on.engine.sched_win is None
    on.engine.set_update_policy(None, None)  # ... and back: nothing is kept
    assert on.engine.opt_rec is None and on.engine.clip_partials is None
    for kw, word in ((dict(schedule=SCHED), "schedule"), (dict(clip_norm=1.0), "clipping")):
        t2 = _torch_trainer("f64", None, x, y, H=24, **kw)
        assert t2.native_plan(t2.epoch_plan()) is None and word in t2.native_reason
        with pytest.raises(ValueError, match="data parallelism"):
            TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", **kw)
    TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", schedule=None, clip_norm=None)
    from cme213_sp18_amd.config import parse_config
    for argv in (["--parallel", "tp", "--lr-schedule", "cosine"], ["--parallel", "tp", "--clip-norm", "1"],
                 ["--clip-norm", "0"], ["--clip-norm", "-2"], ["--lr-schedule", "step", "--lr-gamma", "1.5"],
                 ["--lr-schedule", "step", "--lr-step-size", "0"], ["--warmup", "3"], ["--lr-gamma", "0.5"],
                 ["--lr-schedule", "poly"]):
        with pytest.raises(SystemExit):
            parse_config(argv)
    cfg = parse_config(["--lr-schedule", "exp", "--lr-gamma", "0.9", "--warmup", "2", "--clip-norm", "2.5"])
    assert cfg.schedule == Schedule.exponential(0.9, warmup=2) and cfg.clip_norm == 2.5
    assert parse_config([]).schedule is None and parse_config([]).clip_norm is None
    assert parse_config(["--lr-schedule", "cosine", "--lr-unit", "epoch", "--lr-total", "3", "--lr-min-factor",
                         "0.1"]).schedule == Schedule.cosine(3, 0.1, unit="epoch")


# ------------------------------------------------------------------------------------------------ native driver
@pytest.mark.skipif(shutil.which("cmake") is None, reason="cmake not available")
def test_native_clip_tests_under_asan_ubsan(tmp_path):
    build = tmp_path / "build"
    env = dict(os.environ, TMPDIR=str(tmp_path), NO_COLOR="1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.run(["cmake", "-S", ROOT, "-B", str(build), *gen, "-DCME_SANITIZE=ON", "-DCMAKE_BUILD_TYPE=Debug"],
                   check=True, capture_output=True, env=env, timeout=300)
    subprocess.run(["cmake", "--build", str(build), "-j", "4", "--target", "native_clip_tests"], check=True,
                   capture_output=True, env=env, timeout=600)
    r = subprocess.run([str(build / "native_clip_tests")], capture_output=True, text=True, env=env, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert "0 failed" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
