"""Reduce the learning rate on a validation plateau (csrc/mlp/plateau.h, optim.Plateau, MlpEngine.set_plateau /
enqueue_plateau, DataParallelTrainer(plateau=...), the CLI's --lr-plateau), everything above the kernel on the torch
backend: the rule against torch.optim.lr_scheduler.ReduceLROnPlateau, the trainer against its twin (a trainer without the
rule, run one epoch at a time at the scale torch's scheduler holds), persistence, composition with keep-best and weight
averaging, loopback ranks, the fp64 oracle's lr_scale, the CLI and the native driver."""
import itertools
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
from cme213_sp18_amd.optim import Ema, Optimizer, Plateau, Schedule, new_state
from cme213_sp18_amd.parallel import LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer

from .eval_oracle import eval_data
from .plateau_oracle import (CONFIGS, EPOCHS, INF, NAN, REG, SCRIPTS, assert_matches_twin, assert_reduces, make_trainer,
                             margins, record_fields, rule_for, run_script, run_twin, same_record, start, torch_fields,
                             torch_scheduler)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule vs torch
def _sweep():
    """Both monitors, both threshold modes, patience 0-3, cooldown 0-2, factors 0.1 and 0.5, min_factor 0 and 0.2."""
    for monitor, mode, patience, cooldown, factor, min_factor in itertools.product(
            ("loss", "accuracy"), ("rel", "abs"), (0, 1, 2, 3), (0, 1, 2), (0.1, 0.5), (0.0, 0.2)):
        yield Plateau(factor=factor, patience=patience, threshold=0.125 if mode == "rel" else 0.25,
                      threshold_mode=mode, cooldown=cooldown, min_factor=min_factor, monitor=monitor)


def _random_sequences():
    """200 seeded sequences of 40 metrics: half drawn from eleven dyadic values (repeats and exact ties are the rule),
    half continuous around a slow trend with every fourth value repeated."""
    g = np.random.default_rng(2024)
    out = []
    for i in range(200):
        if i % 2 == 0:
            out.append((g.integers(1, 12, 40) / 8.0).tolist())
        else:
            s = (2.0 - 0.02 * np.arange(40) + 0.3 * g.standard_normal(40)).tolist()
            for k in range(3, 40, 4):
                s[k] = s[k - 1]
            out.append(s)
    return out


def _against_torch(rule, metrics, seen):
    """One sequence through _cpu.plateau_decide_metric and through torch's scheduler: scale, best, bad and cooldown_left
    exactly equal after every step.  ``seen`` counts the branches the sequences hit."""
    opt, sch = torch_scheduler(rule)
    rec = np.asarray(start(rule.monitor))
    assert same_record(rec, cpu().plateau_start(rule.monitor_code))
    for k, m in enumerate(metrics):
        before = rec
        rec, reduced = cpu().plateau_decide_metric(rec, rule.native(), float(m))
        sch.step(float(m))
        assert record_fields(rec) == torch_fields(opt, sch), (rule, k, metrics[:k + 1], rec.tolist(),
                                                              torch_fields(opt, sch))
        assert rec[0] == k + 1 and bool(reduced) == (rec[4] != before[4]) == (rec[5] == before[5] + 1)
        assert rec[7] == (k if reduced else before[7])
        assert same_record(rec[6], NAN) if m != m else rec[6] == m
        seen["reductions"] += bool(reduced)
        seen["cooldown"] += bool(before[3] > 0 and not np.isnan(m) and rec[1] == before[1])  # a bad one, not counted
        seen["clamp"] += bool(reduced and rec[4] == rule.min_factor and before[4] * rule.factor < rule.min_factor)
        seen["ignored"] += bool(not reduced and before[2] + 1 > rule.patience and before[3] == 0
                                and rec[1] == before[1] and rec[2] == 0)
    return rec


def test_rule_equals_torch_over_the_sweep_scripted_and_random():
    seen = dict(reductions=0, cooldown=0, clamp=0, ignored=0)
    rules = list(_sweep())
    assert len(rules) == 192
    scripted = [s for s in SCRIPTS.values() if not any(m != m for m in s)]
    randoms = _random_sequences()
    assert len(randoms) == 200 and all(len(s) == 40 for s in randoms)
    assert any(len(set(s)) < len(s) for s in randoms)  # repeated values
    for rule in rules:
        flip = (lambda s: [4.0 - m for m in s]) if rule.monitor == "accuracy" else (lambda s: s)
        for s in scripted:
            _against_torch(rule, flip(s), seen)
        for s in randoms:
            _against_torch(rule, flip(s), seen)
    print("BRANCHES", seen)
    # a vacuous sweep fails: the sequences reduce, suppress evaluations inside a cooldown, clamp at min_factor and
    # ignore a reduction under eps
    assert seen["reductions"] > 1000 and seen["cooldown"] > 1000 and seen["clamp"] > 100 and seen["ignored"] > 100


@pytest.mark.parametrize("name", ["nan_first", "nan_inside"])
@pytest.mark.parametrize("monitor", ["loss", "accuracy"])
def test_rule_equals_torch_on_nan(name, monitor):
    seen = dict(reductions=0, cooldown=0, clamp=0, ignored=0)
    for patience, cooldown in ((0, 0), (1, 0), (1, 1), (2, 2)):
        rule = Plateau(factor=0.5, patience=patience, threshold=0.0, threshold_mode="abs", cooldown=cooldown,
                       monitor=monitor)
        rec = _against_torch(rule, SCRIPTS[name], seen)
        assert np.isfinite(rec[1])  # a NaN is never better: it never becomes the best
    assert seen["reductions"] >= 2


def test_scripted_branches_by_hand():
    # the reduction at bad = patience + 1 and not at patience
    out = run_script(Plateau(factor=0.1, patience=2, threshold=0.0, threshold_mode="abs"), SCRIPTS["patience_edge"])
    assert [(r[2], r[4], r[5]) for r in out] == [(0, 1.0, 0), (1, 1.0, 0), (2, 1.0, 0), (0, 0.1, 1), (1, 0.1, 1),
                                                 (2, 0.1, 1), (0, 0.1 * 0.1, 2)]
    assert [r[7] for r in out] == [-1, -1, -1, 3, 3, 3, 6]
    # a tie is not better
    out = run_script(Plateau(factor=0.5, patience=1, threshold=0.0, threshold_mode="abs"), SCRIPTS["tie"])
    assert [(r[1], r[2], r[4]) for r in out] == [(2.0, 0, 1.0), (2.0, 1, 1.0), (2.0, 0, 0.5), (1.0, 0, 0.5),
                                                 (1.0, 1, 0.5), (1.0, 0, 0.25)]
    # the first evaluation NaN: best stays +inf, the evaluation is a bad one
    out = run_script(Plateau(factor=0.5, patience=1, threshold=0.0, threshold_mode="abs"), SCRIPTS["nan_first"])
    assert out[0][1] == INF and out[0][2] == 1 and same_record(out[0][6], NAN) and out[1][1] == 2.0
    # a cooldown swallows bad evaluations
    out = run_script(Plateau(factor=0.5, patience=0, threshold=0.0, threshold_mode="abs", cooldown=2),
                     SCRIPTS["cooldown"])
    assert [(r[3], r[4]) for r in out] == [(0, 1.0), (2, 0.5), (1, 0.5), (0, 0.5), (2, 0.25), (1, 0.25), (0, 0.25),
                                           (2, 0.125), (1, 0.125)]
    # the clamp at min_factor, then reductions ignored under eps: the count stays, the cooldown restarts
    out = run_script(Plateau(factor=0.5, patience=0, threshold=0.0, threshold_mode="abs", cooldown=1, min_factor=0.2),
                     SCRIPTS["clamp"])
    assert [r[4] for r in out] == [1.0, 0.5, 0.5, 0.25, 0.25, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]
    assert [r[5] for r in out][-8:] == [3.0] * 8 and [r[3] for r in out][-6:] == [1, 0, 1, 0, 1, 0]
    # the rate: lr_t * scale, one rounding; x * 1.0 is x
    for x in (0.0, 0.1, 1e-300, 0.2 * 0.37, 3e38):
        assert cpu().plateau_rate(x, 1.0) == x
    assert cpu().plateau_rate(0.2 * 0.37, 0.1) == (0.2 * 0.37) * 0.1
    assert cpu().plateau_rate(0.1 * 0.7, 0.3) == (0.1 * 0.7) * 0.3 != 0.1 * (0.7 * 0.3)  # the order matters


def test_three_triples_are_summed_in_rank_order_and_bad_arguments():
    rows = np.array([[3.0, 1.0, 1e16], [2.0, 2.0, 1.0], [1.0, 0.0, 1.0]])  # (1e16 + 1) + 1 != 1e16 + (1 + 1)
    rule = Plateau(factor=0.5, patience=0)
    rec, _ = cpu().plateau_decide(np.asarray(start()), rule.native(), rows)
    assert rec[1] == ((1e16 + 1.0) + 1.0) / 6.0 != (1e16 + 2.0) / 6.0
    rec, _ = cpu().plateau_decide(np.asarray(start("accuracy")), Plateau(monitor="accuracy").native(), rows)
    assert rec[1] == 0.5
    rec, _ = cpu().plateau_decide(np.asarray(start()), rule.native(), np.zeros((1, 3)))  # n = 0: the one NaN, a bad one
    assert rec[1] == INF and same_record(rec[6], NAN) and rec[4] == 0.5
    with pytest.raises(ValueError):
        cpu().plateau_decide(np.zeros(7), rule.native(), rows)
    with pytest.raises(ValueError):
        cpu().plateau_decide(np.asarray(start()), rule.native(), np.zeros((0, 3)))
    for bad in ((2, 0.5, 0, 0.0, 0, 0, 0.0, 0.0), (0, 1.0, 0, 0.0, 0, 0, 0.0, 0.0), (0, 0.5, -1, 0.0, 0, 0, 0.0, 0.0),
                (0, 0.5, 0, -1.0, 0, 0, 0.0, 0.0), (0, 0.5, 0, 0.0, 2, 0, 0.0, 0.0), (0, 0.5, 0, 0.0, 0, -1, 0.0, 0.0),
                (0, 0.5, 0, 0.0, 0, 0, 1.5, 0.0), (0, 0.5, 0, 0.0, 0, 0, 0.0, -1.0), (0, 0.5, 0)):
        with pytest.raises(ValueError):
            cpu().plateau_decide(np.asarray(start()), bad, rows)


def test_plateau_dataclass_validates_and_round_trips():
    p = Plateau()
    assert (p.factor, p.patience, p.threshold, p.threshold_mode, p.cooldown, p.min_factor, p.eps, p.monitor) == (
        0.1, 10, 1e-4, "rel", 0, 0.0, 1e-8, "loss")
    assert p.native() == (0, 0.1, 10, 1e-4, 0, 0, 0.0, 1e-8)
    q = Plateau(0.5, 2, 0.25, "abs", 3, 0.2, 0.0, "accuracy")
    assert q.native() == (1, 0.5, 2, 0.25, 1, 3, 0.2, 0.0) and Plateau.from_meta(q.as_meta()) == q
    assert Plateau.from_meta(json.loads(json.dumps(q.as_meta()))) == q and Plateau.from_meta(None) is None
    for bad in (dict(factor=0.0), dict(factor=1.0), dict(patience=-1), dict(patience=1.5), dict(threshold=-1e-3),
                dict(threshold_mode="pct"), dict(cooldown=-1), dict(min_factor=-0.1), dict(min_factor=1.1),
                dict(eps=-1.0), dict(monitor="f1"), dict(threshold=NAN)):
        with pytest.raises(ValueError):
            Plateau(**bad)


# ------------------------------------------------------------------------------------------------ engine
def test_engine_allocates_only_with_a_rule_and_routes_plain_sgd_through_the_apply_launch():
    e = MlpEngine((784, 16, 10), dtype="f64", max_cols=64, device="cpu", backend="torch")
    assert e._plateau is None and not e.uses_apply_launch and e.opt_rec is None and e.opt_last is None
    for call in (e.plateau_state, e.reset_plateau, lambda: e.enqueue_plateau(0), lambda: e.set_plateau_state(start())):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(TypeError):
        e.set_plateau("loss")
    e.set_plateau(None)
    assert e._plateau is None and e.opt_rec is None
    rule = Plateau(factor=0.5, patience=0)
    e.set_plateau(rule)
    rec = e._plateau["rec"]
    assert rec.shape == (8,) and rec.dtype == torch.float64 and e._plateau["rows"] is None
    assert e.uses_apply_launch and e.policy_set and e.opt_rec is not None and e.opt_last is not None
    assert e.plateau_state() == dict(evals=0, best=INF, bad=0, cooldown_left=0, scale=1.0, reductions=0,
                                     last_metric=pytest.approx(NAN, nan_ok=True), last_reduced_index=-1)
    e.set_plateau(rule)  # the same rule: the record is kept
    assert e._plateau["rec"] is rec
    x, y = eval_data(64, 10)
    e.load_eval(x, y)
    for k in range(2):  # the same weights twice: an improvement from +inf, then a tie -> reduced
        e.enqueue_eval(0)
        e.enqueue_plateau(0)
    st = e.plateau_state()
    assert st["evals"] == 2 and st["scale"] == 0.5 and st["reductions"] == 1 and st["last_reduced_index"] == 1
    r = e.read_eval(0)
    assert st["best"] == st["last_metric"] == r["loss_sum"] / r["n"]
    # the update's rate is (lr * f) * scale, reported by last_update
    e.grads.zero_()
    e.apply(0.3)
    assert e.last_update()["lr"] == 0.3 * 0.5 and e.update_count() == 1
    saved = e.plateau_record()
    e.reset_plateau()
    assert e.plateau_state()["scale"] == 1.0 and e.plateau_state()["evals"] == 0
    e.set_plateau_state(saved)
    assert same_record(e.plateau_record(), saved)
    e.set_plateau_state(st)  # ... or the dict
    assert same_record(e.plateau_record(), saved)
    with pytest.raises(ValueError):
        e.set_plateau_state([1.0, 2.0])
    e.set_plateau(None)  # back to the plain update: nothing is left allocated
    assert e._plateau is None and not e.uses_apply_launch and e.opt_rec is None and e.opt_last is None
    e.set_plateau(rule, ranks=3)
    assert e.plateau_rows.shape == (3, 3)
    with pytest.raises(ValueError):
        e.set_plateau(rule, ranks=0)


def test_oracle_lr_scale_is_the_rate_times_the_scale_in_the_apply_launchs_order():
    x, y = eval_data(256, 10)
    sched = Schedule.cosine(8, 0.1)

    def run(lr, **kw):
        nn = NeuralNetwork([784, 16, 10])
        log = []
        mlp.train(nn, x, y, lr, REG, 2, 64, optimizer=Optimizer.adam(), update_log=log, **kw)
        return nn, log

    a, la = run(0.01, schedule=sched, lr_scale=0.3)
    assert [r[1] for r in la] == [(0.01 * f) * 0.3 for f in sched.factors(0, 8)]
    b, lb = run(0.01, schedule=sched)
    assert [r[1] for r in lb] == [0.01 * f for f in sched.factors(0, 8)] and a.W[0].tobytes() != b.W[0].tobytes()
    c, _ = run(0.01, schedule=sched, lr_scale=1.0)  # x * 1.0 is x: bitwise the run without a scale
    for p, q in zip(b.params, c.params):
        assert p.tobytes() == q.tobytes()
    # plain SGD with a scale runs the stateless kSgd rule and keeps an update count, as under a schedule
    st = new_state(None, 0, policy=True)
    d, e = NeuralNetwork([784, 16, 10]), NeuralNetwork([784, 16, 10])
    mlp.train(d, x, y, 0.2, REG, 1, 64, lr_scale=0.5, optim_state=st)
    mlp.train(e, x, y, 0.2 * 0.5, REG, 1, 64, schedule=Schedule.constant())
    assert st["t"] == 4 and all(p.tobytes() == q.tobytes() for p, q in zip(d.params, e.params))
    with pytest.raises(ValueError):
        mlp.train(d, x, y, 0.2, REG, 1, 64, lr_scale=-1.0)
    n, correct, loss_sum = mlp.eval_triple(d, x, y)
    assert n == 256.0 and 0 <= correct <= 256 and loss_sum > 0 and correct == float((mlp.predict(d, x) == y).sum())


# ------------------------------------------------------------------------------------------------ trainer vs twin
@pytest.fixture(scope="module")
def twins():
    """The twin of each configuration, run once and left unchanged."""
    out = {}
    for name in CONFIGS:
        out[name] = run_twin(name, rule_for(name))
        print("TWIN", name, out[name]["scales"], [round(m, 5) for m in out[name]["metrics"]], out[name]["rec"],
              [round(v, 4) for v in margins(out[name], rule_for(name))])
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_torch_trainer_equals_its_twin(twins, name):
    twin = twins[name]
    assert_reduces(twin)
    kw, lr, _ = CONFIGS[name]
    events = []
    tr = make_trainer(rule_for(name), **kw)
    st = tr.train(EPOCHS, lr, REG, eval_every=1)
    assert_matches_twin(tr, twin)
    ref = twin["optim"]
    got = tr.engine.optim_state()
    assert got["t"] == ref["t"] == 4 * EPOCHS and all(a.tobytes() == b.tobytes()
                                                      for a, b in zip(got["state"], ref["state"]))
    assert st.plateau == tr.plateau_state() and st.plateau["reductions"] == int(twin["rec"][5]) >= 2
    assert st.plateau["scale"] == twin["rec"][4] and [e["loss"] for e in st.evals] == twin["metrics"]
    # the last update ran at the scale the twin's last epoch ran at
    sched = kw.get("schedule")
    f = sched.factor(4 * EPOCHS - 1, 4) if sched is not None else 1.0
    assert tr.engine.last_update()["lr"] == (lr * f) * twin["scales"][-1]
    assert tr.native_plan(tr.epoch_plan()) is None
    if name == "sgd":
        assert "plateau" in tr.native_reason
    # where the host looks anyway, the eval events carry the scale after that evaluation's decision
    tr2 = make_trainer(rule_for(name), **kw)
    tr2.train(EPOCHS, lr, REG, eval_every=1, on_event=events.append, log=lambda *_: None)
    assert [e["lr_scale"] for e in events if e["event"] == "eval"] == [r[4] for r in twin["records"]]
    assert_matches_twin(tr2, twin)


def test_accuracy_monitor_equals_its_twin():
    rule = Plateau(factor=0.5, patience=0, threshold=0.05, threshold_mode="abs", monitor="accuracy", cooldown=1)
    twin = run_twin("momentum", rule)
    print("TWIN accuracy", twin["scales"], twin["metrics"], twin["rec"])
    assert twin["rec"][5] >= 1
    kw, lr, _ = CONFIGS["momentum"]
    tr = make_trainer(rule, **kw)
    tr.train(EPOCHS, lr, REG, eval_every=1)
    assert_matches_twin(tr, twin)


# ------------------------------------------------------------------------------------------------ persistence
@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_two_plus_two_equals_train_four(twins, name):
    kw, lr, _ = CONFIGS[name]
    tr = make_trainer(rule_for(name), **kw)
    s1 = tr.train(2, lr, REG, eval_every=1)
    assert s1.plateau["evals"] == 2
    assert_matches_twin(tr, twins[name], 2)
    s2 = tr.train(2, lr, REG, eval_every=1)
    assert s2.plateau["evals"] == 4
    assert_matches_twin(tr, twins[name], 4)
    whole = make_trainer(rule_for(name), **kw)
    whole.train(4, lr, REG, eval_every=1)
    assert same_record(whole.engine.plateau_record(), tr.engine.plateau_record())
    assert torch.equal(whole.engine.params, tr.engine.params)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_a_rule_that_never_fires_changes_nothing(name):
    kw, lr, _ = CONFIGS[name]
    tr = make_trainer(Plateau(factor=0.5, patience=10 ** 6), **kw)
    st = tr.train(3, lr, REG, eval_every=1)
    assert st.plateau["scale"] == 1.0 and st.plateau["reductions"] == 0 and st.plateau["evals"] == 3
    # plain SGD then runs kSgd through the apply launch: bitwise a run under Schedule.constant(); momentum and Adam are
    # bitwise the run without a rule (x * 1.0 is x)
    ref = make_trainer(None, **({**kw, "schedule": Schedule.constant()} if name == "sgd" else kw))
    ref.train(3, lr, REG, eval_every=1)
    assert torch.equal(tr.engine.params, ref.engine.params)
    for a, b in zip(tr.engine.opt_bufs, ref.engine.opt_bufs):
        assert torch.equal(a, b)
    assert ref.engine._plateau is None and len(ref._snapshot()) == len(tr._snapshot()) - 1


def test_keep_best_and_ema_together_with_the_rule(twins):
    kw, lr, _ = CONFIGS["momentum"]
    rule = rule_for("momentum")
    tr = make_trainer(rule, ema=Ema(0.9), **kw)
    st = tr.train(EPOCHS, lr, REG, eval_every=1, keep_best="loss", eval_weights="current")
    # evaluations of the current weights: the parameters and the decisions are the twin's, whatever else is kept
    assert_matches_twin(tr, twins["momentum"])
    assert st.best is not None and st.best["metric"] == min(twins["momentum"]["metrics"])
    assert tr.engine.ema_count() == 4 * EPOCHS
    # evaluations of the averaged weights: the rule acts on what the evaluation read -- the same metric keep-best saw
    av = make_trainer(rule, ema=Ema(0.9), **kw)
    s2 = av.train(EPOCHS, lr, REG, eval_every=1, keep_best="loss")
    assert [e["weights"] for e in s2.evals] == ["ema"] * EPOCHS
    rec = np.asarray(start())
    for e in s2.evals:
        rec, _ = cpu().plateau_decide_metric(rec, rule.native(), e["loss"])
    assert same_record(av.engine.plateau_record(), rec)
    assert s2.plateau["last_metric"] == av.engine.best_state()["last_metric"] == s2.evals[-1]["loss"]


def test_snapshot_and_restore_carry_the_record(twins):
    kw, lr, _ = CONFIGS["momentum"]
    tr = make_trainer(rule_for("momentum"), **kw)
    tr.train(4, lr, REG, eval_every=1)
    snap, it = tr._snapshot(), tr.iter
    rec = tr.engine.plateau_record()
    tr.train(2, lr, REG, eval_every=1)
    assert_matches_twin(tr, twins["momentum"], 6)
    assert not same_record(tr.engine.plateau_record(), rec)
    tr._restore(snap)
    tr.iter = it
    assert same_record(tr.engine.plateau_record(), rec)
    tr.train(2, lr, REG, eval_every=1)  # the recovered epochs repeat their rates
    assert_matches_twin(tr, twins["momentum"], 6)


# ------------------------------------------------------------------------------------------------ loopback ranks
@pytest.mark.parametrize("keep_best", [None, "loss"])
def test_loopback_world3_uneven_shards_decide_like_one_process(keep_best):
    R, epochs = 3, 4
    rule = Plateau(factor=0.5, patience=0, threshold=0.1)
    comms = LoopbackComm.create(R)
    out = [None] * R

    def work(r):
        torch.set_num_threads(1)
        tr = make_trainer(rule, comm=comms[r], batch=126, nval=256)
        triples, recs = [], []
        for _ in range(epochs):
            tr.train(1, 0.2, REG, eval_every=1, keep_best=keep_best)
            triples.append(tr.engine._slot_triple(tr.engine._eval, 0)[0].tolist())
            recs.append(tr.engine.plateau_record().tolist())
        rows = tr.engine.best_rows if keep_best else tr.engine.plateau_rows
        out[r] = dict(shard=tr.engine.eval_samples, triples=triples, recs=recs, agree=tr.replicas_agree(),
                      params=tr.engine.params.clone(), rows=rows.clone(), state=tr.plateau_state())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert [o["shard"] for o in out] == [85, 85, 86]  # uneven validation shards
    rec = np.asarray(start())
    for k in range(epochs):  # the header over the gathered triples, in rank order
        rows = np.asarray([out[r]["triples"][k] for r in range(R)])
        rec, _ = cpu().plateau_decide(rec, rule.native(), rows)
        for r in range(R):
            assert same_record(out[r]["recs"][k], rec)
    assert rec[5] >= 1
    for o in out:
        assert o["agree"] and torch.equal(o["params"], out[0]["params"]) and torch.equal(o["rows"], out[0]["rows"])
        assert np.asarray(o["rows"]).tolist() == [out[r]["triples"][-1] for r in range(R)]


# ------------------------------------------------------------------------------------------------ refusals and the CLI
def test_refusals():
    kw, lr, _ = CONFIGS["momentum"]
    tr = make_trainer(Plateau(), **kw)
    with pytest.raises(ValueError, match="eval_every"):
        tr.train(1, lr, REG)
    from cme213_sp18_amd.parallel import DataParallelTrainer
    bare = DataParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", dtype="f64", batch_size=128,
                               backend="torch", plateau=Plateau(), use_graphs=False)
    bare.load(*eval_data(512, 10))
    with pytest.raises(RuntimeError, match="load_eval"):
        bare.train(1, lr, REG, eval_every=1)  # no validation set
    with pytest.raises(TypeError):
        make_trainer("loss")
    with pytest.raises(ValueError, match="data parallelism"):
        TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch", plateau=Plateau())
    plain = make_trainer(None, **kw)
    st = plain.train(1, lr, REG, eval_every=1)
    assert plain.engine._plateau is None and st.plateau is None and len(plain._snapshot()) == 5
    from cme213_sp18_amd.config import parse_config
    for argv in (["--lr-plateau", "0.5"], ["--eval-every", "1", "--plateau-patience", "2"],
                 ["--lr-plateau", "0.5", "--eval-every", "1", "--parallel", "tp"],
                 ["--lr-plateau", "1.5", "--eval-every", "1"],
                 ["--lr-plateau", "0.5", "--eval-every", "1", "--plateau-patience", "-1"],
                 ["--lr-plateau", "0.5", "--eval-every", "1", "--plateau-threshold-mode", "pct"],
                 ["--lr-plateau", "0.5", "--eval-every", "1", "--plateau-monitor", "f1"],
                 ["--lr-plateau", "0.5", "--eval-every", "1", "--plateau-min-factor", "2"]):
        with pytest.raises(SystemExit):
            parse_config(argv)
    cfg = parse_config(["--lr-plateau", "0.5", "--eval-every", "2", "--plateau-patience", "3", "--plateau-threshold",
                        "0.01", "--plateau-threshold-mode", "abs", "--plateau-cooldown", "1", "--plateau-min-factor",
                        "0.1", "--plateau-monitor", "accuracy"])
    assert cfg.plateau == Plateau(0.5, 3, 0.01, "abs", 1, 0.1, monitor="accuracy")
    assert parse_config([]).plateau is None


def _cli(tmp_path, *args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--backend", "torch", "--dtype", "f64", "-n",
                        "16", "-b", "128", "--num-train", "640", "--num-test", "64", "-l", "0.2", "--optimizer",
                        "momentum", "--outdir", str(tmp_path / "Outputs"), *args],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


FLAGS = ("--eval-every", "1", "--lr-plateau", "0.5", "--plateau-patience", "0", "--plateau-threshold", "0.1")


def test_cli_logs_the_rule_and_the_plateau_event_and_the_sequential_run_follows(tmp_path):
    log = tmp_path / "run.jsonl"
    r = _cli(tmp_path, *FLAGS, "-e", "6", "-s", "--log-json", str(log), "--ckpt-dir", str(tmp_path / "ck"))
    ev = [json.loads(line) for line in log.read_text().splitlines()]
    head = [e for e in ev if e.get("event") == "config"][0]
    assert head["plateau"] == Plateau(0.5, 0, 0.1).as_meta()
    pl = [e for e in ev if e.get("event") == "plateau"]
    evals = [e for e in ev if e.get("event") == "eval"]
    assert len(pl) == 1 and pl[0]["reductions"] >= 2 and pl[0]["scale"] == 0.5 ** pl[0]["reductions"]
    assert len(evals) == 6 and evals[-1]["lr_scale"] == pl[0]["scale"] and evals[0]["lr_scale"] == 1.0
    assert "Plateau rule (loss): scale" in r.stdout and "Sequential plateau rule: scale" in r.stdout
    summary = [e for e in ev if e.get("event") == "summary"][0]
    assert summary["lr_scale"] == pl[0]["scale"] and summary["lr_reductions"] == pl[0]["reductions"]
    assert summary["seq_lr_reductions"] >= 1
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["plateau"]["rule"] == head["plateau"] and meta["plateau"]["record"][4] == pl[0]["scale"]
    assert meta["plateau"]["record"][0] == 6 and meta["plateau"]["record"][5] == pl[0]["reductions"]


def test_cli_checkpoint_record_round_trips_through_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    _cli(tmp_path, *FLAGS, "-e", "4", "--ckpt-dir", whole)
    _cli(tmp_path, *FLAGS, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *FLAGS, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with the plateau rule" not in r.stdout
    a, b = (json.loads((tmp_path / d / "meta.json").read_text())["plateau"] for d in ("whole", "rest"))
    assert same_record(a["record"], b["record"]) and a["rule"] == b["rule"] and a["record"][0] == 4
    assert a["record"][5] >= 1  # the rate was reduced: the resumed half ran at the checkpoint's scale
    za, zb = (np.load(tmp_path / d / "params.npz") for d in ("whole", "rest"))
    for n in ("W0", "W1", "b0", "b1"):
        assert za[n].tobytes() == zb[n].tobytes()
    other = _cli(tmp_path, "--eval-every", "1", "--lr-plateau", "0.1", "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with the plateau rule" in other.stdout
    none = _cli(tmp_path, "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with the plateau rule" in none.stdout
    for bad in (("--lr-plateau", "0.5"), ("--eval-every", "1", "--plateau-cooldown", "1"),
                ("--eval-every", "1", "--lr-plateau", "0.5", "--parallel", "tp")):
        rr = _cli(tmp_path, *bad, "-e", "1", ok=False)
        assert rr.returncode == 2 and "Loaded" not in rr.stdout  # refused when the flags are parsed


# ------------------------------------------------------------------------------------------------ native driver
@pytest.mark.skipif(shutil.which("cmake") is None, reason="cmake not available")
def test_native_plateau_tests_under_asan_ubsan(tmp_path):
    build = tmp_path / "build"
    env = dict(os.environ, TMPDIR=str(tmp_path), NO_COLOR="1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.run(["cmake", "-S", ROOT, "-B", str(build), *gen, "-DCME_SANITIZE=ON", "-DCMAKE_BUILD_TYPE=Debug"],
                   check=True, capture_output=True, env=env, timeout=300)
    subprocess.run(["cmake", "--build", str(build), "-j", "4", "--target", "native_plateau_tests"], check=True,
                   capture_output=True, env=env, timeout=600)
    r = subprocess.run([str(build / "native_plateau_tests")], capture_output=True, text=True, env=env, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert "0 failed" in r.stdout and "5 tests" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
