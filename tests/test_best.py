"""Keeping the best validation weights and stopping on patience (csrc/mlp/best.h, MlpEngine.enable_keep_best /
enqueue_keep_best, DataParallelTrainer.train(keep_best=...), the CLI's --keep-best), everything above the kernel on the
torch backend: the rule over scripted metric sequences against a Python re-statement, the trainer against its twin (the
same trainer run one epoch at a time and read on the host), loopback ranks, the CLI, checkpoints and the native driver."""
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
from cme213_sp18_amd.parallel import LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer

from .best_oracle import (EPOCHS, LR, NAN, REG, START, assert_interior, assert_matches_twin, make_trainer, py_decide,
                          py_metric, run_twin, same_record)
from .eval_oracle import eval_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"loss": 0, "accuracy": 1}


def _both(rec, monitor, min_delta, patience, triples):
    """One decision through the binding and through the Python re-statement: they must agree bitwise."""
    got, imp = cpu().best_decide(np.asarray(rec, np.float64), CODE[monitor], min_delta,
                                 -1 if patience is None else patience, np.asarray(triples, np.float64).reshape(-1, 3))
    want, wimp = py_decide(list(rec), monitor, min_delta, patience, py_metric(triples, monitor))
    assert same_record(got, want) and bool(imp) == wimp, (got.tolist(), want)
    return list(got), bool(imp)


def _script(monitor, min_delta, patience, metrics):
    """Metrics as single triples with n = 4 (loss_sum = 4 m, correct = 4 m: exact for the dyadic values used)."""
    rec, out = list(START), []
    for m in metrics:
        t = [[0.0, 0.0, 0.0]] if m == "empty" else [[4.0, 4.0 * m, 4.0 * m]]
        rec, imp = _both(rec, monitor, min_delta, patience, t)
        out.append((imp, int(rec[1]), int(rec[3]), int(rec[4]), int(rec[5])))
    return rec, out


# ------------------------------------------------------------------------------------------------ the rule
def test_start_record_and_first_evaluation():
    assert same_record(cpu().best_start(), START)
    rec, out = _script("loss", 0.0, None, [2.0])
    assert out == [(True, 0, 0, 0, -1)] and rec[0] == 1.0 and rec[2] == 2.0 and rec[6] == 2.0


def test_loss_sequence_ties_nan_patience_two_and_improvement_after_the_stop():
    # improve, worse, tie, improve, NaN, worse, worse (stop), improve (ignored)
    rec, out = _script("loss", 0.0, 2, [2.0, 2.5, 2.0, 1.5, NAN, 1.75, 1.5, 0.5])
    assert out == [(True, 0, 0, 0, -1), (False, 0, 1, 0, -1), (False, 0, 2, 0, -1), (True, 3, 0, 0, -1),
                   (False, 3, 1, 0, -1), (False, 3, 2, 0, -1), (False, 3, 3, 1, 6), (False, 3, 3, 1, 6)]
    assert rec[0] == 8.0 and rec[2] == 1.5 and rec[6] == 0.5  # evals and last_metric advance after the stop


@pytest.mark.parametrize("monitor,seq,want", [
    # min_delta 0.25: smaller than, equal to (strict: no) and larger than min_delta
    ("accuracy", [0.25, 0.375, 0.5, 0.75, 0.75], [True, False, False, True, False]),
    ("loss", [1.0, 0.875, 0.75, 0.5, 0.5], [True, False, False, True, False])])
def test_min_delta_is_strict_for_both_monitors(monitor, seq, want):
    _, out = _script(monitor, 0.25, None, seq)
    assert [o[0] for o in out] == want and out[-1][1] == 3


def test_nan_first_empty_set_and_patience_zero_and_none():
    _, out = _script("loss", 0.0, None, [NAN, "empty", 3.0])
    assert out == [(False, -1, 1, 0, -1), (False, -1, 2, 0, -1), (True, 2, 0, 0, -1)]
    _, out = _script("accuracy", 0.0, 0, [0.5, 0.75, 0.75, 1.0])  # patience 0: the first non-improving one stops
    assert out == [(True, 0, 0, 0, -1), (True, 1, 0, 0, -1), (False, 1, 1, 1, 2), (False, 1, 1, 1, 2)]
    _, out = _script("loss", 0.0, 0, ["empty", 1.0])  # n = 0 before any best: a bad evaluation too
    assert out == [(False, -1, 1, 1, 0), (False, -1, 1, 1, 0)]
    _, out = _script("loss", 0.0, None, [1.0] + [2.0] * 30)  # no patience: never stops
    assert out[-1] == (False, 0, 30, 0, -1)


def test_three_triples_are_summed_in_rank_order():
    rows = [[3.0, 1.0, 1e16], [2.0, 2.0, 1.0], [1.0, 0.0, 1.0]]  # (1e16 + 1) + 1 != 1e16 + (1 + 1)
    rec, imp = _both(START, "loss", 0.0, None, rows)
    assert imp and rec[2] == ((1e16 + 1.0) + 1.0) / 6.0 != (1e16 + 2.0) / 6.0
    rec, _ = _both(START, "accuracy", 0.0, None, rows)
    assert rec[2] == 0.5
    with pytest.raises(ValueError):
        cpu().best_decide(np.zeros(7), 0, 0.0, -1, np.zeros((1, 3)))
    with pytest.raises(ValueError):
        cpu().best_decide(np.asarray(START), 2, 0.0, -1, np.zeros((1, 3)))
    with pytest.raises(ValueError):
        cpu().best_decide(np.asarray(START), 0, -1.0, -1, np.zeros((1, 3)))


# ------------------------------------------------------------------------------------------------ engine
def test_engine_api_allocates_only_when_enabled():
    e = MlpEngine((784, 16, 10), dtype="f64", max_cols=64, device="cpu", backend="torch")
    assert e._best is None
    for call in (e.best_state, e.best_params, e.restore_best, e.reset_best, lambda: e.enqueue_keep_best(0)):
        with pytest.raises(RuntimeError):
            call()
    e.enable_keep_best("loss", 0.0, 2)
    arena = e._best["arena"]
    assert arena.numel() == e.layout.status and arena.dtype == e.params.dtype
    e.enable_keep_best("loss", 0.0, 2)  # the same rule: a no-op
    assert e._best["arena"] is arena
    assert e.best_params() is None and e.best_state()["best_index"] == -1
    with pytest.raises(RuntimeError):
        e.restore_best()  # no best yet
    x, y = eval_data(64, 10)
    e.load_eval(x, y)
    e.enqueue_eval(0)
    e.enqueue_keep_best(0)
    with pytest.raises(RuntimeError):
        e.enable_keep_best("accuracy")  # another rule without reset_best()
    st = e.best_state()
    assert st["evals"] == 1 and st["best_index"] == 0 and st["monitor"] == "loss" and st["patience"] == 2
    for a, b in zip(e.best_params(), e.get_params()):
        np.testing.assert_array_equal(a, b)
    e.reset_best()
    assert e.best_params() is None
    e.enable_keep_best("accuracy", 0.5)
    assert e.best_state()["monitor"] == "accuracy" and e.best_state()["min_delta"] == 0.5
    for bad in (dict(monitor="f1"), dict(min_delta=-1.0), dict(patience=-1)):
        with pytest.raises(ValueError):
            MlpEngine((784, 16, 10), dtype="f64", device="cpu", backend="torch").enable_keep_best(**bad)


# ------------------------------------------------------------------------------------------------ trainer vs twin
@pytest.fixture(scope="module")
def twins():
    """The twin of each monitor, run once (patience 2) and left unchanged."""
    return {m: run_twin(make_trainer(), m, 0.0, 2) for m in ("loss", "accuracy")}


@pytest.mark.parametrize("monitor", ["loss", "accuracy"])
def test_torch_trainer_equals_its_twin(twins, monitor):
    twin = twins[monitor]
    print("TWIN", monitor, [round(m, 4) for m in twin["metrics"]], twin["rec"])
    if monitor == "loss":
        assert_interior(twin, 2)
        assert int(twin["rec"][1]) == 6 and int(twin["rec"][5]) == 9 and twin["rec"][4] == 1.0
    else:
        assert 0 < int(twin["rec"][1]) < EPOCHS - 1
    tr = make_trainer()
    st = tr.train(EPOCHS, LR, REG, eval_every=1, keep_best=monitor, patience=2)
    assert_matches_twin(tr, twin)
    bi = int(twin["rec"][1])
    assert st.best["index"] == bi == st.best["epoch"] and st.best["iter"] == 4 * (bi + 1)
    assert st.best["metric"] == twin["metrics"][bi] == st.best[monitor] and st.best["monitor"] == monitor
    assert st.stopped == bool(twin["rec"][4]) and st.stop_index == int(twin["rec"][5])
    assert st.steps == 4 * EPOCHS  # nobody looked: every epoch ran
    # train() never restores by itself: nn holds the last epoch's weights
    np.testing.assert_array_equal(tr.nn.W[1], twin["params"][-1][2])


def test_patience_one_stops_at_eight_and_the_blind_epoch_cannot_replace_the_best(twins):
    twin = run_twin(make_trainer(), "loss", 0.0, 1)
    assert int(twin["rec"][1]) == 6 and int(twin["rec"][5]) == 8 and twin["rec"][0] == 10.0
    tr = make_trainer()
    st = tr.train(EPOCHS, LR, REG, eval_every=1, keep_best="loss", patience=1)
    assert_matches_twin(tr, twin)
    assert st.stopped and st.stop_index == 8 and st.steps == 4 * EPOCHS
    # ... and exactly the best weights of a run that had stopped there
    short = make_trainer()
    short.train(9, LR, REG, eval_every=1, keep_best="loss", patience=1)
    for a, b in zip(short.engine.best_params(), tr.engine.best_params()):
        assert a.tobytes() == b.tobytes()
    assert same_record(short.engine.best_records()[0][1:6], tr.engine.best_records()[0][1:6])


def test_train_five_plus_five_equals_train_ten(twins):
    tr = make_trainer()
    s1 = tr.train(5, LR, REG, eval_every=1, keep_best="loss", patience=2)
    assert s1.best["index"] == 4 and s1.best["epoch"] == 4 and not s1.stopped
    s2 = tr.train(5, LR, REG, eval_every=1, keep_best="loss", patience=2)
    assert_matches_twin(tr, twins["loss"])
    assert s2.best["index"] == 6 and s2.best["epoch"] == 1 and s2.best["iter"] == 28 and s2.stopped
    # a best that dates from an earlier call: no epoch in this one
    s3 = tr.train(1, LR, REG, eval_every=1, keep_best="loss", patience=2)
    assert s3.best["index"] == 6 and s3.best["epoch"] is None and s3.best["iter"] == 28 and s3.best["loss"] is None
    with pytest.raises(RuntimeError):
        tr.train(1, LR, REG, eval_every=1, keep_best="accuracy")  # another rule without reset_best()


def test_restore_best_makes_nn_and_predict_those_of_the_best_epoch(twins):
    twin = twins["loss"]
    tr = make_trainer()
    with pytest.raises(RuntimeError):
        tr.restore_best()
    tr.train(EPOCHS, LR, REG, eval_every=1, keep_best="loss", patience=2)
    it = tr.iter
    rec = tr.restore_best()
    assert rec["best_index"] == 6 and rec["iter"] == 28 and tr.iter == it
    best = twin["params"][6]
    for got, want in zip((tr.nn.W[0], tr.nn.b[0], tr.nn.W[1], tr.nn.b[1]), best):
        assert np.asarray(got).tobytes() == want.tobytes()
    for got, want in zip(tr.engine.get_params(), best):
        assert got.tobytes() == want.tobytes()
    ref = make_trainer()
    ref.engine.set_params(*best)
    xv, _ = eval_data(256, 10, 28, 5)
    np.testing.assert_array_equal(tr.predict(xv), ref.predict(xv))
    assert (tr.predict(xv) != make_trainer().predict(xv)).any()


def test_stop_check_every_returns_after_the_stop_epoch(twins):
    tr = make_trainer()
    st = tr.train(EPOCHS + 5, LR, REG, eval_every=1, keep_best="loss", patience=1, stop_check_every=1)
    assert st.stopped and st.stop_index == 8 and st.steps == 4 * 9 and tr.iter == 36 and len(st.evals) == 9
    blind = make_trainer()
    blind.train(EPOCHS, LR, REG, eval_every=1, keep_best="loss", patience=1)
    for a, b in zip(tr.engine.best_params(), blind.engine.best_params()):
        assert a.tobytes() == b.tobytes()
    assert tr.best_state()["best_index"] == blind.best_state()["best_index"] == 6
    # every second evaluated epoch: the flag of evaluation 8 is seen after evaluation 9
    two = make_trainer()
    s2 = two.train(EPOCHS + 5, LR, REG, eval_every=1, keep_best="loss", patience=1, stop_check_every=2)
    assert s2.stopped and s2.steps == 4 * 10
    # a host that looks at every epoch anyway (on_event) needs no stop_check_every
    ev = make_trainer()
    s3 = ev.train(EPOCHS + 5, LR, REG, eval_every=1, keep_best="loss", patience=1, on_event=lambda r: None,
                  log=lambda *_: None)
    assert s3.stopped and s3.steps == 4 * 9


def test_refusals():
    tr = make_trainer()
    with pytest.raises(ValueError):
        tr.train(1, LR, REG, keep_best="loss")  # no eval_every
    with pytest.raises(ValueError):
        tr.train(1, LR, REG, eval_every=1, patience=2)  # no keep_best
    with pytest.raises(ValueError):
        tr.train(1, LR, REG, eval_every=1, keep_best="f1")
    assert tr.engine._best is None
    st = tr.train(1, LR, REG, eval_every=1)
    assert tr.engine._best is None and st.best is None and not st.stopped and len(tr._snapshot()) == 5
    tp = TensorParallelTrainer(NeuralNetwork([784, 16, 10]), device="cpu", backend="torch")
    with pytest.raises(ValueError, match="data parallelism"):
        tp.train(1, LR, REG, keep_best="loss")
    from cme213_sp18_amd.config import parse_config
    for argv in (["--keep-best", "loss"], ["--eval-every", "1", "--patience", "2"],
                 ["--eval-every", "1", "--restore-best"], ["--eval-every", "1", "--min-delta", "0.1"],
                 ["--eval-every", "1", "--stop-check-every", "1"],
                 ["--keep-best", "loss", "--eval-every", "1", "--parallel", "tp"],
                 ["--keep-best", "loss", "--eval-every", "1", "--patience", "-1"],
                 ["--keep-best", "f1", "--eval-every", "1"]):
        with pytest.raises(SystemExit):
            parse_config(argv)
    cfg = parse_config(["--keep-best", "accuracy", "--eval-every", "2", "--patience", "0", "--min-delta", "0.01",
                        "--stop-check-every", "3", "--restore-best"])
    assert (cfg.keep_best, cfg.patience, cfg.min_delta, cfg.stop_check_every, cfg.restore_best) == (
        "accuracy", 0, 0.01, 3, True)
    assert parse_config([]).keep_best == "" and parse_config([]).patience is None


def test_snapshot_and_restore_carry_the_best(twins):
    tr = make_trainer()
    tr.train(7, LR, REG, eval_every=1, keep_best="loss", patience=2)
    snap = tr._snapshot()
    rec, best, iters = tr.engine.best_records(), tr.engine.best_params(), list(tr._best_iters)
    tr.train(3, LR, REG, eval_every=1, keep_best="loss", patience=2)
    tr.engine._best["arena"].add_(1.0)
    tr._restore(snap)
    assert same_record(tr.engine.best_records(), rec) and tr._best_iters == iters
    for a, b in zip(tr.engine.best_params(), best):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ loopback ranks
def test_loopback_world3_uneven_shards_decide_alike():
    R, epochs = 3, 4
    comms = LoopbackComm.create(R)
    out = [None] * R

    def work(r):
        torch.set_num_threads(1)
        tr = make_trainer(comm=comms[r], batch=126, nval=256)
        triples, recs = [], []
        for _ in range(epochs):
            tr.train(1, LR, REG, eval_every=1, keep_best="loss", patience=0)
            triples.append(tr.engine._slot_triple(tr.engine._eval, 0)[0].tolist())
            recs.append(tr.engine.best_records()[0].tolist())
        out[r] = dict(shard=tr.engine.eval_samples, triples=triples, recs=recs, agree=tr.replicas_agree(),
                      arena=tr.engine._best["arena"].clone(), params=tr.engine.params.clone(),
                      rows=tr.engine.best_rows.clone(), state=tr.best_state())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert [o["shard"] for o in out] == [85, 85, 86]  # uneven validation shards
    rec = list(START)
    for k in range(epochs):  # the header over the gathered triples, in rank order
        rows = [out[r]["triples"][k] for r in range(R)]
        rec, _ = cpu().best_decide(np.asarray(rec), 0, 0.0, 0, np.asarray(rows))
        for r in range(R):
            assert same_record(out[r]["recs"][k], rec)
    for o in out:
        assert o["agree"] and torch.equal(o["arena"], out[0]["arena"]) and torch.equal(o["rows"], out[0]["rows"])
        assert o["state"] == out[0]["state"] and o["state"]["iter"] is not None
    assert int(rec[1]) >= 0 and np.asarray(out[0]["rows"]).tolist() == [out[r]["triples"][-1] for r in range(R)]


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


def test_cli_keep_best_logs_the_best_event_and_restores(tmp_path):
    log = tmp_path / "run.jsonl"
    r = _cli(tmp_path, "-e", "6", "--eval-every", "1", "--keep-best", "loss", "--patience", "1", "--restore-best",
             "--log-json", str(log), "--ckpt-dir", str(tmp_path / "ck"))
    ev = [json.loads(line) for line in log.read_text().splitlines()]
    best = [e for e in ev if e.get("event") == "best"]
    evals = [e for e in ev if e.get("event") == "eval"]
    assert len(best) == 1 and best[0]["restored"] is True and best[0]["monitor"] == "loss"
    losses = [e["loss"] for e in evals]
    bi = best[0]["index"]
    assert best[0]["metric"] == losses[bi] == min(losses[:bi + 1]) and best[0]["iter"] == evals[bi]["iter"]
    stops = [e for e in ev if e.get("event") == "early_stop"]
    assert len(stops) == int(best[0]["stopped"])
    if stops:  # (--log-json makes the host look at every epoch: the run ends at the stop epoch)
        assert stops[0]["stop_index"] == len(evals) - 1 and stops[0]["epochs_run"] == len(evals)
    assert "Best evaluation: index" in r.stdout
    # --restore-best: the final checkpoint holds the best weights, which are also under best/
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["best"]["monitor"] == "loss" and meta["best"]["patience"] == 1 and meta["best"]["record"][1] == bi
    assert meta["best"]["iter"] == best[0]["iter"]
    from cme213_sp18_amd.utils.checkpoint import load_raw_ascii
    z = np.load(tmp_path / "ck" / "params.npz")
    np.testing.assert_array_equal(load_raw_ascii(str(tmp_path / "ck" / "best" / "W0.mat")), z["W0"])
    np.testing.assert_array_equal(load_raw_ascii(str(tmp_path / "ck" / "best" / "b1.mat")).ravel(), z["b1"])


def test_cli_checkpoint_best_round_trips_through_resume(tmp_path):
    flags = ("--eval-every", "1", "--keep-best", "accuracy", "--patience", "3")
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole)
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with keep-best" not in r.stdout
    a, b = (json.loads((tmp_path / d / "meta.json").read_text())["best"] for d in ("whole", "rest"))
    assert a == b and a["record"][0] == 4 and len(a["iters"]) == 4
    for n in ("W0", "W1", "b0", "b1"):
        assert (tmp_path / "whole" / "best" / f"{n}.mat").read_bytes() == (
            tmp_path / "rest" / "best" / f"{n}.mat").read_bytes()
    other = _cli(tmp_path, "--eval-every", "1", "--keep-best", "loss", "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with keep-best" in other.stdout
    for bad in (("--keep-best", "loss"), ("--eval-every", "1", "--patience", "1"),
                ("--eval-every", "1", "--keep-best", "loss", "--parallel", "tp")):
        rr = _cli(tmp_path, *bad, "-e", "1", ok=False)
        assert rr.returncode == 2 and "Loaded" not in rr.stdout  # refused when the flags are parsed


# ------------------------------------------------------------------------------------------------ native driver
@pytest.mark.skipif(shutil.which("cmake") is None, reason="cmake not available")
def test_native_best_tests_under_asan_ubsan(tmp_path):
    build = tmp_path / "build"
    env = dict(os.environ, TMPDIR=str(tmp_path), NO_COLOR="1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.run(["cmake", "-S", ROOT, "-B", str(build), *gen, "-DCME_SANITIZE=ON", "-DCMAKE_BUILD_TYPE=Debug"],
                   check=True, capture_output=True, env=env, timeout=300)
    subprocess.run(["cmake", "--build", str(build), "-j", "4", "--target", "native_best_tests"], check=True,
                   capture_output=True, env=env, timeout=600)
    r = subprocess.run([str(build / "native_best_tests")], capture_output=True, text=True, env=env, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    assert "0 failed" in r.stdout and "4 tests" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
