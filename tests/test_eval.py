"""Evaluation of a resident validation set (MlpEngine.load_eval / enqueue_eval / read_eval and DataParallelTrainer's
load_eval / evaluate / train(eval_every)), everything above the kernel on the torch backend: against the fp64 host
oracle, sharded over LoopbackComm and gloo ranks, and through the CLI's --eval-every."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.launcher import spawn

from .eval_oracle import TOL, check_against_oracle, eval_data, eval_dp_worker, eval_params, oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dt,path,shape,side", [("f64", "mfma", (784, 100, 10), 28),
                                                ("f32", "split3", (784, 100, 47), 28),
                                                ("f32", "mfma", (256, 64, 5), 16)])
def test_torch_evaluate_matches_the_fp64_oracle(dt, path, shape, side):
    P, H, C = shape
    x, y = eval_data(1000, C, side)
    params = eval_params(P, H, C)
    e = MlpEngine(shape, dtype=dt, max_cols=256, device="cpu", backend="torch", path=path)
    e.set_params(*params)
    e.load_eval(x, y, eval_chunk=256, eval_slots=2)
    got = e.evaluate(1)
    ref = oracle(x, y, *params)
    check_against_oracle(got, ref, y, TOL[(dt, path)], f"torch {dt} {shape}")
    # a range of the set, into the other slot; the first slot is untouched and a re-enqueue overwrites
    part = e.evaluate(0, first=100, count=300)
    assert part["n"] == 300
    np.testing.assert_array_equal(part["confusion"].sum(1), np.bincount(y[100:400], minlength=C))
    again = e.read_eval(1)
    assert again["n"] == 1000 and again["loss_sum"] == got["loss_sum"]
    np.testing.assert_array_equal(again["confusion"], got["confusion"])
    one = MlpEngine(shape, dtype=dt, max_cols=256, device="cpu", backend="torch", path=path)
    one.set_params(*params)
    one.load_eval(x, y, eval_chunk=1000)
    single = one.evaluate()
    np.testing.assert_array_equal(single["confusion"], got["confusion"])
    assert single["correct"] == got["correct"]
    assert abs(single["loss_sum"] - got["loss_sum"]) <= 1e-9 * abs(got["loss_sum"])


def test_load_eval_checks_its_inputs():
    x, y = eval_data(64, 10)
    e = MlpEngine((784, 16, 10), dtype="f32", max_cols=64, device="cpu", backend="torch")
    with pytest.raises(RuntimeError):
        e.enqueue_eval(0)
    with pytest.raises(ValueError):
        e.load_eval(x, np.full(64, 10))  # a label outside [0, C)
    with pytest.raises(ValueError):
        e.load_eval(x.astype(np.float32) / 255.0, y)  # the split path keeps raw pixels
    e.load_eval(x, y)
    with pytest.raises(IndexError):
        e.enqueue_eval(1)
    with pytest.raises(IndexError):
        e.enqueue_eval(0, first=60, count=5)


def _trainer(C=10, H=16, comm=None, dtype="f64"):
    nn = NeuralNetwork([784, H, C])
    _, _, W2, b2 = eval_params(784, H, C)
    nn.W[1][...], nn.b[1][...] = W2, b2
    return DataParallelTrainer(nn, comm=comm, device="cpu", dtype=dtype, batch_size=800, backend="torch",
                               use_graphs=False), nn


def test_loopback_world4_uneven_shards_count_every_sample_once():
    C, H, n = 10, 16, 1003
    xv, yv = eval_data(n, C, 28, 5)
    single, nn = _trainer(C, H)
    single.load_eval(xv, yv)
    want = single.evaluate()
    ref = oracle(xv, yv, *nn.params)
    check_against_oracle(dict(n=want["n"], correct=round(want["accuracy"] * n), loss_sum=want["loss"] * n,
                              confusion=want["confusion"]), ref, yv, TOL[("f64", "mfma")], "trainer f64")
    comms = LoopbackComm.create(4)
    out, shards = [None] * 4, [0] * 4

    def work(r):
        torch.set_num_threads(1)
        tr, _ = _trainer(C, H, comms[r])
        tr.load_eval(xv, yv)
        shards[r] = tr.engine.eval_samples
        out[r] = tr.evaluate()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert shards == [250, 251, 251, 251] and sum(shards) == n
    for r in out:
        assert r["n"] == n and r["accuracy"] == want["accuracy"]
        np.testing.assert_array_equal(r["confusion"], want["confusion"])
        assert r["loss"] == out[0]["loss"]  # every rank returns the same record
        assert abs(r["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])  # (fp64 sums of another partition)


def test_gloo_world2_evaluate_and_eval_every(tmp_path):
    C, H, N, n = 10, 16, 1600, 1003
    spawn(eval_dp_worker, 2, args=(str(tmp_path), H, C, N, n), backend="gloo")
    r0, r1 = (np.load(tmp_path / f"eval{r}.npz") for r in range(2))
    assert int(r0["shard"]) + int(r1["shard"]) == n and int(r0["shard"]) == 501
    for k in ("n", "loss", "accuracy", "confusion", "t_loss", "t_conf", "t_iter"):
        np.testing.assert_array_equal(r0[k], r1[k])
    xv, yv = eval_data(n, C, 28, 5)
    single, _ = _trainer(C, H)
    single.load(*eval_data(N, C))
    single.load_eval(xv, yv)
    want = single.evaluate()
    assert int(r0["n"]) == n
    np.testing.assert_array_equal(r0["confusion"], want["confusion"])
    assert abs(float(r0["loss"]) - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert r0["t_conf"].shape == (2, C, C) and list(r0["t_iter"]) == [2, 4]
    assert (r0["t_conf"].sum((1, 2)) == n).all()


def test_train_eval_every_records_equal_evaluate_after_each_epoch():
    C, H = 10, 16
    x, y = eval_data(1600, C)
    xv, yv = eval_data(500, C, 28, 5)
    events = []
    tr, _ = _trainer(C, H)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(4, 0.001, 1e-4, eval_every=2, on_event=events.append, log=lambda *_: None)
    assert [(e["epoch"], e["iter"]) for e in st.evals] == [(1, 4), (3, 8)]
    ev = [e for e in events if e["event"] == "eval"]
    assert [(e["epoch"], e["loss"]) for e in ev] == [(e["epoch"], e["loss"]) for e in st.evals]
    assert all("confusion" not in e for e in ev)
    twin, _ = _trainer(C, H)
    twin.load(x, y)
    twin.load_eval(xv, yv)
    twin.train(2, 0.001, 1e-4)
    want = twin.evaluate()
    assert st.evals[0]["loss"] == want["loss"] and st.evals[0]["n"] == 500
    np.testing.assert_array_equal(st.evals[0]["confusion"], want["confusion"])
    # without a host that looks: the same records, read once at the end
    quiet, _ = _trainer(C, H)
    quiet.load(x, y)
    quiet.load_eval(xv, yv)
    sq = quiet.train(4, 0.001, 1e-4, eval_every=2)
    assert [e["loss"] for e in sq.evals] == [e["loss"] for e in st.evals]
    np.testing.assert_array_equal(sq.evals[1]["confusion"], st.evals[1]["confusion"])


def test_eval_every_zero_enqueues_nothing():
    tr, _ = _trainer()
    tr.load(*eval_data(1600, 10))
    assert tr.train(1, 0.001, 1e-4).evals == []
    tr.load_eval(*eval_data(100, 10, 28, 5))
    assert tr.train(1, 0.001, 1e-4, eval_every=0).evals == []
    bare, _ = _trainer()
    bare.load(*eval_data(1600, 10))
    with pytest.raises(RuntimeError):
        bare.train(1, 0.001, 1e-4, eval_every=1)  # no validation set loaded


def test_cli_eval_every_logs_eval_events(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    log = tmp_path / "run.jsonl"
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16",
                        "-e", "3", "--num-train", "2000", "--num-test", "100", "--eval-every", "1", "--log-json", str(log),
                        "--outdir", str(tmp_path / "Outputs")],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ev = [json.loads(line) for line in log.read_text().splitlines()]
    evals = [e for e in ev if e.get("event") == "eval"]
    assert [e["epoch"] for e in evals] == [0, 1, 2]
    assert all(e["n"] == evals[0]["n"] > 0 and 0.0 <= e["accuracy"] <= 1.0 and np.isfinite(e["loss"]) for e in evals)
    assert r.stdout.count("Validation after epoch") == 3
    assert "Precision on validation set for parallel training" in r.stdout
