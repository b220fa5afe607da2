"""Shared by tests/test_best.py and tests/test_gpu_best.py: a Python fp64 re-statement of the keep-best rule
(csrc/mlp/best.h), the configuration whose validation loss is not monotone, the trainer's twin (the same trainer run one
epoch at a time, evaluated and read on the host after each, the rule applied in Python) and the comparison against it."""
import math

import numpy as np

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd.optim import Optimizer

from .eval_oracle import eval_data

NAN = float("nan")
START = [0.0, -1.0, NAN, 0.0, 0.0, -1.0, NAN, 0.0]
LR, REG, EPOCHS = 0.2, 1e-4, 10


def py_metric(triples, monitor):
    """Rank-order sums of {n, correct, loss_sum}, then one division (Python floats are fp64)."""
    n = c = l = 0.0
    for t in triples:
        n, c, l = n + float(t[0]), c + float(t[1]), l + float(t[2])
    num = c if monitor == "accuracy" else l
    m = NAN if n == 0.0 else num / n
    return NAN if m != m else m  # (the header stores every NaN metric as the one quiet NaN)


def py_decide(rec, monitor, min_delta, patience, metric):
    """(record, improved) of one decision; patience None = never stop."""
    evals, bi, bm, bad, stopped, si, _, spare = rec
    improved = False
    if stopped == 0.0:
        if bi < 0:
            improved = not math.isnan(metric)
        elif monitor == "accuracy":
            improved = metric > bm + min_delta
        else:
            improved = metric < bm - min_delta
        if improved:
            bi, bm, bad = evals, metric, 0.0
        else:
            bad += 1.0
            if patience is not None and bad >= patience + 1:
                stopped, si = 1.0, evals
    return [evals + 1.0, bi, bm, bad, stopped, si, metric, spare], improved


def same_record(a, b):
    """Bitwise, NaN payloads included."""
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def data(ntrain=512, nval=256):
    return eval_data(ntrain, 10), eval_data(nval, 10, 28, 5)


def make_trainer(dtype="f64", H=16, batch=128, device="cpu", backend="torch", comm=None, ntrain=512, nval=256, **kw):
    """784-H-10 with momentum 0.9 on 512 training / 256 validation samples, batch 128: at lr 0.2, reg 1e-4 in fp64 the
    validation loss falls for seven epochs and rises for three."""
    from cme213_sp18_amd.parallel import DataParallelTrainer

    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), comm=comm, device=device, dtype=dtype, batch_size=batch,
                             backend=backend, optimizer=Optimizer("momentum", momentum=0.9),
                             **{"use_graphs": False, **kw})
    (x, y), (xv, yv) = data(ntrain, nval)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    return tr


def run_twin(tr, monitor, min_delta=0.0, patience=None, epochs=EPOCHS, lr=LR, reg=REG, **train_kw):
    """``tr`` one epoch at a time: after each, the evaluation and the parameters are read on the host and the rule is
    applied in Python.  Returns dict(records, metrics, triples, params (per epoch), best (the params of the last accepted
    decision or None), rec (the final record))."""
    rec, best = list(START), None
    out = dict(records=[], metrics=[], triples=[], params=[], improved=[])
    for _ in range(epochs):
        tr.train(1, lr, reg, **train_kw)
        r = tr.engine.evaluate(0)
        t = [[float(r["n"]), float(r["correct"]), r["loss_sum"]]]
        m = py_metric(t, monitor)
        rec, imp = py_decide(rec, monitor, min_delta, patience, m)
        p = tr.engine.get_params()
        if imp:
            best = p
        out["records"].append(list(rec))
        out["metrics"].append(m)
        out["triples"].append(t[0])
        out["params"].append(p)
        out["improved"].append(imp)
    out.update(best=best, rec=rec)
    return out


def assert_interior(twin, patience):
    """Conditions on the twin alone: the best is neither the first nor the last evaluation and at least patience + 1
    evaluations follow it, so 'keeps the best, not the last' and 'stops on patience' are both exercised."""
    n = len(twin["metrics"])
    bi = int(twin["rec"][1])
    assert 0 < bi < n - 1, (bi, twin["metrics"])
    assert n - 1 - bi >= patience + 1, (bi, twin["metrics"])


def assert_matches_twin(tr, twin, decisions=None):
    """Every workgroup's record and the best arena are bitwise the twin's after ``decisions`` decisions (default: all)."""
    e = tr.engine
    k = len(twin["records"]) if decisions is None else int(decisions)
    want = twin["records"][k - 1]
    for r in e.best_records():
        assert same_record(r, want), (r.tolist(), want)
    bi = int(want[1])
    best = twin["params"][bi] if bi >= 0 else None
    got = e.best_params()
    assert (got is None) == (best is None)
    if got is not None:
        for a, b in zip(got, best):
            assert a.tobytes() == b.tobytes()
