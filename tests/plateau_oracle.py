"""Shared by tests/test_plateau.py and tests/test_gpu_plateau.py: the scripted metric sequences of the plateau rule
(csrc/mlp/plateau.h), torch's ReduceLROnPlateau as the rule's reference, the trainer configurations whose runs are
certain to reduce, and the trainer's twin: a trainer WITHOUT the rule run one epoch at a time, evaluated and read on the
host after each, its next epoch run at ``lr * scale`` with the scale torch's scheduler holds."""
import numpy as np
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.optim import Optimizer, Plateau, Schedule

from .eval_oracle import eval_data

NAN = float("nan")
INF = float("inf")
REG, EPOCHS = 1e-4, 6
# name -> (trainer keywords, lr, threshold): plain SGD, momentum, and Adam under a cosine schedule with clipping.
# Reductions are made certain by a large relative threshold with patience 0: an evaluation that does not lower the best
# loss by that fraction counts as a plateau.  The thresholds are set per configuration (on the fp64 torch backend) so
# that within EPOCHS epochs the rate is reduced at least twice AND at least one later evaluation still improves.
CONFIGS = {
    "sgd": (dict(optimizer=None), 0.2, 0.03),
    "momentum": (dict(optimizer=Optimizer("momentum", momentum=0.9)), 0.2, 0.1),
    "adam": (dict(optimizer=Optimizer.adam(), schedule=Schedule.cosine(4 * EPOCHS, 0.1), clip_norm=1.0), 0.01, 0.02),
}


def rule_for(name, **over):
    """The rule of configuration ``name``: factor 0.5 (a power-of-two scale: see run_twin), patience 0."""
    return Plateau(**{**dict(factor=0.5, patience=0, threshold=CONFIGS[name][2], threshold_mode="rel"), **over})

# scripted sequences (loss-like values; the accuracy sweeps negate the ordering by using 4 - m): each hits a branch
SCRIPTS = {
    "nan_first": [NAN, 2.0, 2.0, 2.0],
    "tie": [2.0, 2.0, 2.0, 1.0, 1.0, 1.0],
    "patience_edge": [2.0, 2.5, 2.5, 2.5, 2.5, 2.5, 2.5],
    "cooldown": [2.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0],
    "clamp": [2.0] + [3.0] * 12,
    "nan_inside": [2.0, NAN, 1.5, NAN, NAN, NAN, 1.0],
    "improving": [4.0, 2.0, 1.0, 0.5, 0.25],
}


def same_record(a, b):
    """Bitwise, NaN payloads included."""
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def start(monitor="loss"):
    return [0.0, -INF if monitor == "accuracy" else INF, 0.0, 0.0, 1.0, 0.0, NAN, -1.0]


def torch_scheduler(rule: Plateau):
    """torch's ReduceLROnPlateau on a dummy one-parameter SGD with lr = 1.0: its lr is the rule's scale."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(
        opt, mode="max" if rule.monitor == "accuracy" else "min", factor=rule.factor, patience=rule.patience,
        threshold=rule.threshold, threshold_mode=rule.threshold_mode, cooldown=rule.cooldown, min_lr=rule.min_factor,
        eps=rule.eps)
    return opt, sch


def torch_fields(opt, sch):
    """(scale, best, bad, cooldown_left) as torch holds them."""
    return (float(opt.param_groups[0]["lr"]), float(sch.best), float(sch.num_bad_epochs), float(sch.cooldown_counter))


def record_fields(rec):
    return (float(rec[4]), float(rec[1]), float(rec[2]), float(rec[3]))


def triple_of(metric, n=4.0):
    """A single triple whose loss AND accuracy metric is ``metric`` (exact for the dyadic values of the scripts)."""
    return np.array([[n, n * metric, n * metric]], np.float64)


def run_script(rule: Plateau, metrics):
    """The record after each metric through _cpu.plateau_decide_metric: a list of 8-double lists."""
    rec, out = np.asarray(start(rule.monitor)), []
    for m in metrics:
        rec, _ = cpu().plateau_decide_metric(rec, rule.native(), float(m))
        out.append(rec.tolist())
    return out


def data(ntrain=512, nval=256):
    return eval_data(ntrain, 10), eval_data(nval, 10, 28, 5)


def make_trainer(plateau=None, dtype="f64", H=16, batch=128, device="cpu", backend="torch", comm=None, ntrain=512,
                 nval=256, optimizer=Optimizer("momentum", momentum=0.9), **kw):
    """784-H-10 on 512 training / 256 validation samples, batch 128 (4 steps per epoch)."""
    from cme213_sp18_amd.parallel import DataParallelTrainer

    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), comm=comm, device=device, dtype=dtype, batch_size=batch,
                             backend=backend, optimizer=optimizer, plateau=plateau, **{"use_graphs": False, **kw})
    (x, y), (xv, yv) = data(ntrain, nval)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    return tr


def run_twin(name, rule: Plateau, epochs=EPOCHS, **kw):
    """The twin of configuration ``name``: the same trainer without the rule (plain SGD under Schedule.constant(), so
    that it runs the apply launch's kSgd rule too), one epoch at a time at ``lr * scale``; after each epoch the
    evaluation is read on the host, torch's scheduler takes the decision and _cpu.plateau_decide is checked against it.
    The twin forms (lr * scale) * f where the rule forms (lr * f) * scale: bitwise the same for a power-of-two scale,
    which is why the twins' rules use factor 0.5 and min_factor 0.
    Returns dict(records, metrics, scales (the scale each epoch ran at), params (per epoch), rec)."""
    tkw, lr, _ = CONFIGS[name]
    tkw = dict(tkw)
    if name == "sgd":
        tkw["schedule"] = Schedule.constant()
    tr = make_trainer(None, **{**tkw, **kw})
    opt, sch = torch_scheduler(rule)
    rec = np.asarray(start(rule.monitor))
    out = dict(records=[], metrics=[], scales=[], params=[], lr=lr)
    for _ in range(epochs):
        scale = float(opt.param_groups[0]["lr"])
        out["scales"].append(scale)
        tr.train(1, lr * scale, REG, eval_every=1)
        r = tr.engine.evaluate(0)
        t = np.array([[float(r["n"]), float(r["correct"]), r["loss_sum"]]], np.float64)
        m = float(t[0, 1] / t[0, 0]) if rule.monitor == "accuracy" else float(t[0, 2] / t[0, 0])
        sch.step(m)
        rec, _ = cpu().plateau_decide(rec, rule.native(), t)
        assert record_fields(rec) == torch_fields(opt, sch), (rec.tolist(), torch_fields(opt, sch))
        out["records"].append(rec.tolist())
        out["metrics"].append(m)
        out["params"].append(tr.engine.get_params())
    out.update(rec=rec.tolist(), optim=tr.engine.optim_state())
    return out


def margins(twin, rule):
    """The relative distance of every metric after the first from the threshold it was compared with (loss monitor,
    rel mode): how far the run is from taking another decision."""
    out, best = [], INF
    for m, r in zip(twin["metrics"], twin["records"]):
        if best != INF:
            out.append(abs(m - best * (1.0 - rule.threshold)) / abs(m))
        best = r[1]
    return out


def assert_reduces(twin):
    """Conditions on the twin alone: at least two reductions and at least one improving evaluation after the first, so
    that both branches of the rule act on the run."""
    recs = twin["records"]
    assert recs[-1][5] >= 2.0, recs
    best = [r[1] for r in recs]
    assert any(b < a for a, b in zip(best, best[1:])) or any(b > a for a, b in zip(best, best[1:])), best


def assert_matches_twin(tr, twin, epochs=None):
    """Parameters, optimizer state and the record are bitwise the twin's after ``epochs`` epochs (default: all)."""
    k = len(twin["records"]) if epochs is None else int(epochs)
    assert same_record(tr.engine.plateau_record(), twin["records"][k - 1]), (
        tr.engine.plateau_record().tolist(), twin["records"][k - 1])
    for a, b in zip(tr.engine.get_params(), twin["params"][k - 1]):
        assert a.tobytes() == b.tobytes()
