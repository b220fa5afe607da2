"""An exponential moving average of the weights on the GPU: the kernel (csrc/mlp/ema.hip) bitwise against the header on
the host (_cpu.ema_step), the skip words, graph replay, the hip trainer against the host recurrence over an eager twin's
per-step parameters, averaged evaluations against a fresh engine and the fp64 oracle, keep-best over averaged
evaluations, snapshots, and two ranks sharing the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd._native import cpu, hip
from cme213_sp18_amd.optim import Optimizer
from cme213_sp18_amd.parallel import MlpEngine
from tests.best_oracle import START, data, py_decide, py_metric, same_record
from tests.ema_workers import LR, REG, RULE, average, live, make_trainer, recurrence, same, twin_steps
from tests.eval_oracle import TOL, check_against_oracle, oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2048 * 256 * 4 + 3  # past the 2048-workgroup cap: the grid-stride loop wraps and a scalar tail is left
GUARD = 16                # sentinel elements behind the average: nothing may be written past `count`
DECAY = 0.999


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Problem:
    """Device buffers of one kernel problem: parameters, the average (+ sentinels), one record per workgroup, and the
    host's copy of the average and the count."""

    def __init__(self, tdt, count, offset, warmup):
        self.tdt, self.count, self.warmup = tdt, count, bool(warmup)
        self.ndt = np.float32 if tdt == torch.float32 else np.float64
        self.rng = np.random.default_rng(count + offset)
        # offset != 0: both buffers start `offset` elements past their allocation (16-byte misaligned: scalar path)
        self.p = torch.zeros(count + offset, dtype=tdt, device="cuda")[offset:]
        self.ebuf = torch.full((count + offset + GUARD,), -7.0, dtype=tdt, device="cuda")
        self.e = self.ebuf[offset:offset + count]
        self.guard = self.ebuf[offset + count:]
        self.he = self.rng.standard_normal(count).astype(self.ndt)
        self.e.copy_(torch.from_numpy(self.he))
        self.nrec = int(hip().ema_grid(count))
        self.rec = torch.zeros(self.nrec, 4, dtype=torch.float64, device="cuda")
        self.t = 0
        self.status = torch.zeros(1, dtype=tdt, device="cuda")
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def fresh_params(self):
        h = (self.he + self.rng.standard_normal(self.count) * 0.01).astype(self.ndt)
        h[::5] = self.he[::5]  # fixed points
        self.p.copy_(torch.from_numpy(h))
        return h

    def launch(self, status=True, err=True):
        hip().mlp_ema_step(0 if self.tdt == torch.float32 else 1, DECAY, int(self.warmup), self.p.data_ptr(),
                           self.e.data_ptr(), self.count, self.rec.data_ptr(), self.nrec,
                           self.status.data_ptr() if status else 0, self.err.data_ptr() if err else 0, _stream())

    def host(self, hp):
        d = cpu().ema_decay(DECAY, self.warmup, self.t)
        self.t = cpu().ema_step(self.he, hp, DECAY, self.warmup, self.t)
        return d

    def check(self, d):
        torch.cuda.synchronize()
        rec = self.rec.cpu().numpy()
        want = np.array([float(self.t), d, 0.0, 0.0])
        for w in range(self.nrec):  # EVERY workgroup's record
            assert same_record(rec[w], want), (w, rec[w].tolist(), want.tolist())
        assert np.array_equal(self.e.cpu().numpy().view(np.uint8), self.he.view(np.uint8))
        assert bool((self.guard == -7.0).all())


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("count", [1, 255, 257, BIG])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_kernel_is_bitwise_the_header_over_five_updates(tdt, count, offset, warmup):
    pr = Problem(tdt, count, offset, warmup)
    assert (pr.p.data_ptr() % 16 != 0) == bool(offset) and (pr.e.data_ptr() % 16 != 0) == bool(offset)
    assert pr.nrec == min(2048, -(-count // 1024))
    for k in range(5):
        hp = pr.fresh_params()
        pr.launch(status=bool(k % 2), err=bool(k & 2))  # (zero skip words, given or not, change nothing)
        pr.check(pr.host(hp))
    assert pr.t == 5


@pytest.mark.parametrize("tdt,count,offset", [(torch.float32, 257, 0), (torch.float64, 5000, 1),
                                              (torch.float32, BIG, 0)])
def test_a_set_skip_word_leaves_the_average_and_every_record_alone(tdt, count, offset):
    pr = Problem(tdt, count, offset, True)
    hp = pr.fresh_params()
    pr.launch()
    d = pr.host(hp)
    pr.check(d)
    pr.fresh_params()
    pr.status.fill_(1.0)
    pr.launch()
    pr.check(d)  # the status element: nothing moved, no record advanced
    pr.status.zero_()
    pr.err.fill_(3)
    pr.launch()
    pr.check(d)  # the sticky hand-off word
    pr.launch(err=False)  # the same launch without that word applies
    pr.check(pr.host(pr.p.cpu().numpy()))
    assert pr.t == 2


def test_launcher_refuses_what_an_index_depends_on():
    p = torch.zeros(64, device="cuda")
    e = torch.zeros(64, device="cuda")
    rec = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    ok = dict(dt=0, decay=0.5, warmup=0, params=p.data_ptr(), ema=e.data_ptr(), count=64, rec=rec.data_ptr(), nrec=1)
    hip().mlp_ema_step(**ok)
    for bad in (dict(nrec=2), dict(count=0), dict(dt=2), dict(decay=1.0), dict(decay=-0.1), dict(ema=0), dict(rec=0),
                dict(ema=p.data_ptr()), dict(params=p.data_ptr() + 2), dict(err=p.data_ptr() + 2)):
        with pytest.raises(ValueError):
            hip().mlp_ema_step(**{**ok, **bad})
    torch.cuda.synchronize()
    assert float(rec[0, 0]) == 1.0 and float(rec[1:].abs().sum()) == 0.0


def test_three_captured_replays_equal_three_eager_launches():
    a, b = Problem(torch.float32, 5000, 0, True), Problem(torch.float32, 5000, 0, True)
    b.launch()  # (the kernel is loaded before the capture; b's state is put back)
    torch.cuda.synchronize()
    b.e.copy_(a.e)
    b.rec.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.launch()
    torch.cuda.synchronize()
    assert float(a.rec.abs().sum()) == 0.0  # a capture runs nothing
    for _ in range(3):
        hp = a.fresh_params()
        b.p.copy_(a.p)
        g.replay()
        b.launch()
        d = a.host(hp)
        a.check(d)
        assert torch.equal(a.e, b.e) and torch.equal(a.rec, b.rec)
    assert a.t == 3


# ------------------------------------------------------------------------------------------------ the hip trainer
def _hip_trainer(dtype, opt="sgd", executor="graph", H=100, **kw):
    return make_trainer(opt, dtype=dtype, H=H, device="cuda", backend="hip", use_graphs=True, executor=executor, **kw)


_TWINS: dict = {}


def _twin(dtype, opt):
    """Computed once, shared, left unchanged: the start, the per-step parameters of an eager trainer without averaging
    over 3 epochs, and the parameters of a graph-replayed trainer without averaging after them."""
    if (dtype, opt) not in _TWINS:
        tw = _hip_trainer(dtype, opt, "eager", ema=None)
        e0 = live(tw)
        seq = twin_steps(tw, 3, LR)
        g = _hip_trainer(dtype, opt, "graph", ema=None)
        g.train(3, LR, REG)
        _TWINS[dtype, opt] = dict(e0=e0, seq=seq, graph=live(g))
    return _TWINS[dtype, opt]


@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
@pytest.mark.parametrize("dtype,opt", [("f32", "sgd"), ("bf16", "sgd"), ("f64", "sgd"), ("f32", "momentum")])
def test_hip_trainer_parameters_are_untouched_and_the_average_is_the_host_recurrence(dtype, opt, executor):
    """784-100-10, batch 128, 512 samples, 3 epochs: f32 (split3), bf16 and f64 with plain SGD -- the fused step plus
    the averaging launch, replayed from the epoch graph -- and f32 with momentum (gradient mode + apply + the launch)."""
    tw = _twin(dtype, opt)
    tr = _hip_trainer(dtype, opt, executor)
    assert tr.native_plan(tr.epoch_plan()) is None and "averag" in tr.native_reason
    tr.train(3, LR, REG)
    torch.cuda.synchronize()
    assert same(live(tr), tw["graph"])
    assert same(tw["seq"][-1], tw["graph"])
    want, t = recurrence(tw["e0"], tw["seq"], RULE)
    assert t == 12 and same(average(tr), want)
    for r in tr.engine.ema_records():
        assert r[0] == 12.0 and r[1] == RULE.decay_at(11)
    assert not same(want, tw["graph"])


def test_without_ema_native_plan_is_what_it_was():
    tr = _hip_trainer("f32", "sgd", "auto", ema=None)
    # consecutive full batches on the fused single-process path: the native loop takes the plan
    assert tr.engine._ema is None and tr.native_plan(tr.epoch_plan()) == (0, 4) and tr.native_reason == ""
    tr.train(1, LR, REG)  # (the native loop: its sums are the pipeline's own, not compared with the two-launch step's)
    assert tr.engine._ema is None and tr.native_reason == ""
    g = _hip_trainer("f32", "sgd", "graph", ema=None)
    assert g.native_plan(g.epoch_plan()) is None and g.native_reason == ""
    m = _hip_trainer("f32", "momentum", "auto", ema=None)
    assert m.native_plan(m.epoch_plan()) is None and "stateful optimizer" in m.native_reason


# ------------------------------------------------------------------------------------------------ averaged evaluation
def _fresh(tr, weights):
    (x, y), (xv, yv) = data()
    e = tr.engine
    f = MlpEngine((e.P, e.H, e.C), e.dtype, max_cols=128, device="cuda", backend="hip", path=e.path)
    f.load_dataset(x, y)
    f.set_params(*weights)
    f.load_eval(xv, yv)
    return f


def _same_eval(a, b):
    assert a["n"] == b["n"] and a["correct"] == b["correct"]
    assert np.float64(a["loss_sum"]).tobytes() == np.float64(b["loss_sum"]).tobytes()
    np.testing.assert_array_equal(a["confusion"], b["confusion"])


def _within_tol(got, ref, lab, tol, tag):
    """bf16 only (fp32 and fp64 go through eval_oracle.check_against_oracle whole).  Within eval_oracle.TOL of the fp64
    oracle, by the formulas of check_against_oracle: n exact, the
    confusion row sums equal the label histogram, trace == correct, the mean loss within bound = tol . max|z2| of the
    oracle's, and the L1 distance between the confusion matrices <= 2 u, u the samples whose fp64 top-2 z2 margin is
    below 2 . bound.  That function also caps u at 2 % of n, a condition its own synthetic W2 ~ N(0, 1) is chosen to
    meet; weights trained for an epoch or two have small margins (|z2| <= 1.4), and at the bf16 tolerance 3e-2 a fifth of
    the 256 samples is undecided whatever the code does (35 - 61 on the torch backend over epochs 1 - 8; 0 - 1 at the
    fp32 tolerance), so the cap is not asserted here; u is printed."""
    import json

    n, C = ref["n"], ref["confusion"].shape[0]
    z2 = ref["z2"]
    bound = tol * float(np.abs(z2).max())
    top = np.sort(z2, axis=1)
    u = int(((top[:, -1] - top[:, -2]) < 2 * bound).sum())
    conf = np.asarray(got["confusion"], np.int64)
    l1 = int(np.abs(conf - ref["confusion"]).sum())
    dloss = abs(got["loss_sum"] / n - ref["loss_sum"] / n)
    print("NUMERICS " + json.dumps(dict(test=tag, n=n, bound=bound, undecided=u, l1=l1, mean_loss_err=dloss,
                                        mean_loss=ref["loss_sum"] / n, accuracy=ref["correct"] / n)))
    assert got["n"] == n and conf.shape == (C, C)
    np.testing.assert_array_equal(conf.sum(1), np.bincount(np.asarray(lab, np.int64), minlength=C))
    assert int(np.trace(conf)) == got["correct"]
    assert l1 <= 2 * u, (l1, u)
    assert dloss <= bound, (dloss, bound)


@pytest.mark.parametrize("dtype,H", [("f32", 100), ("bf16", 100), ("f64", 100), ("f32", 512)])
def test_averaged_evaluation_is_a_fresh_engines_and_leaves_training_alone(dtype, H):
    (_, _), (xv, yv) = data()
    tr = _hip_trainer(dtype, "sgd", "graph", H=H)
    never = _hip_trainer(dtype, "sgd", "graph", H=H)
    never.train(2, LR, REG)
    for k in range(2):  # twice, with training in between: stale derived copies of the averaged W1 would show
        tr.train(1, LR, REG)
        before = live(tr)
        got = tr.engine.evaluate(0, weights="ema")
        avg = tr.ema_params()
        _same_eval(got, _fresh(tr, avg).evaluate(0))
        ref = oracle(xv, yv, *avg, xscale=tr.engine.xscale)
        # (bf16: the trained weights' margins cannot meet check_against_oracle's cap on undecided samples -- _within_tol)
        (_within_tol if dtype == "bf16" else check_against_oracle)(got, ref, yv, TOL[dtype, tr.engine.path],
                                                                   f"ema-{dtype}-{H}-{k}")
        cur = tr.engine.evaluate(0)
        _same_eval(cur, _fresh(tr, tr.engine.get_params()).evaluate(0))
        assert cur["loss_sum"] != got["loss_sum"]
        assert same(live(tr), before)  # the live parameters were not overwritten for the evaluation
        np.testing.assert_array_equal(tr.predict(xv, weights="ema"), _fresh(tr, avg).predict(xv))
    torch.cuda.synchronize()
    # training that continued after averaged evaluations is the run that never evaluated
    assert same(live(tr), live(never)) and same(average(tr), average(never))
    assert tr.engine.ema_count() == never.engine.ema_count() == 8


def test_captured_averaged_evaluation_resplits_inside_the_graph():
    """A captured evaluation is replayed after updates the host does not see: the derived copies of the averaged W1 are
    rebuilt inside the capture (H = 512: the forward reads the bf16 planes)."""
    tr = _hip_trainer("f32", "sgd", "graph", H=512)
    tr.train(1, LR, REG)
    tr.engine.evaluate(0, weights="ema")  # (kernels loaded, buffers allocated)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.engine.enqueue_eval(0, weights="ema")
    for _ in range(2):
        tr.train(1, LR, REG)
        g.replay()
        got = tr.engine.read_eval(0)
        _same_eval(got, _fresh(tr, tr.ema_params()).evaluate(0))


# ------------------------------------------------------------------------------------------------ keep-best
def test_keep_best_over_averaged_evaluations_with_adam_from_graphs():
    """train(epochs=3, eval_every=1, keep_best="loss") with Adam, replayed from graphs, against twins stopped after each
    epoch: every record, the best arena and the average are bitwise the twins'."""
    lr = 0.01
    kw = dict(optimizer=Optimizer.adam())
    tr = _hip_trainer("f32", "sgd", "graph", **kw)
    st = tr.train(3, lr, REG, eval_every=1, keep_best="loss")
    twin = _hip_trainer("f32", "sgd", "graph", **kw)
    rec, best, losses = list(START), None, []
    for _ in range(3):
        twin.train(1, lr, REG)
        r = twin.engine.evaluate(0, weights="ema")
        m = py_metric([[float(r["n"]), float(r["correct"]), r["loss_sum"]]], "loss")
        rec, imp = py_decide(rec, "loss", 0.0, None, m)
        losses.append(m)
        if imp:
            best = twin.ema_params()
    print("AVERAGED LOSSES", losses, rec)
    for r in tr.engine.best_records():
        assert same_record(r, rec), (r.tolist(), rec)
    assert [e["loss"] for e in st.evals] == losses and [e["weights"] for e in st.evals] == ["ema"] * 3
    for a, b in zip(tr.engine.best_params(), best):
        assert same(a, b)
    assert same(average(tr), average(twin)) and same(live(tr), live(twin))
    assert tr.engine.ema_count() == 12
    avg = tr.ema_params()
    tr.adopt_ema()
    for a, b in zip(tr.engine.get_params(), avg):
        assert same(a, b)
    _same_eval(tr.engine.evaluate(0), _fresh(tr, avg).evaluate(0))


# ------------------------------------------------------------------------------------------------ snapshots
def test_snapshot_and_restore_carry_the_average_and_the_count():
    tr = _hip_trainer("f32", "momentum", "graph")
    tr.train(1, LR, REG)
    snap = tr._snapshot()
    avg, p, recs = average(tr), live(tr), tr.engine.ema_records()
    tr.train(2, LR, REG)
    assert tr.engine.ema_count() == 12 and not same(average(tr), avg)
    tr._restore(snap)
    torch.cuda.synchronize()
    assert same(average(tr), avg) and same(live(tr), p) and same(tr.engine.ema_records(), recs)
    assert tr.engine.ema_count() == 4
    plain = _hip_trainer("f32", "momentum", "graph", ema=None)
    assert plain.engine._ema is None and len(plain._snapshot()) == 5


# ------------------------------------------------------------------------------------------------ two ranks, one GPU
def test_two_ranks_sharing_the_gpu_average_alike(tmp_path):
    mode = "rccl"
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.ema_workers import gpu_shared_ema_main; " \
           f"gpu_shared_ema_main({str(tmp_path)!r}, {mode!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = [dict(np.load(tmp_path / f"ema_{mode}_{rank}.npz")) for rank in range(2)]
    # the communicator's all-reduce on device gradients (gradient mode + all-reduce + apply + the averaging launch with
    # the status element): the path RCCL takes with one process per GPU; two processes sharing one GPU cannot form an
    # RCCL group, so the group is gloo's -- neither xGMI nor the host-staged all-reduce ran
    assert str(z[0]["impl"]) == str(z[1]["impl"]) == "gloo"
    # the average is the single-process host recurrence over the per-step parameters, on every rank alike
    want, t = recurrence(z[0]["e0"], list(z[0]["seq"]), RULE)
    assert t == 8
    for rank in range(2):
        assert float(z[rank]["agree"]) == 1.0
        assert same(z[rank]["avg"], want)
        for w in z[rank]["recs"]:
            assert w[0] == 8.0 and w[1] == RULE.decay_at(7)
        for w in z[rank]["recs2"]:
            assert w[0] == 12.0
    for k in ("seq", "avg", "params", "avg2", "recs2"):
        assert np.array_equal(z[0][k].view(np.uint8), z[1][k].view(np.uint8)), k
    assert not same(z[0]["avg2"], z[0]["params"])
