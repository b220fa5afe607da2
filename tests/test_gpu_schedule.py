"""Learning-rate schedules and gradient-norm clipping on the GPU (csrc/mlp/clip.hip, the extended apply launch of
csrc/mlp/optim.hip, MlpEngine.set_update_policy, DataParallelTrainer(schedule=, clip_norm=)): both kernels bitwise
against the host evaluation of the same headers, their status / window / graph contract, and the trainer bitwise against
a hand-driven twin, against the fp64 oracle and on two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu, hip
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.optim import Optimizer, Schedule
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.eval_oracle import TOL
from tests.sched_workers import (LR, ORACLE_CLIP, ORACLE_LR, REG, RULES, SCHED, padded_arena, pick_clip, rule_code)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2048 * 256 + 3  # wraps the grid-stride loops of both fixed grids (64 and 2048 workgroups), scalar tails
WINDOW = (1, np.array([0.5, 2.0, 0.125]))  # t0 = 1: launch 0 clamps below the window, launch 4 above it


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _dev(a, offset=0):
    """The array on the device, `offset` elements past a fresh allocation (1: 16-byte misaligned)."""
    pad = np.zeros(offset, a.dtype)
    return torch.from_numpy(np.concatenate([pad, a])).cuda()[offset:]


# ------------------------------------------------------------------------------------------ the sum-of-squares kernel
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("count", [1, 255, 257, 1025, BIG])
@pytest.mark.parametrize("ndt", [np.float32, np.float64])
def test_sumsq_kernel_is_bitwise_the_host_header(ndt, count, offset):
    g, segs = padded_arena(count, ndt)
    want, norm = cpu().grad_sumsq(g, segs)
    dg = _dev(g, offset)
    assert (dg.data_ptr() % 16 != 0) == bool(offset)
    npart = int(hip().clip_grid(count))
    assert npart == len(want) == int(cpu().clip_grid(count)) and 1 <= npart <= 64
    part = torch.full((64,), -1.0, dtype=torch.float64, device="cuda")
    dt = 0 if ndt == np.float32 else 1
    hip().grad_sumsq(dt, dg.data_ptr(), g.size, segs, part.data_ptr(), npart, _stream())
    # the norm as the apply launch forms it from the partials: a kSgd launch over one element at rate 0
    p = torch.zeros(1, dtype=dg.dtype, device="cuda")
    rec = torch.tensor([[0.0, 1.0, 1.0, 0.0]], dtype=torch.float64, device="cuda")
    last = torch.zeros(4, dtype=torch.float64, device="cuda")
    hip().optim_apply(dt, 2, *Optimizer.sgd().hyper(0.0), p.data_ptr(), dg[segs[0][0]:].data_ptr(), 0, 0, 1,
                      rec=rec.data_ptr(), nrec=1, partials=part.data_ptr(), npart=npart, clip_norm=1e300,
                      last=last.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    got = part.cpu().numpy()
    assert np.array_equal(_bits(got[:npart]), _bits(want)) and bool((got[npart:] == -1.0).all())
    assert np.isfinite(norm) and np.array_equal(_bits(last.cpu().numpy()[2:3]), _bits(np.array([norm])))
    ref = np.sqrt(sum(float((g[o:o + s].astype(np.float64) ** 2).sum()) for o, s in segs))
    assert abs(norm - ref) <= (count + 2) * 2.0 ** -53 * ref


def test_sumsq_launcher_refuses_segments_outside_the_bucket():
    g = torch.zeros(128, device="cuda")
    part = torch.zeros(64, dtype=torch.float64, device="cuda")
    for segs, npart in (([(0, 129)], 1), ([(64, 65)], 1), ([(-1, 4)], 1), ([(0, 128)], 2)):
        with pytest.raises(Exception):
            hip().grad_sumsq(0, g.data_ptr(), 128, segs, part.data_ptr(), npart, _stream())
    with pytest.raises(Exception):  # more partials than one wave combines
        hip().optim_apply(0, 2, *Optimizer.sgd().hyper(0.1), g.data_ptr(), g.data_ptr(), 0, 0, 128,
                          rec=part.data_ptr(), nrec=1, partials=part.data_ptr(), npart=65, clip_norm=1.0)
    with pytest.raises(Exception):  # a window without a capacity
        hip().optim_apply(0, 2, *Optimizer.sgd().hyper(0.1), g.data_ptr(), g.data_ptr(), 0, 0, 128,
                          rec=part.data_ptr(), nrec=1, window=part.data_ptr(), wcap=0)


# ------------------------------------------------------------------------------------------------- the apply launch
class Arena:
    """Device buffers of one apply-launch problem and their host twins (numpy, same dtype)."""

    def __init__(self, tdt, opt, count, w1n, np_, clip=0.0, window=WINDOW, seed=0):
        self.rng = np.random.default_rng(seed + count)
        self.ndt = np.float32 if tdt == torch.float32 else np.float64
        self.tdt, self.opt, self.count, self.w1n, self.np_, self.clip = tdt, opt, count, w1n, np_, float(clip)
        self.hp = self.rng.standard_normal(count).astype(self.ndt)
        self.hs = [np.zeros(count, self.ndt) for _ in range(opt.num_state)]
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0
        self.p = _dev(self.hp)
        self.g = _dev(np.zeros(count, self.ndt))
        self.s = [_dev(s) for s in self.hs]
        self.rec = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).repeat(hip().optim_grid(count), 1).cuda()
        self.planes = torch.full((max(np_, 1), max(w1n, 1)), 7.0, dtype=torch.bfloat16, device="cuda")
        self.status = torch.zeros(1, dtype=tdt, device="cuda")
        self.last = torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
        self.part = torch.zeros(64, dtype=torch.float64, device="cuda")
        self.hlast = None
        # the norm leaves the last element out (as the status element is) once there is more than one
        self.segs = [(0, count)] if count < 8 else [(0, count // 3), (count // 3, count - count // 3 - 1)]
        self.win = None
        self.set_window(window)

    def set_window(self, window, cap=8):
        self.window = window
        if window is None:
            return
        host = np.concatenate([[float(window[0]), float(len(window[1]))], window[1]])
        if self.win is None:
            self.win = torch.zeros(2 + cap, dtype=torch.float64, device="cuda")
        self.win[:host.size].copy_(torch.from_numpy(host))  # (in place: the address a captured graph holds)

    def grads(self, k):
        g = self.rng.standard_normal(self.count).astype(self.ndt)
        if self.count > 8:
            g[5] = 0.0
            g[7] = np.float32(1e-42) if self.ndt == np.float32 else 5e-320  # denormal
        return g

    def launch(self, lr=LR):
        o = self.opt
        dt = 0 if self.tdt == torch.float32 else 1
        npart = 0
        if self.clip > 0:
            npart = int(hip().clip_grid(sum(s for _, s in self.segs)))
            hip().grad_sumsq(dt, self.g.data_ptr(), self.count, self.segs, self.part.data_ptr(), npart, _stream())
        hip().optim_apply(dt, rule_code(o), *o.hyper(lr), self.p.data_ptr(), self.g.data_ptr(),
                          self.s[0].data_ptr() if self.s else 0, self.s[1].data_ptr() if len(self.s) > 1 else 0,
                          self.count, self.planes.data_ptr() if self.np_ else 0, self.np_,
                          self.w1n if self.np_ else 0, self.status.data_ptr(), self.rec.data_ptr(),
                          int(self.rec.shape[0]), self.win.data_ptr() if self.win is not None else 0,
                          int(self.win.numel()) - 2 if self.win is not None else 0,
                          self.part.data_ptr() if npart else 0, npart, self.clip, self.last.data_ptr(), _stream())

    def host_step(self, g, lr=LR):
        o = self.opt
        g = g.copy()
        lr_t = lr if self.window is None else cpu().window_rate(lr, self.window[0], self.window[1], self.t)
        norm, coef = float("nan"), 1.0
        if self.clip > 0:
            norm, coef = cpu().grad_clip(g, self.segs, self.clip)
        self.hlast = np.array([float(self.t), lr_t, norm, coef])
        self.t, self.b1p, self.b2p = cpu().optim_step(rule_code(o), o.hyper(lr_t), self.hp, g,
                                                      self.hs[0] if self.hs else None,
                                                      self.hs[1] if len(self.hs) > 1 else None, self.t, self.b1p,
                                                      self.b2p)
        return coef

    def tensors(self):
        return (self.p, *self.s, self.rec, self.planes, self.last)

    def check(self, tag):
        torch.cuda.synchronize()
        assert np.array_equal(_bits(self.p.cpu().numpy()), _bits(self.hp)), (tag, "params")
        for i, (d, h) in enumerate(zip(self.s, self.hs)):
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(h)), (tag, "state", i)
        rec = self.rec.cpu()
        want = torch.tensor([float(self.t), self.b1p, self.b2p, 0.0], dtype=torch.float64)
        assert torch.equal(rec, want.expand_as(rec)), (tag, "records")
        assert np.array_equal(_bits(self.last.cpu().numpy()), _bits(self.hlast)), (tag, "last", self.last, self.hlast)
        if self.np_ and self.w1n:
            pl = self.planes[:, :self.w1n].float()
            if self.np_ == 3:
                assert torch.equal((pl[0] + pl[1]) + pl[2], self.p[:self.w1n].float()), (tag, "planes")
            else:
                assert torch.equal(self.planes[0, :self.w1n], self.p[:self.w1n].to(torch.bfloat16)), (tag, "shadow")


W1NS = {1: 0, 257: 131, BIG: 300004}


@pytest.mark.parametrize("count", [1, 257, BIG])
@pytest.mark.parametrize("kind", list(RULES))
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 0), (torch.float32, 1), (torch.float32, 3), (torch.float64, 0)])
def test_apply_launch_is_bitwise_the_host_evaluation_of_the_headers(tdt, np_, kind, count):
    """Five launches over a 3-entry window with t0 = 1 (launches 0 and 4 clamp at either end); no clipping, a threshold
    above every norm (bitwise the unclipped launch) and one below every norm.  N(0, 1) gradients: the norm is about
    sqrt(count), so sqrt(count) / 4 clips every launch and 4 sqrt(count) + 4 none."""
    opt, w1n = RULES[kind], W1NS[count] if np_ else 0
    root = float(np.sqrt(count))
    runs = {c: Arena(tdt, opt, count, w1n, np_, clip=c) for c in (0.0, 4 * root + 4, root / 4)}
    plain = runs[0.0]
    rates = []
    for k in range(5):
        g = plain.grads(k)
        for c, a in runs.items():
            a.g.copy_(torch.from_numpy(g))
            a.launch()
            coef = a.host_step(g)
            a.check((c, k))
            if c:
                assert (coef < 1.0) == (c < root), (c, coef)
        rates.append(plain.hlast[1])
        above = runs[4 * root + 4]
        for x, y in zip(plain.tensors()[:-1], above.tensors()[:-1]):  # (all but the last-update record: its norm)
            assert torch.equal(x, y), ("above the norm", k)
    assert plain.t == 5
    assert rates == [LR * f for f in (0.5, 0.5, 2.0, 0.125, 0.125)]


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 3), (torch.float64, 0)])
def test_nonzero_status_changes_nothing(tdt, np_, kind):
    a = Arena(tdt, RULES[kind], 2000, 900, np_, clip=5.0)
    g = a.grads(0)
    a.g.copy_(torch.from_numpy(g))
    a.launch()
    assert a.host_step(g) < 1.0
    a.check("before")
    held = [t.clone() for t in a.tensors()]
    for bad in (1.0, 2.0, float("nan")):
        a.status.fill_(bad)
        a.launch()
        torch.cuda.synchronize()
        for t, h in zip(a.tensors(), held):
            assert t.dtype == h.dtype and bool((t.view(torch.uint8) == h.view(torch.uint8)).all()), bad
    a.status.zero_()
    a.launch()
    a.host_step(g)
    a.check("after")
    assert a.t == 2


@pytest.mark.parametrize("kind", ["sgd", "nesterov"])
def test_graph_replays_follow_the_window_and_a_refill_needs_no_recapture(kind):
    w5 = (0, np.array([1.0, 0.5, 0.25, 2.0, 0.75]))
    a, b = (Arena(torch.float32, RULES[kind], 5000, 1300, 3, clip=30.0, window=w5) for _ in range(2))
    g = a.grads(0)
    for x in (a, b):
        x.g.copy_(torch.from_numpy(g))
    c = Arena(torch.float32, RULES[kind], 5000, 1300, 3, clip=30.0, window=w5)
    c.launch()  # (kernels loaded before the capture, on buffers of its own)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.launch()  # the sum of squares and the apply launch
    torch.cuda.synchronize()
    assert float(a.rec[0, 0]) == 0.0  # a capture runs nothing
    for _ in range(5):
        graph.replay()
        b.launch()
        b.host_step(g)
    torch.cuda.synchronize()
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)
    b.check("eager")
    assert float(a.last[1]) == LR * 0.75 and float(a.last[0]) == 4.0
    # refill in place: updates 5 .. 7 get new factors, the same graph replays them
    w3 = (5, np.array([3.0, 0.1, 0.2]))
    for x in (a, b):
        x.set_window(w3)
    for _ in range(3):
        graph.replay()
        b.launch()
        b.host_step(g)
    torch.cuda.synchronize()
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)
    b.check("refilled")
    assert float(a.last[1]) == LR * 0.2 and float(a.rec[0, 0]) == 8.0


# ------------------------------------------------------------------ the trainer against a hand-driven twin
def _data(shape, N, normalised):
    if normalised:
        rng = np.random.default_rng(7)
        return rng.random((N, shape[0])), rng.integers(0, shape[2], N).astype(np.int32)
    return synthetic_mnist(N, seed=3, num_classes=shape[2])


def _trainer(shape, dtype, opt, executor, x, y, B=64, **kw):
    tr = DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor, optimizer=opt,
                             **kw)
    tr.load(x, y)
    return tr


class Twin:
    """engine.run(sgd=False) -> gradients to the host -> _cpu.grad_clip, the rate lr * factor(t), _cpu.optim_step on
    the arena -> set_params.  clip None: no clipping, but the norms are recorded."""

    def __init__(self, shape, dtype, opt, x, y, schedule, clip, B=64):
        self.tr = _trainer(shape, dtype, None, "eager", x, y, B)
        e = self.tr.engine
        self.opt, self.schedule, self.clip = opt, schedule, clip
        self.p = e.params.cpu().numpy().copy()
        self.s = [np.zeros_like(self.p) for _ in range(opt.num_state)]
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0
        self.norms, self.coefs, self.rates = [], [], []

    def epoch(self, lr=LR, reg=REG):
        e, o = self.tr.engine, self.opt
        steps = self.tr.epoch_plan().steps
        for s, n in steps:
            e.run(s, n, 1.0 / n, reg, lr, sgd=False)
            torch.cuda.synchronize()
            g = e.grads.cpu().numpy()
            lr_t = lr * self.schedule.factor(self.t, len(steps)) if self.schedule is not None else lr
            if self.clip is None:
                norm, coef = cpu().grad_sumsq(g, e.clip_segments())[1], 1.0
            else:
                norm, coef = cpu().grad_clip(g, e.clip_segments(), self.clip)
            self.norms.append(norm)
            self.coefs.append(coef)
            self.rates.append(lr_t)
            self.t, self.b1p, self.b2p = cpu().optim_step(rule_code(o), o.hyper(lr_t), self.p, g,
                                                          self.s[0] if self.s else None,
                                                          self.s[1] if len(self.s) > 1 else None, self.t, self.b1p,
                                                          self.b2p)
            e.set_params(*(v.numpy() for v in e.layout.views(torch.from_numpy(self.p))))


def _same_as_twin(tr, tw):
    torch.cuda.synchronize()
    e = tr.engine
    assert np.array_equal(_bits(e.params.cpu().numpy()), _bits(tw.p))
    for b, s in zip(e.opt_bufs, tw.s):
        assert np.array_equal(_bits(b.cpu().numpy()), _bits(s))
    st = e.optim_state()
    assert (st["t"], st["b1p"], st["b2p"]) == (tw.t, tw.b1p, tw.b2p)
    up = e.last_update()
    assert (up["t"], up["lr"], up["grad_norm"], up["clip_coef"]) == (tw.t - 1, tw.rates[-1], tw.norms[-1], tw.coefs[-1])


SHAPES = [((784, 100, 10), "f32", "split3", False),
          ((784, 100, 10), "f64", "mfma", False),
          ((784, 100, 47), "f32", "split3", False),   # the many-class head
          ((784, 512, 10), "f32", "split3", False),   # a wide engine
          ((100, 32, 5), "f32", "mfma", True)]        # normalised inputs: the plain MFMA path
_CLIPS: dict = {}


def _twin_clip(shape, dtype, normalised, kind):
    """The threshold of one (shape, rule): from the norms an UNCLIPPED twin run records, once per session."""
    key = (shape, dtype, kind)
    if key not in _CLIPS:
        x, y = _data(shape, 256, normalised)
        tw = Twin(shape, dtype, RULES[kind], x, y, SCHED, None)
        tw.epoch()
        tw.epoch()
        _CLIPS[key] = pick_clip(tw.norms)
        print(f"NUMERICS twin norms {key}: {[round(v, 4) for v in tw.norms]} -> clip {_CLIPS[key]:.4f}")
    return _CLIPS[key]


@pytest.mark.parametrize("executor", ["graph", "eager"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("shape,dtype,path,normalised", SHAPES)
def test_trainer_is_bitwise_the_hand_driven_twin(shape, dtype, path, normalised, kind, executor):
    x, y = _data(shape, 256, normalised)
    opt = RULES[kind]
    clip = _twin_clip(shape, dtype, normalised, kind)
    tr = _trainer(shape, dtype, opt, executor, x, y, schedule=SCHED, clip_norm=clip)
    assert tr.engine.path == path
    tr.train(2, LR, REG)
    tw = Twin(shape, dtype, opt, x, y, SCHED, clip)
    tw.epoch()
    tw.epoch()
    _same_as_twin(tr, tw)
    assert tr.iter == 8 and tw.t == 8
    assert len(set(tw.rates)) == 5
    print(f"NUMERICS twin coefficients {[round(c, 4) for c in tw.coefs]}")
    assert any(c < 1.0 for c in tw.coefs) and any(c >= 1.0 for c in tw.coefs)  # clipped and unclipped updates
    if tr.engine.np == 3 and tr.engine.w1_planes_maintained():
        assert torch.equal(tr.engine.W1p.float().sum(0), tr.engine.W1)


def test_hand_driven_steps_get_the_same_rates():
    x, y = synthetic_mnist(256, seed=3)
    a = _trainer((784, 100, 10), "f32", None, "graph", x, y, schedule=SCHED)
    b = _trainer((784, 100, 10), "f32", None, "eager", x, y, schedule=SCHED)
    a.train(2, LR, REG)
    for _ in range(2):
        for s, n in b.epoch_plan().steps:
            b.step(s, n, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.opt_rec, b.engine.opt_rec)
    assert a.engine.last_update()["lr"] == b.engine.last_update()["lr"] == LR * SCHED.factor(7)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_two_plus_two_epochs_equal_four_and_a_restore_continues_the_rates(kind):
    x, y = synthetic_mnist(200, seed=3)
    sch = Schedule.cosine(total=4, unit="epoch", warmup=1)
    a, b, c = (_trainer((784, 100, 10), "f32", RULES[kind], "graph", x, y, schedule=sch, clip_norm=200.0)
               for _ in range(3))
    a.train(2, LR, REG)
    a.train(2, LR, REG)
    b.train(4, LR, REG)
    c.train(1, LR, REG)
    snap, it = c._snapshot(), c.iter
    c.train(1, LR, REG)  # the epoch a recovery discards
    c._restore(snap)
    c.iter = it
    assert c.engine.update_count() == 4
    c.train(3, LR, REG)
    torch.cuda.synchronize()
    for o in (a, c):
        assert torch.equal(o.engine.params, b.engine.params) and torch.equal(o.engine.opt_rec, b.engine.opt_rec)
        for u, v in zip(o.engine.opt_bufs, b.engine.opt_bufs):
            assert torch.equal(u, v)
        assert o.engine.last_update() == b.engine.last_update()
    assert b.engine.update_count() == 16 and b.engine.last_update()["lr"] == LR * sch.factor(15, 4)
    assert len(a._graphs) == 1  # one capture served every rate


def test_scheduled_runs_take_neither_the_native_loop_nor_the_fused_update():
    x, y = synthetic_mnist(192, seed=3)  # full batches only: the plain-SGD plan qualifies for the native loop
    plain = _trainer((784, 100, 10), "f32", None, "auto", x, y)
    assert plain.native_plan(plain.epoch_plan()) is not None and plain.engine.opt_rec is None
    assert plain.engine.sched_win is None and plain.engine.clip_partials is None and plain.engine.opt_last is None
    for kw, word in ((dict(schedule=SCHED), "schedule"), (dict(clip_norm=1.0), "clipping")):
        tr = _trainer((784, 100, 10), "f32", None, "auto", x, y, **kw)
        assert tr.native_plan(tr.epoch_plan()) is None and word in tr.native_reason
        assert tr.engine._hip_step().xstep_reason == tr.native_reason
        assert not tr.fused_allreduce and tr._xgmi_fused is None
        assert tr.engine.opt_rec is not None and tr.engine.opt_bufs == [] and tr.engine.optimizer is None
        tr.train(1, LR, REG)
        assert tr.engine._hip_step().xstep_used == 0 and tr.engine.update_count() == 3


def test_bf16_shadow_is_the_rounded_master_after_a_scheduled_clipped_run():
    x, y = synthetic_mnist(256, seed=3)
    tr = _trainer((784, 100, 10), "bf16", RULES["nesterov"], "graph", x, y, schedule=SCHED, clip_norm=ORACLE_CLIP)
    assert tr.engine.path == "split1"
    tr.train(2, ORACLE_LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.W1p[0], tr.engine.W1.to(torch.bfloat16))
    assert tr.engine.update_count() == 8


@pytest.mark.parametrize("dtype,path", [("f32", "split3"), ("bf16", "split1")])
def test_low_precision_runs_are_bound_to_the_fp64_oracle(dtype, path):
    """Momentum is linear in the gradient and the clip coefficient is a smooth function of it: the parameters within
    TOL of the fp64 oracle's (schedule, clip at the oracle's own threshold, ORACLE_LR)."""
    shape = (784, 100, 10)
    x, y = synthetic_mnist(256, seed=3)
    opt = Optimizer.momentum(0.9, False)
    tr = _trainer(shape, dtype, opt, "graph", x, y, schedule=SCHED, clip_norm=ORACLE_CLIP)
    assert tr.engine.path == path
    tr.train(2, ORACLE_LR, REG)
    ref, log = NeuralNetwork(list(shape)), []
    mlp.train(ref, x, y, ORACLE_LR, REG, 2, 64, optimizer=opt, schedule=SCHED, clip_norm=ORACLE_CLIP, update_log=log)
    assert any(r[3] < 1.0 for r in log) and any(r[3] >= 1.0 for r in log)
    up = tr.engine.last_update()
    assert up["t"] == log[-1][0] == 7 and up["lr"] == log[-1][1]
    tol = TOL[(dtype, path)]
    for name, got, want in zip(("W1", "b1", "W2", "b2"), tr.engine.get_params(), ref.params):
        rel = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
        print(f"NUMERICS {dtype} {name} rel {rel:.3e} (bound {tol})")
        assert rel < tol, (name, rel)


@pytest.mark.parametrize("mode", ["rccl", "xgmi"])
def test_two_ranks_sharing_the_gpu(tmp_path, mode):
    x, y = synthetic_mnist(384, seed=11)
    log = []  # the threshold: from the fp64 oracle's own unclipped norms of this run
    mlp.train(NeuralNetwork([784, 100, 10]), x, y, ORACLE_LR, REG, 2, 128, schedule=SCHED, clip_norm=1e30,
              update_log=log)
    clip = pick_clip([r[2] for r in log])
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.sched_workers import gpu_shared_sched_main; " \
           f"gpu_shared_sched_main({str(tmp_path)!r}, {mode!r}, {clip!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tol = TOL[("f32", "split3")]
    z = [dict(np.load(tmp_path / f"sched_{mode}_{rank}.npz")) for rank in range(2)]
    for kind in ("sgd", "nesterov"):
        one = _trainer((784, 100, 10), "f32", RULES[kind], "graph", x, y, B=128, schedule=SCHED, clip_norm=clip)
        one.train(2, ORACLE_LR, REG)
        ref = one.engine.params.cpu().double()
        for rank in range(2):
            assert float(z[rank][f"{kind}_agree"]) == 1.0 and int(z[rank][f"{kind}_t"]) == 6, (rank, kind)
            assert float(z[rank][f"{kind}_fused"]) == 0.0
            got = torch.from_numpy(z[rank][f"{kind}_params"]).double()
            rel = float((got - ref).abs().max() / ref.abs().max())
            print(f"NUMERICS {mode} {kind} rank {rank} rel {rel:.3e} (bound {tol}) impl {z[rank]['impl']}")
            assert rel < tol, (mode, kind, rank, rel)
            assert z[rank][f"{kind}_last"][1] == one.engine.last_update()["lr"]
        keys = [f"{kind}_params", f"{kind}_rec", f"{kind}_last"] + ([f"{kind}_state"] if kind != "sgd" else [])
        for k in keys:  # replicas bitwise equal: counter records and the coefficient of the last update included
            assert np.array_equal(_bits(z[0][k]), _bits(z[1][k])), (mode, k)
