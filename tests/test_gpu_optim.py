"""The stateful optimizers on the GPU (csrc/mlp/optim.hip, MlpEngine.apply, DataParallelTrainer(optimizer=...)): the
kernel bitwise against the host evaluation of the same header (_cpu.optim_step), its status / counter / graph contract,
and the trainer bitwise against a hand-driven twin on every single-process step form and on two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu, hip
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.optim import Optimizer, new_state
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.eval_oracle import TOL
from tests.optim_workers import check_adam_drift, check_adam_first_update, first_update_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4
# comparisons with the fp64 oracle over a whole run, held to the bound TOL sets for ONE gradient step, run at the CLI's
# default rate (config.TrainConfig.learning_rate; tests/test_optim.py ORACLE_LR says why); the bitwise tests keep 0.05
ORACLE_LR = 1e-3
KINDS = {"momentum": Optimizer.momentum(0.9, False), "nesterov": Optimizer.momentum(0.8, True),
         "adam": Optimizer.adam(0.9, 0.999, 1e-8)}
BIG = 2048 * 256 + 3  # wraps the grid-stride loop of the 2048-workgroup grid and leaves a scalar tail
W1NS = {1: (0,), 255: (100,), 257: (132, 131), BIG: (300004, 300001)}  # w1n < count, never a multiple of 256 but 0;
#                                                                       # % 4 == 0 (8-byte plane stores) and odd


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Arena:
    """Device buffers of one kernel problem and their host twins (numpy, same dtype)."""

    def __init__(self, tdt, opt, count, w1n, np_, seed=0, offset=0):
        rng = np.random.default_rng(seed + count)
        ndt = np.float32 if tdt == torch.float32 else np.float64
        self.tdt, self.opt, self.count, self.w1n, self.np_ = tdt, opt, count, w1n, np_
        p = rng.standard_normal(count).astype(ndt)
        if count > 8:
            p[3] = 0.0
        self.hp = p
        self.hs = [np.zeros(count, ndt) for _ in range(opt.num_state)]
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0
        dev = "cuda"
        # offset != 0: every buffer starts `offset` elements past its allocation (16-byte misaligned: scalar path)
        mk = lambda src: torch.from_numpy(np.concatenate([np.zeros(offset, ndt), src])).to(dev)[offset:]  # noqa: E731
        self.p = mk(p)
        self.g = mk(np.zeros(count, ndt))
        self.s = [mk(s) for s in self.hs]
        self.rec = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).repeat(hip().optim_grid(count), 1).to(dev)
        self.planes = torch.full((max(np_, 1), max(w1n, 1)), 7.0, dtype=torch.bfloat16, device=dev)
        self.status = torch.zeros(1, dtype=tdt, device=dev)
        self.rng, self.ndt = rng, ndt

    def grads(self, k):
        """Launch k's gradient: N(0, 1) with zeros, one denormal and (index 5) a gradient that is 0 in every launch."""
        g = self.rng.standard_normal(self.count).astype(self.ndt)
        if self.count > 8:
            g[5] = 0.0                       # adam: m = s = 0 throughout, the update is exactly 0
            g[6] = 0.0 if k % 2 else g[6]
            g[7] = np.float32(1e-42) if self.ndt == np.float32 else 5e-320  # denormal
        return g

    def launch(self, lr=LR):
        o = self.opt
        hip().optim_step(0 if self.tdt == torch.float32 else 1, o.code, *o.hyper(lr), self.p.data_ptr(),
                         self.g.data_ptr(), self.s[0].data_ptr(), self.s[1].data_ptr() if len(self.s) > 1 else 0,
                         self.count, self.planes.data_ptr() if self.np_ else 0, self.np_,
                         self.w1n if self.np_ else 0, self.status.data_ptr(), self.rec.data_ptr(),
                         int(self.rec.shape[0]), _stream())

    def host_step(self, g, lr=LR):
        o = self.opt
        self.t, self.b1p, self.b2p = cpu().optim_step(o.code, o.hyper(lr), self.hp, g, self.hs[0],
                                                      self.hs[1] if len(self.hs) > 1 else None, self.t, self.b1p,
                                                      self.b2p)

    def check(self, tag):
        torch.cuda.synchronize()
        assert np.array_equal(self.p.cpu().numpy().view(np.uint8), self.hp.view(np.uint8)), (tag, "params")
        for i, (d, h) in enumerate(zip(self.s, self.hs)):
            assert np.array_equal(d.cpu().numpy().view(np.uint8), h.view(np.uint8)), (tag, "state", i)
        rec = self.rec.cpu()
        want = torch.tensor([float(self.t), self.b1p, self.b2p, 0.0], dtype=torch.float64)
        assert torch.equal(rec, want.expand_as(rec)), (tag, "records")
        if self.np_ and self.w1n:
            pl = self.planes[:, :self.w1n].float()
            w1 = self.p[:self.w1n].float()
            if self.np_ == 3:  # the exact split: the planes sum (in this order, exactly) to the new fp32 W1
                assert torch.equal((pl[0] + pl[1]) + pl[2], w1), (tag, "planes")
            else:
                assert torch.equal(self.planes[0, :self.w1n], self.p[:self.w1n].to(torch.bfloat16)), (tag, "shadow")


@pytest.mark.parametrize("count", [1, 255, 257, BIG])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 0), (torch.float32, 1), (torch.float32, 3), (torch.float64, 0)])
def test_kernel_is_bitwise_the_host_evaluation_of_the_header(tdt, np_, kind, count):
    for w1n in (W1NS[count] if np_ else W1NS[count][:1]):
        a = Arena(tdt, KINDS[kind], count, w1n, np_)
        p0 = a.hp.copy()
        for k in range(5):  # adam's counter goes 1 .. 5
            g = a.grads(k)
            a.g.copy_(torch.from_numpy(g))
            a.launch()
            a.host_step(g)
            a.check((w1n, k))
        assert a.t == 5
        if count > 8 and kind == "adam":
            assert a.hp[5] == p0[5] and float(a.p[5]) == float(p0[5])  # s = 0, g = 0: exactly no update
        if np_ and w1n < a.planes.shape[1]:
            assert bool((a.planes[:, w1n:] == 7.0).all())  # nothing written past w1n


@pytest.mark.parametrize("kind", ["nesterov", "adam"])
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 3), (torch.float64, 0)])
def test_kernel_misaligned_buffers_take_the_scalar_path(tdt, np_, kind):
    a = Arena(tdt, KINDS[kind], 257, 131, np_, offset=1)
    assert a.p.data_ptr() % 16 != 0
    for k in range(2):
        g = a.grads(k)
        a.g.copy_(torch.from_numpy(g))
        a.launch()
        a.host_step(g)
        a.check(k)


@pytest.mark.parametrize("kind", ["momentum", "adam"])
@pytest.mark.parametrize("tdt,np_", [(torch.float32, 3), (torch.float64, 0)])
def test_nonzero_status_changes_nothing(tdt, np_, kind):
    a = Arena(tdt, KINDS[kind], 2000, 900, np_)
    g = a.grads(0)
    a.g.copy_(torch.from_numpy(g))
    a.launch()
    a.host_step(g)
    a.check("before")
    held = [t.clone() for t in (a.p, *a.s, a.rec, a.planes)]
    for bad in (1.0, 2.0, float("nan")):
        a.status.fill_(bad)
        a.launch()
        torch.cuda.synchronize()
        for t, h in zip((a.p, *a.s, a.rec, a.planes), held):
            assert t.dtype == h.dtype and bool((t.view(torch.uint8) == h.view(torch.uint8)).all()), bad
    a.status.zero_()
    a.launch()
    a.host_step(g)
    a.check("after")
    assert a.t == 2


@pytest.mark.parametrize("kind", ["nesterov", "adam"])
def test_graph_replays_advance_the_device_counter(kind):
    a, b = (Arena(torch.float32, KINDS[kind], 5000, 1300, 3) for _ in range(2))
    g = a.grads(0)
    for x in (a, b):
        x.g.copy_(torch.from_numpy(g))
    b.launch()  # (kernel loaded before the capture; b is the eager side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            a.launch()
    torch.cuda.synchronize()
    assert float(a.rec[0, 0]) == 0.0  # a capture runs nothing
    graph.replay()
    graph.replay()
    for _ in range(5):
        b.launch()
    torch.cuda.synchronize()
    for x, y in zip((a.p, *a.s, a.rec, a.planes), (b.p, *b.s, b.rec, b.planes)):
        assert torch.equal(x, y)
    assert float(a.rec[0, 0]) == 6.0 and bool((a.rec == a.rec[0]).all())


# ------------------------------------------------------------------ the trainer against a hand-driven twin
def _data(shape, N, normalised):
    if normalised:
        rng = np.random.default_rng(7)
        return rng.random((N, shape[0])), rng.integers(0, shape[2], N).astype(np.int32)
    return synthetic_mnist(N, seed=3, num_classes=shape[2])


def _trainer(shape, dtype, path, opt, executor, x, y, B=64, **kw):
    tr = DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, path=path, executor=executor,
                             optimizer=opt, **kw)
    tr.load(x, y)
    return tr


class Twin:
    """engine.run(sgd=False) -> gradients to the host -> _cpu.optim_step on the arena -> set_params."""

    def __init__(self, shape, dtype, path, opt, x, y, B=64):
        self.tr = _trainer(shape, dtype, path, None, "eager", x, y, B)
        e = self.tr.engine
        self.opt = opt
        self.p = e.params.cpu().numpy().copy()
        self.s = [np.zeros_like(self.p) for _ in range(opt.num_state)]
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0

    def epoch(self, lr=LR, reg=REG):
        e, o = self.tr.engine, self.opt
        for s, n in self.tr.epoch_plan().steps:
            e.run(s, n, 1.0 / n, reg, lr, sgd=False)
            torch.cuda.synchronize()
            g = e.grads.cpu().numpy()
            self.t, self.b1p, self.b2p = cpu().optim_step(o.code, o.hyper(lr), self.p, g, self.s[0],
                                                          self.s[1] if len(self.s) > 1 else None, self.t, self.b1p,
                                                          self.b2p)
            e.set_params(*(v.numpy() for v in e.layout.views(torch.from_numpy(self.p))))


def _same_as_twin(tr, tw):
    torch.cuda.synchronize()
    e = tr.engine
    assert np.array_equal(e.params.cpu().numpy().view(np.uint8), tw.p.view(np.uint8))
    for b, s in zip(e.opt_bufs, tw.s):
        assert np.array_equal(b.cpu().numpy().view(np.uint8), s.view(np.uint8))
    st = e.optim_state()
    assert (st["t"], st["b1p"], st["b2p"]) == (tw.t, tw.b1p, tw.b2p)


SHAPES = [((784, 100, 10), "f32", "split3", False),
          ((784, 100, 10), "f64", "mfma", False),
          ((784, 100, 47), "f32", "split3", False),   # the many-class head
          ((784, 512, 10), "f32", "split3", False),   # a wide engine
          ((100, 32, 5), "f32", "mfma", True)]        # normalised inputs: the plain MFMA path


@pytest.mark.parametrize("executor", ["graph", "eager"])
@pytest.mark.parametrize("kind", ["nesterov", "adam"])
@pytest.mark.parametrize("shape,dtype,path,normalised", SHAPES)
def test_trainer_is_bitwise_the_hand_driven_twin(shape, dtype, path, normalised, kind, executor):
    x, y = _data(shape, 256, normalised)
    opt = KINDS[kind]
    tr = _trainer(shape, dtype, "auto", opt, executor, x, y)
    assert tr.engine.path == path
    tr.train(2, LR, REG)
    tw = Twin(shape, dtype, "auto", opt, x, y)
    tw.epoch()
    tw.epoch()
    _same_as_twin(tr, tw)
    assert tr.iter == 8 and tw.t == 8
    if tr.engine.np == 3 and tr.engine.w1_planes_maintained():
        assert torch.equal(tr.engine.W1p.float().sum(0), tr.engine.W1)


@pytest.mark.parametrize("dtype,path", [("bf16", "split1"), ("f32", "split3")])
@pytest.mark.parametrize("kind", ["momentum", "nesterov", "adam"])
def test_low_precision_runs_are_bound_to_the_fp64_oracle(kind, dtype, path):
    """Momentum and Nesterov are linear in the gradient: the parameters within TOL of the fp64 oracle's.  Adam divides
    by sqrt(s), so TOL does not carry over to its parameters (tests/optim_workers.py derives what does): TOL on the
    first update's m and s per tensor, and the elementwise drift bound 2 lr sum_t c_t on the parameters."""
    shape = (784, 100, 10)
    x, y = _data(shape, 256, False)
    opt = KINDS[kind]
    lr = ORACLE_LR
    tr = _trainer(shape, dtype, "auto", opt, "graph", x, y)
    assert tr.engine.path == path
    first = first_update_state(tr, lr, REG)
    tr.train(2, lr, REG)
    ref = NeuralNetwork(list(shape))
    mlp.train(ref, x, y, lr, REG, 2, 64, optimizer=opt)
    tol = TOL[(dtype, path)]
    if kind == "adam":
        one = NeuralNetwork(list(shape))
        st = new_state(opt, one.num_params())
        mlp.train(one, x[:64], y[:64], lr, REG, 1, 64, optimizer=opt, optim_state=st)
        check_adam_first_update(list(shape), first, st["state"], tol, f"{dtype} hip")
        check_adam_drift(opt, lr, 8, np.concatenate([p.ravel() for p in tr.engine.get_params()]),
                         np.concatenate([p.ravel() for p in ref.params]), f"{dtype} hip")
    for name, got, want in zip(("W1", "b1", "W2", "b2"), tr.engine.get_params(), ref.params):
        rel = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
        print(f"NUMERICS {dtype} {kind} {name} rel {rel:.3e} (bound {tol})")
        if kind != "adam":
            assert rel < tol, (name, rel)
    if dtype == "bf16":  # the shadow is the rounded master
        assert torch.equal(tr.engine.W1p[0], tr.engine.W1.to(torch.bfloat16))


def test_stateful_runs_take_neither_the_native_loop_nor_the_fused_update():
    x, y = synthetic_mnist(192, seed=3)  # full batches only: the plain-SGD plan qualifies for the native loop
    plain = _trainer((784, 100, 10), "f32", "auto", None, "auto", x, y)
    assert plain.native_plan(plain.epoch_plan()) is not None and plain.native_reason == ""
    assert plain.engine.optimizer is None and plain.engine.opt_bufs == [] and plain.engine.opt_rec is None
    sgd = _trainer((784, 100, 10), "f32", "auto", Optimizer.sgd(), "auto", x, y)
    assert sgd.native_plan(sgd.epoch_plan()) is not None and sgd.engine.opt_rec is None
    plain.train(2, LR, REG)
    sgd.train(2, LR, REG)
    assert torch.equal(plain.engine.params, sgd.engine.params)
    tr = _trainer((784, 100, 10), "f32", "auto", KINDS["momentum"], "auto", x, y)
    assert tr.native_plan(tr.epoch_plan()) is None and "stateful optimizer" in tr.native_reason
    assert tr.engine._hip_step().xstep_reason == tr.native_reason
    assert not tr.fused_allreduce and tr._xgmi_fused is None
    tr.train(1, LR, REG)
    assert tr.engine._hip_step().xstep_used == 0
    assert tr.engine.optim_state()["t"] == 3
    assert len(tr.engine.opt_bufs) == 1 and tr.engine.opt_bufs[0].dtype == tr.engine.params.dtype


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_two_plus_two_epochs_equal_four_and_capture_leaves_the_state(kind):
    x, y = synthetic_mnist(200, seed=3)
    a = _trainer((784, 100, 10), "f32", "auto", KINDS[kind], "graph", x, y)
    b = _trainer((784, 100, 10), "f32", "auto", KINDS[kind], "graph", x, y)
    a.capture(a.epoch_plan(), LR, REG)  # the warm-up step is undone: parameters, state and counters
    st = a.engine.optim_state()
    assert st["t"] == 0 and st["b1p"] == 1.0 and all(not s.any() for s in st["state"])
    assert torch.equal(a.engine.params, b.engine.params)
    a.train(2, LR, REG)
    a.train(2, LR, REG)
    b.train(4, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params)
    for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs):
        assert torch.equal(u, v)
    assert a.engine.optim_state()["t"] == b.engine.optim_state()["t"] == 16


def test_snapshot_and_restore_carry_state_and_counters():
    x, y = synthetic_mnist(200, seed=3)
    a = _trainer((784, 100, 10), "f32", "auto", KINDS["adam"], "graph", x, y)
    b = _trainer((784, 100, 10), "f32", "auto", KINDS["adam"], "graph", x, y)
    a.train(1, LR, REG)
    snap = a._snapshot()
    it = a.iter
    a.train(1, LR, REG)  # the epoch a recovery discards
    a._restore(snap)
    a.iter = it
    st = a.engine.optim_state()
    assert st["t"] == 4
    a.train(1, LR, REG)
    b.train(2, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params)
    for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs):
        assert torch.equal(u, v)
    assert torch.equal(a.engine.opt_rec, b.engine.opt_rec)
    # set_optim_state(optim_state()) round-trips, reset_optimizer() zeroes
    st = a.engine.optim_state()
    a.engine.reset_optimizer()
    assert a.engine.optim_state()["t"] == 0 and not a.engine.opt_bufs[0].any()
    a.engine.set_optim_state(st)
    for u, v in zip(a.engine.opt_bufs, b.engine.opt_bufs):
        assert torch.equal(u, v)
    assert torch.equal(a.engine.opt_rec, b.engine.opt_rec)


def test_shuffled_run_with_eval_every_equals_the_twin_stopped_after_each_epoch():
    shape, N, seed, opt = (784, 100, 10), 200, 5, KINDS["momentum"]
    x, y = synthetic_mnist(N, seed=3)
    xv, yv = synthetic_mnist(150, seed=8)
    tr = _trainer(shape, "f32", "auto", opt, "auto", x, y, shuffle_seed=seed)
    tr.load_eval(xv, yv)
    st = tr.train(3, LR, REG, eval_every=1)
    tw = DataParallelTrainer(NeuralNetwork(list(shape)), dtype="f32", batch_size=64, optimizer=opt)
    want = []
    for _ in range(3):  # reload per epoch; the optimizer state and the iteration counter carry over
        perm = cpu().epoch_permutation(N, seed, tw.iter)
        tw.load(x[perm], y[perm])
        tw.train(1, LR, REG)
        tw.load_eval(xv, yv)
        want.append(tw.evaluate())
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.params, tw.engine.params) and torch.equal(tr.engine.opt_bufs[0], tw.engine.opt_bufs[0])
    assert len(st.evals) == 3
    for got, ref in zip(st.evals, want):
        assert got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"]
        np.testing.assert_array_equal(got["confusion"], ref["confusion"])


@pytest.mark.parametrize("mode", ["rccl", "host", "xgmi"])
def test_two_ranks_sharing_the_gpu(tmp_path, mode):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.optim_workers import gpu_shared_optim_main; " \
           f"gpu_shared_optim_main({str(tmp_path)!r}, {mode!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # the single-process run of the same global batches
    x, y = synthetic_mnist(384, seed=11)
    tol = TOL[("f32", "split3")]
    for kind in ("nesterov", "adam"):
        one = _trainer((784, 100, 10), "f32", "auto", KINDS[kind], "graph", x, y, B=128)
        first = first_update_state(one, ORACLE_LR, REG)
        one.train(2, ORACLE_LR, REG)
        ref = one.engine.params.cpu().double()
        z = [dict(np.load(tmp_path / f"optim_{mode}_{rank}.npz")) for rank in range(2)]
        for rank in range(2):
            assert float(z[rank][f"{kind}_agree"]) == 1.0 and int(z[rank][f"{kind}_t"]) == 6, (rank, kind)
            assert float(z[rank][f"{kind}_fused"]) == 0.0
            got = torch.from_numpy(z[rank][f"{kind}_params"]).double()
            rel = float((got - ref).abs().max() / ref.abs().max())
            print(f"NUMERICS {mode} {kind} rank {rank} rel {rel:.3e} (bound {tol}) impl {z[rank]['impl']}")
            if kind == "adam":  # (tests/optim_workers.py: the bounds derived for Adam across summation orders)
                n = one.nn.num_params()
                fr = z[rank]["adam_first"]
                check_adam_first_update([784, 100, 10], [fr[:n], fr[n:]], first, tol, f"{mode} rank {rank}")
                check_adam_drift(KINDS[kind], ORACLE_LR, 6, got.numpy(), ref.numpy(), f"{mode} rank {rank}")
            else:
                assert rel < tol, (mode, kind, rank, rel)
        for k in (f"{kind}_params", f"{kind}_state"):  # replicas bitwise equal, state included
            assert np.array_equal(z[0][k].view(np.uint8), z[1][k].view(np.uint8)), (mode, k)
    if mode == "rccl":  # the bucketed, overlapped backward: same gradients in another order of launches
        for rank in range(2):
            assert float(z[rank]["bucketed_agree_1"]) == 1.0 and float(z[rank]["bucketed_agree_0"]) == 1.0
            assert float(z[rank]["bucketed_rel"]) < tol, float(z[rank]["bucketed_rel"])
