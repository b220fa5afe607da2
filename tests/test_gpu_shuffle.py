"""The per-epoch shuffle on the GPU (csrc/mlp/shuffle.hip, MlpEngine.enqueue_shuffle, the trainers' shuffle_seed):
the kernel's order against the host's, every resident layout against a fresh load of the permuted set, and training,
evaluation and two ranks bitwise against the reload-per-epoch twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.resident_layouts import LAYOUTS, engine as _engine, same_layouts as _same_layouts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


def perm_of(n, seed, key):
    return cpu().epoch_permutation(n, seed, key)


def _data(path, N, P, seed=0):
    rng = np.random.default_rng(1000 * seed + N + P)
    y = rng.integers(0, 10, N).astype(np.int32)
    if path == "mfma":  # non-integer, normalised input
        return rng.random((N, P)), y
    return rng.integers(0, 256, (N, P)).astype(np.uint8), y


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200, 1031])
def test_kernel_order_equals_the_host_permutation(N):
    x, y = _data("split3", N, 64)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    assert torch.equal(e.permutation().cpu(), torch.arange(N, dtype=torch.int32))
    for seed, key in ((0, 0), (9, 4), (2**32 - 1, 2**32 - 1)):
        e.enqueue_shuffle(seed, key)
        assert np.array_equal(e.permutation().cpu().numpy(), perm_of(N, seed, key)), (seed, key)
    e.unshuffle()
    assert torch.equal(e.permutation().cpu(), torch.arange(N, dtype=torch.int32))


@pytest.mark.parametrize("path,dtype,H,P,N,held", [
    ("split3", "f32", 100, 784, 1031, ("Xs",)),   # last workgroup guard, Xs padding
    ("split3", "f32", 37, 777, 65, ("Xs",)),      # rows not 16-byte aligned
    ("split3", "f32", 100, 30, 17, ("Xs",)),
    ("split1", "bf16", 512, 784, 200, ("Xw", "XTw")),  # the bf16 wide copies
    ("split3", "f32", 512, 776, 130, ("Xw", "XTw")),
    ("mfma", "f64", 100, 30, 65, ()),             # 8-byte elements
    ("mfma", "f32", 100, 784, 200, ()),           # 4-byte elements
    ("split3", "f32", 100, 784, 1024, ("Xs",)),   # N % 16 == 0: the 16-byte feature-major stores
    ("split1", "bf16", 512, 784, 192, ("Xw", "XTw")),
])
def test_every_layout_equals_a_fresh_load_of_the_permuted_set(path, dtype, H, P, N, held):
    x, y = _data(path, N, P)
    e = _engine(path, dtype, H, x, y, keep=True)
    assert e.path == path and all(getattr(e, n) is not None for n in ("X", "XT", "labels") + held)
    ptrs = {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    for key in (0, 7):  # the second order is x[perm2], not perm2 of perm1
        e.enqueue_shuffle(3, key)
        perm = perm_of(N, 3, key)
        _same_layouts(e, _engine(path, dtype, H, x[perm], y[perm]), f"key {key}")
    e.unshuffle()
    _same_layouts(e, _engine(path, dtype, H, x, y), "unshuffle")
    assert ptrs == {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    assert e.shuffle_launches == 3


def _trainer(shape, dtype, B, executor, seed=None):
    return DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor,
                               shuffle_seed=seed)


def _twin(shape, dtype, B, executor, x, y, seed, epochs, xv=None, yv=None, eval_every=0):
    """Reload per epoch: load(x[perm_e], y[perm_e]) + train(1), ``iter`` carried.  Returns (trainer, evals)."""
    tw = _trainer(shape, dtype, B, executor)
    evals = []
    for ep in range(epochs):
        perm = perm_of(x.shape[0], seed, tw.iter)
        tw.load(x[perm], y[perm])
        tw.train(1, LR, REG)
        if eval_every and (ep + 1) % eval_every == 0:
            tw.load_eval(xv, yv)
            evals.append(tw.evaluate())
    return tw, evals


@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
@pytest.mark.parametrize("shape,dtype,N", [((784, 100, 10), "f32", 200),   # three full batches + a remainder of 8
                                           ((784, 100, 10), "f32", 192),   # full batches only: the native loop
                                           ((784, 100, 47), "f32", 200),   # the four-launch many-class step
                                           ((784, 512, 10), "bf16", 130)])  # the wide engines' bf16 copies
def test_shuffled_training_is_bitwise_the_reload_per_epoch_twin(shape, dtype, N, executor):
    x, y = synthetic_mnist(N, seed=3, num_classes=shape[2])
    tr = _trainer(shape, dtype, 64, executor, seed=5)
    tr.load(x, y)
    tr.train(3, LR, REG)
    tw, _ = _twin(shape, dtype, 64, executor, x, y, 5, 3)
    torch.cuda.synchronize()
    assert tr.iter == tw.iter
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert tr.engine.shuffle_launches == 3 and tw.engine.shuffle_launches == 0
    if executor == "auto" and N == 192:
        assert tr.native_plan(tr.epoch_plan()) is not None  # the shuffle keeps "consecutive full batches" true


def test_eval_every_with_a_shuffle_equals_the_twin():
    shape, N, seed = (784, 100, 10), 200, 5
    x, y = synthetic_mnist(N, seed=3)
    xv, yv = synthetic_mnist(150, seed=8)
    tr = _trainer(shape, "f32", 64, "auto", seed=seed)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(4, LR, REG, eval_every=2)
    _, want = _twin(shape, "f32", 64, "auto", x, y, seed, 4, xv, yv, eval_every=2)
    assert len(st.evals) == len(want) == 2
    for got, ref in zip(st.evals, want):
        assert got["n"] == ref["n"] == 150 and got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"]
        np.testing.assert_array_equal(got["confusion"], ref["confusion"])
    assert torch.equal(tr.engine._eval["X"].cpu(), torch.from_numpy(xv))  # the validation set is never shuffled


def test_two_ranks_sharing_the_gpu(tmp_path):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.shuffle_workers import gpu_shared_shuffle_main; " \
           f"gpu_shared_shuffle_main({str(tmp_path)!r}, 384, 128, 5)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        z = dict(np.load(tmp_path / f"gpu_shuffle{rank}.npz"))
        for k in ("x_equal", "y_equal", "agree", "perm2_equal"):
            assert float(z[k]) == 1.0, (rank, k, str(z["impl"]))
        assert float(z["launches_1"]) == 1.0 and float(z["iter"]) == 6.0


def test_without_a_seed_nothing_is_kept_or_launched():
    x, y = synthetic_mnist(200, seed=3)
    runs = []
    for kw in ({}, {"shuffle_seed": None}):
        tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), dtype="f32", batch_size=64, **kw)
        tr.load(x, y)
        tr.train(2, LR, REG)
        e = tr.engine
        assert e.X0 is None and e.labels0 is None and e._perm is None and e.shuffle_launches == 0
        with pytest.raises(RuntimeError):
            e.enqueue_shuffle(1, 0)
        runs.append(e.params.clone())
    # the code path from before the shuffle existed: the engine loaded with that call, the epoch plan run as it is
    ref = DataParallelTrainer(NeuralNetwork([784, 100, 10]), dtype="f32", batch_size=64)
    ref.engine.load_dataset(x, y, normalize=False)
    ref.N = ref.engine.num_samples
    for _ in range(2):
        ref.run_plan(ref.epoch_plan(), LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], ref.engine.params)
