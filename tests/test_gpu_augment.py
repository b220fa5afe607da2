"""Random-shift augmentation on the GPU (csrc/mlp/augment.hip, MlpEngine.enqueue_augment, the trainers' augment=): the
kernel's shifts and order against the host's, every resident layout against a fresh load of the host-shifted permuted
set, and training, evaluation, keep-best and two ranks bitwise against the reload-per-epoch twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import Shift, apply_shifts, epoch_shifts
from cme213_sp18_amd.optim import Optimizer
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.resident_layouts import LAYOUTS, engine as _engine, same_layouts as _same_layouts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


def perm_of(n, seed, key):
    return np.arange(n, dtype=np.int32) if seed is None else cpu().epoch_permutation(n, seed, key)


def augmented(x, y, aug, seed, key):
    """The host's epoch: (x[perm] shifted by shifts[perm], y[perm], perm, shifts[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh = epoch_shifts(n, aug, key)[perm]
    return apply_shifts(x[perm], sh, h, w), y[perm], perm, sh


def _data(path, N, P, seed=0):
    rng = np.random.default_rng(1000 * seed + N + P)
    y = rng.integers(0, 10, N).astype(np.int32)
    if path == "mfma":  # non-integer, normalised input (never zero: a zero marks a pixel moved in from outside)
        return rng.random((N, P)) * 0.5 + 0.25, y
    return rng.integers(1, 256, (N, P)).astype(np.uint8), y


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200, 1031])
def test_kernel_shifts_and_order_equal_the_host(N):
    x, y = _data("split3", N, 64)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    assert not e.shifts().any() and tuple(e.shifts().shape) == (N, 2)
    for seed, key in ((0, 0), (9, 4), (2**32 - 1, 2**32 - 1)):
        aug = Shift(2, seed=seed)
        for shuffle_seed in (seed, None):
            e.enqueue_augment(aug, key, shuffle_seed)
            perm = perm_of(N, shuffle_seed, key)
            assert np.array_equal(e.permutation().cpu().numpy(), perm), (seed, key, shuffle_seed)
            assert np.array_equal(e.shifts().cpu().numpy(), epoch_shifts(N, aug, key)[perm]), (seed, key)
    e.unshuffle()
    assert torch.equal(e.permutation().cpu(), torch.arange(N, dtype=torch.int32)) and not e.shifts().any()


SHAPES = [
    ("split3", "f32", 100, 28, 28, 1031, ("Xs",)),        # last-workgroup guard; shifts cross the 256-byte chunks
    ("split3", "f32", 100, 28, 28, 1024, ("Xs",)),        # N % 16 == 0: the 16-byte feature-major stores
    ("split3", "f32", 37, 21, 37, 65, ("Xs",)),           # rows not 16-byte aligned
    ("split3", "f32", 100, 5, 6, 17, ("Xs",)),            # tiny non-square image
    ("split1", "bf16", 512, 28, 28, 200, ("Xw", "XTw")),  # the bf16 wide copies
    ("split1", "bf16", 512, 28, 28, 192, ("Xw", "XTw")),
    ("mfma", "f64", 100, 8, 9, 65, ()),                   # 8-byte elements, 3 chunks per row
    ("mfma", "f64", 100, 5, 6, 65, ()),                   # 8-byte elements, one chunk per row
    ("mfma", "f32", 100, 28, 28, 200, ()),                # 4-byte elements
]


@pytest.mark.parametrize("bounds", ["two", "extreme", "x_only"])
@pytest.mark.parametrize("path,dtype,H,h,w,N,held", SHAPES)
def test_every_layout_equals_a_fresh_load_of_the_shifted_permuted_set(path, dtype, H, h, w, N, held, bounds):
    square = {} if h == w else {"height": h, "width": w}
    aug = {"two": Shift(2, seed=4, **square), "extreme": Shift(w - 1, h - 1, seed=4, **square),
           "x_only": Shift(3, 0, seed=4, **square)}[bounds]
    x, y = _data(path, N, h * w)
    e = _engine(path, dtype, H, x, y, keep=True)
    assert e.path == path and all(getattr(e, n) is not None for n in ("X", "XT", "labels") + held)
    ptrs = {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    for key, seed in ((0, 3), (7, 3), (7, None)):  # each state derives from the pristine rows, not from the last one
        e.enqueue_augment(aug, key, seed)
        xa, ya, perm, sh = augmented(x, y, aug, seed, key)
        assert np.array_equal(e.shifts().cpu().numpy(), sh) and np.array_equal(e.permutation().cpu().numpy(), perm)
        _same_layouts(e, _engine(path, dtype, H, xa, ya), f"key {key} seed {seed}")
    e.unshuffle()
    _same_layouts(e, _engine(path, dtype, H, x, y), "unshuffle")
    assert ptrs == {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    assert e.augment_launches == 3 and e.shuffle_launches == 1 and not e.shifts().any()


def _trainer(shape, dtype, B, executor, seed=None, aug=None, **kw):
    return DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor,
                               shuffle_seed=seed, augment=aug, **kw)


def _twin(shape, dtype, B, executor, x, y, aug, seed, epochs, **kw):
    """Reload per epoch: load the host's augmented epoch + train(1), ``iter`` carried."""
    tw = _trainer(shape, dtype, B, executor, **kw)
    for _ in range(epochs):
        xa, ya, _, _ = augmented(x, y, aug, seed, tw.iter)
        tw.load(xa, ya)
        tw.train(1, LR, REG)
    return tw


@pytest.mark.parametrize("seed", [None, 5])
@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
@pytest.mark.parametrize("shape,dtype,N", [((784, 100, 10), "f32", 200),   # three full batches + a remainder of 8
                                           ((784, 100, 10), "f32", 192),   # full batches only: the native loop
                                           ((784, 100, 47), "f32", 200),   # the four-launch many-class step
                                           ((784, 512, 10), "bf16", 130)])  # the wide engines' bf16 copies
def test_augmented_training_is_bitwise_the_reload_per_epoch_twin(shape, dtype, N, executor, seed):
    x, y = synthetic_mnist(N, seed=3, num_classes=shape[2])
    aug = Shift(2, seed=4)
    tr = _trainer(shape, dtype, 64, executor, seed=seed, aug=aug)
    tr.load(x, y)
    tr.train(3, LR, REG)
    tw = _twin(shape, dtype, 64, executor, x, y, aug, seed, 3)
    torch.cuda.synchronize()
    assert tr.iter == tw.iter
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert tr.engine.augment_launches == 3 and tr.engine.shuffle_launches == 0
    assert tw.engine.augment_launches == 0 and tw.engine.shuffle_launches == 0
    if executor == "auto" and N == 192:
        assert tr.native_plan(tr.epoch_plan()) is not None  # the gather keeps "consecutive full batches" true


def test_adam_eval_every_and_keep_best_equal_the_twin():
    shape, N, seed = (784, 100, 10), 200, 5
    x, y = synthetic_mnist(N, seed=3)
    xv, yv = synthetic_mnist(150, seed=8)
    aug = Shift(2, seed=4)
    tr = _trainer(shape, "f32", 64, "auto", seed=seed, aug=aug, optimizer=Optimizer.adam())
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(4, 0.001, REG, eval_every=1, keep_best="loss")
    tw = _trainer(shape, "f32", 64, "auto", optimizer=Optimizer.adam())
    tw.load_eval(xv, yv)
    want = []
    for _ in range(4):
        xa, ya, _, _ = augmented(x, y, aug, seed, tw.iter)
        tw.load(xa, ya)
        want += tw.train(1, 0.001, REG, eval_every=1, keep_best="loss").evals
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert len(st.evals) == len(want) == 4
    for got, ref in zip(st.evals, want):
        assert got["n"] == ref["n"] == 150 and got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"]
        np.testing.assert_array_equal(got["confusion"], ref["confusion"])
    a, b = tr.best_state(), tw.best_state()
    for k in ("best_index", "best_metric", "evals", "stopped", "iter"):
        assert a[k] == b[k], k
    for got, ref in zip(tr.engine.best_params(), tw.engine.best_params()):
        np.testing.assert_array_equal(got, ref)
    assert torch.equal(tr.engine._eval["X"].cpu(), torch.from_numpy(xv))  # the validation set is never augmented


def test_train_2_plus_2_equals_train_4():
    x, y = synthetic_mnist(200, seed=3)
    aug = Shift(2, seed=4)
    a, b = (_trainer((784, 100, 10), "f32", 64, "auto", seed=5, aug=aug) for _ in range(2))
    for t in (a, b):
        t.load(x, y)
    a.train(4, LR, REG)
    b.train(2, LR, REG)
    b.train(2, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params)
    assert torch.equal(a.engine.X, b.engine.X) and torch.equal(a.engine.shifts(), b.engine.shifts())


def test_two_ranks_sharing_the_gpu(tmp_path):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.augment_workers import gpu_shared_augment_main; " \
           f"gpu_shared_augment_main({str(tmp_path)!r}, 384, 128, 5, {Shift(2, seed=4).to_meta()!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        z = dict(np.load(tmp_path / f"gpu_augment{rank}.npz"))
        for k in ("x_equal", "y_equal", "agree", "perm2_equal", "shifts2_equal"):
            assert float(z[k]) == 1.0, (rank, k, str(z["impl"]))
        assert float(z["launches_1"]) == 1.0 and float(z["shuffle_launches"]) == 0.0 and float(z["iter"]) == 6.0


def test_without_an_augmentation_nothing_is_kept_or_launched():
    x, y = synthetic_mnist(200, seed=3)
    tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), dtype="f32", batch_size=64, augment=None)
    tr.load(x, y)
    tr.train(2, LR, REG)
    e = tr.engine
    assert e.X0 is None and e._perm is None and e._shifts is None
    assert e.augment_launches == 0 and e.shuffle_launches == 0
    with pytest.raises(RuntimeError):
        e.enqueue_augment(Shift(2), 0)
    assert not e.shifts().any()
