"""Affine augmentation on the GPU (csrc/mlp/affine.hip, MlpEngine.enqueue_augment with an augment.Affine, the trainers'
augment=): the kernel's transforms, shifts and order against the host's, every resident layout against a fresh load of
the host-transformed permuted set, and training, evaluation, keep-best and two ranks bitwise against the
reload-per-epoch twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import Affine, Shift, apply_affine, epoch_shifts, epoch_transforms
from cme213_sp18_amd.optim import Optimizer
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.resident_layouts import LAYOUTS, engine as _engine, same_layouts as _same_layouts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


def perm_of(n, seed, key):
    return np.arange(n, dtype=np.int32) if seed is None else cpu().epoch_permutation(n, seed, key)


def resident(x, dtype):
    """The rows as the engine of that dtype keeps them (what the rule blends), as an array numpy can hold: bf16 as its
    bits (uint16)."""
    if x.dtype == np.uint8:
        return x
    if dtype == "f64":
        return np.ascontiguousarray(x, np.float64)
    x32 = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x32
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def loadable(rows):
    """What load_dataset takes for rows in resident() form (bf16 bits -> the float32 of the same value)."""
    if rows.dtype == np.uint16:
        return torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy()
    return rows


def augmented(x, y, aug, seed, key, dtype="f32"):
    """The host's epoch: (x[perm] through entries[perm] and shifts[perm], y[perm], perm, shifts[perm], index[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh = epoch_shifts(n, aug, key)[perm]
    idx = epoch_transforms(n, aug, key)[perm]
    rows = apply_affine(resident(x, dtype)[perm], sh, aug.table()[idx], h, w)
    return loadable(rows), y[perm], perm, sh, idx


def _data(path, N, P, seed=0):
    rng = np.random.default_rng(1000 * seed + N + P)
    y = rng.integers(0, 10, N).astype(np.int32)
    if path == "mfma":  # non-integer, normalised input (never zero: a zero marks a pixel without a tap)
        return rng.random((N, P)) * 0.5 + 0.25, y
    return rng.integers(1, 256, (N, P)).astype(np.uint8), y


@pytest.mark.parametrize("T", [1, 1024])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200])
def test_kernel_transforms_shifts_and_order_equal_the_host(N, T):
    x, y = _data("split3", N, 64)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    assert not e.transforms().any() and tuple(e.transforms().shape) == (N,)
    for seed, key in ((0, 0), (9, 4), (2**32 - 1, 2**32 - 1)):
        aug = Affine(15, (0.9, 1.1), 10, max_dx=2, seed=seed, table=T)
        for shuffle_seed in (seed, None):
            e.enqueue_augment(aug, key, shuffle_seed)
            perm = perm_of(N, shuffle_seed, key)
            assert np.array_equal(e.permutation().cpu().numpy(), perm), (seed, key, shuffle_seed)
            assert np.array_equal(e.shifts().cpu().numpy(), epoch_shifts(N, aug, key)[perm]), (seed, key)
            assert np.array_equal(e.transforms().cpu().numpy(), epoch_transforms(N, aug, key)[perm]), (seed, key)
    e.unshuffle()
    assert torch.equal(e.permutation().cpu(), torch.arange(N, dtype=torch.int32))
    assert not e.shifts().any() and not e.transforms().any()


SHAPES = [
    ("split3", "f32", 100, 28, 28, 1031, ("Xs",)),        # last-workgroup guard; taps cross the 256-byte chunks
    ("split3", "f32", 100, 28, 28, 1024, ("Xs",)),        # N % 16 == 0: the 16-byte feature-major stores
    ("split3", "f32", 37, 21, 37, 65, ("Xs",)),           # rows not 16-byte aligned
    ("split3", "f32", 100, 5, 6, 17, ("Xs",)),            # tiny non-square image
    ("split1", "bf16", 512, 28, 28, 200, ("Xw", "XTw")),  # the bf16 wide copies
    ("split1", "bf16", 512, 28, 28, 192, ("Xw", "XTw")),
    ("mfma", "f64", 100, 8, 9, 65, ()),                   # 8-byte elements, 3 chunks per row
    ("mfma", "f64", 100, 5, 6, 65, ()),                   # 8-byte elements, one chunk per row
    ("mfma", "f32", 100, 28, 28, 200, ()),                # 4-byte elements
    ("mfma", "bf16", 100, 5, 6, 65, ()),                  # 2-byte elements (the mfma path's bf16 pixels)
]


def _policy(name, h, w, seed=4):
    square = {} if h == w else {"height": h, "width": w}
    if name == "mild":
        return Affine(15, (0.9, 1.1), 10, max_dx=min(2, w - 1), max_dy=min(2, h - 1), seed=seed, **square)
    if name == "extreme":  # every side of the image is left, and some images have no taps at all
        return Affine(180, (0.25, 4), 45, max_dx=w - 1, max_dy=h - 1, seed=seed, **square)
    return Affine(0, 1, 0, max_dx=min(2, w - 1), max_dy=min(2, h - 1), seed=seed, **square)


@pytest.mark.parametrize("policy", ["mild", "extreme", "identity"])
@pytest.mark.parametrize("path,dtype,H,h,w,N,held", SHAPES)
def test_every_layout_equals_a_fresh_load_of_the_transformed_permuted_set(path, dtype, H, h, w, N, held, policy):
    aug = _policy(policy, h, w)
    x, y = _data(path, N, h * w)
    e = _engine(path, dtype, H, x, y, keep=True)
    assert e.path == path and all(getattr(e, n) is not None for n in ("X", "XT", "labels") + held)
    assert e.X.element_size() == {"split3": 1, "split1": 1}.get(path, {"f64": 8, "f32": 4, "bf16": 2}[dtype])
    ptrs = {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    for key, seed in ((0, 3), (7, 3), (7, None)):  # each state derives from the pristine rows, not from the last one
        e.enqueue_augment(aug, key, seed)
        xa, ya, perm, sh, idx = augmented(x, y, aug, seed, key, dtype)
        assert np.array_equal(e.shifts().cpu().numpy(), sh) and np.array_equal(e.permutation().cpu().numpy(), perm)
        assert np.array_equal(e.transforms().cpu().numpy(), idx)
        _same_layouts(e, _engine(path, dtype, H, xa, ya), f"key {key} seed {seed}")
    if policy == "identity":  # ... which must equal the Shift launch's layouts
        f = _engine(path, dtype, H, x, y, keep=True)
        f.enqueue_augment(Shift(aug.max_dx, aug.max_dy, aug.height, aug.width, aug.seed), 7, None)
        _same_layouts(e, f, "the Shift launch")
        assert torch.equal(e.shifts(), f.shifts()) and f.augment_launches == 1 and f.affine_launches == 0
    e.unshuffle()
    _same_layouts(e, _engine(path, dtype, H, x, y), "unshuffle")
    assert ptrs == {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
    assert e.affine_launches == 3 and e.augment_launches == 0 and e.shuffle_launches == 1
    assert not e.shifts().any() and not e.transforms().any()


def test_the_launcher_refuses_a_missing_table_and_a_foreign_kind():
    from cme213_sp18_amd._native import hip

    x, y = _data("split3", 20, 64)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    aug = Affine(15, max_dx=1)
    e.prepare_augment(aug)
    table = e._affine_table[1]

    def launch(tab, T, kind):
        e._gather_launch(hip().mlp_affine, e._shifts.data_ptr(), e._transforms.data_ptr(), tab, T, kind, 20, 64, 1, 8,
                         8, 1, 1, 0, 0, 0, 0)

    for tab, T, kind in ((0, 1024, 0), (table.data_ptr() + 4, 1023, 0), (table.data_ptr(), 0, 0),
                         (table.data_ptr(), 65537, 0), (table.data_ptr(), 1024, 2), (table.data_ptr(), 1024, 7)):
        with pytest.raises(Exception):
            launch(tab, T, kind)
    launch(table.data_ptr(), 1024, 0)
    torch.cuda.synchronize()
    assert np.array_equal(e.transforms().cpu().numpy(), epoch_transforms(20, aug, 0))


def _trainer(shape, dtype, B, executor, seed=None, aug=None, **kw):
    return DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor,
                               shuffle_seed=seed, augment=aug, **kw)


def _twin(shape, dtype, B, executor, x, y, aug, seed, epochs, **kw):
    """Reload per epoch: load the host's augmented epoch + train(1), ``iter`` carried."""
    tw = _trainer(shape, dtype, B, executor, **kw)
    for _ in range(epochs):
        xa, ya = augmented(x, y, aug, seed, tw.iter)[:2]
        tw.load(xa, ya)
        tw.train(1, LR, REG)
    return tw


AUG = dict(rotate=15, scale=(0.9, 1.1), shear=10, max_dx=2, seed=4)


@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
def test_augmented_training_is_bitwise_the_reload_per_epoch_twin(executor):
    shape, N, seed = (784, 100, 10), 256, 5
    x, y = synthetic_mnist(N, seed=3)
    aug = Affine(**AUG)
    plain = _trainer(shape, "f32", 64, executor, seed=seed)
    plain.load(x, y)
    plain.train(3, LR, REG)
    tr = _trainer(shape, "f32", 64, executor, seed=seed, aug=aug)
    tr.load(x, y)
    tr.train(3, LR, REG)
    tw = _twin(shape, "f32", 64, executor, x, y, aug, seed, 3)
    torch.cuda.synchronize()
    assert tr.iter == tw.iter
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert not torch.equal(tr.engine.params, plain.engine.params)  # (the transforms reached the step kernels)
    assert tr.engine.affine_launches == 3 and tr.engine.augment_launches == 0 and tr.engine.shuffle_launches == 0
    assert tw.engine.affine_launches == 0 and tw.engine.shuffle_launches == 0
    # the one-launch pipeline still takes the epoch: as without an augmentation
    assert tr.engine._hip_step().xstep_used == plain.engine._hip_step().xstep_used
    if executor == "auto":
        assert tr.native_plan(tr.epoch_plan()) is not None  # the gather keeps "consecutive full batches" true


def test_adam_eval_every_and_keep_best_from_graphs_equal_the_twin():
    shape, N, seed = (784, 100, 10), 256, 5
    x, y = synthetic_mnist(N, seed=3)
    xv, yv = synthetic_mnist(150, seed=8)
    aug = Affine(**AUG)
    tr = _trainer(shape, "f32", 64, "graph", seed=seed, aug=aug, optimizer=Optimizer.adam())
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(3, 0.001, REG, eval_every=1, keep_best="loss")
    tw = _trainer(shape, "f32", 64, "graph", optimizer=Optimizer.adam())
    tw.load_eval(xv, yv)
    want = []
    for _ in range(3):
        xa, ya = augmented(x, y, aug, seed, tw.iter)[:2]
        tw.load(xa, ya)
        want += tw.train(1, 0.001, REG, eval_every=1, keep_best="loss").evals
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert len(st.evals) == len(want) == 3
    for got, ref in zip(st.evals, want):
        assert got["n"] == ref["n"] == 150 and got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"]
        np.testing.assert_array_equal(got["confusion"], ref["confusion"])
    a, b = tr.best_state(), tw.best_state()
    for k in ("best_index", "best_metric", "evals", "stopped", "iter"):
        assert a[k] == b[k], k
    for got, ref in zip(tr.engine.best_params(), tw.engine.best_params()):
        np.testing.assert_array_equal(got, ref)
    assert torch.equal(tr.engine._eval["X"].cpu(), torch.from_numpy(xv))  # the validation set is never augmented


def test_train_1_plus_2_equals_train_3():
    x, y = synthetic_mnist(256, seed=3)
    aug = Affine(**AUG)
    a, b = (_trainer((784, 100, 10), "f32", 64, "auto", seed=5, aug=aug) for _ in range(2))
    for t in (a, b):
        t.load(x, y)
    a.train(3, LR, REG)
    b.train(1, LR, REG)
    b.train(2, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params)
    assert torch.equal(a.engine.X, b.engine.X) and torch.equal(a.engine.shifts(), b.engine.shifts())
    assert torch.equal(a.engine.transforms(), b.engine.transforms()) and a.engine.transforms().any()


def test_two_ranks_sharing_the_gpu(tmp_path):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.affine_workers import gpu_shared_affine_main; " \
           f"gpu_shared_affine_main({str(tmp_path)!r}, 384, 128, 5, {Affine(**AUG).to_meta()!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        z = dict(np.load(tmp_path / f"gpu_affine{rank}.npz"))
        for k in ("x_equal", "y_equal", "agree", "perm2_equal", "shifts2_equal", "transforms2_equal"):
            assert float(z[k]) == 1.0, (rank, k, str(z["impl"]))
        assert float(z["launches_1"]) == 1.0 and float(z["shuffle_launches"]) == 0.0 and float(z["iter"]) == 6.0
