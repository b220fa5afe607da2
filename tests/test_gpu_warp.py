"""Elastic distortion on the GPU (csrc/mlp/warp.hip, MlpEngine.enqueue_augment with an augment.Warp, the trainers'
augment=): the kernel's nodes, shifts, transforms and order against the host's, every resident layout against a fresh
load of the host-warped permuted set, the launcher's refusals, and training, evaluation, keep-best and two ranks
bitwise against the reload-per-epoch twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import (Affine, Warp, apply_affine, apply_warp, epoch_nodes, epoch_shifts,
                                     epoch_transforms)
from cme213_sp18_amd.optim import Optimizer
from cme213_sp18_amd.parallel import DataParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests.resident_layouts import LAYOUTS, engine as _engine, same_layouts as _same_layouts
from tests.test_gpu_affine import SHAPES, _data, loadable, perm_of, resident

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


def warped(x, y, aug, seed, key, dtype="f32"):
    """The host's epoch: (x[perm] through entries[perm], shifts[perm] and nodes[perm], y[perm], perm, shifts[perm],
    index[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh = epoch_shifts(n, aug, key)[perm]
    idx = epoch_transforms(n, aug, key)[perm]
    rows = apply_warp(resident(x, dtype)[perm], sh, aug.table()[idx], epoch_nodes(n, aug, key)[perm], aug, h, w)
    return loadable(rows), y[perm], perm, sh, idx


def _probe(N):
    """8 x 8 images whose pixels make the field observable: a ramp along x and along y (never zero), steep enough that
    a displacement of a fraction of a pixel changes the blended byte."""
    yy, xx = np.mgrid[0:8, 0:8]
    img = (16 + 24 * xx + 5 * yy).astype(np.uint8).reshape(-1)
    x = np.tile(img, (N, 1))
    x[1::2] = (16 + 5 * xx + 24 * yy).astype(np.uint8).reshape(-1)
    return x, (np.arange(N) % 10).astype(np.int32)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 200])
def test_kernel_nodes_shifts_transforms_and_order_equal_the_host(N):
    x, y = _probe(N)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    for seed, key in ((0, 0), (9, 4), (2**32 - 1, 2**32 - 1)):
        aug = Warp(3.0, (2, 3), rotate=5, max_dx=1, seed=seed)
        for shuffle_seed in (seed, None):
            e.enqueue_augment(aug, key, shuffle_seed)
            perm = perm_of(N, shuffle_seed, key)
            assert np.array_equal(e.permutation().cpu().numpy(), perm), (seed, key, shuffle_seed)
            sh, idx = epoch_shifts(N, aug, key)[perm], epoch_transforms(N, aug, key)[perm]
            assert np.array_equal(e.shifts().cpu().numpy(), sh), (seed, key)
            assert np.array_equal(e.transforms().cpu().numpy(), idx), (seed, key)
            # the nodes, through the pixels they move: the host's rows with the host's nodes, and not the rows without
            rows = x[perm]
            want = apply_warp(rows, sh, aug.table()[idx], epoch_nodes(N, aug, key)[perm], aug, 8, 8)
            got = e.X.cpu().numpy()
            assert np.array_equal(got, want), (seed, key, shuffle_seed)
            still = apply_affine(rows, sh, aug.table()[idx], 8, 8)
            assert all((got[i] != still[i]).any() for i in range(N)), "the field moved no pixel of a sample"
    e.unshuffle()
    assert torch.equal(e.permutation().cpu(), torch.arange(N, dtype=torch.int32))
    assert not e.shifts().any() and not e.transforms().any()
    assert torch.equal(e.X.cpu(), torch.from_numpy(x))


def _policies(name, h, w, seed=4):
    square = {} if h == w else {"height": h, "width": w}
    small = dict(max_dx=min(2, w - 1), max_dy=min(2, h - 1), seed=seed, **square)
    if name == "mild":
        return [Warp(3.0, 3, rotate=15, scale=(0.9, 1.1), shear=10, **small)]
    if name == "extreme":  # taps leave every side of the image, and some images have no taps at all
        full = dict(rotate=180, scale=(0.25, 4), max_dx=w - 1, max_dy=h - 1, seed=seed, **square)
        return [Warp(8.0, (5, 1), **full), Warp(8.0, (1, 5), **full)]
    return [Warp(0.0, 3, rotate=15, scale=(0.9, 1.1), shear=10, **small)]


@pytest.mark.parametrize("policy", ["mild", "extreme", "still"])
@pytest.mark.parametrize("path,dtype,H,h,w,N,held", SHAPES)
def test_every_layout_equals_a_fresh_load_of_the_warped_permuted_set(path, dtype, H, h, w, N, held, policy):
    x, y = _data(path, N, h * w)
    for aug in _policies(policy, h, w):
        e = _engine(path, dtype, H, x, y, keep=True)
        assert e.path == path and all(getattr(e, n) is not None for n in ("X", "XT", "labels") + held)
        ptrs = {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
        for key, seed in ((0, 3), (7, 3), (7, None)):  # each state derives from the pristine rows, not the last one
            e.enqueue_augment(aug, key, seed)
            xa, ya, perm, sh, idx = warped(x, y, aug, seed, key, dtype)
            assert np.array_equal(e.shifts().cpu().numpy(), sh) and np.array_equal(e.permutation().cpu().numpy(), perm)
            assert np.array_equal(e.transforms().cpu().numpy(), idx)
            _same_layouts(e, _engine(path, dtype, H, xa, ya), f"{aug!r} key {key} seed {seed}")
        if policy == "still":  # ... which must equal the Affine launch's layouts
            f = _engine(path, dtype, H, x, y, keep=True)
            f.enqueue_augment(aug.affine, 7, None)
            _same_layouts(e, f, "the Affine launch")
            assert torch.equal(e.shifts(), f.shifts()) and torch.equal(e.transforms(), f.transforms())
            assert f.affine_launches == 1 and f.warp_launches == 0
        e.unshuffle()
        _same_layouts(e, _engine(path, dtype, H, x, y), "unshuffle")
        assert ptrs == {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
        assert e.warp_launches == 3 and e.affine_launches == 0 and e.augment_launches == 0
        assert e.shuffle_launches == 1
        assert not e.shifts().any() and not e.transforms().any()


def test_the_launcher_refuses_bad_tables_grids_bounds_and_kinds():
    from cme213_sp18_amd._native import hip

    x, y = _probe(20)
    e = _engine("split3", "f32", 16, x, y, keep=True)
    aug = Warp(2.0, 3, rotate=15, max_dx=1)
    e.prepare_augment(aug)
    table, axes = e._affine_table[1].data_ptr(), e._warp_axes[1].data_ptr()

    def launch(tab=table, T=1024, kind=0, ax=axes, gy=3, gx=3, A=512, h=8, w=8):
        e._gather_launch(hip().mlp_warp, e._shifts.data_ptr(), e._transforms.data_ptr(), tab, T, kind, ax, gy, gx, A,
                         20, 64, 1, h, w, 1, 1, 0, 0, 0, 0)

    for bad in (dict(tab=0), dict(tab=table + 4, T=1023), dict(T=0), dict(T=65537), dict(ax=0), dict(ax=axes + 2),
                dict(gy=0), dict(gy=6), dict(gx=0), dict(gx=6), dict(A=-1), dict(A=2049), dict(kind=2), dict(kind=7),
                dict(h=7, w=9)):
        with pytest.raises(Exception):
            launch(**bad)
    launch()
    torch.cuda.synchronize()
    assert np.array_equal(e.transforms().cpu().numpy(), epoch_transforms(20, aug, 0))
    want = apply_warp(x, epoch_shifts(20, aug, 0), aug.table()[epoch_transforms(20, aug, 0)], epoch_nodes(20, aug, 0),
                      aug, 8, 8)
    assert np.array_equal(e.X.cpu().numpy(), want)


def _trainer(shape, dtype, B, executor, seed=None, aug=None, **kw):
    return DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor,
                               shuffle_seed=seed, augment=aug, **kw)


def _twin(shape, dtype, B, executor, x, y, aug, seed, epochs, **kw):
    """Reload per epoch: load the host's warped epoch + train(1), ``iter`` carried."""
    tw = _trainer(shape, dtype, B, executor, **kw)
    for _ in range(epochs):
        xa, ya = warped(x, y, aug, seed, tw.iter)[:2]
        tw.load(xa, ya)
        tw.train(1, LR, REG)
    return tw


AUG = dict(alpha=4.0, grid=3, rotate=10, scale=(0.9, 1.1), max_dx=2, seed=4)


@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
def test_warped_training_is_bitwise_the_reload_per_epoch_twin(executor):
    shape, N, seed = (784, 100, 10), 256, 5
    x, y = synthetic_mnist(N, seed=3)
    aug = Warp(**AUG)
    plain = _trainer(shape, "f32", 64, executor, seed=seed, aug=aug.affine)
    plain.load(x, y)
    plain.train(3, LR, REG)
    tr = _trainer(shape, "f32", 64, executor, seed=seed, aug=aug)
    tr.load(x, y)
    tr.train(3, LR, REG)
    tw = _twin(shape, "f32", 64, executor, x, y, aug, seed, 3)
    torch.cuda.synchronize()
    assert tr.iter == tw.iter
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert not torch.equal(tr.engine.params, plain.engine.params)  # (the field reached the step kernels)
    assert tr.engine.warp_launches == 3 and tr.engine.affine_launches == 0 and tr.engine.augment_launches == 0
    assert tr.engine.shuffle_launches == 0
    assert tw.engine.warp_launches == 0 and tw.engine.shuffle_launches == 0
    # the one-launch pipeline still takes the epoch: as with the affine policy
    assert tr.engine._hip_step().xstep_used == plain.engine._hip_step().xstep_used
    if executor == "auto":
        assert tr.native_plan(tr.epoch_plan()) is not None  # the gather keeps "consecutive full batches" true


def test_adam_eval_every_and_keep_best_from_graphs_equal_the_twin():
    shape, N, seed = (784, 100, 10), 256, 5
    x, y = synthetic_mnist(N, seed=3)
    xv, yv = synthetic_mnist(150, seed=8)
    aug = Warp(**AUG)
    tr = _trainer(shape, "f32", 64, "graph", seed=seed, aug=aug, optimizer=Optimizer.adam())
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(3, 0.001, REG, eval_every=1, keep_best="loss")
    tw = _trainer(shape, "f32", 64, "graph", optimizer=Optimizer.adam())
    tw.load_eval(xv, yv)
    want = []
    for _ in range(3):
        xa, ya = warped(x, y, aug, seed, tw.iter)[:2]
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
    assert torch.equal(tr.engine._eval["X"].cpu(), torch.from_numpy(xv))  # the validation set is never warped
    assert tr.engine.warp_launches == 3


def test_train_1_plus_2_equals_train_3():
    x, y = synthetic_mnist(256, seed=3)
    aug = Warp(**AUG)
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
    assert a.engine.warp_launches == b.engine.warp_launches == 3


def test_two_ranks_sharing_the_gpu(tmp_path):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.warp_workers import gpu_shared_warp_main; " \
           f"gpu_shared_warp_main({str(tmp_path)!r}, 384, 128, 5, {Warp(**AUG).to_meta()!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        z = dict(np.load(tmp_path / f"gpu_warp{rank}.npz"))
        for k in ("x_equal", "y_equal", "agree", "perm2_equal", "shifts2_equal", "transforms2_equal", "x2_equal"):
            assert float(z[k]) == 1.0, (rank, k, str(z["impl"]))
        assert float(z["launches_1"]) == 1.0 and float(z["shuffle_launches"]) == 0.0 and float(z["iter"]) == 6.0
        assert float(z["other_launches"]) == 0.0
