"""Sampling with replacement on the GPU (csrc/mlp/sample.h inside the four gather kernels, MlpEngine.prepare_sampler /
enqueue_shuffle / enqueue_augment with ``sampler=``, the trainers' ``sampler=``): every resident layout against a fresh
load of the host-drawn set, the augmentations keyed by the destination, the launchers' new arguments at their defaults,
and training on every executor bitwise against the reload-per-epoch twin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd.augment import (Affine, Shift, Warp, apply_affine, apply_shifts, apply_warp, epoch_nodes,
                                     epoch_shifts, epoch_transforms)
from cme213_sp18_amd.optim import Optimizer
from cme213_sp18_amd.parallel import DataParallelTrainer, MlpEngine
from cme213_sp18_amd.sampling import Balanced, Weighted
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests import sampling_cases as sc
from tests.resident_layouts import LAYOUTS, same_layouts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


def _engine(path, dtype, H, x, y, keep=False):
    e = MlpEngine((x.shape[1], H, 62), dtype=dtype, max_cols=64, path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


def _pixels(path, N, P):
    rng = np.random.default_rng(N + P)
    if path == "mfma":  # non-integer input, never zero (a zero marks a pixel moved in from outside)
        return rng.random((N, P)) * 0.5 + 0.25
    return rng.integers(1, 256, (N, P)).astype(np.uint8)


# path, dtype, H, P, the layouts held besides X / XT / labels
FORMS = [
    ("split3", "f32", 100, 784, ("Xs",)),         # 1-byte elements, 16-byte rows (VEC), the fragment-order copy
    ("split1", "bf16", 512, 784, ("Xw", "XTw")),  # 1-byte elements and the wide engines' bf16 copies
    ("mfma", "bf16", 100, 20, ()),                # 2-byte elements, 40-byte rows: one element per lane
    ("mfma", "f32", 100, 20, ()),                 # 4-byte elements, 80-byte rows (VEC)
    ("mfma", "f64", 100, 20, ()),                 # 8-byte elements
]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200, 1000])
@pytest.mark.parametrize("path,dtype,H,P,held", FORMS)
def test_every_layout_equals_a_fresh_load_of_the_host_drawn_set(path, dtype, H, P, held, N):
    x = _pixels(path, N, P)
    ran = 0
    for k, name in enumerate(sc.SETS):
        case = sc.policy_of(name, N, seed=k)
        if case is None:
            continue
        policy, y = case
        e = _engine(path, dtype, H, x, y, keep=True)
        assert e.path == path and all(getattr(e, n) is not None for n in ("X", "XT", "labels") + held)
        ptrs = {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
        for key in (0, 7 + k):  # each state derives from the pristine rows, not from the last one
            e.enqueue_shuffle(0, key, sampler=policy)
            d = policy.draws(y, key)
            assert np.array_equal(e.permutation().cpu().numpy(), d), (name, key)
            same_layouts(e, _engine(path, dtype, H, x[d], y[d]), f"{name} key {key}")
        if name == "one_nonzero":  # every destination reads the same row
            assert np.array_equal(d, np.full(N, N // 3)) and bool((e.X == e.X[0]).all())
        e.unshuffle()
        same_layouts(e, _engine(path, dtype, H, x, y), f"{name} unshuffle")
        assert ptrs == {n: getattr(e, n).data_ptr() for n in LAYOUTS if getattr(e, n) is not None}
        assert e.shuffle_launches == 3
        ran += 1
    assert ran >= 4


def _host_augmented(x, y, aug, policy, key, h, w):
    """The host's epoch with a sampler: x[draws] augmented with everything keyed by the DESTINATION."""
    n = x.shape[0]
    d = policy.draws(y, key)
    sh = epoch_shifts(n, aug, key)
    tf = None
    if isinstance(aug, (Affine, Warp)):
        tf = epoch_transforms(n, aug, key)
        entries = aug.table()[tf]
        if isinstance(aug, Warp):
            xa = apply_warp(x[d], sh, entries, epoch_nodes(n, aug, key), aug, h, w)
        else:
            xa = apply_affine(x[d], sh, entries, h, w)
    else:
        xa = apply_shifts(x[d], sh, h, w)
    return xa, y[d], d, sh, tf


AUGS = {"shift": lambda kw: Shift(2, seed=4, **kw), "affine": lambda kw: Affine(15.0, (0.9, 1.1), 5.0, 1, seed=4, **kw),
        "warp": lambda kw: Warp(3.0, 3, 10.0, (0.9, 1.1), 0.0, 1, seed=4, **kw)}


@pytest.mark.parametrize("kind", ["shift", "affine", "warp"])
@pytest.mark.parametrize("path,dtype,H,h,w,N", [("split3", "f32", 100, 28, 28, 65),
                                                ("split3", "f32", 100, 28, 28, 200),
                                                ("split1", "bf16", 512, 28, 28, 200),
                                                ("mfma", "f64", 100, 5, 4, 65)])
def test_augmenting_gathers_with_a_table_key_by_the_destination(path, dtype, H, h, w, N, kind):
    aug = AUGS[kind]({} if h == w else {"height": h, "width": w})
    x = _pixels(path, N, h * w)
    for name in ("zipf62_balanced", "one_nonzero"):
        policy, y = sc.policy_of(name, N, seed=3)
        e = _engine(path, dtype, H, x, y, keep=True)
        for key in (0, 5):
            e.enqueue_augment(aug, key, sampler=policy)
            xa, ya, d, sh, tf = _host_augmented(x, y, aug, policy, key, h, w)
            assert np.array_equal(e.permutation().cpu().numpy(), d)
            assert np.array_equal(e.shifts().cpu().numpy(), sh)
            if tf is not None:
                assert np.array_equal(e.transforms().cpu().numpy(), tf)
            same_layouts(e, _engine(path, dtype, H, xa, ya), f"{kind} {name} key {key}")
        if name == "one_nonzero" and N >= 65:
            # one source row at every destination, and the copies carry different augmentations
            assert len(set(d.tolist())) == 1 and len({tuple(s) for s in sh.tolist()}) > 5
            assert not bool((e.X == e.X[0]).all())
        e.unshuffle()
        same_layouts(e, _engine(path, dtype, H, x, y), "unshuffle")


@pytest.mark.parametrize("kind", ["shuffle", "shift", "affine", "warp"])
@pytest.mark.parametrize("path,dtype,H,N", [("split3", "f32", 100, 200), ("split1", "bf16", 512, 65),
                                            ("mfma", "f64", 100, 65)])
def test_null_sampler_arguments_are_the_launch_without_them(path, dtype, H, N, kind):
    """The launchers' new trailing arguments left at their defaults against the same launch with them passed
    explicitly as null: bitwise equal (the old tests pin the values; this pins the binding)."""
    h = w = 28 if path != "mfma" else 6
    x = _pixels(path, N, h * w)
    y = sc.zipf_labels(N)
    a, b = (_engine(path, dtype, H, x, y, keep=True) for _ in range(2))
    b._sampler_kw = lambda sampler: {"sample_table": 0, "sample_seed": 0}
    for seed, key in ((3, 0), (None, 9), (8, 2**32 - 1)):
        for e in (a, b):
            if kind == "shuffle":
                e.enqueue_shuffle(seed or 0, key)
            else:
                e.enqueue_augment(AUGS[kind]({}), key, seed)
        same_layouts(a, b, f"{kind} {seed} {key}")
        assert torch.equal(a.permutation(), b.permutation()) and torch.equal(a.shifts(), b.shifts())
        assert torch.equal(a.transforms(), b.transforms())
    assert a._sampler is None and b._sampler is None


# ---------------------------------------------------------------------------------------------------- training
def _imbalanced(n, classes=10, seed=3):
    x, _ = synthetic_mnist(n, seed=seed)
    return x, np.sort(sc.zipf_labels(n, classes=classes, seed=seed)).astype(np.int32)


def _trainer(shape, dtype, B, executor, sampler=None, **kw):
    return DataParallelTrainer(NeuralNetwork(list(shape)), dtype=dtype, batch_size=B, executor=executor,
                               sampler=sampler, **kw)


def _twin(shape, dtype, B, executor, x, y, sampler, epochs, lr=LR, **kw):
    """Reload per epoch: load the host-drawn set + train(1), ``iter`` carried."""
    tw = _trainer(shape, dtype, B, executor, **kw)
    for _ in range(epochs):
        d = sampler.draws(y, tw.iter)
        tw.load(x[d], y[d])
        tw.train(1, lr, REG)
    return tw


@pytest.mark.parametrize("executor", ["auto", "graph", "eager"])
@pytest.mark.parametrize("shape,dtype,N,B", [((784, 100, 10), "f32", 1600, 800),
                                             ((784, 100, 10), "bf16", 1600, 800),
                                             ((784, 100, 10), "f64", 1600, 800),
                                             ((784, 512, 10), "bf16", 130, 64)])  # the wide engines: Xw / XTw
def test_sampled_training_is_bitwise_the_reload_per_epoch_twin(shape, dtype, N, B, executor):
    x, y = _imbalanced(N)
    smp = Balanced(5)
    tr = _trainer(shape, dtype, B, executor, smp)
    tr.load(x, y)
    tr.train(3, LR, REG)
    tw = _twin(shape, dtype, B, executor, x, y, smp, 3)
    torch.cuda.synchronize()
    assert tr.iter == tw.iter
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert tr.engine.shuffle_launches == 3 and tw.engine.shuffle_launches == 0
    assert np.array_equal(tr.engine.permutation().cpu().numpy(), smp.draws(y, tr.iter - tr.iter // 3))
    if shape[1] == 512:
        assert tr.engine.Xw is not None and tr.engine.XTw is not None
    if executor == "auto" and dtype == "f32":
        assert tr.native_plan(tr.epoch_plan()) is not None  # the gather keeps "consecutive full batches" true


def test_train_2_plus_2_equals_train_4_and_captured_equals_eager():
    x, y = _imbalanced(1600)
    a, b, c = (_trainer((784, 100, 10), "f32", 800, ex, Balanced(5)) for ex in ("graph", "graph", "eager"))
    for t in (a, b, c):
        t.load(x, y)
    a.train(4, LR, REG)
    b.train(2, LR, REG)
    b.train(2, LR, REG)
    c.train(4, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.params, c.engine.params)
    assert torch.equal(a.engine.X, b.engine.X) and torch.equal(a.engine.permutation(), c.engine.permutation())


def test_adam_keep_best_balanced_and_warp_from_graphs_equal_the_twin():
    shape, N = (784, 100, 10), 400
    x, y = _imbalanced(N)
    xv, yv = synthetic_mnist(150, seed=8)
    smp, aug = Balanced(5), Warp(3.0, 3, 10.0, (0.9, 1.1), 0.0, 1, seed=4)
    tr = _trainer(shape, "f32", 200, "graph", smp, augment=aug, optimizer=Optimizer.adam())
    tr.load(x, y)
    tr.load_eval(xv, yv)
    st = tr.train(3, 0.001, REG, eval_every=1, keep_best="loss")
    tw = _trainer(shape, "f32", 200, "graph", optimizer=Optimizer.adam())
    tw.load_eval(xv, yv)
    want = []
    for _ in range(3):
        xa, ya, _, _, _ = _host_augmented(x, y, aug, smp, tw.iter, 28, 28)
        tw.load(xa, ya)
        want += tw.train(1, 0.001, REG, eval_every=1, keep_best="loss").evals
    torch.cuda.synchronize()
    assert torch.equal(tr.engine.params, tw.engine.params)
    assert tr.engine.warp_launches == 3 and tr.engine.shuffle_launches == 0
    for got, ref in zip(st.evals, want):
        assert got["loss"] == ref["loss"] and got["accuracy"] == ref["accuracy"]
    a, b = tr.best_state(), tw.best_state()
    for k in ("best_index", "best_metric", "evals", "stopped", "iter"):
        assert a[k] == b[k], k
    for got, ref in zip(tr.engine.best_params(), tw.engine.best_params()):
        np.testing.assert_array_equal(got, ref)
    assert torch.equal(tr.engine._eval["X"].cpu(), torch.from_numpy(xv))  # the validation set is never sampled


def test_a_recovery_snapshot_repeats_the_epochs_draws():
    x, y = _imbalanced(1600)
    a, b = (_trainer((784, 100, 10), "f32", 800, "graph", Balanced(5)) for _ in range(2))
    for t in (a, b):
        t.load(x, y)
    a.train(1, LR, REG)
    snap, it = a._snapshot(), a.iter
    a.train(1, LR, REG)  # the epoch a recovery discards
    first = a.engine.permutation().clone()
    a._restore(snap)
    a.iter = it
    a.train(1, LR, REG)
    b.train(2, LR, REG)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.permutation(), first) and torch.equal(a.engine.params, b.engine.params)


def test_two_ranks_sharing_the_gpu(tmp_path):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.sampling_workers import gpu_shared_sampling_main; " \
           f"gpu_shared_sampling_main({str(tmp_path)!r}, 384, 128, 5)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        z = dict(np.load(tmp_path / f"gpu_sampling{rank}.npz"))
        for k in ("x_equal", "y_equal", "agree", "perm2_equal"):
            assert float(z[k]) == 1.0, (rank, k, str(z["impl"]))
        assert float(z["launches_1"]) == 1.0 and float(z["iter"]) == 6.0


def test_without_a_sampler_nothing_is_kept_or_launched():
    x, y = _imbalanced(200)
    tr = _trainer((784, 100, 10), "f32", 64, "auto")
    tr.load(x, y)
    tr.train(2, LR, REG)
    e = tr.engine
    assert e.X0 is None and e._perm is None and e._sampler is None and e.shuffle_launches == 0
    with pytest.raises(RuntimeError):
        e.enqueue_shuffle(0, 0, sampler=Balanced())
    k = _engine("split3", "f32", 100, x, y, keep=True)
    with pytest.raises(ValueError):
        k.enqueue_shuffle(0, 0, sampler=Weighted(np.ones(199)))
