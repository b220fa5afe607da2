"""Affine augmentation above the kernel: the rule of csrc/mlp/affine.h through _cpu.affine_table /
_cpu.epoch_transforms / _cpu.affine_rows against restatements in Python integers and exact fractions, its distance from
a plain fp64 bilinear resampling, the torch-backend engine and trainers, the augmented fp64 oracle, loopback ranks and
the CLI's --augment-rotate / --augment-scale / --augment-shear / --augment-table."""
import json
import math
import os
import subprocess
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd import augment as augment_mod
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import Affine, Shift, apply_affine, apply_shifts, epoch_shifts, epoch_transforms
from cme213_sp18_amd.config import parse_config
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
TABLE_STREAM, INDEX_STREAM, AUGMENT_STREAM = 0x3c6ef372fe94f82b, 0x71374491b5c0fbcf, 0xa5a5c3c35a5a3c3c
EXTREME = dict(rotate=180, scale=(0.25, 4), shear=45)
MILD = dict(rotate=15, scale=(0.9, 1.1), shear=10, max_dx=2)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def uniforms(seed, k):
    s0 = mix64(seed ^ TABLE_STREAM)
    return [(mix64((s0 + (3 * k + j + 1) * GOLDEN) & M64) >> 11) * 2.0 ** -53 for j in range(3)]


def inverse_map(seed, k, rotate, lo, hi, shear):
    """The unquantised inverse of A = s R(theta) [[1, tan phi], [0, 1]] of table entry k, in the header's order."""
    u1, u2, u3 = uniforms(seed, k)
    rad = 3.14159265358979323846 / 180.0
    theta, s, phi = rotate * (2.0 * u1 - 1.0) * rad, lo + (hi - lo) * u2, shear * (2.0 * u3 - 1.0) * rad
    c, sn, t, inv = math.cos(theta), math.sin(theta), math.tan(phi), 1.0 / s
    return [(c + t * sn) * inv, (sn - t * c) * inv, -sn * inv, c * inv]


def taps_of(y, x, dx, dy, q, h, w):
    """Python integers (unbounded, floor shifts): [(weight, source feature)] of the present taps, in the order 00, 01,
    10, 11."""
    u, v = 2 * x - (w - 1) - 2 * dx, 2 * y - (h - 1) - 2 * dy
    sx = q[0] * u + q[1] * v + (w - 1) * 65536
    sy = q[2] * u + q[3] * v + (h - 1) * 65536
    ix, iy, fx, fy = sx >> 17, sy >> 17, (sx >> 9) & 255, (sy >> 9) & 255
    out = []
    for ty, tx, wt in ((iy, ix, (256 - fy) * (256 - fx)), (iy, ix + 1, (256 - fy) * fx),
                       (iy + 1, ix, fy * (256 - fx)), (iy + 1, ix + 1, fy * fx)):
        if wt != 0 and 0 <= ty < h and 0 <= tx < w:
            out.append((wt, ty * w + tx))
    return out


def restated_u8(x, shifts, entries, h, w):
    out = np.zeros_like(x)
    for i in range(x.shape[0]):
        q, (dx, dy) = [int(v) for v in entries[i]], (int(v) for v in shifts[i])
        row = [int(v) for v in x[i]]
        for yy in range(h):
            for xx in range(w):
                total = sum(wt * row[sf] for wt, sf in taps_of(yy, xx, dx, dy, q, h, w))
                out[i, yy * w + xx] = (total + 32768) >> 16
    return out


def restated_float(x, shifts, entries, h, w, final):
    """Exact products and sums as fractions, rounded to a double once per operation (float(Fraction) is correctly
    rounded): no fma of the platform enters.  ``final``: double -> the element."""
    out = np.zeros_like(x)
    for i in range(x.shape[0]):
        q, (dx, dy) = [int(v) for v in entries[i]], (int(v) for v in shifts[i])
        row = [Fraction(float(v)) for v in x[i]]
        for yy in range(h):
            for xx in range(w):
                acc = None
                for wt, sf in taps_of(yy, xx, dx, dy, q, h, w):
                    acc = float(wt * row[sf]) if acc is None else float(wt * row[sf] + Fraction(acc))
                if acc is not None:
                    out[i, yy * w + xx] = final(float(Fraction(acc) / 65536))
    return out


def _policy_arrays(aug, n, key):
    return epoch_shifts(n, aug, key), aug.table()[epoch_transforms(n, aug, key)]


@pytest.mark.parametrize("h,w", [(28, 28), (5, 6), (21, 37), (1, 7), (1, 1)])
def test_uint8_rule_equals_the_python_integer_restatement(h, w):
    rng = np.random.default_rng(h * 100 + w)
    n = 6
    x = rng.integers(0, 256, (n, h * w)).astype(np.uint8)
    x[0] = 255
    for kw in (dict(EXTREME, max_dx=w - 1, max_dy=h - 1), dict(MILD, max_dx=min(2, w - 1), max_dy=min(2, h - 1))):
        aug = Affine(**kw, height=h, width=w, seed=5)
        sh, en = _policy_arrays(aug, n, 3)
        got = apply_affine(x, sh, en, h, w)
        assert got.dtype == np.uint8 and np.array_equal(got, restated_u8(x, sh, en, h, w))


@pytest.mark.parametrize("h,w", [(5, 6), (8, 9)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, "bf16"])
def test_float_rule_equals_the_fraction_restatement(h, w, dtype):
    rng = np.random.default_rng(h * 100 + w)
    n = 8
    vals = (rng.random((n, h * w)) - 0.3) * 3.0
    aug = Affine(**EXTREME, max_dx=w - 1, max_dy=h - 1, height=h, width=w, seed=5)
    sh, en = _policy_arrays(aug, n, 3)
    if dtype == "bf16":
        bits = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        as_f32 = (bits.astype(np.uint32) << 16).view(np.float32)

        def rne(v):  # the double -> f32 (one rounding) -> bf16 (round to nearest even on the bits)
            b = int(np.float32(v).view(np.uint32))
            return np.float32(np.uint32(((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16).view(np.float32))

        want = restated_float(as_f32, sh, en, h, w, rne)
        got = apply_affine(bits, sh, en, h, w)
        assert got.dtype == np.uint16
        assert np.array_equal((got.astype(np.uint32) << 16).view(np.float32).view(np.uint32), want.view(np.uint32))
        return
    x = vals.astype(dtype)
    got = apply_affine(x, sh, en, h, w)
    want = restated_float(x, sh, en, h, w, dtype)
    view = np.uint32 if dtype is np.float32 else np.uint64
    assert got.dtype == x.dtype and np.array_equal(got.view(view), want.view(view))
    assert (got == 0).any() and (got != 0).any()  # pixels without a tap, and blended ones


def test_table_equals_the_restated_formulas_and_identity_parameters_give_identity_entries():
    for kw in (dict(rotate=15.0, lo=0.9, hi=1.1, shear=10.0), dict(rotate=180.0, lo=0.25, hi=4.0, shear=45.0),
               dict(rotate=0.0, lo=1 / 16, hi=16.0, shear=60.0)):
        for seed in (0, 7, 2**32 - 1):
            aug = Affine(kw["rotate"], (kw["lo"], kw["hi"]), kw["shear"], seed=seed, table=64)
            tab = aug.table()
            assert tab.dtype == np.int32 and tab.shape == (64, 4) and not tab.flags.writeable
            want = np.array([[round(m * 65536.0) for m in inverse_map(seed, k, **kw)] for k in range(64)])
            # the same formulas in the same order through the same libm: equal, but for a product and a sum that a
            # compiler may contract into one fma -- one rounding of a double of magnitude < 2^23 apart, which moves
            # the rounded Q16 value by at most one step
            assert np.abs(tab.astype(np.int64) - want).max() <= 1
            assert np.abs(tab).max() < 1 << 23
    for seed in (0, 9):
        assert np.array_equal(Affine(0, 1, 0, seed=seed, table=33).table(), np.tile([65536, 0, 0, 65536], (33, 1)))
    assert np.array_equal(Affine(0, (1.0, 1.0), 0.0, max_dx=3).table()[5], [65536, 0, 0, 65536])
    a = Affine(**MILD, seed=3)
    assert np.array_equal(a.table(), Affine(**MILD, seed=3).table()) and a.table_checksum() == Affine(
        **MILD, seed=3).table_checksum()
    assert not np.array_equal(a.table(), Affine(**MILD, seed=4).table())
    assert a.table_checksum() != Affine(**MILD, seed=4).table_checksum() and 0 <= a.table_checksum() < 1 << 64


def test_epoch_transforms_restated_cover_the_table_and_differ_between_epochs():
    aug = Affine(**MILD, seed=7, table=1024)
    key = mix64((((7 << 32) ^ 1234) ^ AUGMENT_STREAM) & M64)  # augment_key(seed, iter)
    k2 = mix64(key ^ INDEX_STREAM)
    want = [((mix64((k2 + (i + 1) * GOLDEN) & M64) & 0xffffffff) * 1024) >> 32 for i in range(500)]
    assert np.array_equal(epoch_transforms(500, aug, 1234), want)
    t = epoch_transforms(60000, aug, 0)
    assert t.dtype == np.int32 and t.min() == 0 and t.max() == 1023
    counts = np.bincount(t, minlength=1024)
    assert counts.min() > 20 and counts.max() < 110  # mean 58.6, sd 7.7: beyond six sd either way
    assert not np.array_equal(t, epoch_transforms(60000, aug, 75))
    assert np.array_equal(t[:100], epoch_transforms(100, aug, 0))  # the sample's own: the set's size does not enter
    assert not epoch_transforms(100, Affine(**MILD, table=1), 5).any()
    assert np.array_equal(epoch_shifts(300, aug, 9), epoch_shifts(300, Shift(2, seed=7), 9))  # the shifts are Shift's


def bilinear_fp64(x, shifts, maps, h, w):
    """A plain fp64 bilinear resampling through the unquantised inverse maps, zeros outside the image."""
    n = x.shape[0]
    src = np.zeros((n, h + 2, w + 2))
    src[:, 1:-1, 1:-1] = x.reshape(n, h, w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w))
    for i in range(n):
        m, (dx, dy) = maps[i], shifts[i]
        u, v = xx - (w - 1) / 2 - dx, yy - (h - 1) / 2 - dy
        sx, sy = m[0] * u + m[1] * v + (w - 1) / 2, m[2] * u + m[3] * v + (h - 1) / 2
        ix, iy = np.floor(sx), np.floor(sy)
        fx, fy = sx - ix, sy - iy
        ix, iy = np.clip(ix, -1, w - 1).astype(int) + 1, np.clip(iy, -1, h - 1).astype(int) + 1
        inside = (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
        blend = ((1 - fy) * (1 - fx) * src[i, iy, ix] + (1 - fy) * fx * src[i, iy, np.minimum(ix + 1, w + 1)]
                 + fy * (1 - fx) * src[i, np.minimum(iy + 1, h + 1), ix]
                 + fy * fx * src[i, np.minimum(iy + 1, h + 1), np.minimum(ix + 1, w + 1)])
        out[i] = np.where(inside, blend, 0.0)
    return out.reshape(n, h * w)


@pytest.mark.parametrize("h,w", [(28, 28), (5, 6), (21, 37)])
def test_uint8_rule_is_within_3_grey_levels_of_fp64_bilinear(h, w):
    """255 * (2 / 256) from the two truncated fractions + 0.5 from the final rounding + the Q16 quantisation."""
    rng = np.random.default_rng(h * 100 + w)
    n, T, seed = 96, 64, 11
    x = rng.integers(0, 256, (n, h * w)).astype(np.uint8)
    aug = Affine(**EXTREME, max_dx=2, max_dy=2, height=h, width=w, seed=seed, table=T)
    sh, idx = epoch_shifts(n, aug, 3), epoch_transforms(n, aug, 3)
    got = apply_affine(x, sh, aug.table()[idx], h, w).astype(np.float64)
    maps = [inverse_map(seed, int(k), 180.0, 0.25, 4.0, 45.0) for k in idx]
    worst = np.abs(got - bilinear_fp64(x.astype(np.float64), sh, maps, h, w)).max()
    print(f"{h}x{w}: worst difference {worst:.3f} grey levels")
    assert worst <= 3.0


def test_affine_validates_and_round_trips():
    a = Affine(12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=77)
    assert (a.rotate, a.scale, a.shear, a.max_dx, a.max_dy, a.seed, a.table_size) == (12.5, (0.8, 1.25), 5.0, 2, 1, 4, 77)
    assert a.shape(784) == (28, 28) and a.to_meta()["kind"] == "affine" and a.table().shape == (77, 4)
    assert Affine.from_meta(json.loads(json.dumps(a.to_meta()))) == a and Affine.from_meta(None) is None
    assert augment_mod.from_meta(a.to_meta()) == a and augment_mod.from_meta(None) is None
    assert augment_mod.from_meta(Shift(2, seed=3).to_meta()) == Shift(2, seed=3)
    assert a != Affine(12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=78) and a != Shift(2, 1, seed=4)
    assert Affine(10, 1.5).scale == (1.5, 1.5) and Affine(3, height=5, width=6).shape(30) == (5, 6)
    assert "Affine(rotate=12.5" in repr(a)
    with pytest.raises(ValueError):
        Shift.from_meta(a.to_meta())  # a foreign kind, as before
    for bad in (lambda: Affine(-1), lambda: Affine(181), lambda: Affine(shear=61), lambda: Affine(scale=(0.05, 1)),
                lambda: Affine(scale=(1.2, 1.1)), lambda: Affine(scale=17), lambda: Affine(table=0),
                lambda: Affine(table=65537), lambda: Affine(max_dx=-1), lambda: Affine(seed=2**32),
                lambda: Affine(height=5), lambda: Affine(max_dx=6, height=5, width=6), lambda: a.shape(30),
                lambda: augment_mod.from_meta({"kind": "elastic"}), lambda: Affine.from_meta(Shift(2).to_meta())):
        with pytest.raises(ValueError):
            bad()
    x = np.zeros((2, 30), np.uint8)
    for bad in (lambda: apply_affine(x, np.zeros((2, 2)), np.zeros((2, 4)), 5, 7),
                lambda: apply_affine(x, np.zeros((3, 2)), np.zeros((2, 4)), 5, 6),
                lambda: apply_affine(x, np.zeros((2, 2)), np.zeros((2, 3)), 5, 6),
                lambda: apply_affine(x, np.full((2, 2), 6), np.zeros((2, 4)), 5, 6),
                lambda: apply_affine(x, np.zeros((2, 2)), np.full((2, 4), 1 << 23), 5, 6),
                lambda: apply_affine(x.astype(np.int32), np.zeros((2, 2)), np.zeros((2, 4)), 5, 6)):
        with pytest.raises(ValueError):
            bad()


def resident(x, dtype):
    """The rows as the engine of that dtype keeps them (what the rule blends); bf16 as its bits (uint16)."""
    if dtype == "u8":
        return x
    if dtype == "f64":
        return np.ascontiguousarray(x, np.float64)
    x32 = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x32
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def loadable(rows):
    if rows.dtype == np.uint16:
        return torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy()
    return rows


def perm_of(n, seed, key):
    return np.arange(n, dtype=np.int32) if seed is None else cpu().epoch_permutation(n, seed, key)


def augmented(x, y, aug, seed, key, kind="u8"):
    """The host's epoch: (x[perm] through entries[perm] and shifts[perm], y[perm], perm, shifts[perm], index[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh, idx = epoch_shifts(n, aug, key)[perm], epoch_transforms(n, aug, key)[perm]
    return loadable(apply_affine(resident(x, kind)[perm], sh, aug.table()[idx], h, w)), y[perm], perm, sh, idx


def _engine(x, y, dtype="f32", path="auto", keep=False, H=16):
    e = MlpEngine((x.shape[1], H, 10), dtype=dtype, max_cols=64, device="cpu", backend="torch", path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


KINDS = {("f32", "split3"): "u8", ("f64", "mfma"): "f64", ("f32", "mfma"): "f32", ("bf16", "mfma"): "bf16"}


@pytest.mark.parametrize("dtype,path", list(KINDS))
@pytest.mark.parametrize("seed", [None, 5])
def test_torch_engine_affine_equals_a_fresh_load(dtype, path, seed):
    x, y = synthetic_mnist(75, seed=2)
    if path == "mfma":  # non-integer values, so that the engine keeps them in the element type
        x = x.astype(np.float64) / 255.0 + 0.125
    aug = Affine(**MILD, seed=4)
    e = _engine(x, y, dtype, path, keep=True)
    assert e.path == path
    names = [n for n in ("X", "XT", "labels") if getattr(e, n) is not None]
    ptrs = [getattr(e, n).data_ptr() for n in names]
    assert not e.transforms().any() and e.transforms().shape == (75,) and e.transforms().dtype == torch.int32
    for key in (0, 9):  # the second is a fresh load of the second epoch's set: not composed with the first
        e.enqueue_augment(aug, key, seed)
        xa, ya, perm, sh, idx = augmented(x, y, aug, seed, key, KINDS[dtype, path])
        assert sh.any() and idx.any()
        f = _engine(xa, ya, dtype, path)
        assert np.array_equal(e.permutation().numpy(), perm) and np.array_equal(e.shifts().numpy(), sh)
        assert np.array_equal(e.transforms().numpy(), idx)
        for name in names:
            assert torch.equal(getattr(e, name), getattr(f, name)), (name, key)
    e.enqueue_augment(Shift(2, seed=4), 9, seed)  # a Shift takes no transform
    assert not e.transforms().any() and e.shifts().any()
    e.enqueue_augment(aug, 9, seed)
    e.unshuffle()
    f = _engine(x, y, dtype, path)
    for name in names:
        assert torch.equal(getattr(e, name), getattr(f, name)), name
    assert np.array_equal(e.permutation().numpy(), np.arange(75)) and not e.shifts().any()
    assert not e.transforms().any()
    assert ptrs == [getattr(e, n).data_ptr() for n in names]  # rewritten in place
    assert e.affine_launches == 0 and e.augment_launches == 0  # (the kernels' counters: the hip backend's)


def _trainer(seed=None, aug=None, H=16, B=64, dtype="f64", cls=DataParallelTrainer, comm=None):
    nn = NeuralNetwork([784, H, 10])
    kw = dict(use_graphs=False) if cls is DataParallelTrainer else {}
    if comm is not None:
        kw["comm"] = comm
    return cls(nn, device="cpu", dtype=dtype, batch_size=B, backend="torch", shuffle_seed=seed, augment=aug, **kw)


def _twin_epochs(twin, x, y, aug, seed, epochs, lr, reg):
    """The reload-per-epoch twin: load the host's augmented epoch and train(1), ``iter`` carried."""
    for _ in range(epochs):
        xa, ya = augmented(x, y, aug, seed, twin.iter, "f64")[:2]
        twin.load(xa, ya)
        twin.train(1, lr, reg)


def test_identity_transforms_are_bitwise_a_shift():
    s = 9
    ident, shift = Affine(0, 1, 0, max_dx=2, seed=s), Shift(2, seed=s)
    x, y = synthetic_mnist(100, seed=3)
    sh = epoch_shifts(100, ident, 6)
    en = ident.table()[epoch_transforms(100, ident, 6)]
    assert np.array_equal(sh, epoch_shifts(100, shift, 6))
    rng = np.random.default_rng(0)
    floats = rng.random(x.shape) - 0.5
    floats[0, :5] = [-0.0, 0.0, np.inf, -np.inf, 5e-324]
    for rows in (x, floats, floats.astype(np.float32), resident(floats, "bf16")):
        a, b = apply_affine(rows, sh, en, 28, 28), apply_shifts(rows, sh, 28, 28)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for dtype, path in (("f32", "split3"), ("f64", "mfma")):
        e, f = (_engine(x, y, dtype, path, keep=True) for _ in range(2))
        e.enqueue_augment(ident, 6, 4)
        f.enqueue_augment(shift, 6, 4)
        for name in ("X", "XT", "labels"):
            assert torch.equal(getattr(e, name), getattr(f, name)), name
        assert torch.equal(e.shifts(), f.shifts()) and torch.equal(e.permutation(), f.permutation())
    a, b = _trainer(6, ident), _trainer(6, shift)
    for t in (a, b):
        t.load(x, y)
        t.train(2, 0.05, 1e-4)
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.X, b.engine.X)


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
@pytest.mark.parametrize("seed", [None, 6])
def test_torch_trainer_equals_the_reload_per_epoch_twin(cls, seed):
    x, y = synthetic_mnist(200, seed=3)  # batch 64: three full batches and a remainder of 8
    aug = Affine(**MILD, seed=4)
    tr = _trainer(seed, aug, cls=cls)
    tr.load(x, y)
    assert tr.engine.X0 is not None and tr.engine._affine_table is not None  # (the table is uploaded by load())
    tr.train(3, 0.05, 1e-4)
    twin = _trainer(None, None, cls=cls)
    _twin_epochs(twin, x, y, aug, seed, 3, 0.05, 1e-4)
    assert tr.iter == twin.iter == 12
    assert torch.equal(tr.engine.params, twin.engine.params)
    xa, _, perm, sh, idx = augmented(x, y, aug, seed, 8, "f64")  # the set stays in the last epoch's state
    assert torch.equal(tr.engine.X, torch.from_numpy(xa).to(tr.engine.X.dtype))
    assert np.array_equal(tr.engine.permutation().numpy(), perm) and np.array_equal(tr.engine.shifts().numpy(), sh)
    assert np.array_equal(tr.engine.transforms().numpy(), idx)
    shifted = _trainer(seed, Shift(2, seed=4), cls=cls)
    shifted.load(x, y)
    shifted.train(3, 0.05, 1e-4)
    assert not torch.equal(shifted.engine.params, tr.engine.params)  # the transforms matter
    assert np.array_equal(tr.predict(x[:50]), twin.predict(x[:50]))  # predict() is never augmented


def test_train_2_twice_equals_train_4_and_the_per_step_path():
    x, y = synthetic_mnist(200, seed=3)
    aug = Affine(**MILD, seed=4)
    a, b = _trainer(6, aug), _trainer(6, aug)
    for t in (a, b):
        t.load(x, y)
    a.train(4, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4, print_every=3, log=lambda *_: None)  # the host-in-the-loop path augments too
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.X, b.engine.X)
    with pytest.raises(ValueError):
        _trainer(None, Affine(10, height=5, width=6)).load(x, y)  # validated against the engine's P at load()


@pytest.mark.parametrize("seed", [None, 6])
def test_augmented_oracle_equals_the_manual_per_epoch_loop(seed):
    H, N, B, E, lr, reg = 24, 600, 200, 2, 0.05, 1e-4
    x, y = synthetic_mnist(N, seed=11)
    aug = Affine(**MILD, seed=3)
    for kind in ("u8", "f64"):  # bytes are blended as bytes (the trainers' resident pixels), anything else in fp64
        xin = resident(x, kind)
        seq = NeuralNetwork([784, H, 10])
        mlp.train(seq, xin, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed, augment=aug)
        man = NeuralNetwork([784, H, 10])
        it = 0
        for _ in range(E):
            xa, ya = augmented(x, y, aug, seed, it, kind)[:2]
            mlp.train(man, xa, ya, lr, reg, epochs=1, batch_size=B, iter0=it)
            it += 3
        for i in range(2):
            assert np.array_equal(seq.W[i], man.W[i]) and np.array_equal(seq.b[i], man.b[i])
    # ... and the f64 torch-backend trainer agrees with the fp64 form at the bound tests/test_dist.py holds the f64
    # engine to
    tr = _trainer(seed, aug, H=H, B=B)
    tr.load(x, y)
    tr.train(E, lr, reg)
    for i in range(2):
        assert np.abs(tr.nn.W[i] - seq.W[i]).max() / np.abs(seq.W[i]).max() < 1e-12
    plain = NeuralNetwork([784, H, 10])
    mlp.train(plain, x, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed)
    assert np.abs(plain.W[0] - seq.W[0]).max() / np.abs(seq.W[0]).max() > 1e-6


def _loopback(world, cls, x, y, B, epochs, seed, aug, twin):
    comms = LoopbackComm.create(world)
    out = [None] * world

    def work(r):
        torch.set_num_threads(1)
        tr = _trainer(None if twin else seed, None if twin else aug, H=24, B=B, cls=cls, comm=comms[r])
        if twin:
            _twin_epochs(tr, x, y, aug, seed, epochs, 0.05, 1e-4)
        else:
            tr.load(x, y)
            tr.train(epochs, 0.05, 1e-4)
        out[r] = (tr.engine.params.clone(), tr.engine.X.clone())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
def test_loopback_ranks_with_uneven_shards_equal_their_twin(cls):
    """Three ranks, batches of 200 and a last one of 100: shards of 66 and 33 columns.  Every rank forms the same
    pixels, and the run is bitwise the reload-per-epoch twin's."""
    x, y = synthetic_mnist(500, seed=11)
    aug = Affine(**MILD, seed=4)
    got = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=False)
    want = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=True)
    for r in range(3):
        assert torch.equal(got[r][1], got[0][1])  # the same pixels on every rank
        assert torch.equal(got[r][0], want[r][0]), r


def _cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "800", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_affine_checkpoint_and_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--augment-rotate", "15", "--augment-scale", "0.9:1.1", "--augment-shift", "2", "--augment-seed", "1",
             "--augment-table", "256")
    want = Affine(15, (0.9, 1.1), 0, max_dx=2, seed=1, table=256)
    log = tmp_path / "run.jsonl"
    _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "--log-json", str(log))
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert augment_mod.from_meta(meta["augment"]) == want and meta["epochs"] == 4
    assert meta["augment"]["kind"] == "affine" and int(meta["augment"]["table_checksum"], 16) == want.table_checksum()
    head = json.loads(log.read_text().splitlines()[0])
    assert head["event"] == "config" and head["augment"] == meta["augment"]  # the run header names the policy
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with augmentation" not in r.stdout
    assert "transform table has checksum" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])  # 2 of 4 epochs, resumed == the unbroken run
    # other flags: the policy's warning; the same flags and another table: the checksum's
    other = _cli(tmp_path, "--augment-rotate", "20", "--augment-seed", "1", "-e", "1", "--resume", half, "--ckpt-dir",
                 str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with augmentation" in other.stdout
    shifted = _cli(tmp_path, "--augment-shift", "2", "--augment-seed", "1", "-e", "1", "--resume", half)
    assert "warning: the checkpoint was trained with augmentation" in shifted.stdout
    half_meta = tmp_path / "half" / "meta.json"
    m = json.loads(half_meta.read_text())
    m["augment"]["table_checksum"] = f"{want.table_checksum() ^ 1:016x}"
    half_meta.write_text(json.dumps(m))
    odd = _cli(tmp_path, *flags, "-e", "1", "--resume", half)
    assert "transform table has checksum" in odd.stdout
    assert "warning: the checkpoint was trained with augmentation" not in odd.stdout


@pytest.mark.parametrize("argv", [("--augment-rotate", "181"), ("--augment-shear", "61"), ("--augment-scale", "0.01"),
                                  ("--augment-scale", "1.2:1.1"), ("--augment-scale", "a:b"),
                                  ("--augment-scale", "1:2:3"), ("--augment-rotate", "5", "--augment-table", "0"),
                                  ("--augment-table", "64"), ("--augment-shift", "2", "--augment-table", "64"),
                                  ("--augment-rotate", "5", "--image-shape", "28x27"),
                                  ("--augment-rotate", "5", "--augment-shift", "28")])
def test_cli_refuses_bad_flags_at_parse_time(argv, capsys):
    with pytest.raises(SystemExit) as ex:
        parse_config(list(argv))
    assert ex.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_cli_flags_make_the_policy():
    assert parse_config(["--augment-shift", "2", "--augment-seed", "9"]).augment == Shift(2, seed=9)  # as before
    assert parse_config(["--augment-rotate", "15"]).augment == Affine(15, 1.0, 0.0)
    assert parse_config(["--augment-scale", "0.9"]).augment == Affine(0, 0.9, 0)
    assert parse_config(["--augment-shear", "8", "--augment-seed", "3"]).augment == Affine(0, 1, 8, seed=3)
    cfg = parse_config(["--augment-rotate", "10", "--augment-scale", "0.8:1.25", "--augment-shear", "5",
                        "--augment-shift", "3", "--augment-shift-y", "1", "--image-shape", "16x49", "--augment-table",
                        "99", "--augment-seed", "2"])
    assert cfg.augment == Affine(10, (0.8, 1.25), 5, 3, 1, 16, 49, 2, 99)
