"""Elastic distortion above the kernel: the rule of csrc/mlp/warp.h through _cpu.warp_axes / _cpu.epoch_nodes /
_cpu.warp_field / _cpu.warp_rows against a restatement in Python integers written from the header comment, the integer
field against the fp64 B-spline field at the header's derived bound, whole images against a plain fp64 restatement, the
torch-backend engine and trainers, the warped fp64 oracle, loopback ranks and the CLI's --augment-warp /
--augment-warp-grid."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd import augment as augment_mod
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import (Affine, Shift, Warp, apply_affine, apply_shifts, apply_warp, epoch_nodes,
                                     epoch_shifts, epoch_transforms, warp_field)
from cme213_sp18_amd.config import parse_config
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
AUGMENT_STREAM, NODE_STREAM = 0xa5a5c3c35a5a3c3c, 0x8f1bbcdc6ed9eba1
SHAPES = [(28, 28), (5, 6), (21, 37), (8, 9)]
GRIDS = [(3, 3), (5, 5), (1, 1), (2, 3), (5, 1)]
MILD = dict(alpha=4.0, grid=3, rotate=15, scale=(0.9, 1.1), shear=10, max_dx=2)


# ---- the header comment, restated in Python integers
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def reduce_to(h32, m):
    return ((h32 * (2 * m + 1)) >> 32) - m


def restated_nodes(n, seed, it, L, A):
    key = mix64((((seed << 32) ^ it) ^ AUGMENT_STREAM) & M64)  # augment.h augment_key
    base = mix64(key ^ NODE_STREAM)
    out = np.zeros((n, L, 2), np.int32)
    for src in range(n):
        nk = mix64((base + (src + 1) * GOLDEN) & M64)
        for j in range(L):
            h = mix64((nk + (j + 1) * GOLDEN) & M64)
            out[src, j] = reduce_to(h & 0xffffffff, A), reduce_to(h >> 32, A)
    return out


def bspline(t):
    s = 1.0 - t
    return [s * s * s / 6.0, (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0,
            (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0, t * t * t / 6.0]


def restated_axis(n, g):
    rows = []
    for x in range(n):
        num, den = (2 * x + 1) * g, 2 * n
        i = num // den
        w = [round(b * 4096) for b in bspline((num - i * den) / den)]  # round(): to nearest, ties to even, as llrint
        w[w.index(max(w))] += 4096 - sum(w)
        rows.append([i] + w)
    return rows


def restated_axes(h, w, gy, gx):
    return np.array(restated_axis(h, gy) + restated_axis(w, gx), np.int32)


def restated_field(nodes_i, axes, h, w, gx):
    out = np.zeros((h, w, 2), np.int64)
    nd = [[int(v) for v in p] for p in nodes_i]
    ax = [[int(v) for v in e] for e in axes]
    for y in range(h):
        ay = ax[y]
        for x in range(w):
            ex = ax[h + x]
            for c in range(2):
                d = 0
                for a in range(4):
                    r = sum(ex[1 + b] * nd[(ay[0] + a) * (gx + 3) + ex[0] + b][c] for b in range(4))
                    assert abs(r) <= 2048 * 4096
                    d += ay[1 + a] * r
                out[y, x, c] = (d + (1 << 14)) >> 15
    return out


def real_field(nodes_i, h, w, gy, gx):
    """The fp64 cubic B-spline field of the same Q8 nodes, in pixels: [h][w][2]."""
    nd = np.asarray(nodes_i, np.float64).reshape(gy + 3, gx + 3, 2) / 256.0
    out = np.zeros((h, w, 2))
    for y in range(h):
        uy = (2 * y + 1) * gy / (2 * h)
        iy = min(int(np.floor(uy)), gy - 1)
        by = bspline(uy - iy)
        for x in range(w):
            ux = (2 * x + 1) * gx / (2 * w)
            ix = min(int(np.floor(ux)), gx - 1)
            bx = bspline(ux - ix)
            out[y, x] = sum(by[a] * bx[b] * nd[iy + a, ix + b] for a in range(4) for b in range(4))
    return out


@pytest.mark.parametrize("gy,gx", GRIDS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_nodes_axes_and_field_equal_the_python_restatement(h, w, gy, gx):
    aug = Warp(8.0, (gy, gx), height=h, width=w, seed=7)
    L = (gy + 3) * (gx + 3)
    assert aug.nodes == L and aug.bound == 2048
    nodes = epoch_nodes(6, aug, 5)
    assert nodes.shape == (6, L, 2) and nodes.dtype == np.int32
    assert np.array_equal(nodes, restated_nodes(6, 7, 5, L, 2048))
    axes = aug.axes(h, w)
    assert axes.shape == (h + w, 5) and axes.dtype == np.int32
    assert np.array_equal(axes, restated_axes(h, w, gy, gx))
    assert (axes[:, 1:].sum(1) == 4096).all() and (axes[:, 1:] >= 0).all()
    assert (axes[:h, 0] >= 0).all() and (axes[:h, 0] < gy).all() and (axes[h:, 0] < gx).all()
    for i in range(2):
        got = warp_field(nodes[i], aug, h, w)
        assert got.shape == (h, w, 2) and got.dtype == np.int32
        assert np.array_equal(got, restated_field(nodes[i], axes, h, w, gx))


def test_nodes_reach_both_ends_and_depend_on_epoch_and_sample_only():
    aug = Warp(0.02, 1, seed=3)  # A = 5: 11 values, so 100 000 draws reach both ends
    assert aug.bound == 5 and aug.nodes == 16
    nodes = epoch_nodes(3200, aug, 1)  # 3200 * 16 * 2 = 102 400 draws
    assert nodes.min() == -5 and nodes.max() == 5
    assert np.bincount((nodes + 5).ravel(), minlength=11).min() > 8000  # near 9309 each
    wide = Warp(8.0, 5, seed=3)
    big = epoch_nodes(800, wide, 1)  # 102 400 draws of 4097 values
    assert big.min() >= -2048 and big.max() <= 2048 and big.min() < -2040 and big.max() > 2040
    assert not np.array_equal(nodes, epoch_nodes(3200, aug, 2))  # between epochs
    assert len({nodes[i].tobytes() for i in range(50)}) == 50  # between samples
    assert not np.array_equal(nodes, epoch_nodes(3200, Warp(0.02, 1, seed=4), 1))
    assert np.array_equal(nodes[:10], epoch_nodes(10, aug, 1))  # a sample's nodes do not depend on n ...
    # ... nor on the order: the engine's rows after a shuffle are the loaded samples' nodes, permuted (below)
    assert not epoch_nodes(5, Warp(0.0), 1).any()


def _rows_of_every_kind(n, P, seed=0):
    rng = np.random.default_rng(seed)
    floats = rng.random((n, P)) - 0.5
    floats[0, :5] = [-0.0, 0.0, np.inf, -np.inf, 5e-324]
    bf16 = torch.from_numpy(floats.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return [rng.integers(0, 256, (n, P)).astype(np.uint8), bf16, floats.astype(np.float32), floats]


@pytest.mark.parametrize("h,w", [(28, 28), (5, 6)])
def test_alpha_zero_is_bitwise_an_affine_and_with_an_identity_table_a_shift(h, w):
    n = 12
    moving = Warp(0.0, 3, rotate=30, scale=(0.8, 1.2), shear=10, max_dx=2, height=h, width=w, seed=5)
    ident = Warp(0.0, (2, 5), max_dx=2, height=h, width=w, seed=5)
    for aug in (moving, ident):
        sh, en = epoch_shifts(n, aug, 6), aug.table()[epoch_transforms(n, aug, 6)]
        nodes = epoch_nodes(n, aug, 6)
        assert not nodes.any() and not warp_field(nodes[0], aug, h, w).any()
        for rows in _rows_of_every_kind(n, h * w):
            a, b = apply_warp(rows, sh, en, nodes, aug, h, w), apply_affine(rows, sh, en, h, w)
            assert a.dtype == b.dtype == rows.dtype and a.tobytes() == b.tobytes()
            if aug is ident:
                assert a.tobytes() == apply_shifts(rows, sh, h, w).tobytes()


@pytest.mark.parametrize("gy,gx", [(3, 3), (5, 1), (1, 1)])
def test_a_constant_lattice_displaces_every_pixel_by_exactly_c_over_256(gy, gx):
    h, w, n = 9, 11, 4
    aug = Warp(8.0, (gy, gx), height=h, width=w)
    for c in (-2048, -256, 1, 512, 2048):
        nodes = np.full((n, aug.nodes, 2), c, np.int32)
        assert (warp_field(nodes[0], aug, h, w) == 512 * c).all()  # c / 256 pixel in units of 2^-17
    # a whole pixel (c = 256 k) moves the source position by (k, k): the image moves by (-k, -k), for every kind
    zero = np.zeros((n, 2), np.int32)
    ident = np.tile(np.array([65536, 0, 0, 65536], np.int32), (n, 1))
    for rows in _rows_of_every_kind(n, h * w):
        for k in (-2, 1, 3):
            got = apply_warp(rows, zero, ident, np.full((n, aug.nodes, 2), 256 * k, np.int32), aug, h, w)
            want = apply_shifts(rows, np.full((n, 2), -k, np.int32), h, w)
            assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("gy,gx", GRIDS + [(4, 2)])
@pytest.mark.parametrize("h,w", SHAPES + [(33, 3), (64, 64)])
def test_integer_field_is_within_the_derived_bound_of_the_fp64_bspline_field(h, w, gy, gx):
    """csrc/mlp/warp.h: |d17 / 2^17 - D| <= 6 alpha / 4096 + 2^-18 pixel."""
    alpha = 8.0
    aug = Warp(alpha, (gy, gx), height=h, width=w, seed=2)
    bound = 6.0 * alpha / 4096 + 2.0 ** -18
    nodes = epoch_nodes(4, aug, 9)
    # the corners of the nodes' range too: every node at the bound, and alternating signs
    alt = np.where((np.arange(aug.nodes) % 2 == 0)[:, None], 2048, -2048) * np.ones((1, 2), np.int64)
    worst = 0.0
    for nd in list(nodes) + [np.full((aug.nodes, 2), 2048), alt]:
        got = warp_field(nd, aug, h, w) / 2.0 ** 17
        worst = max(worst, np.abs(got - real_field(nd, h, w, gy, gx)).max())
    print(f"{h}x{w} grid {gy}x{gx}: worst distance {worst:.5f} pixel (bound {bound:.5f})")
    assert worst <= bound


def warped_fp64(x, shifts, maps, fields, h, w):
    """A plain fp64 restatement: the fp64 field (pixels, [n][h][w][2]), the unquantised inverse maps, fp64 bilinear
    blending, zeros outside the image."""
    n = x.shape[0]
    src = np.zeros((n, h + 2, w + 2))
    src[:, 1:-1, 1:-1] = x.reshape(n, h, w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w))
    for i in range(n):
        m, (dx, dy) = maps[i], shifts[i]
        u, v = xx - (w - 1) / 2 - dx, yy - (h - 1) / 2 - dy
        sx = m[0] * u + m[1] * v + (w - 1) / 2 + fields[i][:, :, 0]
        sy = m[2] * u + m[3] * v + (h - 1) / 2 + fields[i][:, :, 1]
        ix, iy = np.floor(sx), np.floor(sy)
        fx, fy = sx - ix, sy - iy
        ix, iy = np.clip(ix, -1, w - 1).astype(int) + 1, np.clip(iy, -1, h - 1).astype(int) + 1
        inside = (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
        blend = ((1 - fy) * (1 - fx) * src[i, iy, ix] + (1 - fy) * fx * src[i, iy, np.minimum(ix + 1, w + 1)]
                 + fy * (1 - fx) * src[i, np.minimum(iy + 1, h + 1), ix]
                 + fy * fx * src[i, np.minimum(iy + 1, h + 1), np.minimum(ix + 1, w + 1)])
        out[i] = np.where(inside, blend, 0.0)
    return out.reshape(n, h * w)


WHOLE_IMAGE_BOUND = 5.0  # grey levels: twice the measured worst case, rounded up (the docstring below)


@pytest.mark.parametrize("h,w", [(28, 28), (5, 6), (21, 37)])
def test_uint8_rule_is_close_to_the_fp64_restatement_on_noise(h, w):
    """The images are uint8 noise, the worst case for the gradient, under the extreme affine map and alpha = 8.  The
    bound cannot be derived tightly (the truncated 8-bit fractions, the field's 0.0117 pixel and the Q16 map all act
    through a gradient of up to 255 grey levels per pixel), so it is measured: the worst case of these three cases on
    the CPU is 2.024 grey levels (28 x 28: 2.014, 5 x 6: 1.808, 21 x 37: 2.024).  Asserted at twice that, rounded up
    to a whole grey level: 5.  Other seeds move the figure, and a looser bound would hide a wrong tap."""
    from tests.test_affine import inverse_map

    rng = np.random.default_rng(h * 100 + w)
    n, T, seed = 96, 64, 11
    x = rng.integers(0, 256, (n, h * w)).astype(np.uint8)
    aug = Warp(8.0, 3, rotate=180, scale=(0.25, 4), shear=45, max_dx=2, max_dy=2, height=h, width=w, seed=seed,
               table=T)
    sh, idx, nodes = epoch_shifts(n, aug, 3), epoch_transforms(n, aug, 3), epoch_nodes(n, aug, 3)
    got = apply_warp(x, sh, aug.table()[idx], nodes, aug, h, w).astype(np.float64)
    maps = [inverse_map(seed, int(k), 180.0, 0.25, 4.0, 45.0) for k in idx]
    fields = [real_field(nodes[i], h, w, 3, 3) for i in range(n)]
    worst = np.abs(got - warped_fp64(x.astype(np.float64), sh, maps, fields, h, w)).max()
    print(f"{h}x{w}: worst difference {worst:.3f} grey levels")
    assert worst <= WHOLE_IMAGE_BOUND


def test_warp_validates_and_round_trips():
    a = Warp(2.5, (2, 4), 12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=77)
    assert (a.alpha, a.grid, a.rotate, a.scale, a.shear) == (2.5, (2, 4), 12.5, (0.8, 1.25), 5.0)
    assert (a.max_dx, a.max_dy, a.seed, a.table_size, a.bound, a.nodes) == (2, 1, 4, 77, 640, 35)
    assert a.shape(784) == (28, 28) and a.to_meta()["kind"] == "warp" and a.table().shape == (77, 4)
    assert a.affine == Affine(12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=77)
    assert np.array_equal(a.table(), a.affine.table()) and not isinstance(a, Affine)
    assert Warp.from_meta(json.loads(json.dumps(a.to_meta()))) == a and Warp.from_meta(None) is None
    assert augment_mod.from_meta(a.to_meta()) == a
    assert augment_mod.from_meta(a.affine.to_meta()) == a.affine  # the other kinds, as before
    assert augment_mod.from_meta(Shift(2, seed=3).to_meta()) == Shift(2, seed=3)
    assert a != Warp(2.5, (2, 3), 12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=77)
    assert a != Warp(2.0, (2, 4), 12.5, (0.8, 1.25), 5, max_dx=2, max_dy=1, seed=4, table=77) and a != a.affine
    d = Warp()
    assert (d.alpha, d.grid, d.rotate, d.scale, d.shear, d.max_dx, d.table_size) == (4.0, (3, 3), 0.0, (1.0, 1.0), 0.0,
                                                                                   0, 1024)
    assert Warp(1, 2).grid == (2, 2) and Warp(1, height=5, width=6).shape(30) == (5, 6)
    assert "Warp(alpha=2.5, grid=(2, 4), rotate=12.5" in repr(a)
    assert a.axes(28, 28) is a.axes(28, 28) and not a.axes(28, 28).flags.writeable
    assert a.table_checksum(28, 28) != a.table_checksum() == a.affine.table_checksum()
    assert a.table_checksum(28, 28) != Warp(2.5, (2, 5), 12.5, (0.8, 1.25), 5, 2, 1, seed=4, table=77).table_checksum(28, 28)
    for bad in (lambda: Warp(-0.1), lambda: Warp(8.01), lambda: Warp(1, 0), lambda: Warp(1, 6), lambda: Warp(1, (3, 0)),
                lambda: Warp(1, 2.5), lambda: Warp(1, rotate=181), lambda: Warp(1, scale=17), lambda: Warp(1, table=0),
                lambda: Warp(1, max_dx=-1), lambda: Warp(1, seed=2**32), lambda: Warp(1, height=5),
                lambda: Warp(1, max_dx=6, height=5, width=6), lambda: a.shape(30),
                lambda: Warp.from_meta(a.affine.to_meta()), lambda: Affine.from_meta(a.to_meta()),
                lambda: Shift.from_meta(a.to_meta())):
        with pytest.raises(ValueError):
            bad()
    x = np.zeros((2, 30), np.uint8)
    w56 = Warp(1, 3, height=5, width=6)
    z2, z4, zn = np.zeros((2, 2)), np.zeros((2, 4)), np.zeros((2, 36, 2))
    assert not apply_warp(x, z2, z4, zn, w56, 5, 6).any()
    for bad in (lambda: apply_warp(x, z2, z4, zn, w56, 5, 7), lambda: apply_warp(x, np.zeros((3, 2)), z4, zn, w56, 5, 6),
                lambda: apply_warp(x, z2, np.zeros((2, 3)), zn, w56, 5, 6),
                lambda: apply_warp(x, z2, z4, np.zeros((2, 35, 2)), w56, 5, 6),
                lambda: apply_warp(x, z2, z4, np.zeros((1, 36, 2)), w56, 5, 6),
                lambda: apply_warp(x, z2, z4, np.full((2, 36, 2), 2049), w56, 5, 6),
                lambda: apply_warp(x, np.full((2, 2), 6), z4, zn, w56, 5, 6),
                lambda: apply_warp(x, z2, np.full((2, 4), 1 << 23), zn, w56, 5, 6),
                lambda: apply_warp(x.astype(np.int32), z2, z4, zn, w56, 5, 6),
                lambda: warp_field(np.zeros((35, 2)), w56, 5, 6), lambda: warp_field(np.full((36, 2), -2049), w56, 5, 6),
                lambda: cpu().warp_axes(5, 6, 0, 3), lambda: cpu().warp_axes(5, 6, 3, 6), lambda: cpu().warp_axes(0, 6, 3, 3),
                lambda: cpu().epoch_nodes(4, 0, 0, 65, 10), lambda: cpu().epoch_nodes(4, 0, 0, 16, 2049),
                lambda: cpu().epoch_nodes(-1, 0, 0, 16, 10)):
        with pytest.raises(ValueError):
            bad()
    # tables that would leave the lattice or the int32 range are refused, not indexed
    axes = w56.axes(5, 6).copy()
    for k, v in ((0, 3), (0, -1), (1, 5000), (2, -1)):
        broken = axes.copy()
        broken[3, k] = v
        with pytest.raises(ValueError):
            cpu().warp_field(np.zeros((36, 2), np.int32), broken, 5, 6, 3, 3)


# ---- the torch-backend engine and the trainers
def resident(x, kind):
    if kind == "u8":
        return x
    if kind == "f64":
        return np.ascontiguousarray(x, np.float64)
    x32 = np.ascontiguousarray(x, np.float32)
    if kind == "f32":
        return x32
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def loadable(rows):
    if rows.dtype == np.uint16:
        return torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy()
    return rows


def perm_of(n, seed, key):
    return np.arange(n, dtype=np.int32) if seed is None else cpu().epoch_permutation(n, seed, key)


def warped(x, y, aug, seed, key, kind="u8"):
    """The host's epoch: (x[perm] through entries[perm], shifts[perm] and nodes[perm], y[perm], perm, shifts[perm],
    index[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh, idx = epoch_shifts(n, aug, key)[perm], epoch_transforms(n, aug, key)[perm]
    rows = apply_warp(resident(x, kind)[perm], sh, aug.table()[idx], epoch_nodes(n, aug, key)[perm], aug, h, w)
    return loadable(rows), y[perm], perm, sh, idx


def _engine(x, y, dtype="f32", path="auto", keep=False, H=16):
    e = MlpEngine((x.shape[1], H, 10), dtype=dtype, max_cols=64, device="cpu", backend="torch", path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


KINDS = {("f32", "split3"): "u8", ("f64", "mfma"): "f64", ("f32", "mfma"): "f32", ("bf16", "mfma"): "bf16"}


@pytest.mark.parametrize("dtype,path", list(KINDS))
@pytest.mark.parametrize("seed", [None, 5])
def test_torch_engine_warp_equals_a_fresh_load(dtype, path, seed):
    x, y = synthetic_mnist(75, seed=2)
    if path == "mfma":  # non-integer values, so that the engine keeps them in the element type
        x = x.astype(np.float64) / 255.0 + 0.125
    aug = Warp(**MILD, seed=4)
    e = _engine(x, y, dtype, path, keep=True)
    assert e.path == path and e.warp_launches == 0
    names = [n for n in ("X", "XT", "labels") if getattr(e, n) is not None]
    ptrs = [getattr(e, n).data_ptr() for n in names]
    for key in (0, 9):  # the second is a fresh load of the second epoch's set: not composed with the first
        e.enqueue_augment(aug, key, seed)
        xa, ya, perm, sh, idx = warped(x, y, aug, seed, key, KINDS[dtype, path])
        assert sh.any() and idx.any()
        f = _engine(xa, ya, dtype, path)
        assert np.array_equal(e.permutation().numpy(), perm) and np.array_equal(e.shifts().numpy(), sh)
        assert np.array_equal(e.transforms().numpy(), idx)
        for name in names:
            assert torch.equal(getattr(e, name), getattr(f, name)), (name, key)
    still = _engine(x, y, dtype, path, keep=True)  # the field matters: the Affine alone gives other pixels
    still.enqueue_augment(aug.affine, 9, seed)
    assert not torch.equal(still.X, e.X) and torch.equal(still.transforms(), e.transforms())
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
    assert e.warp_launches == 0 and e.affine_launches == 0 and e.augment_launches == 0  # (the hip backend's counters)


def _trainer(seed=None, aug=None, H=16, B=64, dtype="f64", cls=DataParallelTrainer, comm=None):
    nn = NeuralNetwork([784, H, 10])
    kw = dict(use_graphs=False) if cls is DataParallelTrainer else {}
    if comm is not None:
        kw["comm"] = comm
    return cls(nn, device="cpu", dtype=dtype, batch_size=B, backend="torch", shuffle_seed=seed, augment=aug, **kw)


def _twin_epochs(twin, x, y, aug, seed, epochs, lr, reg):
    """The reload-per-epoch twin: load the host's warped epoch and train(1), ``iter`` carried."""
    for _ in range(epochs):
        xa, ya = warped(x, y, aug, seed, twin.iter, "f64")[:2]
        twin.load(xa, ya)
        twin.train(1, lr, reg)


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
@pytest.mark.parametrize("seed", [None, 6])
def test_torch_trainer_equals_the_reload_per_epoch_twin(cls, seed):
    x, y = synthetic_mnist(200, seed=3)  # batch 64: three full batches and a remainder of 8
    aug = Warp(**MILD, seed=4)
    tr = _trainer(seed, aug, cls=cls)
    tr.load(x, y)
    assert tr.engine.X0 is not None and tr.engine._affine_table is not None  # (the tables are uploaded by load())
    assert tr.engine._warp_axes is not None and tuple(tr.engine._warp_axes[1].shape) == (56, 5)
    tr.train(3, 0.05, 1e-4)
    twin = _trainer(None, None, cls=cls)
    _twin_epochs(twin, x, y, aug, seed, 3, 0.05, 1e-4)
    assert tr.iter == twin.iter == 12
    assert torch.equal(tr.engine.params, twin.engine.params)
    xa, _, perm, sh, idx = warped(x, y, aug, seed, 8, "f64")  # the set stays in the last epoch's state
    assert torch.equal(tr.engine.X, torch.from_numpy(xa).to(tr.engine.X.dtype))
    assert np.array_equal(tr.engine.permutation().numpy(), perm) and np.array_equal(tr.engine.shifts().numpy(), sh)
    assert np.array_equal(tr.engine.transforms().numpy(), idx)
    plain = _trainer(seed, aug.affine, cls=cls)
    plain.load(x, y)
    plain.train(3, 0.05, 1e-4)
    assert not torch.equal(plain.engine.params, tr.engine.params)  # the field matters
    assert np.array_equal(tr.predict(x[:50]), twin.predict(x[:50]))  # predict() is never warped


def test_train_2_twice_equals_train_4_and_the_per_step_path():
    x, y = synthetic_mnist(200, seed=3)
    aug = Warp(**MILD, seed=4)
    a, b = _trainer(6, aug), _trainer(6, aug)
    for t in (a, b):
        t.load(x, y)
    a.train(4, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4, print_every=3, log=lambda *_: None)  # the host-in-the-loop path warps too
    assert torch.equal(a.engine.params, b.engine.params) and torch.equal(a.engine.X, b.engine.X)
    with pytest.raises(ValueError):
        _trainer(None, Warp(2, height=5, width=6)).load(x, y)  # validated against the engine's P at load()


@pytest.mark.parametrize("seed", [None, 6])
def test_warped_oracle_equals_the_manual_per_epoch_loop(seed):
    H, N, B, E, lr, reg = 24, 600, 200, 2, 0.05, 1e-4
    x, y = synthetic_mnist(N, seed=11)
    aug = Warp(**MILD, seed=3)
    for kind in ("u8", "f64"):  # bytes are blended as bytes (the trainers' resident pixels), anything else in fp64
        xin = resident(x, kind)
        seq = NeuralNetwork([784, H, 10])
        mlp.train(seq, xin, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed, augment=aug)
        man = NeuralNetwork([784, H, 10])
        it = 0
        for _ in range(E):
            xa, ya = warped(x, y, aug, seed, it, kind)[:2]
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
    flat = NeuralNetwork([784, H, 10])
    mlp.train(flat, x.astype(np.float64), y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed, augment=aug.affine)
    assert np.abs(flat.W[0] - seq.W[0]).max() / np.abs(seq.W[0]).max() > 1e-6


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
    aug = Warp(**MILD, seed=4)
    got = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=False)
    want = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=True)
    for r in range(3):
        assert torch.equal(got[r][1], got[0][1])  # the same pixels on every rank
        assert torch.equal(got[r][0], want[r][0]), r


# ---- the CLI
def _cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "800", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_warp_checkpoint_and_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--augment-warp", "3", "--augment-warp-grid", "2x4", "--augment-rotate", "10", "--augment-shift", "2",
             "--augment-seed", "1", "--augment-table", "256")
    want = Warp(3.0, (2, 4), rotate=10, max_dx=2, seed=1, table=256)
    log = tmp_path / "run.jsonl"
    _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "--log-json", str(log))
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert augment_mod.from_meta(meta["augment"]) == want and meta["epochs"] == 4
    assert meta["augment"]["kind"] == "warp"
    assert int(meta["augment"]["table_checksum"], 16) == want.table_checksum(28, 28)
    head = json.loads(log.read_text().splitlines()[0])
    assert head["event"] == "config" and head["augment"] == meta["augment"]  # the run header names the policy
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with augmentation" not in r.stdout
    assert "transform table has checksum" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])  # 2 of 4 epochs, resumed == the unbroken run
    # other flags: the policy's warning (the Affine of the same map is another policy); another table: the checksum's
    other = _cli(tmp_path, "--augment-rotate", "10", "--augment-shift", "2", "--augment-seed", "1", "--augment-table",
                 "256", "-e", "1", "--resume", half, "--ckpt-dir", str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with augmentation" in other.stdout
    half_meta = tmp_path / "half" / "meta.json"
    m = json.loads(half_meta.read_text())
    m["augment"]["table_checksum"] = f"{want.table_checksum(28, 28) ^ 1:016x}"
    half_meta.write_text(json.dumps(m))
    odd = _cli(tmp_path, *flags, "-e", "1", "--resume", half)
    assert "transform table has checksum" in odd.stdout
    assert "warning: the checkpoint was trained with augmentation" not in odd.stdout


@pytest.mark.parametrize("argv", [("--augment-warp", "8.5"), ("--augment-warp", "-1"), ("--augment-warp-grid", "0"),
                                  ("--augment-warp-grid", "6"), ("--augment-warp-grid", "3x6"),
                                  ("--augment-warp-grid", "3x"), ("--augment-warp-grid", "2x3x4"),
                                  ("--augment-warp-grid", "a"), ("--augment-warp", "2", "--augment-rotate", "181"),
                                  ("--augment-warp", "2", "--augment-table", "0"),
                                  ("--augment-warp", "2", "--image-shape", "28x27"),
                                  ("--augment-warp", "2", "--augment-shift", "28")])
def test_cli_refuses_bad_flags_at_parse_time(argv, capsys):
    with pytest.raises(SystemExit) as ex:
        parse_config(list(argv))
    assert ex.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_cli_flags_make_the_policy():
    assert parse_config([]).augment is None
    assert parse_config(["--augment-shift", "2", "--augment-seed", "9"]).augment == Shift(2, seed=9)  # as before
    assert parse_config(["--augment-rotate", "15"]).augment == Affine(15, 1.0, 0.0)
    assert parse_config(["--augment-warp", "4"]).augment == Warp(4.0, 3)
    assert parse_config(["--augment-warp", "0"]).augment == Warp(0.0)
    assert parse_config(["--augment-warp-grid", "2"]).augment == Warp(4.0, 2)  # either flag makes the policy
    assert parse_config(["--augment-warp-grid", "5x1", "--augment-seed", "3"]).augment == Warp(4.0, (5, 1), seed=3)
    cfg = parse_config(["--augment-warp", "2.5", "--augment-warp-grid", "2X4", "--augment-rotate", "10",
                        "--augment-scale", "0.8:1.25", "--augment-shear", "5", "--augment-shift", "3",
                        "--augment-shift-y", "1", "--image-shape", "16x49", "--augment-table", "99", "--augment-seed",
                        "2"])
    assert cfg.augment == Warp(2.5, (2, 4), 10, (0.8, 1.25), 5, 3, 1, 16, 49, 2, 99)
    cfg = parse_config(["-s", "--augment-warp", "4", "--augment-rotate", "10", "--augment-shift", "2"])
    assert cfg.augment == Warp(4.0, 3, rotate=10, max_dx=2)
