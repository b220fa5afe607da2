"""Augmentation of the resident training set: random shifts, affine maps and elastic distortions, per epoch.

``Shift`` describes the policy the trainers take as ``augment=``: before every epoch each training image is moved by
its own ``(dx, dy)``, ``|dx| <= max_dx`` and ``|dy| <= max_dy``, and the pixels moved in from outside are zeros.  The
shift of a sample depends on ``(seed, iteration counter at the epoch start, loaded sample index)`` alone
(csrc/mlp/augment.h -- the one header the gather kernel csrc/mlp/augment.hip and the host compile), so a re-run epoch
or a resumed run reproduces it, the shuffle's order does not change it, and every rank forms the same pixels.

``Affine`` adds a small rotation, scaling and shear per image and epoch (csrc/mlp/affine.h, the header of the gather
kernel csrc/mlp/affine.hip): a table of Q16 inverse maps is built once on the host from the policy's fields, a second
keyed hash picks each sample's entry, and every destination pixel is a bilinear blend of four source taps -- integers
for uint8 pixels, one fixed fp64 chain for float elements.  Its shifts are ``Shift``'s, so an ``Affine`` with identity
transforms is bitwise a ``Shift``.

``Warp`` adds an elastic distortion (csrc/mlp/warp.h, the header of the gather kernel csrc/mlp/warp.hip): every image
gets its own coarse lattice of keyed random displacements, bounded by ``alpha`` pixels, and a cubic B-spline through
integer axis tables turns it into a smooth displacement of every pixel's source position on top of the affine map.
With ``alpha = 0`` a ``Warp`` is bitwise its ``Affine``.
"""
from __future__ import annotations

import math

import numpy as np


class Shift:
    def __init__(self, max_dx: int = 2, max_dy: int | None = None, height: int | None = None,
                 width: int | None = None, seed: int = 0):
        self.max_dx = int(max_dx)
        self.max_dy = self.max_dx if max_dy is None else int(max_dy)
        self.height = None if height is None else int(height)
        self.width = None if width is None else int(width)
        self.seed = int(seed)
        if self.max_dx < 0 or self.max_dy < 0:
            raise ValueError("Shift: max_dx and max_dy must be >= 0")
        if (self.height is None) != (self.width is None):
            raise ValueError("Shift: give both height and width, or neither (a square image)")
        if self.height is not None and (self.height < 1 or self.width < 1):
            raise ValueError("Shift: height and width must be >= 1")
        if not 0 <= self.seed < 1 << 32:
            raise ValueError("Shift: the seed must be in [0, 2^32)")
        if self.height is not None:
            self._check(self.height, self.width)

    def _check(self, h: int, w: int) -> None:
        if not (self.max_dx < w and self.max_dy < h):
            raise ValueError(f"Shift: the bounds ({self.max_dx}, {self.max_dy}) must be smaller than the image "
                             f"({w} wide, {h} high)")

    def shape(self, P: int) -> tuple[int, int]:
        """(height, width) of the images of an engine with P input features; raises when they do not fit."""
        P = int(P)
        if self.height is None:
            r = math.isqrt(P)
            if r * r != P:
                raise ValueError(f"Shift: {P} input features are no square image: give height and width")
            h, w = r, r
        else:
            h, w = self.height, self.width
            if h * w != P:
                raise ValueError(f"Shift: a {h} x {w} image does not have {P} input features")
        self._check(h, w)
        return h, w

    def to_meta(self) -> dict:
        return {"kind": "shift", "max_dx": self.max_dx, "max_dy": self.max_dy, "height": self.height,
                "width": self.width, "seed": self.seed}

    @classmethod
    def from_meta(cls, meta: dict | None) -> "Shift | None":
        if meta is None:
            return None
        if meta.get("kind", "shift") != "shift":
            raise ValueError(f"unknown augmentation {meta.get('kind')!r}")
        return cls(meta["max_dx"], meta.get("max_dy"), meta.get("height"), meta.get("width"), meta.get("seed", 0))

    def __eq__(self, other) -> bool:
        return isinstance(other, Shift) and self.to_meta() == other.to_meta()

    def __repr__(self) -> str:
        shape = "" if self.height is None else f", height={self.height}, width={self.width}"
        return f"Shift(max_dx={self.max_dx}, max_dy={self.max_dy}{shape}, seed={self.seed})"


class Affine:
    """rotate / shear: the bounds in degrees of the uniform angle per image; scale: a factor or a (lo, hi) range;
    max_dx, max_dy, height, width, seed: as for ``Shift``; table: the number of distinct transforms."""

    def __init__(self, rotate: float = 15.0, scale=(0.9, 1.1), shear: float = 0.0, max_dx: int = 0,
                 max_dy: int | None = None, height: int | None = None, width: int | None = None, seed: int = 0,
                 table: int = 1024):
        self.rotate, self.shear = float(rotate), float(shear)
        lo, hi = scale if isinstance(scale, (tuple, list)) else (scale, scale)
        self.scale = (float(lo), float(hi))
        self.table_size = int(table)
        # the shifts, the image shape and the seed are a Shift's (validated there)
        self._shift = Shift(max_dx, max_dy, height, width, seed)
        if not 0.0 <= self.rotate <= 180.0:
            raise ValueError("Affine: rotate must be in [0, 180] degrees")
        if not 0.0 <= self.shear <= 60.0:
            raise ValueError("Affine: shear must be in [0, 60] degrees")
        if not 1.0 / 16 <= self.scale[0] <= self.scale[1] <= 16.0:
            raise ValueError("Affine: scale must satisfy 1/16 <= lo <= hi <= 16")
        if not 1 <= self.table_size <= 65536:
            raise ValueError("Affine: table must be in [1, 65536]")
        self._table = None

    max_dx = property(lambda self: self._shift.max_dx)
    max_dy = property(lambda self: self._shift.max_dy)
    height = property(lambda self: self._shift.height)
    width = property(lambda self: self._shift.width)
    seed = property(lambda self: self._shift.seed)

    def shape(self, P: int) -> tuple[int, int]:
        """(height, width) of the images of an engine with P input features; raises when they do not fit."""
        h, w = self._shift.shape(P)
        if max(h, w) > 1 << 24:
            raise ValueError("Affine: the image sides must be <= 2^24")
        return h, w

    def table(self) -> np.ndarray:
        """int32 [table][4]: the Q16 inverse maps {q00, q01, q10, q11}, a pure function of this policy's fields."""
        if self._table is None:
            from ._native import cpu

            self._table = cpu().affine_table(self.seed, self.table_size, self.rotate, self.scale[0], self.scale[1],
                                             self.shear)
            self._table.setflags(write=False)
        return self._table

    def table_checksum(self) -> int:
        """A 64-bit FNV-1a checksum of the table's little-endian bytes (meta.json: the table goes through libm)."""
        h = 0xcbf29ce484222325
        for b in self.table().astype("<i4").tobytes():
            h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
        return h

    def to_meta(self) -> dict:
        return {"kind": "affine", "rotate": self.rotate, "scale": list(self.scale), "shear": self.shear,
                "max_dx": self.max_dx, "max_dy": self.max_dy, "height": self.height, "width": self.width,
                "seed": self.seed, "table": self.table_size}

    @classmethod
    def from_meta(cls, meta: dict | None) -> "Affine | None":
        if meta is None:
            return None
        if meta.get("kind") != "affine":
            raise ValueError(f"unknown augmentation {meta.get('kind')!r}")
        return cls(meta["rotate"], tuple(meta["scale"]), meta["shear"], meta["max_dx"], meta.get("max_dy"),
                   meta.get("height"), meta.get("width"), meta.get("seed", 0), meta.get("table", 1024))

    def __eq__(self, other) -> bool:
        return isinstance(other, Affine) and self.to_meta() == other.to_meta()

    def __repr__(self) -> str:
        shape = "" if self.height is None else f", height={self.height}, width={self.width}"
        return (f"Affine(rotate={self.rotate}, scale={self.scale}, shear={self.shear}, max_dx={self.max_dx}, "
                f"max_dy={self.max_dy}{shape}, seed={self.seed}, table={self.table_size})")


class Warp:
    """alpha: the bound in pixels of a control node's displacement (0 .. 8); grid: cells per axis, an int or (gy, gx),
    each 1 .. 5; every other field: as for ``Affine``, whose map and shift the displacement is added to."""

    def __init__(self, alpha: float = 4.0, grid=3, rotate: float = 0.0, scale=1.0, shear: float = 0.0,
                 max_dx: int = 0, max_dy: int | None = None, height: int | None = None, width: int | None = None,
                 seed: int = 0, table: int = 1024):
        self.alpha = float(alpha)
        gy, gx = grid if isinstance(grid, (tuple, list)) else (grid, grid)
        if int(gy) != gy or int(gx) != gx:
            raise ValueError("Warp: grid must be an integer or a pair of integers")
        self.grid = (int(gy), int(gx))
        # the map, the shifts, the image shape, the seed and the table are an Affine's (validated there)
        self._affine = Affine(rotate, scale, shear, max_dx, max_dy, height, width, seed, table)
        if not 0.0 <= self.alpha <= 8.0:
            raise ValueError("Warp: alpha must be in [0, 8] pixels")
        if not all(1 <= g <= 5 for g in self.grid):
            raise ValueError("Warp: grid must be in [1, 5] cells per axis")
        self._axes = {}

    affine = property(lambda self: self._affine)
    rotate = property(lambda self: self._affine.rotate)
    scale = property(lambda self: self._affine.scale)
    shear = property(lambda self: self._affine.shear)
    table_size = property(lambda self: self._affine.table_size)
    max_dx = property(lambda self: self._affine.max_dx)
    max_dy = property(lambda self: self._affine.max_dy)
    height = property(lambda self: self._affine.height)
    width = property(lambda self: self._affine.width)
    seed = property(lambda self: self._affine.seed)

    @property
    def bound(self) -> int:
        """A: the nodes' bound in Q8 pixel."""
        return int(round(self.alpha * 256.0))

    @property
    def nodes(self) -> int:
        """L: the nodes of a sample's lattice."""
        return (self.grid[0] + 3) * (self.grid[1] + 3)

    def shape(self, P: int) -> tuple[int, int]:
        """(height, width) of the images of an engine with P input features; raises when they do not fit."""
        return self._affine.shape(P)

    def table(self) -> np.ndarray:
        """The Affine's table: int32 [table][4]."""
        return self._affine.table()

    def axes(self, h: int, w: int) -> np.ndarray:
        """int32 [h + w][5]: the axis tables {cell, w0, w1, w2, w3} of an h x w image, the y axis first; a pure
        function of (grid, h, w)."""
        key = (int(h), int(w))
        if key not in self._axes:
            from ._native import cpu

            ax = cpu().warp_axes(key[0], key[1], self.grid[0], self.grid[1])
            ax.setflags(write=False)
            self._axes[key] = ax
        return self._axes[key]

    def table_checksum(self, h: int | None = None, w: int | None = None) -> int:
        """A 64-bit FNV-1a checksum of the little-endian bytes of the transform table and, with a shape, of the axis
        tables after it (meta.json: both are built in floating point on the host)."""
        data = self.table().astype("<i4").tobytes()
        if h is not None:
            data += self.axes(h, w).astype("<i4").tobytes()
        hsh = 0xcbf29ce484222325
        for b in data:
            hsh = ((hsh ^ b) * 0x100000001b3) & 0xffffffffffffffff
        return hsh

    def to_meta(self) -> dict:
        return {"kind": "warp", "alpha": self.alpha, "grid": list(self.grid), "rotate": self.rotate,
                "scale": list(self.scale), "shear": self.shear, "max_dx": self.max_dx, "max_dy": self.max_dy,
                "height": self.height, "width": self.width, "seed": self.seed, "table": self.table_size}

    @classmethod
    def from_meta(cls, meta: dict | None) -> "Warp | None":
        if meta is None:
            return None
        if meta.get("kind") != "warp":
            raise ValueError(f"unknown augmentation {meta.get('kind')!r}")
        return cls(meta["alpha"], tuple(meta["grid"]), meta.get("rotate", 0.0), tuple(meta.get("scale", (1.0, 1.0))),
                   meta.get("shear", 0.0), meta.get("max_dx", 0), meta.get("max_dy"), meta.get("height"),
                   meta.get("width"), meta.get("seed", 0), meta.get("table", 1024))

    def __eq__(self, other) -> bool:
        return isinstance(other, Warp) and self.to_meta() == other.to_meta()

    def __repr__(self) -> str:
        shape = "" if self.height is None else f", height={self.height}, width={self.width}"
        return (f"Warp(alpha={self.alpha}, grid={self.grid}, rotate={self.rotate}, scale={self.scale}, "
                f"shear={self.shear}, max_dx={self.max_dx}, max_dy={self.max_dy}{shape}, seed={self.seed}, "
                f"table={self.table_size})")


def from_meta(meta: dict | None):
    """The policy a ``to_meta()`` dict describes (``Shift``, ``Affine`` or ``Warp``, by its ``kind``), or None."""
    if meta is None:
        return None
    kind = meta.get("kind", "shift")
    if kind == "shift":
        return Shift.from_meta(meta)
    if kind == "affine":
        return Affine.from_meta(meta)
    if kind == "warp":
        return Warp.from_meta(meta)
    raise ValueError(f"unknown augmentation {kind!r}")


def epoch_shifts(n: int, aug, key: int) -> np.ndarray:
    """int32 [n][2]: (dx, dy) of LOADED sample i in the epoch that starts at iteration counter ``key``."""
    from ._native import cpu

    return cpu().epoch_shifts(int(n), aug.seed, int(key), aug.max_dx, aug.max_dy)


def apply_shifts(x, shifts, h: int, w: int) -> np.ndarray:
    """Rows of h x w images ([N][h * w]; uint8, float32, float64 or any 1 / 2 / 4 / 8-byte element), row i moved by
    ``shifts[i] = (dx, dy)``: ``out[i, y, x] = in[i, y - dy, x - dx]``, zero where that lies outside the image."""
    from ._native import cpu

    return cpu().augment_rows(np.ascontiguousarray(x), np.ascontiguousarray(shifts, dtype=np.int32), int(h), int(w))


def epoch_transforms(n: int, aug, key: int) -> np.ndarray:
    """int32 [n]: the table index of LOADED sample i in the epoch that starts at iteration counter ``key``."""
    from ._native import cpu

    return cpu().epoch_transforms(int(n), aug.seed, int(key), aug.table_size)


_KINDS = {"uint8": 0, "float32": 2, "float64": 3}


def apply_affine(x, shifts, entries, h: int, w: int) -> np.ndarray:
    """Rows of h x w images ([N][h * w]; uint8, float32, float64, or bf16 as 2-byte integers), row i resampled through
    ``entries[i] = (q00, q01, q10, q11)`` (a row of ``Affine.table()``) and moved by ``shifts[i] = (dx, dy)``: the
    host's form of the rule of csrc/mlp/affine.h."""
    from ._native import cpu

    x = np.ascontiguousarray(x)
    kind = _KINDS.get(x.dtype.name, 1 if x.dtype.itemsize == 2 and x.dtype.kind in "iu" else None)
    if kind is None:
        raise ValueError(f"apply_affine: elements must be uint8, float32, float64 or bf16 bits, got {x.dtype}")
    return cpu().affine_rows(x, np.ascontiguousarray(shifts, dtype=np.int32),
                             np.ascontiguousarray(entries, dtype=np.int32), int(h), int(w), kind)


def epoch_nodes(n: int, aug: Warp, key: int) -> np.ndarray:
    """int32 [n][L][2]: (ddx, ddy) in Q8 pixel of lattice node j of LOADED sample i in the epoch that starts at
    iteration counter ``key``."""
    from ._native import cpu

    return cpu().epoch_nodes(int(n), aug.seed, int(key), aug.nodes, aug.bound)


def warp_field(nodes_i, aug: Warp, h: int, w: int) -> np.ndarray:
    """int32 [h][w][2]: the displacement (x, y) in 2^-17 pixel of every destination pixel's source position, of one
    sample's nodes ``nodes_i`` (int32 [L][2])."""
    from ._native import cpu

    return cpu().warp_field(np.ascontiguousarray(nodes_i, dtype=np.int32), aug.axes(h, w), int(h), int(w),
                            aug.grid[0], aug.grid[1])


def apply_warp(x, shifts, entries, nodes, aug: Warp, h: int, w: int) -> np.ndarray:
    """``apply_affine`` with row i's source positions moved by the field of ``nodes[i]`` (int32 [N][L][2]): the host's
    form of the rule of csrc/mlp/warp.h."""
    from ._native import cpu

    x = np.ascontiguousarray(x)
    kind = _KINDS.get(x.dtype.name, 1 if x.dtype.itemsize == 2 and x.dtype.kind in "iu" else None)
    if kind is None:
        raise ValueError(f"apply_warp: elements must be uint8, float32, float64 or bf16 bits, got {x.dtype}")
    return cpu().warp_rows(x, np.ascontiguousarray(shifts, dtype=np.int32),
                           np.ascontiguousarray(entries, dtype=np.int32),
                           np.ascontiguousarray(nodes, dtype=np.int32), aug.axes(h, w), int(h), int(w), aug.grid[0],
                           aug.grid[1], kind)
