"""Augmentation of the resident training set: random shifts per epoch.

``Shift`` describes the policy the trainers take as ``augment=``: before every epoch each training image is moved by
its own ``(dx, dy)``, ``|dx| <= max_dx`` and ``|dy| <= max_dy``, and the pixels moved in from outside are zeros.  The
shift of a sample depends on ``(seed, iteration counter at the epoch start, loaded sample index)`` alone
(csrc/mlp/augment.h -- the one header the gather kernel csrc/mlp/augment.hip and the host compile), so a re-run epoch
or a resumed run reproduces it, the shuffle's order does not change it, and every rank forms the same pixels.
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


def epoch_shifts(n: int, aug: Shift, key: int) -> np.ndarray:
    """int32 [n][2]: (dx, dy) of LOADED sample i in the epoch that starts at iteration counter ``key``."""
    from ._native import cpu

    return cpu().epoch_shifts(int(n), aug.seed, int(key), aug.max_dx, aug.max_dy)


def apply_shifts(x, shifts, h: int, w: int) -> np.ndarray:
    """Rows of h x w images ([N][h * w]; uint8, float32, float64 or any 1 / 2 / 4 / 8-byte element), row i moved by
    ``shifts[i] = (dx, dy)``: ``out[i, y, x] = in[i, y - dy, x - dx]``, zero where that lies outside the image."""
    from ._native import cpu

    return cpu().augment_rows(np.ascontiguousarray(x), np.ascontiguousarray(shifts, dtype=np.int32), int(h), int(w))
