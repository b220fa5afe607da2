"""Sampling the resident training set with replacement: class-balanced and weighted epochs.

A policy is what the trainers take as ``sampler=``: before every epoch the resident set is rewritten so that sample i
is a DRAW from the loaded set -- row ``j`` with probability ``w[j] / sum(w)`` -- instead of row i or a permutation's.
An epoch still holds ``N`` samples; rows may repeat and rows may be missing.  The draws of the epoch that starts at
iteration counter ``iter`` depend on ``(seed, iter)`` and the weights alone (csrc/mlp/sample.h -- the one header the
four gather kernels and the host compile): a re-run epoch or a resumed run reproduces them and every rank forms the
same set.  The draw goes through a Walker / Vose alias table that the host builds once from the weights.

``Balanced`` weighs every sample by ``1 / count[its label]``, so every class present in the data is drawn equally
often in expectation.  ``Weighted`` takes per-sample weights as given.
"""
from __future__ import annotations

import numpy as np


def _fnv64(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


class _Policy:
    kind = ""

    def __init__(self, seed: int = 0):
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 32:
            raise ValueError(f"{type(self).__name__}: the seed must be in [0, 2^32)")
        self._cache = None  # (key of the labels, table)

    def weights(self, labels) -> np.ndarray:
        raise NotImplementedError

    def table(self, labels) -> np.ndarray:
        """uint32 [N][2] = {threshold, alias}: the alias table of ``weights(labels)`` (csrc/mlp/sample.h), a pure
        function of the weights.  Raises ValueError for weights the rule refuses."""
        from ._native import cpu

        labels = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int64)
        key = (labels.shape[0], hash(labels.tobytes()) if self.kind == "balanced" else 0)  # (in-process only)
        if self._cache is None or self._cache[0] != key:
            t = cpu().alias_table(self.weights(labels))
            t.setflags(write=False)
            self._cache = (key, t)
        return self._cache[1]

    def checksum(self, labels) -> int:
        """A 64-bit FNV-1a checksum of the table's little-endian bytes (meta.json: the table is built in floating
        point on the host)."""
        return _fnv64(self.table(labels).astype("<u4").tobytes())

    def draws(self, labels, key: int) -> np.ndarray:
        """int32 [N]: the source row of every sample of the epoch that starts at iteration counter ``key``."""
        from ._native import cpu

        t = self.table(labels)
        return cpu().epoch_draws(int(t.shape[0]), self.seed, int(key), t)

    def key(self) -> tuple:
        """What identifies the policy: its kind, its seed and (Weighted) its weights -- not where they came from."""
        return (self.kind, self.seed)

    def __eq__(self, other) -> bool:
        return type(other) is type(self) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())


class Balanced(_Policy):
    kind = "balanced"

    def weights(self, labels) -> np.ndarray:
        """float64 [N]: 1 / count[label] -- a class absent from the data gets nothing, since no row carries it."""
        labels = np.asarray(labels).reshape(-1).astype(np.int64)
        if labels.size and labels.min() < 0:
            raise ValueError("Balanced: labels must be >= 0")
        count = np.bincount(labels)
        return 1.0 / count[labels].astype(np.float64)

    def to_meta(self) -> dict:
        return {"kind": "balanced", "seed": self.seed}

    def __repr__(self) -> str:
        return f"Balanced(seed={self.seed})"


class Weighted(_Policy):
    kind = "weighted"

    def __init__(self, weights, seed: int = 0, source: str | None = None):
        super().__init__(seed)
        w = np.asarray(weights)
        if w.ndim != 1:
            raise ValueError("Weighted: the weights must be a vector, one per training sample")
        self._weights = np.ascontiguousarray(w, dtype=np.float64)
        self._weights.setflags(write=False)
        self.source = source  # where the weights came from (the CLI's file): recorded, never compared
        self._wsum = _fnv64(self._weights.astype("<f8").tobytes())

    def key(self) -> tuple:
        return (self.kind, self.seed, int(self._weights.shape[0]), self._wsum)

    def weights(self, labels) -> np.ndarray:
        n = int(np.asarray(labels).reshape(-1).shape[0])
        if self._weights.shape[0] != n:
            raise ValueError(f"Weighted: {self._weights.shape[0]} weights for {n} training samples")
        return self._weights

    def to_meta(self) -> dict:
        return {"kind": "weighted", "seed": self.seed, "n": int(self._weights.shape[0]), "source": self.source,
                "weights_checksum": self._wsum}

    def __repr__(self) -> str:
        return f"Weighted(n={self._weights.shape[0]}, seed={self.seed})"


def from_meta(meta: dict | None, weights=None):
    """The policy a ``to_meta()`` dict describes, or None.  A ``Weighted`` record does not carry its weights: pass them
    (the run's ``--sample-weights`` file) as ``weights``."""
    if meta is None:
        return None
    kind = meta.get("kind")
    if kind == "balanced":
        return Balanced(meta.get("seed", 0))
    if kind == "weighted":
        if weights is None:
            raise ValueError("a weighted sampler's record does not hold the weights: pass them")
        return Weighted(weights, meta.get("seed", 0), meta.get("source"))
    raise ValueError(f"unknown sampler {kind!r}")


def resolve(sampler, shuffle_seed=None):
    """What the trainers and the oracle do with their ``sampler=`` argument: None or a policy, and never both orders."""
    if sampler is None:
        return None
    if not isinstance(sampler, _Policy):
        raise TypeError("sampler must be a sampling.Balanced, a sampling.Weighted or None")
    if shuffle_seed is not None:
        raise ValueError("sampler and shuffle_seed together: the draws are already in random order, and two orders "
                         "would be ambiguous")
    return sampler
