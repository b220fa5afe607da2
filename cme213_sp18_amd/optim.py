"""The update rule of a training run: plain SGD (the reference's ``w -= lr g``), momentum / Nesterov, or Adam.

``Optimizer`` only names the rule and its hyper-parameters; the learning rate stays the ``lr`` of ``train()`` and
``step()``.  The rules themselves live in one header for host and device (csrc/mlp/optim.h): the gfx950 kernel
(csrc/mlp/optim.hip, ``MlpEngine.apply``), the CPU implementation (``_cpu.optim_step``) and the fp64 oracle
(``models.mlp.train(optimizer=...)``) evaluate the same functions.

  * momentum: ``v = mu v + g; d = g + mu v if nesterov else v; p -= lr d`` -- torch.optim.SGD(momentum=mu,
    dampening=0, nesterov=...) with v0 = 0;
  * adam: ``m = b1 m + (1 - b1) g; s = b2 s + (1 - b2) g g; p -= (lr / (1 - b1^t)) m / (sqrt(s) / sqrt(1 - b2^t) +
    eps)`` -- torch.optim.Adam without weight decay or amsgrad, t the count of applied updates from 1.

``g`` is the gradient as the step leaves it: scaled by the batch, the regulariser included.
"""
from __future__ import annotations

import dataclasses

import numpy as np

KINDS = ("sgd", "momentum", "adam")
KIND_CODES = {"momentum": 0, "adam": 1}  # csrc/mlp/optim.h OptimKind


@dataclasses.dataclass(frozen=True)
class Optimizer:
    kind: str = "sgd"
    momentum: float = 0.9
    nesterov: bool = False
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"optimizer kind must be one of {KINDS}, got {self.kind!r}")
        if not 0.0 <= float(self.momentum) < 1.0:
            raise ValueError(f"momentum must be in [0, 1), got {self.momentum}")
        for name in ("beta1", "beta2"):
            if not 0.0 <= float(getattr(self, name)) < 1.0:
                raise ValueError(f"{name} must be in [0, 1), got {getattr(self, name)}")
        if not float(self.eps) > 0.0:
            raise ValueError(f"eps must be > 0, got {self.eps}")

    @classmethod
    def sgd(cls) -> "Optimizer":
        return cls("sgd")

    @classmethod
    def momentum_(cls, mu: float = 0.9, nesterov: bool = False) -> "Optimizer":
        return cls("momentum", momentum=float(mu), nesterov=bool(nesterov))

    @classmethod
    def adam(cls, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> "Optimizer":
        return cls("adam", beta1=float(beta1), beta2=float(beta2), eps=float(eps))

    @property
    def stateful(self) -> bool:
        return self.kind != "sgd"

    @property
    def code(self) -> int:
        return KIND_CODES[self.kind]

    @property
    def num_state(self) -> int:
        """Arena-sized state buffers: 0 (sgd), 1 (momentum: v), 2 (adam: m, s)."""
        return {"sgd": 0, "momentum": 1, "adam": 2}[self.kind]

    def hyper(self, lr: float) -> tuple:
        """(lr, mu, nesterov, beta1, beta2, eps): the native calls' hyper-parameter tuple."""
        return (float(lr), float(self.momentum), bool(self.nesterov), float(self.beta1), float(self.beta2),
                float(self.eps))

    def key(self) -> tuple:
        return (self.kind,) + self.hyper(0.0)[1:]

    def as_meta(self) -> dict:
        return dataclasses.asdict(self)

    @classmethod
    def from_meta(cls, d: dict | None) -> "Optimizer":
        return cls(**d) if d else cls.sgd()


# ``Optimizer.momentum(mu, nesterov)`` and the field ``momentum`` share a name: a data descriptor, attached after the
# dataclass is built, gives the class the constructor helper and every instance its own value
class _MomentumHelper:
    """Class access -> Optimizer.momentum_; instance access -> the field, kept in the instance's __dict__ (the frozen
    dataclass's __init__ stores through object.__setattr__, which lands in __set__)."""

    def __get__(self, obj, owner):
        if obj is None:
            return owner.momentum_
        return obj.__dict__["momentum"]

    def __set__(self, obj, value):
        obj.__dict__["momentum"] = value


Optimizer.momentum = _MomentumHelper()


def resolve(opt) -> Optimizer | None:
    """None / Optimizer.sgd() -> None (the plain-SGD code as it stands); a stateful Optimizer -> itself."""
    if opt is None:
        return None
    if not isinstance(opt, Optimizer):
        raise TypeError("optimizer must be an Optimizer or None")
    return opt if opt.stateful else None


def new_state(opt: Optimizer | None, count: int) -> dict | None:
    """A fresh host state for ``count`` parameters ([W1|b1|W2|b2], unpadded): fp64 buffers and the counter
    {t, b1^t, b2^t} -- what ``models.mlp.train(optim_state=...)`` carries and ``MlpEngine.optim_state()`` returns."""
    opt = resolve(opt)
    if opt is None:
        return None
    return {"kind": opt.kind, "t": 0, "b1p": 1.0, "b2p": 1.0,
            "state": [np.zeros(int(count), np.float64) for _ in range(opt.num_state)]}
