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
import math

import numpy as np

KINDS = ("sgd", "momentum", "adam")
KIND_CODES = {"momentum": 0, "adam": 1}  # csrc/mlp/optim.h OptimKind
SGD_CODE = 2  # kSgd: the stateless rule plain SGD runs through the apply launch under a schedule or clipping
SCHEDULES = ("constant", "step", "exponential", "linear", "cosine")
UNITS = ("step", "epoch")


@dataclasses.dataclass(frozen=True)
class Schedule:
    """A learning-rate schedule: the rate of applied update ``t`` (0-based) is ``lr * factor(t, steps_per_epoch)``,
    ``lr`` still the ``lr`` of ``train()`` / ``step()``.  Only the host evaluates the formulas (in fp64); the device
    reads the factors from a window the trainer fills (csrc/mlp/optim.h).

    With ``u = t`` (unit "step") or ``t // steps_per_epoch`` (unit "epoch") and ``v = u - warmup``:
      * ``u < warmup``: ``warmup_start + (1 - warmup_start) * u / warmup``;
      * constant ``1``; step ``gamma ** (v // size)``; exponential ``gamma ** v``;
      * linear ``1 + (end_factor - 1) * min(v, total) / total``;
      * cosine ``min_factor + (1 - min_factor) * (1 + cos(pi * min(v, total) / total)) / 2``.
    """
    kind: str = "constant"
    unit: str = "step"
    warmup: int = 0
    warmup_start: float = 0.0
    size: int = 1
    gamma: float = 1.0
    total: int = 1
    end_factor: float = 1.0
    min_factor: float = 0.0

    def __post_init__(self):
        if self.kind not in SCHEDULES:
            raise ValueError(f"schedule kind must be one of {SCHEDULES}, got {self.kind!r}")
        if self.unit not in UNITS:
            raise ValueError(f"schedule unit must be one of {UNITS}, got {self.unit!r}")
        for name in ("warmup", "size", "total"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if int(self.warmup) < 0:
            raise ValueError(f"warmup must be >= 0, got {self.warmup}")
        if int(self.size) < 1:
            raise ValueError(f"size must be >= 1, got {self.size}")
        if int(self.total) < 1:
            raise ValueError(f"total must be >= 1, got {self.total}")
        if not 0.0 < float(self.gamma) <= 1.0:
            raise ValueError(f"gamma must be in (0, 1], got {self.gamma}")
        for name in ("warmup_start", "end_factor", "min_factor"):
            if not float(getattr(self, name)) >= 0.0:
                raise ValueError(f"{name} must be >= 0, got {getattr(self, name)}")

    @staticmethod
    def _common(unit, warmup, warmup_start) -> dict:
        return dict(unit=unit, warmup=warmup, warmup_start=float(warmup_start))

    @classmethod
    def constant(cls, unit: str = "step", warmup: int = 0, warmup_start: float = 0.0) -> "Schedule":
        return cls("constant", **cls._common(unit, warmup, warmup_start))

    @classmethod
    def step(cls, size: int, gamma: float, unit: str = "step", warmup: int = 0,
             warmup_start: float = 0.0) -> "Schedule":
        return cls("step", size=size, gamma=float(gamma), **cls._common(unit, warmup, warmup_start))

    @classmethod
    def exponential(cls, gamma: float, unit: str = "step", warmup: int = 0, warmup_start: float = 0.0) -> "Schedule":
        return cls("exponential", gamma=float(gamma), **cls._common(unit, warmup, warmup_start))

    @classmethod
    def linear(cls, total: int, end_factor: float, unit: str = "step", warmup: int = 0,
               warmup_start: float = 0.0) -> "Schedule":
        return cls("linear", total=total, end_factor=float(end_factor), **cls._common(unit, warmup, warmup_start))

    @classmethod
    def cosine(cls, total: int, min_factor: float = 0.0, unit: str = "step", warmup: int = 0,
               warmup_start: float = 0.0) -> "Schedule":
        return cls("cosine", total=total, min_factor=float(min_factor), **cls._common(unit, warmup, warmup_start))

    def factor(self, t: int, steps_per_epoch: int = 1) -> float:
        t = int(t)
        if t < 0:
            raise ValueError("t is the 0-based index of an applied update")
        if self.unit == "epoch":
            if int(steps_per_epoch) < 1:
                raise ValueError("steps_per_epoch must be >= 1")
            u = t // int(steps_per_epoch)
        else:
            u = t
        w = int(self.warmup)
        if u < w:
            return float(self.warmup_start + (1.0 - self.warmup_start) * u / w)
        v = u - w
        if self.kind == "constant":
            return 1.0
        if self.kind == "step":
            return float(self.gamma ** (v // int(self.size)))
        if self.kind == "exponential":
            return float(self.gamma ** v)
        total = int(self.total)
        if self.kind == "linear":
            return float(1.0 + (self.end_factor - 1.0) * min(v, total) / total)
        return float(self.min_factor + (1.0 - self.min_factor) * (1.0 + math.cos(math.pi * min(v, total) / total)) / 2.0)

    def factors(self, t0: int, n: int, steps_per_epoch: int = 1) -> np.ndarray:
        """factor(t0 .. t0 + n) as a float64 array: one schedule window."""
        return np.array([self.factor(int(t0) + i, steps_per_epoch) for i in range(int(n))], np.float64)

    def key(self) -> tuple:
        return dataclasses.astuple(self)

    def as_meta(self) -> dict:
        return dataclasses.asdict(self)

    @classmethod
    def from_meta(cls, d: dict | None) -> "Schedule | None":
        return cls(**d) if d else None


def resolve_policy(schedule, clip_norm) -> tuple:
    """(schedule | None, clip_norm as a float, 0.0 = no clipping), validated."""
    if schedule is not None and not isinstance(schedule, Schedule):
        raise TypeError("schedule must be a Schedule or None")
    c = 0.0 if clip_norm is None else float(clip_norm)
    if clip_norm is not None and not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"clip_norm must be a finite number > 0 (None: no clipping), got {clip_norm}")
    return schedule, c


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


@dataclasses.dataclass(frozen=True)
class Ema:
    """An exponential moving average of the parameters, kept next to them and folded in after every applied update
    (csrc/mlp/ema.h): ``e = fma(1 - d_t, p - e, e)`` with ``d_t = decay``, or with ``warmup``
    ``min(decay, (1 + t) / (10 + t))``, t the 0-based count of averaged updates -- torch.lerp(e, p, 1 - d) and
    torch.optim.swa_utils.get_ema_multi_avg_fn.  The average starts as a copy of the parameters."""
    decay: float = 0.999
    warmup: bool = False

    def __post_init__(self):
        if not 0.0 <= float(self.decay) < 1.0:
            raise ValueError(f"decay must be in [0, 1), got {self.decay}")

    def decay_at(self, t: int) -> float:
        """d_t in fp64, as the header forms it."""
        d = float(self.decay)
        if not self.warmup:
            return d
        return min(d, (1.0 + float(t)) / (10.0 + float(t)))

    def key(self) -> tuple:
        return ("ema", float(self.decay), bool(self.warmup))

    def as_meta(self) -> dict:
        return {"decay": float(self.decay), "warmup": bool(self.warmup)}

    @classmethod
    def from_meta(cls, d: dict | None) -> "Ema | None":
        return cls(float(d["decay"]), bool(d.get("warmup", False))) if d else None


PLATEAU_MONITORS = ("loss", "accuracy")  # csrc/mlp/best.h BestMonitor: mode min / mode max
PLATEAU_THRESHOLD_MODES = ("rel", "abs")  # csrc/mlp/plateau.h PlateauThresholdMode
PLATEAU_FIELDS = ("evals", "best", "bad", "cooldown_left", "scale", "reductions", "last_metric",
                  "last_reduced_index")  # the record's 8 doubles, in order


@dataclasses.dataclass(frozen=True)
class Plateau:
    """Reduce the learning rate when the validation metric stops improving (csrc/mlp/plateau.h):
    torch.optim.lr_scheduler.ReduceLROnPlateau, decided on the device behind every evaluation.  The rule keeps a
    ``scale`` (1.0 at the start) that multiplies every update's rate after the schedule's factor: ``(lr * f) * scale``.
    After more than ``patience`` evaluations that are not better than the best by ``threshold`` (``rel``: a fraction of
    the best; ``abs``: a difference) the scale becomes ``max(scale * factor, min_factor)`` -- unless that changes it by
    no more than ``eps`` -- and the next ``cooldown`` evaluations are not counted.  ``monitor``: the validation
    ``loss`` (lower is better) or ``accuracy`` (higher is better)."""
    factor: float = 0.1
    patience: int = 10
    threshold: float = 1e-4
    threshold_mode: str = "rel"
    cooldown: int = 0
    min_factor: float = 0.0
    eps: float = 1e-8
    monitor: str = "loss"

    def __post_init__(self):
        if not 0.0 < float(self.factor) < 1.0:
            raise ValueError(f"factor must be in (0, 1), got {self.factor}")
        for name in ("patience", "cooldown"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < 0 or int(v) >= 2 ** 31:
                raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
        if not (float(self.threshold) >= 0.0 and math.isfinite(float(self.threshold))):
            raise ValueError(f"threshold must be >= 0, got {self.threshold}")
        if self.threshold_mode not in PLATEAU_THRESHOLD_MODES:
            raise ValueError(f"threshold_mode must be one of {PLATEAU_THRESHOLD_MODES}, got {self.threshold_mode!r}")
        if not 0.0 <= float(self.min_factor) <= 1.0:
            raise ValueError(f"min_factor must be in [0, 1], got {self.min_factor}")
        if not (float(self.eps) >= 0.0 and math.isfinite(float(self.eps))):
            raise ValueError(f"eps must be >= 0, got {self.eps}")
        if self.monitor not in PLATEAU_MONITORS:
            raise ValueError(f"monitor must be one of {PLATEAU_MONITORS}, got {self.monitor!r}")

    @property
    def monitor_code(self) -> int:
        return PLATEAU_MONITORS.index(self.monitor)

    def native(self) -> tuple:
        """(monitor, factor, patience, threshold, threshold_mode, cooldown, min_factor, eps): the native calls' rule."""
        return (self.monitor_code, float(self.factor), int(self.patience), float(self.threshold),
                PLATEAU_THRESHOLD_MODES.index(self.threshold_mode), int(self.cooldown), float(self.min_factor),
                float(self.eps))

    def key(self) -> tuple:
        return ("plateau",) + self.native()

    def as_meta(self) -> dict:
        return {"factor": float(self.factor), "patience": int(self.patience), "threshold": float(self.threshold),
                "threshold_mode": self.threshold_mode, "cooldown": int(self.cooldown),
                "min_factor": float(self.min_factor), "eps": float(self.eps), "monitor": self.monitor}

    @classmethod
    def from_meta(cls, d: dict | None) -> "Plateau | None":
        return cls(**d) if d else None


def resolve_plateau(plateau) -> Plateau | None:
    if plateau is not None and not isinstance(plateau, Plateau):
        raise TypeError("plateau must be a Plateau or None")
    return plateau


def plateau_record_dict(rec) -> dict:
    """The record's 8 doubles as a dict: counts as ints, ``best`` / ``scale`` / ``last_metric`` as floats."""
    r = [float(v) for v in np.asarray(rec, np.float64).reshape(-1)]
    ints = ("evals", "bad", "cooldown_left", "reductions", "last_reduced_index")
    return {k: (int(v) if k in ints else v) for k, v in zip(PLATEAU_FIELDS, r)}


def plateau_record_array(d) -> np.ndarray:
    """The inverse of ``plateau_record_dict`` (a dict, or 8 numbers) as a float64 array."""
    if isinstance(d, dict):
        return np.array([float(d[k]) for k in PLATEAU_FIELDS], np.float64)
    a = np.array(d, np.float64).reshape(-1)
    if a.size != len(PLATEAU_FIELDS):
        raise ValueError("a plateau record holds 8 numbers")
    return a


def resolve_ema(ema) -> Ema | None:
    if ema is not None and not isinstance(ema, Ema):
        raise TypeError("ema must be an Ema or None")
    return ema


def new_ema_state(nn) -> dict:
    """A fresh host state of the average for ``models.mlp.train(ema=, ema_state=)``: {"t": 0, "avg": a copy of the
    parameters, fp64 over [W1|b1|W2|b2]}."""
    W1, b1, W2, b2 = nn.params
    return {"t": 0, "avg": np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in (W1, b1, W2, b2)])}


def resolve(opt) -> Optimizer | None:
    """None / Optimizer.sgd() -> None (the plain-SGD code as it stands); a stateful Optimizer -> itself."""
    if opt is None:
        return None
    if not isinstance(opt, Optimizer):
        raise TypeError("optimizer must be an Optimizer or None")
    return opt if opt.stateful else None


def new_state(opt: Optimizer | None, count: int, policy: bool = False) -> dict | None:
    """A fresh host state for ``count`` parameters ([W1|b1|W2|b2], unpadded): fp64 buffers and the counter
    {t, b1^t, b2^t} -- what ``models.mlp.train(optim_state=...)`` carries and ``MlpEngine.optim_state()`` returns.
    ``policy``: a schedule or clipping is set, so plain SGD keeps a counter too (kind "sgd", no buffers)."""
    opt = resolve(opt)
    if opt is None and policy:
        return {"kind": "sgd", "t": 0, "b1p": 1.0, "b2p": 1.0, "state": []}
    if opt is None:
        return None
    return {"kind": opt.kind, "t": 0, "b1p": 1.0, "b2p": 1.0,
            "state": [np.zeros(int(count), np.float64) for _ in range(opt.num_state)]}
