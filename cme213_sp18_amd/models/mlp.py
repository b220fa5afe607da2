"""The 2-layer MLP model (784-H-10, sigmoid hidden layer, softmax output).

Parity with the reference's ``class NeuralNetwork`` (fpcode/inc/neural_network.h:8-31):
  * ``H = [784, hidden, 10]``, ``W[i]`` is ``H[i+1] x H[i]``, ``b[i]`` has ``H[i+1]`` entries.
  * Init: layer i is seeded with ``i``, ``W[i] = 0.01 * randn``, ``b[i] = 0`` -- identical on every
    rank, so data-parallel replicas need no broadcast (native C++ init, see csrc/cpu/mlp_cpu.cpp).

Parameters are host float64 numpy arrays (the oracle's precision); GPU engines
copy them to device in their own dtype and write them back on ``sync``.
CPU math below (feedforward/backprop/loss/predict/numgrad/train) runs in the
native fp64 OpenMP runtime (``_cpu``): the reference's sequential trainer
(fpcode/neural_network.cpp:91-279).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .._native import cpu


class NeuralNetwork:
    num_layers = 2

    def __init__(self, H=(784, 100, 10), init: bool = True):
        H = [int(h) for h in H]
        if len(H) != 3:
            raise ValueError("NeuralNetwork is a 2-layer MLP: H must be [inputs, hidden, classes]")
        if H[2] > 64:
            raise ValueError("at most 64 output classes are supported (the many-class MFMA head holds 4 class tiles "
                             "of 16)")
        self.H = H
        self.W = [np.zeros((H[1], H[0])), np.zeros((H[2], H[1]))]
        self.b = [np.zeros(H[1]), np.zeros(H[2])]
        if init:
            cpu().init_params(self.W[0], self.b[0], self.W[1], self.b[1])

    # -- convenience -------------------------------------------------------
    @property
    def params(self):
        return self.W[0], self.b[0], self.W[1], self.b[1]

    def copy(self) -> "NeuralNetwork":
        nn = NeuralNetwork(self.H, init=False)
        for i in range(2):
            nn.W[i][...] = self.W[i]
            nn.b[i][...] = self.b[i]
        return nn

    def num_params(self) -> int:
        return sum(w.size for w in self.W) + sum(b.size for b in self.b)

    def __repr__(self) -> str:
        return f"NeuralNetwork(H={self.H})"


@dataclasses.dataclass
class Cache:
    """Forward cache (fpcode/utils/common.h:15-20): a1 [n][H], yc [n][C] (sample-major)."""
    X: np.ndarray
    a1: np.ndarray
    yc: np.ndarray


@dataclasses.dataclass
class Grads:
    dW: list
    db: list


def _x64(X) -> np.ndarray:
    return np.ascontiguousarray(X, dtype=np.float64)


def feedforward(nn: NeuralNetwork, X, shift: bool = True) -> Cache:
    """z1 = W1 x + b1; a1 = sigmoid(z1); z2 = W2 a1 + b2; yc = softmax(z2) per sample."""
    X = _x64(X)
    a1, yc = cpu().feedforward(*nn.params, X, shift)
    return Cache(X, a1, yc)


def backprop(nn: NeuralNetwork, labels, reg: float, cache: Cache, scale: float | None = None) -> Grads:
    """Gradients of the regularised cross-entropy (neural_network.cpp:123-139); scale = 1/N."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    n = labels.shape[0]
    dW1, db1, dW2, db2 = cpu().backprop(*nn.params, cache.X, labels, float(reg), cache.a1, cache.yc,
                                        1.0 / n if scale is None else float(scale))
    return Grads([dW1, dW2], [db1, db2])


def loss(nn: NeuralNetwork, yc, labels, reg: float) -> float:
    return float(cpu().loss(*nn.params, np.ascontiguousarray(yc, np.float64),
                            np.ascontiguousarray(labels, np.int32), float(reg)))


def predict(nn: NeuralNetwork, X, shift: bool = True) -> np.ndarray:
    """argmax class per sample (neural_network.cpp:159-169)."""
    return cpu().predict(*nn.params, _x64(X), shift)


def eval_triple(nn: NeuralNetwork, X, labels, shift: bool = True) -> tuple[float, float, float]:
    """(n, correct, loss_sum) of a labelled set in fp64 on the host -- what a device evaluation leaves in its stats slot
    (csrc/mlp/eval.h): the count, the count of first-maximum predictions that hit the label and the sum of
    -log(yhat[label]) without the regulariser."""
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    yc = feedforward(nn, X, shift).yc
    n = labels.shape[0]
    correct = int((yc.argmax(1) == labels).sum())
    return float(n), float(correct), float(-np.log(yc[np.arange(n), labels]).sum())


def numgrad(nn: NeuralNetwork, X, labels, reg: float, shift: bool = True) -> Grads:
    dW1, db1, dW2, db2 = cpu().numgrad(*nn.params, _x64(X), np.ascontiguousarray(labels, np.int32), float(reg),
                                       shift)
    return Grads([dW1, dW2], [db1, db2])


def train(nn: NeuralNetwork, X, labels, learning_rate: float, reg: float = 0.0, epochs: int = 15,
          batch_size: int = 800, grad_check: bool = False, print_every: int = -1, debug: bool = False,
          outdir: str = "Outputs", shift: bool = True, ckpt_precision: int = 12, iter0: int = 0,
          shuffle_seed: int | None = None, optimizer=None, optim_state: dict | None = None, schedule=None,
          clip_norm: float | None = None, update_log: list | None = None, augment=None, ema=None,
          ema_state: dict | None = None, lr_scale: float | None = None, sampler=None) -> list[float]:
    """Sequential fp64 minibatch SGD on the CPU -- the oracle (neural_network.cpp:219-279).

    ``optimizer``: an ``optim.Optimizer`` (None or ``Optimizer.sgd()``: the reference's plain update).  A stateful
    rule (momentum, Adam; csrc/mlp/optim.h) keeps its state in ``optim_state`` -- ``optim.new_state(optimizer,
    nn.num_params())``, updated in place, so a later call (a resumed run, or one epoch at a time) continues it; None:
    a fresh state for this call.

    ``schedule`` (an ``optim.Schedule``) and ``clip_norm``: the rate of applied update t is ``learning_rate *
    schedule.factor(t, steps per epoch)`` -- the native loop takes the table of this call's rates -- and the gradient's
    global norm is clipped at ``clip_norm`` in the one summation order of csrc/mlp/clip.h (torch's clip_grad_norm_ with
    the L2 term in the loss).  With either set, plain SGD runs the stateless kSgd rule of csrc/mlp/optim.h and keeps its
    update count in ``optim_state`` too (``optim.new_state(optimizer, n, policy=True)``: kind "sgd", no buffers).
    ``update_log``: a list that receives one ``(t, rate, grad_norm, clip_coef)`` per update (norm NaN, coefficient 1
    without clipping).

    ``iter0``: the iteration counter at the start -- a resumed run continues the loss / snapshot numbering.

    ``shuffle_seed``: the parallel trainers' per-epoch shuffle (DataParallelTrainer(shuffle_seed=...)): one native
    epoch at a time on ``X[perm_e]``, perm_e = epoch_permutation(N, seed, iteration counter at the epoch start) -- the
    one implementation in csrc/mlp/shuffle.h -- with the counter carried, so the oracle stays comparable with a
    shuffled parallel run.

    ``augment`` (an ``augment.Shift``; the parallel trainers' ``augment=``): one native epoch at a time on
    ``apply_shifts(X[perm_e], shifts_e[perm_e], h, w)``, shifts_e = the keyed shifts of the loaded samples in the epoch
    that starts at that iteration counter (csrc/mlp/augment.h); without ``shuffle_seed`` the order is the loaded one.
    An ``augment.Affine`` goes through ``apply_affine`` with the samples' table entries instead (csrc/mlp/affine.h):
    uint8 ``X`` is blended by the integer rule, as the trainers' resident bytes are, anything else in fp64.  An
    ``augment.Warp`` goes through ``apply_warp`` with the samples' lattice nodes besides (csrc/mlp/warp.h).

    ``sampler`` (a ``sampling.Balanced`` / ``Weighted``; the parallel trainers' ``sampler=``; not together with
    ``shuffle_seed``): every epoch runs on the rows ``sampler.draws(labels, iteration counter)`` -- a draw with
    replacement (csrc/mlp/sample.h) -- and an augmentation is then keyed by the position in the epoch, not by the row.

    ``ema`` (an ``optim.Ema``; the parallel trainer's ``ema=``): after every update the parameters are folded into an
    average by the rule of csrc/mlp/ema.h.  ``ema_state`` -- ``optim.new_ema_state(nn)``: {"t": the count of averaged
    updates, "avg": fp64 over [W1|b1|W2|b2]}, the average starting as a copy of the parameters -- is updated in place
    and so returned, and a later call continues it; None: a fresh one for this call, dropped afterwards.

    ``lr_scale`` (the parallel trainer's ``plateau=``): the oracle evaluates no validation set, so it takes the scale
    the plateau rule holds (csrc/mlp/plateau.h) from the caller and stays comparable one epoch at a time: every rate of
    this call is ``(learning_rate * factor) * lr_scale`` -- the product the apply launch forms, in its order -- and,
    as under a schedule, plain SGD runs the stateless kSgd rule with its update count in ``optim_state``.

    ``grad_check`` runs a numerical gradient check on the first batch (the
    reference's threshold of 1000 made it a no-op; we assert a real bound).
    """
    X_raw = X if isinstance(X, np.ndarray) and X.dtype == np.uint8 else None  # (an Affine blends bytes as bytes)
    X = _x64(X)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if grad_check:
        from ..utils.common import gradcheck

        n = min(batch_size, X.shape[0])
        c = feedforward(nn, X[:n], shift)
        g = backprop(nn, labels[:n], reg, c)
        ng = numgrad(nn, X[:n], labels[:n], reg, shift)
        if not gradcheck(ng, g):
            raise AssertionError("gradient check failed")
    from ..optim import SGD_CODE, Optimizer, new_state, resolve, resolve_policy

    opt = resolve(optimizer)
    schedule, clip = resolve_policy(schedule, clip_norm)
    policy = schedule is not None or clip > 0.0 or lr_scale is not None
    kw = {}
    n, nb = X.shape[0], (X.shape[0] + int(batch_size) - 1) // int(batch_size)
    rates = None
    if opt is not None or policy:
        st = optim_state if optim_state is not None else new_state(opt, nn.num_params(), policy=policy)
        kind = opt.kind if opt is not None else "sgd"
        if st["kind"] != kind or len(st["state"]) != (opt.num_state if opt is not None else 0) or any(
                s.size != nn.num_params() or s.dtype != np.float64 for s in st["state"]):
            raise ValueError("optim_state does not belong to this optimizer and network")
        counter = np.array([st["t"], st["b1p"], st["b2p"]], np.float64)
        kw["optim"] = (opt.code if opt is not None else SGD_CODE,
                       (opt if opt is not None else Optimizer.sgd()).hyper(learning_rate),
                       st["state"][0] if st["state"] else None, st["state"][1] if len(st["state"]) > 1 else None,
                       counter)
        if policy:
            kw["clip_norm"] = clip
            kw["update_log"] = update_log
        if schedule is not None:  # lr * factor: the fp64 product the apply launch forms
            rates = float(learning_rate) * schedule.factors(int(st["t"]), int(epochs) * nb, nb)
        if lr_scale is not None:  # (lr * f) * scale: csrc/mlp/plateau.h plateau_rate
            if not float(lr_scale) >= 0.0:
                raise ValueError(f"lr_scale must be >= 0, got {lr_scale}")
            base = rates if rates is not None else np.full(int(epochs) * nb, float(learning_rate), np.float64)
            rates = np.array([cpu().plateau_rate(float(r), float(lr_scale)) for r in base], np.float64)
    elif update_log is not None:
        raise ValueError("update_log needs a schedule, clip_norm or a stateful optimizer")
    from ..optim import new_ema_state, resolve_ema

    ema = resolve_ema(ema)
    if ema is not None:
        est = ema_state if ema_state is not None else new_ema_state(nn)
        if est["avg"].size != nn.num_params() or est["avg"].dtype != np.float64:
            raise ValueError("ema_state does not belong to this network")
        ema_t = np.array([float(est["t"])], np.float64)
        kw["ema"] = (float(ema.decay), bool(ema.warmup), est["avg"], ema_t)
    from ..sampling import resolve as resolve_sampler

    sampler = resolve_sampler(sampler, shuffle_seed)
    try:
        if shuffle_seed is None and augment is None and sampler is None:
            if rates is not None:
                kw["rates"] = rates
            return list(cpu().train(*nn.params, X, labels, float(learning_rate), float(reg), int(epochs),
                                    int(batch_size), int(print_every), bool(debug), outdir, shift,
                                    int(ckpt_precision), int(iter0), **kw))
        losses: list[float] = []
        it = int(iter0)
        if augment is not None:
            from ..augment import (Affine, Warp, apply_affine, apply_shifts, apply_warp, epoch_nodes, epoch_shifts,
                                   epoch_transforms)

            img_h, img_w = augment.shape(X.shape[1])
            warp = isinstance(augment, Warp)
            affine = warp or isinstance(augment, Affine)
        for ep in range(int(epochs)):
            perm = (cpu().epoch_permutation(n, int(shuffle_seed), it) if shuffle_seed is not None
                    else np.arange(n, dtype=np.int32))
            ids = perm  # what the augmentation rules hash: the loaded index, or with a sampler the position
            if sampler is not None:
                perm, ids = sampler.draws(labels, it), np.arange(n)
            if rates is not None:
                kw["rates"] = np.ascontiguousarray(rates[ep * nb:(ep + 1) * nb])
            Xe = np.ascontiguousarray(X[perm])
            if augment is not None and affine:  # (csrc/mlp/affine.h: the sample's table entry, then its shift)
                entries = augment.table()[epoch_transforms(n, augment, it)[ids]]
                Xe = X_raw[perm] if X_raw is not None else Xe
                if warp:  # (csrc/mlp/warp.h: the affine map with the field of the sample's nodes on top)
                    Xe = _x64(apply_warp(Xe, epoch_shifts(n, augment, it)[ids], entries,
                                         epoch_nodes(n, augment, it)[ids], augment, img_h, img_w))
                else:
                    Xe = _x64(apply_affine(Xe, epoch_shifts(n, augment, it)[ids], entries, img_h, img_w))
            elif augment is not None:
                Xe = apply_shifts(Xe, epoch_shifts(n, augment, it)[ids], img_h, img_w)
            losses += cpu().train(*nn.params, Xe, np.ascontiguousarray(labels[perm]),
                                  float(learning_rate), float(reg), 1, int(batch_size), int(print_every),
                                  bool(debug), outdir, shift, int(ckpt_precision), it, **kw)
            it += nb
        return losses
    finally:
        if opt is not None or policy:
            st["t"], st["b1p"], st["b2p"] = int(counter[0]), float(counter[1]), float(counter[2])
        if ema is not None:
            est["t"] = int(ema_t[0])
