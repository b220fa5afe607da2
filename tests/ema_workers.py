"""Shared by tests/test_ema.py and tests/test_gpu_ema.py: a Python re-statement of the averaging rule (csrc/mlp/ema.h) in
exact rational arithmetic, the trainers of the tests, the host recurrence over a twin's per-step parameters, and the
worker of the two-rank GPU test (started by cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device,
*args))."""
import os
from fractions import Fraction

import numpy as np

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.optim import Ema, Optimizer, Schedule

from .best_oracle import data

LR, REG = 0.2, 1e-4
RULE = Ema(0.9, warmup=True)  # (12 - 16 updates in these tests: the warmup's decays 0.1 .. 0.64, then the cap is far)
MANT = {np.float32: 24, np.float64: 53}


def py_decay(decay, warmup, t):
    """d_t in Python floats (fp64): the header's expression, operation by operation."""
    if not warmup:
        return float(decay)
    w = (1.0 + float(t)) / (10.0 + float(t))
    return w if w < decay else float(decay)


def round_frac(fr, mant):
    """The value of Fraction ``fr`` rounded once to ``mant`` significant bits, ties to even, as a Fraction (normal range:
    no overflow or subnormals in these tests)."""
    if fr == 0:
        return Fraction(0)
    s, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    ulp = Fraction(2) ** (e - mant + 1)  # 2^e <= a < 2^(e+1)
    q = a / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return s * n * ulp


def frac_update(e, p, d, dtype):
    """One element of one update in exact arithmetic: omd = T(1 - d) (1 - d formed in fp64, rounded to T once), the
    difference p - e rounded to T once, the fused product-sum rounded to T once; p == e returns e."""
    mant = MANT[dtype]
    if p == e:
        return dtype(e)
    omd = Fraction(float(dtype(1.0 - d)))
    diff = round_frac(Fraction(float(p)) - Fraction(float(e)), mant)
    out = round_frac(omd * diff + Fraction(float(e)), mant)
    return dtype(float(out))  # (exactly representable: the conversions do not round)


def recurrence(e0, params_seq, rule, t0=0):
    """The host recurrence: e0 (a flat array in the parameter dtype) folded with every array of ``params_seq`` by
    _cpu.ema_step.  Returns (average, count)."""
    e = np.array(e0, copy=True)
    t = int(t0)
    for p in params_seq:
        t = cpu().ema_step(e, np.ascontiguousarray(p), float(rule.decay), bool(rule.warmup), t)
    return e, t


OPTS = {
    "sgd": dict(),
    "momentum": dict(optimizer=Optimizer("momentum", momentum=0.9)),
    "adam_cosine_clip": dict(optimizer=Optimizer.adam(), schedule=Schedule.cosine(16, 0.1), clip_norm=1.0),
}
OPT_LR = {"sgd": LR, "momentum": LR, "adam_cosine_clip": 0.01}


def make_trainer(opt="momentum", ema=RULE, dtype="f64", H=16, batch=128, device="cpu", backend="torch", comm=None,
                 ntrain=512, nval=256, **kw):
    """784-H-10 on best_oracle's 512 training / 256 validation samples, batch 128, with the update rule ``opt``."""
    from cme213_sp18_amd.parallel import DataParallelTrainer

    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), comm=comm, device=device, dtype=dtype, batch_size=batch,
                             backend=backend, ema=ema, **{"use_graphs": False, **OPTS[opt], **kw})
    (x, y), (xv, yv) = data(ntrain, nval)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    return tr


def arena(t):
    """A flat device tensor's averaged / parameter elements (without the status element) as a host array."""
    return t.detach().cpu().numpy().copy()


def live(tr):
    e = tr.engine
    return arena(e.params[:e.ema_count_elems])


def average(tr):
    e = tr.engine
    return arena(e._ema["arena"][:e.ema_count_elems])


def twin_steps(tr, epochs, lr, reg=REG):
    """``tr`` (a trainer WITHOUT averaging) stepped eagerly through ``epochs`` epochs of its plan; the parameters are read
    on the host after every step.  Returns the list of flat arrays."""
    import torch

    seq = []
    n = int(tr.engine.layout.status)
    for _ in range(epochs):
        for s, ln in tr.epoch_plan().steps:
            tr.step(s, ln, lr, reg)
            if tr.engine.device.type == "cuda":
                torch.cuda.synchronize()
            seq.append(arena(tr.engine.params[:n]))
        tr.iter += len(tr.epoch_plan().steps)
    return seq


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---------------------------------------------------------------------------------------------- two ranks, one GPU
EPOCHS2 = 2


def gpu_shared_ema_worker(rank, world, comm, device, out_dir, mode):
    """Two processes sharing GPU 0 (gloo group, hip backend), the all-reduce of ``mode`` (rccl = the communicator's):
    two epochs step by step, the parameters read after every step, then one epoch through train().  Every rank saves
    its per-step parameters, its average before and after train(), every record and replicas_agree()."""
    import torch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    tr = make_trainer("momentum", dtype="f32", H=100, device=dev, backend="hip", comm=comm, allreduce=mode,
                      use_graphs=True)
    e0 = live(tr)
    seq = twin_steps(tr, EPOCHS2, LR)
    avg, recs = average(tr), tr.engine.ema_records()
    tr.train(1, LR, REG)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"ema_{mode}_{rank}.npz"), e0=e0, seq=np.stack(seq), avg=avg, recs=recs,
             params=live(tr), avg2=average(tr), recs2=tr.engine.ema_records(), agree=float(tr.replicas_agree()),
             impl=tr.allreduce_impl)
    tr.close()


def gpu_shared_ema_main(out_dir, mode):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_ema_worker, 2, (out_dir, mode), backend="gloo")
