"""Shared by tests/test_schedule.py and tests/test_gpu_schedule.py: the padded gradient arenas of the sum-of-squares
tests, the schedule and rules the two files use, and the worker of the two-rank GPU test (importable by spawn)."""
import os

import numpy as np
import torch

from cme213_sp18_amd.optim import SGD_CODE, Optimizer, Schedule

LR, REG = 0.05, 1e-4
ORACLE_LR = 1e-3  # (tests/test_optim.py ORACLE_LR: the runs compared with another summation order)
RULES = {"sgd": Optimizer.sgd(), "nesterov": Optimizer.momentum(0.8, True), "adam": Optimizer.adam(0.9, 0.999, 1e-8)}
# warm-up over two updates, then the rate halves every two: eight updates see the factors 0.1 0.55 1 1 0.5 0.5 0.25 0.25
SCHED = Schedule.step(2, 0.5, unit="step", warmup=2, warmup_start=0.1)
# synthetic_mnist(256, seed=3), 784-100-10, reg 1e-4, lr 1e-3, batch 64: the fp64 oracle's eight unclipped norms are
# 1.921 1.927 1.807 1.701 1.767 1.901 1.753 1.688 -- 1.85 separates them with a 2 % margin on either side
ORACLE_CLIP = 1.85


def rule_code(opt: Optimizer) -> int:
    return opt.code if opt.stateful else SGD_CODE


def segment_sizes(count: int) -> list:
    """`count` elements over the four segments; no size a multiple of 4 once count allows it."""
    if count < 16:
        return [count, 0, 0, 0]
    s0 = count * 7 // 10
    s0 += s0 % 4 == 0
    r = count - s0
    s1 = min(7, r)
    s3 = min(3, r - s1)
    s2 = r - s1 - s3
    if s2 and s2 % 4 == 0:
        s2, s3 = s2 - 1, s3 + 1
    assert s0 + s1 + s2 + s3 == count and all(s % 4 or s == 0 for s in (s0, s1, s2))
    return [s0, s1, s2, s3]


def padded_arena(count: int, ndt, seed: int = 0):
    """A gradient bucket laid out as FlatLayout does -- every segment padded to 64 elements, then the status element
    and its padding -- with NaN in every padding slot and in the status element.  Returns (array, segments)."""
    rng = np.random.default_rng(seed + count)
    parts, segs, o = [], [], 0
    for s in segment_sizes(count):
        pad = -(-s // 64) * 64 - s
        segs.append((o, s))
        parts += [rng.standard_normal(s), np.full(pad, np.nan)]
        o += s + pad
    parts.append(np.full(64, np.nan))  # the status element and its padding
    return np.concatenate(parts).astype(ndt), segs


def pick_clip(norms) -> float:
    """A threshold from the norms an UNCLIPPED run recorded, such that the clipped run is known to hold both kinds of
    update.  A clipped run equals the unclipped one up to and including its first clipped update, so with k an update
    whose norm exceeds every earlier one and c between max(norms[:k]) and norms[k], updates 0 .. k - 1 are not clipped
    and update k is: the k with the widest ratio is taken and c is the geometric mean.  Where the first norm is never
    exceeded by enough, c goes between norms[0] and norms[1] < norms[0]: update 0 is clipped, and update 1 sees
    parameters that differ from the unclipped run's only by the shorter first step.  The margin to the nearer norm
    (sqrt of the ratio) must be at least 1 %: far above what separates two evaluations of the same run."""
    n = np.asarray(norms, np.float64)
    assert n.size >= 2 and n.min() > 0
    best, c = n[0] / n[1], float(np.sqrt(n[0] * n[1]))
    for k in range(1, n.size):
        m = n[:k].max()
        if n[k] / m > best:
            best, c = n[k] / m, float(np.sqrt(n[k] * m))
    assert best >= 1.02, (best, n)
    return c


# ------------------------------------------------------------------------------------------------- two-rank worker
def gpu_shared_sched_worker(rank, world, comm, device, out_dir, mode, clip):
    """Two processes sharing GPU 0 (gloo group, hip backend): gradient mode, the all-reduce of ``mode`` (rccl = the
    communicator's, xgmi = the separate peer-to-peer kernel), then the sum-of-squares and the apply launch on the summed
    gradient.  Every rank saves its arena, state and counter records; replicas_agree() covers them."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x, y = synthetic_mnist(384, seed=11)
    res = {}
    for kind in ("sgd", "nesterov"):
        tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), comm=comm, device=dev, batch_size=128, allreduce=mode,
                                 optimizer=RULES[kind], schedule=SCHED, clip_norm=float(clip))
        assert (tr.xgmi is not None) == (mode == "xgmi")
        tr.load(x, y)
        tr.train(2, ORACLE_LR, REG)
        torch.cuda.synchronize()
        res[f"{kind}_agree"] = float(tr.replicas_agree())
        res[f"{kind}_fused"] = float(tr.fused_allreduce or tr._xgmi_fused is not None)
        res[f"{kind}_t"] = float(tr.engine.update_count())
        res[f"{kind}_params"] = tr.engine.params.cpu().numpy()
        res[f"{kind}_rec"] = tr.engine.opt_rec.cpu().numpy()
        res[f"{kind}_last"] = tr.engine.opt_last.cpu().numpy()
        if tr.engine.opt_bufs:
            res[f"{kind}_state"] = torch.cat(tr.engine.opt_bufs).cpu().numpy()
        res["impl"] = tr.allreduce_impl
        tr.close()
    np.savez(os.path.join(out_dir, f"sched_{mode}_{rank}.npz"), **{k: np.asarray(v) for k, v in res.items()})


def gpu_shared_sched_main(out_dir, mode, clip):
    """clip: the threshold, taken by the caller from the fp64 oracle's own unclipped norms of this run."""
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_sched_worker, 2, (out_dir, mode, float(clip)), backend="gloo")
