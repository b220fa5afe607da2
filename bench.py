#!/usr/bin/env python3
"""Headline benchmark: MNIST images/sec, 784-100-10 MLP, batch=800, on N MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N>1 it
runs under ``torch.distributed.run`` (one rank per GPU, RCCL) -- started by the
driver, or, when no launcher started this process, by bench.py itself (a child
launcher).  Every rank checks that the job is N ranks on N distinct GPUs and
exits non-zero WITHOUT a record otherwise (ranks_seen / devices_distinct are in
the record, with the measured all-reduce time of the step's bucket).  W untimed
warm-up steps, then EXACTLY K timed optimizer steps bracketed by barrier +
synchronize on both sides; the max time over ranks is reported; rank 0 prints
one JSON line.

What a step is (the reference's ``parallel_train`` inner loop,
fpcode/neural_network.cpp:449-555): one synchronous SGD update -- forward +
backward of the 784-100-10 MLP (random-init weights, seeded as the reference
does) on every rank, gradient all-reduce (xGMI peer kernel with the SGD
fused in, or RCCL with ``--allreduce rccl``), SGD update -- on
synthetic MNIST-shaped images resident on every GPU.  Nothing is skipped
inside the timed region.  Steps cycle over the full batches of the 54,000-image
training split.

Scaling (default ``strong``: the metric's own config).  A global batch of 800
is split over the N ranks, n = 800/N columns each -- the reference's ``-b 800``
run (fpcode/run.sh:39, ``in_proc = min(batch, N - start) / num_procs``,
fpcode/neural_network.cpp:458); ``value`` is that run's images/s.  At N > 1 the
record also carries the weak-scaling run (800 images per GPU per step, global
batch 800*N) as the labelled secondary ``weak`` sub-record when ``--full`` is given
(``--secondary off`` skips it even then).  ``--scaling weak`` swaps the two.  At N = 1
both are batch 800.

A plain run does only what the headline figure needs: set-up, W warm-up steps, the K
timed steps, the record.  ``--full`` adds what takes runs of its own: the secondary
scaling sub-record and the step's all-reduce timed alone (``allreduce_us``,
``allreduce_bytes``, ``allreduce_busbw_GBps``; ``allreduce_us`` is null without it).

``--dump-outputs DIR`` writes what the last timed step left a caller of the step with,
the parameters W1, b1, W2, b2, as ``DIR/<name>.npy`` (float64 for ``--dtype f64``, else
float32; rank 0 writes).  Data and initial weights are seeded, so two builds run with
the same arguments can be compared array for array.

N > 1 choices made by measurement on the node, inside a wall-time budget
(``--tune-budget-s``): the gradient all-reduce (the cost model's xGMI pick, the
two-shot, RCCL) and, for the wide configs (H >= 512), data vs tensor parallel.
Every probe's us/step is in the record next to the cost model's predicted
all-reduce time (``allreduce_pred_us``); candidates the budget did not reach are
recorded as ``"skipped: budget"``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

METRIC = "MNIST images/sec, 784-100-10 MLP batch=800 at 1/2/4/8 MI355X"
BASELINE_VALUE = None  # BASELINE.json "published": {} -- no reference number exists
DATA = "synthetic (MNIST-shaped 784-dim uint8 images, random-init weights)"
DTYPES = {"f32": "fp32", "f64": "fp64", "bf16": "bf16"}
LR, REG = 1e-3, 1e-4  # reference defaults (fpcode/main.cpp:58-60)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--batch", type=int, default=800, help="global batch (strong) or per-GPU batch (weak)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64", "bf16"])
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="strong (default, the metric's config): --batch is the global batch, split over the "
                         "ranks; weak: --batch images per GPU")
    ap.add_argument("--secondary", default="auto", choices=["auto", "off"],
                    help="auto: with --full and N > 1 also time the other scaling mode into a labelled sub-record")
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--executor", default="auto", choices=["auto", "graph", "eager"],
                    help="auto: the native C++ step loop where a step is pure device work (one process, or the "
                         "xGMI-fused all-reduce), else captured HIP graphs; graph: always graphs")
    ap.add_argument("--allreduce", default="auto", choices=["auto", "xgmi", "xgmi2", "rccl", "host"],
                    help="gradient sync for N>1: auto (by bucket size and ranks), the xGMI one-shot peer kernel "
                         "with fused SGD (xgmi), the xGMI two-shot kernel with sharded SGD (xgmi2), RCCL, or "
                         "host-staged gloo (reference-equivalent).  Tensor parallel maps it onto its z2 "
                         "all-reduce (tensor_parallel.tp_allreduce_mode: xgmi2 -> xgmi, host -> rccl)")
    ap.add_argument("--grad-wire", default="auto", choices=["auto", "f32", "bf16"],
                    help="element type of the gradients on the xGMI one-shot wire (bf16: opt-in, half the bytes)")
    ap.add_argument("--mode", default="optimized", choices=["optimized", "reference"],
                    help="reference: the reference's execution model on MI355X -- unfused PyTorch/hipBLAS ops, "
                         "no graphs, host-staged gradient all-reduce (for comparison only)")
    ap.add_argument("--parallel", default="auto", choices=["auto", "dp", "tp"],
                    help="dp: data parallel (the reference's scheme); tp: hidden-dimension tensor parallel "
                         "(one z2 all-reduce per step, every rank runs the whole global batch); auto: dp, except "
                         "for the wide layers (H >= 512) at N > 1, where both are probed and the faster is timed")
    ap.add_argument("--tune-allreduce", default="on", choices=["on", "off"],
                    help="N > 1 with --allreduce auto: time the policy's xGMI pick, the xGMI two-shot (N >= 3) and "
                         "RCCL for --tune-steps steps each before the timed region and run the fastest (the record "
                         "lists every candidate)")
    ap.add_argument("--tune-steps", type=int, default=100)
    ap.add_argument("--tune-budget-s", type=float, default=90.0,
                    help="wall-time cap on all probing (all-reduce and parallelism candidates); candidates past it "
                         "are recorded as 'skipped: budget'")
    ap.add_argument("--train-size", type=int, default=54000)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need (runs of their own): at N > 1 the "
                         "secondary scaling sub-record and the step's all-reduce timed alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the parameters they produced (W1, b1, W2, b2) as DIR/<name>.npy")
    return ap.parse_args(argv)


class Ctx:
    """What every measurement shares: arguments, communicator, device, data, the probe budget."""

    def __init__(self, a, comm, device, placement):
        import torch

        from cme213_sp18_amd.utils.data import synthetic_mnist

        self.a, self.comm, self.device, self.placement = a, comm, device, placement
        self.R, self.rank = comm.world_size, comm.rank
        self.sync = (lambda: torch.cuda.synchronize(device)) if device.type == "cuda" else (lambda: None)
        self.x, self.y = synthetic_mnist(a.train_size, seed=0)  # identical on every rank, no broadcast
        self.t_budget0 = time.perf_counter()

    def budget_left(self) -> bool:
        """Collective: True while probing may go on (every rank gets the same answer)."""
        el = self.comm.allreduce_scalar(time.perf_counter() - self.t_budget0, op="max")
        return el < self.a.tune_budget_s

    def barrier_sync(self):
        self.sync()
        self.comm.barrier()
        self.sync()


def plans_for(full, k: int):
    from cme213_sp18_amd.parallel.trainer import EpochPlan

    out, i = [], 0
    while i < k:
        m = min(len(full), k - i)
        out.append(EpochPlan(full[:m]))
        i += m
    return out


def timed(ctx, runners) -> float:
    """Seconds for the runners, bracketed by barrier + synchronize on both sides, max over ranks."""
    ctx.barrier_sync()
    t0 = time.perf_counter()
    for run in runners:
        run()
    ctx.sync()
    ctx.comm.barrier()
    if ctx.R > 1:  # an RCCL barrier is GPU work; one process has nothing left to wait for
        ctx.sync()
    return ctx.comm.allreduce_scalar(time.perf_counter() - t0, op="max")


# ------------------------------------------------------------------------------------------ data parallel
def dp_prepare(ctx, global_batch: int, allreduce: str, warmup: int, extra_plans: int = 0):
    """Trainer + captured graphs + ``warmup`` warm-up steps.  Returns (trainer, full-batch list).  ``allreduce``:
    an --allreduce value, or "xgmi-push" (the xGMI all-reduce fused into the weight-gradient launch in its
    owner-tile push form; "xgmi" / "auto" fuse the one-shot pull)."""
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer

    a = ctx.a
    nn = NeuralNetwork([784, a.hidden, 10])
    form = "push" if allreduce == "xgmi-push" else "auto"
    tr = DataParallelTrainer(nn, comm=ctx.comm, device=ctx.device, dtype=a.dtype, batch_size=global_batch,
                             backend=a.backend, use_graphs=not a.no_graphs,
                             allreduce="xgmi" if allreduce == "xgmi-push" else allreduce, grad_wire=a.grad_wire,
                             executor="eager" if a.no_graphs else a.executor, fused_form=form)
    tr.load(ctx.x, ctx.y)
    full = [(s, ln) for s, ln in tr.epoch_plan().steps if ln == global_batch]
    if not full:
        raise SystemExit("training split smaller than one global batch")
    warm = plans_for(full, warmup)
    every = warm + plans_for(full, a.steps) + plans_for(full, extra_plans)
    native = all(tr.native_plan(p) is not None for p in every)
    if tr.use_graphs and not native:  # capture outside the timed region (graphs are cached by plan)
        try:
            for p in {tuple(p.steps): p for p in every}.values():
                tr.capture(p, LR, REG)
        except Exception as ex:  # pragma: no cover - depends on the collective backend
            print(f"warning: HIP graph capture failed ({ex!r}); running eager steps", file=sys.stderr)
            tr.use_graphs = False
            tr._graphs.clear()
    # every rank done capturing before the first warm-up step: with the xGMI all-reduce a step waits
    # (bounded) for its peers' same step, so a rank still capturing would count against that bound
    ctx.sync()
    ctx.comm.barrier()
    for p in warm:
        tr.run_plan(p, LR, REG)
    return tr, full


def dp_healthy(tr) -> bool:
    """Collective: no xGMI wait timed out and the replicas agree bitwise."""
    return not tr.comm_failed() and tr.replicas_agree()


def dp_probe(ctx, tr, full, steps: int) -> float:
    """us/step of ``steps`` steps on this trainer, max over ranks (inf if a wait timed out or replicas differ)."""
    runners = [tr.plan_runner(p, LR, REG) for p in plans_for(full, steps)]
    us = 1e6 * timed(ctx, runners) / steps
    return round(us, 3) if dp_healthy(tr) else float("inf")


def dp_tune_allreduce(ctx, global_batch: int, tune: dict) -> str:
    """The gradient sync mode to time (an --allreduce value), chosen by measurement when N > 1 and
    --allreduce auto: the cost model's pick, the other form of the fused xGMI all-reduce (the owner-tile push next
    to the one-shot pull: which is faster rests on a hop latency only the node can tell), the xGMI two-shot
    (N >= 3) and RCCL each run --tune-steps steps from the initial weights (the fastest wins; identical floats on
    every rank: one decision).  Results go into ``tune`` (impl name -> us/step, 'failed', 'unavailable' or
    'skipped: budget')."""
    a = ctx.a
    if not (ctx.R > 1 and a.allreduce == "auto" and a.backend == "hip" and a.tune_allreduce == "on"):
        return a.allreduce
    # the policy's own pick first (its trainer tells which implementation "auto" resolves to)
    tr, full = dp_prepare(ctx, global_batch, "auto", a.warmup, a.tune_steps)
    pick = tr.allreduce_impl
    modes = {pick: "auto"}
    if pick.startswith("xgmi") and (tr.comm_failed() or not tr.replicas_agree()):
        # a bounded peer wait timed out (or a stale read) during the warm-up: the xGMI protocol misbehaves on
        # this node -- every rank drops it together
        tune[pick] = "failed in warm-up"
    else:
        tune[pick] = dp_probe(ctx, tr, full, a.tune_steps)
    tr.close()
    others = ((["xgmi-push"] if pick == "xgmi-fused" else []) + (["xgmi2"] if ctx.R >= 3 and pick != "xgmi-2shot" else [])
              + (["rccl"] if pick.startswith("xgmi") else []))
    for mode in others:
        if not ctx.budget_left():
            tune[{"xgmi-push": "xgmi-push", "xgmi2": "xgmi-2shot", "rccl": ctx.comm.name}[mode]] = "skipped: budget"
            continue
        try:
            tr, full = dp_prepare(ctx, global_batch, mode, a.warmup, a.tune_steps)
        except Exception as ex:  # noqa: BLE001 - a candidate the node cannot run (raised on every rank)
            tune[mode] = "unavailable"
            if ctx.rank == 0:
                print(f"allreduce candidate {mode} unavailable: {ex}", file=sys.stderr, flush=True)
            continue
        modes[tr.allreduce_impl] = mode
        tune[tr.allreduce_impl] = dp_probe(ctx, tr, full, a.tune_steps)
        tr.close()
    nums = {k: v for k, v in tune.items() if isinstance(v, float) and v != float("inf")}
    for k, v in list(tune.items()):
        if v == float("inf"):
            tune[k] = "failed"
    if not nums:
        return "rccl"
    best = min(nums, key=lambda k: (nums[k], k))
    if ctx.rank == 0:
        print(f"allreduce tuned on this node: {tune} -> {best}", file=sys.stderr, flush=True)
    return modes[best]


PROBE_FACTOR = 3.0  # a timed run this many times slower per step than its probe is not trusted


def guard_probe(res: dict, steps: int, probe_us, retime=None) -> dict:
    """First-contact guard: the timed us/step against the probe that chose its configuration (max over
    ranks on both sides, so every rank decides alike).  More than PROBE_FACTOR x off: re-timed on the next
    candidate -- ``retime`` is one callable or a fallback CHAIN of them, tried in order (the owner-tile push form:
    push -> the one-shot pull -> RCCL), each ``() -> (result, its own probe us/step or None)``; the first re-timed run
    that agrees with its probe is reported.  None agrees (or nothing to fall back on): the record is marked
    ``"invalid": "timed run inconsistent with probe"`` instead of reported clean.  The decision and every timing go
    into ``config.probe_guard`` ("first", "retimed" = the last re-time, "chain" = all of them when more than one; a
    re-timed run's own guard record is kept under "inner")."""
    if not isinstance(probe_us, (int, float)) or not probe_us or probe_us == float("inf") or not res.get("ok"):
        return res
    us = 1e6 * res["dt"] / steps
    first = {"timed_us_per_step": round(us, 3), "probe_us_per_step": round(probe_us, 3),
             "what": res["config"].get("allreduce") if res.get("parallelism", "").startswith("dp")
             else res.get("parallelism")}
    if us <= PROBE_FACTOR * probe_us:
        res["config"]["probe_guard"] = {"consistent": True, **first}
        return res
    chain = [] if retime is None else (list(retime) if isinstance(retime, (list, tuple)) else [retime])
    if not chain:
        res["config"]["probe_guard"] = {"consistent": False, "first": first}
    done = []
    for k, fn in enumerate(chain):
        res2, probe2 = fn()
        us2 = 1e6 * res2["dt"] / steps
        ref = probe2 if isinstance(probe2, (int, float)) and probe2 and probe2 != float("inf") else probe_us
        second = {"timed_us_per_step": round(us2, 3), "probe_us_per_step": round(ref, 3),
                  "what": res2["config"].get("allreduce") if res2.get("parallelism", "").startswith("dp")
                  else res2.get("parallelism")}
        done.append(second)
        inner = res2["config"].get("probe_guard")  # the re-timed run's own guard (run_dp), kept, not overwritten
        ok2 = bool(res2.get("ok")) and us2 <= PROBE_FACTOR * ref
        res2["config"]["probe_guard"] = {"consistent": ok2, "first": first, "retimed": second,
                                         **({"chain": list(done)} if len(chain) > 1 else {}),
                                         **({"inner": inner} if inner else {})}
        res = res2
        if ok2:
            return res2
    res["ok"] = False
    res["invalid"] = "timed run inconsistent with probe"
    return res


def run_dp(ctx, global_batch: int, allreduce: str | None = None, tune: dict | None = None) -> dict:
    """One data-parallel measurement: K timed steps of global batch ``global_batch`` (n = global_batch / R per
    rank).  The trainer is always prepared afresh for the timed region (from the initial weights, after W
    warm-up steps), whichever candidate won the tuning.  A timed run far off its probe is re-timed once on RCCL
    (guard_probe)."""
    a = ctx.a
    tune = {} if tune is None else tune
    mode = allreduce if allreduce is not None else dp_tune_allreduce(ctx, global_batch, tune)
    res = _run_dp_timed(ctx, global_batch, mode, tune)
    impl = res["config"]["allreduce"]
    return guard_probe(res, a.steps, tune.get(impl), dp_fallbacks(ctx, global_batch, impl, tune))


def dp_fallbacks(ctx, global_batch: int, impl: str, tune: dict) -> list:
    """The first-contact guard's re-time chain for a data-parallel run on ``impl`` (each entry probes its candidate,
    then times it): the owner-tile push form falls back to the one-shot pull and then RCCL, every other xGMI form
    to RCCL; RCCL itself (and one rank) to nothing."""
    a = ctx.a
    if ctx.R <= 1 or impl == ctx.comm.name:
        return []

    def on(mode):
        def retime():
            tr, full = dp_prepare(ctx, global_batch, mode, a.warmup, a.tune_steps)
            probe = dp_probe(ctx, tr, full, a.tune_steps)
            tr.close()
            return _run_dp_timed(ctx, global_batch, mode, tune), probe
        retime.mode = mode
        return retime
    return ([on("xgmi")] if impl == "xgmi-push" else []) + [on("rccl")]


def _run_dp_timed(ctx, global_batch: int, mode: str, tune: dict) -> dict:
    from cme213_sp18_amd.parallel.trainer import allreduce_cost_us

    a = ctx.a
    tr, full = dp_prepare(ctx, global_batch, mode, a.warmup)
    if tr.allreduce_impl.startswith("xgmi") and mode in ("auto",) and not dp_healthy(tr):
        # a bounded peer wait timed out during the warm-up: every rank drops to RCCL together, from the
        # initial weights, before anything is timed
        if ctx.rank == 0:
            print("warning: xGMI all-reduce failed in warm-up; re-running on RCCL", file=sys.stderr)
        tr.close()
        tune["xgmi"] = "failed in warm-up"
        tr, full = dp_prepare(ctx, global_batch, "rccl", a.warmup)
    forced = os.environ.get("CME_BENCH_TEST_FALLBACK") == "1" and a.allreduce == "auto"
    if ctx.comm.allreduce_scalar(float(forced), op="max") > 0 and tr.allreduce_impl.startswith("xgmi"):
        # test hook: take the fallback as if the warm-up had failed
        tr.close()
        tune["xgmi"] = "failed in warm-up"
        tr, full = dp_prepare(ctx, global_batch, "rccl", a.warmup)
    timed_plans = plans_for(full, a.steps)
    native_exec = all(tr.native_plan(p) is not None for p in timed_plans)
    runners = [tr.plan_runner(p, LR, REG) for p in timed_plans]  # resolved before the clock starts
    dt = timed(ctx, runners)
    # which step form the native loop ran: the XCD-local pipeline (one launch per plan, csrc/mlp/xstep.hip) or the
    # two-launch step (and why not the pipeline)
    step = tr.engine._step if a.backend == "hip" else None
    pipeline = None if step is None else {"used": bool(step.xstep_used), "why_not": step.xstep_reason or None}
    res = _dp_checks(ctx, tr)
    ar = (measure_allreduce(tr, ctx.comm, ctx.sync) if a.full else {"allreduce_us": None}) if res["ok"] else {}
    if a.dump_outputs:
        res["outputs"] = tr.engine.get_params()
    e = tr.engine
    wire = e.params.numel() * (2 if tr.xgmi is not None and tr.xgmi.wire != e.params.dtype else e.params.element_size())
    shots = 0 if tr.xgmi is None else tr.xgmi.shots
    fp_bytes = e.params.numel() * e.params.element_size()
    # strong scaling drops the remainder columns when R does not divide the batch (trainer.shard)
    images = a.steps * (global_batch // ctx.R) * ctx.R
    res.update(dt=dt, images=images, global_batch=global_batch, per_gpu_batch=global_batch // ctx.R,
               parallelism=f"dp{ctx.R}",
               config={"hip_graphs": tr.use_graphs and not native_exec,
                       "executor": "native" if native_exec else ("graph" if tr.use_graphs else "eager"),
                       **({"xstep_pipeline": pipeline} if pipeline is not None and native_exec else {}),
                       "allreduce": tr.allreduce_impl, **ar,
                       "allreduce_pred_us": round(allreduce_cost_us(ctx.R, wire, shots, fp_bytes=fp_bytes), 2)
                       if ctx.R > 1 else None,
                       "allreduce_tuning_us_per_step": tune or None})
    tr.close()
    return res


def _dp_checks(ctx, tr) -> dict:
    """Sanity, agreed by every rank: parameters finite everywhere, no xGMI peer wait or in-launch hand-off
    timed out anywhere, replicas bitwise equal; otherwise the record is marked invalid."""
    import torch

    comm = ctx.comm
    finite = bool(torch.isfinite(tr.engine.params).all().item())
    bad = comm.allreduce_scalar(0.0 if finite else 1.0, op="max") > 0
    comm_failed = tr.comm_failed()
    kerr = comm.allreduce_scalar(1.0 if tr.engine.kernel_error() else 0.0, op="max") > 0
    agree = tr.replicas_agree()
    ok = not bad and not comm_failed and not kerr and agree
    out = {"ok": ok, "checks": {"params_finite": not bad, "comm_ok": not comm_failed, "replicas_bitwise_equal": agree}}
    if not ok:
        out["invalid"] = ("non-finite parameters" if bad else "an xGMI peer wait timed out" if comm_failed
                          else "a forward+head workgroup wait timed out" if kerr else "replicas diverged across ranks")
    return out


def measure_allreduce(tr, comm, sync, iters: int = 20) -> dict:
    """After the timed run: the per-call time of the step's gradient all-reduce on its own (the same
    implementation and bucket bytes, max over ranks), so a scaling curve can be split into compute and
    communication.  The xGMI forms are timed through their one-shot kernel (the fused form runs the same
    protocol inside the wgrad launch); the overlapped RCCL backward through one whole-bucket all-reduce."""
    import torch

    if comm.world_size == 1:
        return {"allreduce_us": None}
    e = tr.engine
    buf = torch.zeros_like(e.grads)
    if tr.xgmi is not None:
        fn, wire = (lambda: tr.xgmi.allreduce_(buf)), tr.xgmi.wire
    elif tr.allreduce_mode == "host":
        import torch.distributed as dist

        def fn():
            g = buf.cpu()
            dist.all_reduce(g, group=tr._host_group)
            buf.copy_(g)
        wire = buf.dtype
    else:
        fn, wire = (lambda: comm.allreduce_(buf)), buf.dtype
    for _ in range(3):
        fn()
    sync()
    comm.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    us = comm.allreduce_scalar(1e6 * (time.perf_counter() - t0) / iters, op="max")
    nbytes = buf.numel() * torch.tensor([], dtype=wire).element_size()
    R = comm.world_size
    return {"allreduce_us": round(us, 2), "allreduce_bytes": int(nbytes),
            "allreduce_busbw_GBps": round(2 * (R - 1) / R * nbytes / (us * 1e-6) / 1e9, 2)}


# ---------------------------------------------------------------------------------------- tensor parallel
def run_tp(ctx, B: int, steps: int | None = None) -> dict:
    """Hidden-sharded tensor-parallel step (parallel/tensor_parallel.py): every rank runs the whole global
    batch B on its H / R hidden units; ``steps`` timed steps (default --steps) bracketed like the DP run."""
    import torch

    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer, tp_allreduce_mode
    from cme213_sp18_amd.parallel.trainer import allreduce_cost_us

    a, comm, R = ctx.a, ctx.comm, ctx.R
    steps = a.steps if steps is None else steps
    nn = NeuralNetwork([784, a.hidden, 10])
    tr = TensorParallelTrainer(nn, comm=comm, device=ctx.device, dtype=a.dtype, batch_size=B, backend=a.backend,
                               allreduce=tp_allreduce_mode(a.allreduce))
    tr.load(ctx.x, ctx.y)
    full = [(s, ln) for s, ln in tr.epoch_plan().steps if ln == B]
    if not full:
        raise SystemExit("training split smaller than one global batch")
    warm, tplans = plans_for(full, a.warmup), plans_for(full, steps)
    graphs = tr.graphs_usable(not a.no_graphs)
    if graphs:  # every distinct plan captured outside the timed region
        for p in {tuple(p.steps): p for p in warm + tplans}.values():
            tr.capture(p, LR, REG)
    for p in warm:
        tr.run_plan(p, LR, REG, use_graphs=graphs)
    dt = timed(ctx, [lambda p=p: tr.run_plan(p, LR, REG, use_graphs=graphs) for p in tplans])
    finite = bool(torch.isfinite(tr.engine.params).all().item())
    ok = comm.allreduce_scalar(0.0 if finite else 1.0, op="max") == 0
    comm_failed = tr.comm_failed()
    ok = ok and not comm_failed
    ar = {"allreduce_us": None}
    if R > 1 and ok and a.full:  # the step's z2 all-reduce on its own (same implementation and bytes), max over ranks
        fn = (lambda: tr._xz.allreduce_(tr.z2)) if tr._xz is not None else (lambda: comm.allreduce_(tr.z2))
        for _ in range(3):
            fn()
        ctx.barrier_sync()
        t1 = time.perf_counter()
        for _ in range(20):
            fn()
        ctx.sync()
        us = comm.allreduce_scalar(1e6 * (time.perf_counter() - t1) / 20, op="max")
        ar = {"allreduce_us": round(us, 2), "allreduce_bytes": int(tr.z2.numel() * 4)}
    impl = tr.allreduce_impl
    outputs = tr.gather_params() if a.dump_outputs else None  # collective: the shards of every rank
    tr.close()
    res = {"ok": ok, "dt": dt, "images": steps * B, "global_batch": B, "per_gpu_batch": B, "parallelism": f"tp{R}",
           "checks": {"params_finite": finite, "comm_ok": not comm_failed},
           "config": {"hidden_per_gpu": a.hidden // R, "hip_graphs": graphs, "allreduce": impl, **ar,
                      "allreduce_pred_us": round(allreduce_cost_us(R, int(tr.z2.numel() * 4), 1 if "xgmi" in impl
                                                                   else 0), 2) if R > 1 else None}}
    if not ok:
        res["invalid"] = "an xGMI peer wait timed out" if comm_failed else "non-finite parameters"
    if outputs is not None:
        res["outputs"] = outputs
    return res


# --------------------------------------------------------------------------------------------- measuring
def choose_parallel(ctx, gb_dp: int, gb_tp: int, ptune: dict) -> str:
    """--parallel auto: dp, except for the wide layers at N > 1 on the hip backend, where DP (the all-reduce
    policy's pick) and TP each run --tune-steps steps and the faster is timed (inside the probe budget)."""
    a = ctx.a
    if a.parallel != "auto":
        return a.parallel
    if not (ctx.R > 1 and a.hidden >= 512 and a.backend == "hip" and a.hidden % ctx.R == 0):
        return "dp"
    tp = run_tp(ctx, gb_tp, steps=a.tune_steps)
    ptune[tp["parallelism"]] = round(1e6 * tp["dt"] / a.tune_steps, 3) if tp["ok"] else "failed"
    if ctx.budget_left():
        tr, full = dp_prepare(ctx, gb_dp, "auto", a.warmup, a.tune_steps)
        ptune[f"dp{ctx.R}"] = dp_probe(ctx, tr, full, a.tune_steps)
        if ptune[f"dp{ctx.R}"] == float("inf"):
            ptune[f"dp{ctx.R}"] = "failed"
        tr.close()
    else:
        ptune[f"dp{ctx.R}"] = "skipped: budget"
    nums = {k: v for k, v in ptune.items() if isinstance(v, float)}
    best = min(nums, key=lambda k: (nums[k], k)) if nums else f"dp{ctx.R}"
    if ctx.rank == 0:
        print(f"parallelism tuned on this node: {ptune} -> {best}", file=sys.stderr, flush=True)
    return "tp" if best.startswith("tp") else "dp"


def measure(ctx, scaling: str, parallel: str | None = None, allreduce: str | None = None) -> dict:
    """One timed run of the given scaling mode.  Returns the run's summary (``parallel`` and the all-reduce mode
    chosen, so a secondary run can reuse them instead of probing again)."""
    a = ctx.a
    gb = a.batch if scaling == "strong" else a.batch * ctx.R
    ptune: dict = {}
    if parallel is None:
        parallel = choose_parallel(ctx, gb, gb, ptune)
    if parallel == "tp":
        res = run_tp(ctx, gb)
        if ptune:  # chosen by probing: a timed run far off its probe is re-timed once on data parallel
            # (the fallback runs the configuration choose_parallel probed -- the all-reduce policy's pick -- without
            # a second all-reduce sweep; its guard is the outer one, against that probe)
            res = guard_probe(res, a.steps, ptune.get(res["parallelism"]),
                              lambda: (run_dp(ctx, gb, allreduce="auto", tune={}), ptune.get(f"dp{ctx.R}")))
            if res["parallelism"].startswith("dp"):
                parallel = "dp"
                res["allreduce_mode"] = _mode_of(res["config"]["allreduce"], ctx)
    else:
        tune: dict = {}
        res = run_dp(ctx, gb, allreduce=allreduce, tune=tune)
        res["allreduce_mode"] = allreduce if allreduce is not None else _mode_of(res["config"]["allreduce"], ctx)
    res["parallel"] = parallel
    res["scaling"] = scaling
    if ptune:
        res["config"]["parallel_tuning_us_per_step"] = ptune
    return res


def _mode_of(impl: str, ctx) -> str:
    """The --allreduce value that reproduces an implementation name (for the secondary run)."""
    if ctx.R == 1:
        return "auto"
    return {"xgmi": "xgmi", "xgmi-fused": "xgmi", "xgmi-push": "xgmi-push", "xgmi-2shot": "xgmi2", "xgmi-bf16wire": "xgmi",
            "host-gloo": "host"}.get(impl, "rccl")


OUTPUT_NAMES = ("W1", "b1", "W2", "b2")
DUMP_CAP_BYTES = 64 * 1000 * 1000


def dump_outputs(directory: str, arrays, dtype: str) -> None:
    """``directory/<name>.npy`` for the parameters the timed steps produced (float64 for f64 runs, else float32:
    exact for fp32 parameters).  Past DUMP_CAP_BYTES in all, an array larger than its share is cut down to a fixed,
    seeded sample of its elements (the same indices in every run, in ascending order)."""
    import numpy as np

    dt = np.float64 if dtype == "f64" else np.float32
    arrays = [np.ascontiguousarray(x, dtype=dt) for x in arrays]
    share = DUMP_CAP_BYTES // len(arrays) // np.dtype(dt).itemsize  # elements
    if sum(x.nbytes for x in arrays) > DUMP_CAP_BYTES:
        rng = np.random.default_rng(0)
        arrays = [x if x.size <= share else x.reshape(-1)[np.sort(rng.choice(x.size, share, replace=False))]
                  for x in arrays]
    os.makedirs(directory, exist_ok=True)
    for name, x in zip(OUTPUT_NAMES, arrays):
        np.save(os.path.join(directory, name + ".npy"), x)


def summary(ctx, res: dict) -> dict:
    a = ctx.a
    value = res["images"] / res["dt"]
    return {"value": round(value, 1), "ms_per_step": round(1e3 * res["dt"] / a.steps, 6),
            "global_batch": res["global_batch"], "per_gpu_batch": res["per_gpu_batch"],
            "parallelism": res["parallelism"]}


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parse(argv)
    if a.mode == "reference":
        a.backend, a.no_graphs, a.allreduce = "torch", True, "host"
    from cme213_sp18_amd.parallel.launcher import PlacementError, self_launch

    # --gpus N without a launcher: start the N ranks here (a child torch.distributed.run, before any GPU
    # call in this process) and pass their exit code through; rank 0 of the child job prints the record
    try:
        rc = self_launch(a.gpus, argv, script=os.path.abspath(__file__), need_gpus=a.backend == "hip")
    except PlacementError as ex:
        print(f"error: {ex}; no record", file=sys.stderr, flush=True)
        return 2
    if rc is not None:
        return rc

    from cme213_sp18_amd.parallel.launcher import init_distributed, shutdown, verify_placement

    comm, device = init_distributed()
    try:  # the job must be exactly --gpus ranks on --gpus distinct GPUs, or it measures nothing
        placement = verify_placement(comm, device, a.gpus)
    except PlacementError as ex:
        print(f"[rank {comm.rank}] error: {ex}; no record", file=sys.stderr, flush=True)
        shutdown()
        return 2
    ctx = Ctx(a, comm, device, placement)
    cost = None
    if ctx.R > 1 and a.backend == "hip":
        # the all-reduce policy's constants measured on this node (<= ~2 s) instead of the planning numbers
        from cme213_sp18_amd.parallel.trainer import measure_cost_model, set_cost_model

        cost = measure_cost_model(comm, device)
        set_cost_model(cost)
        if cost is not None and ctx.rank == 0:
            print(f"cost model measured on this node: {cost.as_record()}", file=sys.stderr, flush=True)
    res = measure(ctx, a.scaling)
    sec = None
    if ctx.R > 1 and a.full and a.secondary == "auto":
        other = "weak" if a.scaling == "strong" else "strong"
        # the secondary reuses the primary's choices (same bucket bytes; no second round of probes)
        sec = measure(ctx, other, parallel=res["parallel"], allreduce=res.get("allreduce_mode"))
    ok = res["ok"] and (sec is None or sec["ok"])
    if ctx.rank == 0:
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, res["outputs"], a.dtype)
        s = summary(ctx, res)
        rec = {
            "metric": METRIC,
            "value": s["value"],
            "unit": "images/s",
            "n_gpus": ctx.R,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": s["ms_per_step"],
            "higher_is_better": True,
            "scaling": a.scaling,
            "vs_baseline": (s["value"] / BASELINE_VALUE) if BASELINE_VALUE else None,
            "dtype": DTYPES[a.dtype],
            "data": DATA,
            "config": {"model": f"784-{a.hidden}-10 MLP", "global_batch": s["global_batch"], "seq_len": None,
                       "parallelism": s["parallelism"], "per_gpu_batch": s["per_gpu_batch"],
                       "backend": a.backend, "mode": a.mode, **res["config"], **res["checks"], **ctx.placement,
                       **({"cost_model_measured": cost.as_record()} if cost is not None else {})},
        }
        if sec is not None:
            ss = summary(ctx, sec)
            rec[sec["scaling"]] = {"value": ss["value"], "unit": "images/s", "ms_per_step": ss["ms_per_step"],
                                   "global_batch": ss["global_batch"], "per_gpu_batch": ss["per_gpu_batch"],
                                   "parallelism": ss["parallelism"], "allreduce": sec["config"].get("allreduce"),
                                   "allreduce_us": sec["config"].get("allreduce_us"),
                                   "note": f"secondary: {sec['scaling']} scaling ({'800 images per GPU' if sec['scaling'] == 'weak' else 'global batch split over the ranks'})",
                                   **({"invalid": sec["invalid"]} if not sec["ok"] else {})}
        if not res["ok"]:
            rec["invalid"] = res["invalid"]
        print(json.dumps(rec), flush=True)
    shutdown()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
