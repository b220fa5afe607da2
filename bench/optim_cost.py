#!/usr/bin/env python3
"""What a stateful optimizer costs (csrc/mlp/optim.hip, MlpEngine.apply, DataParallelTrainer(optimizer=...)): the price
of NOT fusing the update into the weight-gradient launch, for a later change to beat.

For 784-100-10 (79,510 parameters: one latency-bound launch) and 784-4096-10 (3.2 M parameters: a stream over 5 or 7
array passes), fp32 (split3), batch 800, one GPU, a 60 000-sample resident training set:

  launch   the momentum and the Adam launch against split_sgd on the same arena (the same engine: parameters, gradient
           bucket, planes), each captured `--chain` times in one HIP graph and replayed: microseconds per launch; and
           a device-to-device copy of as many bytes as the Adam launch moves, the bandwidth floor;
  step     an epoch (75 steps through plan_runner, graph-replayed) per step: the momentum and the Adam step, the
           gradient-mode plain-SGD step (allreduce="host" at world 1: weight gradients to the bucket, then split_sgd --
           the form the stateful step extends by nothing but its launch), and the fused step of the same build, as a
           graph and on the native loop.

Every figure is taken `--rounds` times, the measurements alternating in one process, after a warm-up of each; the median
is reported with the rounds.  One JSON line per configuration is appended to --out and the table rows for
docs/PERFORMANCE.md are printed at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [100, 4096]
BATCH, N_TRAIN = 800, 60000
LR, REG = 1e-3, 1e-4


def measure(H: int, rounds: int, reps: int, chain: int, epoch_reps: int) -> dict:
    import torch

    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.optim import Optimizer
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N_TRAIN, seed=1)
    opts = {"momentum": Optimizer.momentum(0.9, True), "adam": Optimizer.adam()}

    def trainer(**kw):
        tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, **kw)
        tr.load(x, y)
        return tr

    trs = {k: trainer(optimizer=o, executor="graph") for k, o in opts.items()}
    trs["sgd_gradient_mode"] = trainer(allreduce="host", executor="graph")
    trs["sgd_gradient_mode"].use_graphs = True  # (world 1: nothing is staged through the host, the step is capturable)
    trs["sgd_fused_graph"] = trainer(executor="graph")
    trs["sgd_fused_native"] = trainer(executor="auto")
    assert trs["sgd_fused_native"].native_plan(trs["sgd_fused_native"].epoch_plan()) is not None
    assert trs["momentum"].native_plan(trs["momentum"].epoch_plan()) is None
    plan = trs["adam"].epoch_plan()
    runners = {k: t.plan_runner(plan, LR, REG) for k, t in trs.items()}
    for r in runners.values():
        r()
    torch.cuda.synchronize()

    # ---- the launches alone, chained in one graph each, on the arenas of the stateful trainers' engines
    def chained(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(chain):
                fn()
        return g

    e_m, e_a = trs["momentum"].engine, trs["adam"].engine
    for e in (e_m, e_a):
        e.grads[e.status_index] = 0.0
    graphs = {"split_sgd": chained(lambda: e_a.sgd(0.0)), "momentum": chained(lambda: e_m.apply(0.0)),
              "adam": chained(lambda: e_a.apply(0.0))}
    count = e_a.layout.total
    w1n = e_a.H * e_a.P
    plane_bytes = 2 * e_a.np * w1n
    moved = {"split_sgd": 4 * 3 * count + plane_bytes, "momentum": 4 * 5 * count + plane_bytes,
             "adam": 4 * 7 * count + plane_bytes}
    src = torch.empty(moved["adam"] // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def timed(fn, n, per=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (n * per)

    fns = {f"launch_{k}_us": (lambda g=g: timed(g.replay, reps, chain)) for k, g in graphs.items()}
    fns["copy_adam_bytes_us"] = lambda: timed(lambda: dst.copy_(src), reps * 4)
    fns.update({f"step_{k}_us": (lambda r=r: timed(r, epoch_reps, len(plan.steps))) for k, r in runners.items()})
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    st = e_a.optim_state()  # (also checks that every workgroup's counter record agrees after all the replays)
    return {"kind": "optim_cost", "layers": [784, H, 10], "dtype": "f32", "path": e_a.path, "batch": BATCH,
            "parameters": count, "optim_grid": int(e_a.opt_rec.shape[0]), "adam_updates_applied": st["t"],
            "rounds": rounds, "reps": reps, "chain": chain, "epoch_reps": epoch_reps, "epoch_steps": len(plan.steps),
            "bytes_moved": moved,
            **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            **{k: round(u, 2) for k, u in med.items()},
            "launch_GBps": {k: round(moved[k] / med[f"launch_{k}_us"] / 1e3, 1) for k in graphs},
            "copy_GBps": round(moved["adam"] / med["copy_adam_bytes_us"] / 1e3, 1),
            "momentum_over_split_sgd": round(med["launch_momentum_us"] / med["launch_split_sgd_us"], 2),
            "adam_over_split_sgd": round(med["launch_adam_us"] / med["launch_split_sgd_us"], 2),
            "step_momentum_minus_gradient_mode_us": round(med["step_momentum_us"] - med["step_sgd_gradient_mode_us"], 2),
            "step_adam_minus_gradient_mode_us": round(med["step_adam_us"] - med["step_sgd_gradient_mode_us"], 2),
            "step_momentum_minus_fused_us": round(med["step_momentum_us"] - med["step_sgd_fused_graph_us"], 2),
            "step_adam_minus_fused_us": round(med["step_adam_us"] - med["step_sgd_fused_graph_us"], 2),
            "device": torch.cuda.get_device_name(0)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/optim/optim_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--epoch-reps", type=int, default=10)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/optim_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.chain, a.epoch_reps)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | split_sgd (us) | momentum (us) | adam (us) | copy of adam's bytes (us) | step: fused graph / native "
          "(us) | step: gradient mode + split_sgd (us) | step: momentum (us) | step: adam (us) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['launch_split_sgd_us']} | {r['launch_momentum_us']} | "
              f"{r['launch_adam_us']} | {r['copy_adam_bytes_us']} | {r['step_sgd_fused_graph_us']} / "
              f"{r['step_sgd_fused_native_us']} | {r['step_sgd_gradient_mode_us']} | {r['step_momentum_us']} | "
              f"{r['step_adam_us']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
