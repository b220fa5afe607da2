#!/usr/bin/env python3
"""Step time above 16 output classes (the many-class head and output-layer weight gradients, csrc/mlp/head_mc.hip).

Timing (default): for 784-100-C with C in {10, 26, 47, 62} and for 784-1024-47, fp32 (split3), batch 800, one GPU --
200 warm-up steps, then 2000 graph-replayed SGD steps between device synchronises, the configurations visited in
alternating order, three rounds.  One JSON line per configuration (us/step per round, median) appended to --out.
The C = 10 row is the existing 16-class path (here in its graph-replayed two-launch form), for context only.

Per-kernel split (a run of its own, the profiler slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o mc -- python3 bench/many_classes.py --trace 100,47
    python3 bench/many_classes.py --parse OUT --config 100,47 --out profiles/many_classes.jsonl

--trace H,C runs 20 + 50 eager steps of one configuration; --parse reads the kernel trace and appends, per kernel
that ran in every step, its launches per step and the median duration of its launches in the last 50 steps.
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

CONFIGS = [(100, 10), (100, 26), (100, 47), (100, 62), (1024, 47)]
BATCH, N = 800, 8000  # 10 full batches per replayed graph
LR, REG = 1e-3, 1e-4
TRACE_WARM, TRACE_STEPS = 20, 50


def make_trainer(H: int, C: int, graphs: bool):
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N, seed=1, num_classes=C)
    tr = DataParallelTrainer(NeuralNetwork([784, H, C]), dtype="f32", batch_size=BATCH, use_graphs=graphs,
                             executor="graph" if graphs else "eager")
    tr.load(x, y)
    return tr


def time_all(out: str, warmup: int, steps: int, rounds: int) -> None:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/many_classes.py needs a GPU")
    runs = []
    for H, C in CONFIGS:
        tr = make_trainer(H, C, graphs=True)
        plan = tr.epoch_plan()
        assert len(plan.steps) == N // BATCH and all(ln == BATCH for _, ln in plan.steps)
        tr.capture(plan, LR, REG)
        for _ in range(-(-warmup // len(plan.steps))):
            tr.run_plan(plan, LR, REG)
        torch.cuda.synchronize()
        runs.append({"H": H, "C": C, "tr": tr, "plan": plan, "us": []})
    reps = -(-steps // (N // BATCH))
    for r in range(rounds):
        for run in (runs if r % 2 == 0 else runs[::-1]):
            tr, plan = run["tr"], run["plan"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                tr.run_plan(plan, LR, REG)
            torch.cuda.synchronize()
            run["us"].append((time.perf_counter() - t0) * 1e6 / (reps * len(plan.steps)))
    with open(out, "a") as fh:
        for run in runs:
            p = run["tr"].engine.params
            rec = {"kind": "step_time", "layers": [784, run["H"], run["C"]], "dtype": "f32", "path": run["tr"].engine.path,
                   "batch": BATCH, "warmup_steps": warmup, "timed_steps": reps * (N // BATCH), "executor": "graph",
                   "us_per_step_rounds": [round(u, 3) for u in run["us"]],
                   "us_per_step_median": round(statistics.median(run["us"]), 3),
                   "finite": bool(torch.isfinite(p).all().item()), "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")


def trace_one(H: int, C: int) -> None:
    import torch

    tr = make_trainer(H, C, graphs=False)
    plan = tr.epoch_plan()
    for i in range(TRACE_WARM + TRACE_STEPS):
        s, ln = plan.steps[i % len(plan.steps)]
        tr.step(s, ln, LR, REG)
    torch.cuda.synchronize()


def parse(d: str, H: int, C: int, out: str) -> None:
    import csv
    import glob

    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    by_name: dict[str, list[int]] = {}
    for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
        by_name.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = TRACE_WARM + TRACE_STEPS
    kernels, step_us = [], 0.0
    for name, durs in by_name.items():
        if len(durs) < total or len(durs) % total:
            continue  # set-up kernels (dataset upload, parameter copies, plane splits)
        per = len(durs) // total
        med = statistics.median(durs[-per * TRACE_STEPS:]) / 1e3
        kernels.append({"kernel": name[:120], "launches_per_step": per, "median_us": round(med, 3)})
        step_us += per * med
    rec = {"kind": "kernel_split", "layers": [784, H, C], "dtype": "f32", "batch": BATCH, "executor": "eager",
           "steps": TRACE_STEPS, "kernels": kernels, "sum_of_kernel_medians_us": round(step_us, 3)}
    print(json.dumps(rec), flush=True)
    with open(out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/many_classes.jsonl")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", metavar="H,C", help="run one configuration's eager steps (under rocprofv3)")
    ap.add_argument("--parse", metavar="DIR", help="directory of a rocprofv3 run of --trace")
    ap.add_argument("--config", metavar="H,C", help="the configuration --parse DIR was traced for")
    a = ap.parse_args(argv)
    if a.trace:
        trace_one(*(int(v) for v in a.trace.split(",")))
    elif a.parse:
        if not a.config:
            ap.error("--parse needs --config H,C")
        parse(a.parse, *(int(v) for v in a.config.split(",")), a.out)
    else:
        time_all(a.out, a.warmup, a.steps, a.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
