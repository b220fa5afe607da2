#!/usr/bin/env python3
"""What one validation pass costs next to a training epoch (csrc/mlp/eval.hip, MlpEngine.enqueue_eval).

For 784-100-10, 784-100-47 and 784-4096-10, fp32 (split3), batch 800, one GPU, a 10 000-sample validation set:

  resident   MlpEngine.enqueue_eval of the whole resident set, captured once in a HIP graph and replayed: microseconds
             per evaluation between two device synchronises (no host read inside the window);
  host       the only route without it, on the same process and data: DataParallelTrainer.predict(x) (upload, range
             check, labels back) + utils.common.precision on the host: wall microseconds per call;
  step       one training step (the epoch plan replayed between synchronises), and the epoch of 75 steps (60 000
             samples) it implies.

Every figure is taken `--rounds` times, the three measurements alternating, after a warm-up of each; the median is
reported.  One JSON line per configuration is appended to --out, and the table rows for docs/PERFORMANCE.md are
printed at the end.
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

CONFIGS = [(100, 10), (100, 47), (4096, 10)]
BATCH, N_TRAIN, N_VAL = 800, 8000, 10000
EPOCH_STEPS = 75  # 60 000 samples at batch 800
LR, REG = 1e-3, 1e-4


def measure(H: int, C: int, rounds: int, eval_reps: int, host_reps: int, step_reps: int) -> dict:
    import torch

    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.common import precision
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N_TRAIN, seed=1, num_classes=C)
    xv, yv = synthetic_mnist(N_VAL, seed=2, num_classes=C)
    tr = DataParallelTrainer(NeuralNetwork([784, H, C]), dtype="f32", batch_size=BATCH)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    e = tr.engine
    plan = tr.epoch_plan()
    run_plan = tr.plan_runner(plan, LR, REG)
    run_plan()
    torch.cuda.synchronize()
    # the evaluation as a graph: warm-up on a side stream, then one capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e.enqueue_eval(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.enqueue_eval(0)
    graph.replay()
    first = e.read_eval(0)
    acc_host = precision(tr.predict(xv), yv)
    # (two kernels sum z2 in different orders: a near-tie may fall the other way, nothing more)
    assert first["n"] == N_VAL and abs(first["correct"] / N_VAL - acc_host) <= 1e-3, (first["correct"], acc_host)

    def t_resident() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(eval_reps):
            graph.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / eval_reps

    def t_eager() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(eval_reps):
            e.enqueue_eval(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / eval_reps

    def t_host() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(host_reps):
            precision(tr.predict(xv), yv)
        return (time.perf_counter() - t0) * 1e6 / host_reps

    def t_step() -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(step_reps):
            run_plan()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (step_reps * len(plan.steps))

    fns = {"resident_graph_us": t_resident, "resident_eager_us": t_eager, "host_predict_us": t_host, "step_us": t_step}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    chunks = -(-N_VAL // min(e._eval["chunk"], e._eval["a1"].shape[1]))
    return {"kind": "eval_cost", "layers": [784, H, C], "dtype": "f32", "path": e.path, "batch": BATCH,
            "val_samples": N_VAL, "eval_chunks": chunks, "rounds": rounds,
            "eval_reps": eval_reps, "host_reps": host_reps, "timed_steps": step_reps * len(plan.steps),
            **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            **{k: round(u, 2) for k, u in med.items()},
            "epoch_us_75_steps": round(med["step_us"] * EPOCH_STEPS, 1),
            "resident_over_epoch": round(med["resident_graph_us"] / (med["step_us"] * EPOCH_STEPS), 3),
            "host_over_epoch": round(med["host_predict_us"] / (med["step_us"] * EPOCH_STEPS), 2),
            "accuracy": first["correct"] / first["n"], "device": torch.cuda.get_device_name(0)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/eval/eval_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eval-reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=100, help="replays of the 10-step epoch plan per timing")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/eval_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H, C in CONFIGS:
            rec = measure(H, C, a.rounds, a.eval_reps, a.host_reps, a.step_reps)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | resident evaluation, graph (us) | eager enqueue (us) | predict + precision on the host (us) "
          "| step (us) | epoch of 75 steps (us) | resident / epoch |")
    print("|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['resident_graph_us']} | {r['resident_eager_us']} | "
              f"{r['host_predict_us']} | {r['step_us']} | {r['epoch_us_75_steps']} | {r['resident_over_epoch']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
