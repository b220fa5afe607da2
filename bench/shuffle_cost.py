#!/usr/bin/env python3
"""What the per-epoch shuffle costs (csrc/mlp/shuffle.hip, MlpEngine.enqueue_shuffle) next to the alternatives and
next to an epoch.

For 784-100-10 and 784-4096-10 (the second carries the bf16 copies Xw / XTw), fp32 (split3), batch 800, one GPU, a
60 000-sample resident training set:

  shuffle    (a) the shuffle launch alone, captured once in a HIP graph and replayed (and enqueued eagerly):
             microseconds per launch between two device synchronises;
  copy       (b) in the same process, one device-to-device copy that moves the same number of bytes (a copy of T / 2
             bytes reads T / 2 and writes T / 2, T = the bytes the shuffle reads + writes): the bandwidth floor;
  torch      (c) the same rewrite of the same buffers in torch ops on the device: index_select with a device index,
             transpose, fragment_order_pixels and the bf16 casts;
  host       (d) the host route: DataParallelTrainer.load(x[perm], y[perm]) -- wall microseconds per call;
  epoch      (e) an epoch (the plan of 75 steps through plan_runner) without and with the shuffle enqueued in front.

Every figure is taken `--rounds` times, the measurements alternating, after a warm-up of each; the median is reported.
One JSON line per configuration is appended to --out, and the table rows for docs/PERFORMANCE.md are printed at the
end.
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
BATCH, N_TRAIN, SEED = 800, 60000, 1
LR, REG = 1e-3, 1e-4


def measure(H: int, rounds: int, reps: int, host_reps: int, epoch_reps: int) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.engine import fragment_order_pixels
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N_TRAIN, seed=1)
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, shuffle_seed=SEED)
    tr.load(x, y)
    e = tr.engine
    N, P = e.num_samples, e.P
    held = {n: getattr(e, n) for n in ("X", "XT", "Xs", "Xw", "XTw", "labels") if getattr(e, n) is not None}
    written = sum(t.numel() * t.element_size() for t in held.values()) + 4 * N  # + the order buffer
    if e.XT is not None:
        written -= N * e.XT.element_size()  # (the ones row is not touched)
    if e.XTw is not None:
        written -= N * e.XTw.element_size()
    read = e.X0.numel() * e.X0.element_size() + 4 * N
    traffic = read + written
    plan = tr.epoch_plan()
    run_plan = tr.plan_runner(plan, LR, REG)
    run_plan()
    torch.cuda.synchronize()
    # correctness of what is timed: the kernel's layouts == the torch formulation's
    perm_host = cpu().epoch_permutation(N, SEED, 7)
    idx = torch.from_numpy(perm_host).long().cuda()

    def torch_rewrite():
        e.X.copy_(e.X0.index_select(0, idx))
        e.labels.copy_(e.labels0.index_select(0, idx))
        e.XT[:P].copy_(e.X.t())
        if e.Xs is not None:
            e.Xs.copy_(fragment_order_pixels(e.X))
        if e.Xw is not None:
            e.Xw.copy_(e.X.to(torch.bfloat16))
            e.XTw[:P].copy_(e.XT[:P].to(torch.bfloat16))

    torch_rewrite()
    want = {n: t.clone() for n, t in held.items()}
    e.unshuffle()
    e.enqueue_shuffle(SEED, 7)
    torch.cuda.synchronize()
    assert all(torch.equal(held[n], want[n]) for n in held), "kernel and torch formulation disagree"
    del want
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e.enqueue_shuffle(SEED, 7)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.enqueue_shuffle(SEED, 7)
    src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def timed(fn, n, per=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (n * per)

    keys = iter(range(1, 1 << 30))

    def host_route():
        perm = cpu().epoch_permutation(N, SEED, next(keys))
        tr.load(x[perm], y[perm])

    def epoch_shuffled():
        e.enqueue_shuffle(SEED, next(keys))
        run_plan()

    fns = {"shuffle_graph_us": lambda: timed(graph.replay, reps),
           "shuffle_eager_us": lambda: timed(lambda: e.enqueue_shuffle(SEED, next(keys)), reps),
           "copy_same_bytes_us": lambda: timed(lambda: dst.copy_(src), reps),
           "torch_ops_us": lambda: timed(torch_rewrite, max(1, reps // 4)),
           "epoch_us": lambda: timed(run_plan, epoch_reps),
           "epoch_shuffled_us": lambda: timed(epoch_shuffled, epoch_reps)}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    # the host route last: load() replaces the buffers the graph and the runner were bound to
    got["host_load_us"] = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(host_reps):
            host_route()
        torch.cuda.synchronize()
        got["host_load_us"].append((time.perf_counter() - t0) * 1e6 / host_reps)
    med = {k: statistics.median(v) for k, v in got.items()}
    a = med["shuffle_graph_us"]
    return {"kind": "shuffle_cost", "layers": [784, H, 10], "dtype": "f32", "path": e.path, "batch": BATCH,
            "train_samples": N, "layouts": sorted(held), "bytes_read": read, "bytes_written": written,
            "rounds": rounds, "reps": reps, "host_reps": host_reps, "epoch_reps": epoch_reps,
            "epoch_steps": len(plan.steps),
            **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            **{k: round(u, 2) for k, u in med.items()},
            "shuffle_GBps": round(traffic / a / 1e3, 1), "copy_GBps": round(traffic / med["copy_same_bytes_us"] / 1e3, 1),
            "shuffle_over_copy": round(a / med["copy_same_bytes_us"], 2),
            "shuffle_over_torch": round(a / med["torch_ops_us"], 3),
            "shuffle_over_epoch": round(a / med["epoch_us"], 3),
            "epoch_shuffled_minus_epoch_us": round(med["epoch_shuffled_us"] - med["epoch_us"], 2),
            "host_over_epoch": round(med["host_load_us"] / med["epoch_us"], 1),
            "device": torch.cuda.get_device_name(0)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/shuffle/shuffle_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--epoch-reps", type=int, default=20)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/shuffle_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.host_reps, a.epoch_reps)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | shuffle, graph (us) | eager enqueue (us) | copy of the same bytes (us) | torch ops (us) | "
          "host load (us) | epoch (us) | epoch + shuffle (us) | (a)/(b) | (a)/(c) | (a)/(e) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['shuffle_graph_us']} | {r['shuffle_eager_us']} | "
              f"{r['copy_same_bytes_us']} | {r['torch_ops_us']} | {r['host_load_us']} | {r['epoch_us']} | "
              f"{r['epoch_shuffled_us']} | {r['shuffle_over_copy']} | {r['shuffle_over_torch']} | "
              f"{r['shuffle_over_epoch']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
