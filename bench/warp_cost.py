#!/usr/bin/env python3
"""What the per-epoch elastic distortion costs (csrc/mlp/warp.hip, MlpEngine.enqueue_augment with an augment.Warp)
next to the Affine launch and the Shift launch of the same build in the same run and next to an epoch, and what it
buys.  The method is bench/affine_cost.py's.

For 784-100-10 (X + XT + Xs) and 784-4096-10 (the bf16 copies Xw / XTw), fp32 (split3), batch 800, one GPU, a
60 000-sample resident training set:

  warp       the warping gather alone (Warp(4, 3) over Affine(15, (0.9, 1.1), 10, max_dx=2), shuffled order), captured
             once in a HIP graph and replayed (and enqueued eagerly): microseconds per launch between two device
             synchronises;
  affine     the Affine launch of the same map, measured the same way in the same process: the yardstick of the budget;
  shift      the Shift(2) launch, likewise; the three alternate;
  epoch      an epoch (the plan of 75 steps through plan_runner) alone and with each launch enqueued in front.

Every figure is taken `--rounds` times, the measurements alternating, after a warm-up of each; the median is reported
and every round is written.  One JSON line per configuration is appended to --out, and the table rows for
docs/PERFORMANCE.md are printed at the end.

--accuracy: one measured row instead -- synthetic_mnist, 784-100-10, trained without augmentation, with
Affine(15, (0.9, 1.1), max_dx=2) and with Warp(4, 3) over the same map (same seed, same order), evaluated on a held-out
set and on that set warped by apply_warp with lattices of the same alpha and grid.
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
LAUNCHES = ("warp", "affine", "shift")
MAP = dict(rotate=15, scale=(0.9, 1.1), shear=10, max_dx=2, seed=3)


def measure(H: int, rounds: int, reps: int, epoch_reps: int, alpha: float, grid: int) -> dict:
    import torch

    from cme213_sp18_amd.augment import (Shift, Warp, apply_warp, epoch_nodes, epoch_shifts, epoch_transforms)
    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    wrp = Warp(alpha, grid, **MAP)
    aff, shf = wrp.affine, Shift(2, seed=3)
    policy = {"warp": wrp, "affine": aff, "shift": shf}
    x, y = synthetic_mnist(N_TRAIN, seed=1)
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, shuffle_seed=SEED, augment=wrp)
    tr.load(x, y)
    e = tr.engine
    N = e.num_samples
    held = {n: getattr(e, n) for n in ("X", "XT", "Xs", "Xw", "XTw", "labels") if getattr(e, n) is not None}
    plan = tr.epoch_plan()
    run_plan = tr.plan_runner(plan, LR, REG)
    run_plan()
    torch.cuda.synchronize()
    # correctness of what is timed: the kernel's rows == the host's
    e.enqueue_augment(wrp, 7, SEED)
    torch.cuda.synchronize()
    perm = cpu().epoch_permutation(N, SEED, 7)
    want = apply_warp(x[perm], epoch_shifts(N, wrp, 7)[perm], wrp.table()[epoch_transforms(N, wrp, 7)[perm]],
                      epoch_nodes(N, wrp, 7)[perm], wrp, 28, 28)
    assert torch.equal(e.X.cpu(), torch.from_numpy(want)), "kernel and host disagree"
    del want
    e.enqueue_augment(aff, 7, SEED)  # (allocate nothing new: the shifts, the transforms and the table are held)
    e.enqueue_augment(shf, 7, SEED)
    torch.cuda.synchronize()

    def alone(fn):
        # each launch ALONE: after an affine augmentation the Shift gather also zeroes the transforms (a fill launch),
        # which a run of that policy alone never has -- the buffer is set aside for the call
        def run(key):
            kept = e._transforms
            if fn == "shift":
                e._transforms = None
            e.enqueue_augment(policy[fn], key, SEED)
            e._transforms = kept
        return run

    launch = {name: alone(name) for name in LAUNCHES}
    graphs = {}
    for name in LAUNCHES:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch[name](7)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            launch[name](7)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    keys = iter(range(1, 1 << 30))

    def epoch_with(name):
        def run():
            launch[name](next(keys))
            run_plan()
        return run

    fns = {"epoch_us": lambda: timed(run_plan, epoch_reps)}
    for name in LAUNCHES:
        fns[f"{name}_graph_us"] = lambda name=name: timed(graphs[name].replay, reps)
        fns[f"{name}_eager_us"] = lambda name=name: timed(lambda: launch[name](next(keys)), reps)
        fns[f"epoch_{name}_us"] = lambda name=name: timed(epoch_with(name), epoch_reps)
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    return {"kind": "warp_cost", "layers": [784, H, 10], "dtype": "f32", "path": e.path, "batch": BATCH,
            "train_samples": N, "layouts": sorted(held), "warp": wrp.to_meta(), "shift": shf.to_meta(),
            "rounds": rounds, "reps": reps, "epoch_reps": epoch_reps, "epoch_steps": len(plan.steps),
            **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            **{k: round(u, 2) for k, u in med.items()},
            "warp_over_affine": round(med["warp_graph_us"] / med["affine_graph_us"], 2),
            "warp_over_shift": round(med["warp_graph_us"] / med["shift_graph_us"], 2),
            "warp_over_epoch": round(med["warp_graph_us"] / med["epoch_us"], 3),
            "epoch_warp_minus_epoch_us": round(med["epoch_warp_us"] - med["epoch_us"], 2),
            "launches": {"warp": e.warp_launches, "affine": e.affine_launches, "shift": e.augment_launches},
            "device": torch.cuda.get_device_name(0)}


def accuracy(n_train: int, n_val: int, epochs: int, lr: float, alpha: float, grid: int) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd.augment import Affine, Warp, apply_warp, epoch_nodes
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.common import precision
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(n_train, seed=1)
    xv, yv = synthetic_mnist(n_val, seed=2)
    # the held-out set under elastic distortion alone: lattices of another seed, the identity map, no shift
    probe = Warp(alpha, grid, seed=77)
    ident = np.tile(np.array([65536, 0, 0, 65536], np.int32), (n_val, 1))
    xw = apply_warp(xv, np.zeros((n_val, 2), np.int32), ident, epoch_nodes(n_val, probe, 0), probe, 28, 28)
    rec = {"kind": "warp_accuracy", "layers": [784, 100, 10], "dtype": "f32", "batch": 100, "lr": lr, "reg": REG,
           "train_samples": n_train, "val_samples": n_val, "epochs": epochs, "normalize": True, "alpha": alpha,
           "grid": grid, "device": torch.cuda.get_device_name(0)}
    for name, aug in (("plain", None), ("affine", Affine(15, (0.9, 1.1), max_dx=2, seed=3)),
                      ("warp", Warp(alpha, grid, rotate=15, scale=(0.9, 1.1), max_dx=2, seed=3))):
        tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), dtype="f32", batch_size=100, shuffle_seed=SEED,
                                 augment=aug, normalize=True)
        tr.load(x, y)
        tr.train(epochs, lr, REG)
        torch.cuda.synchronize()
        rec[name + "_val_accuracy"] = round(float(precision(tr.predict(xv), yv)), 4)
        rec[name + "_val_warped_accuracy"] = round(float(precision(tr.predict(xw), yv)), 4)
        tr.engine.unshuffle()
        rec[name + "_train_accuracy"] = round(float(precision(tr.predict(x), y)), 4)
    return rec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default profiles/warp/warp_cost.jsonl (warp_accuracy.jsonl)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--epoch-reps", type=int, default=20)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    ap.add_argument("--alpha", type=float, default=4.0)
    ap.add_argument("--grid", type=int, default=3)
    ap.add_argument("--accuracy", action="store_true", help="the accuracy row instead of the timings")
    ap.add_argument("--acc-train", type=int, default=2000)
    ap.add_argument("--acc-val", type=int, default=10000)
    ap.add_argument("--acc-epochs", type=int, default=300)
    ap.add_argument("--acc-lr", type=float, default=0.1)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/warp_cost.py needs a GPU")
    out = a.out or ("profiles/warp/warp_accuracy.jsonl" if a.accuracy else "profiles/warp/warp_cost.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if a.accuracy:
        rec = accuracy(a.acc_train, a.acc_val, a.acc_epochs, a.acc_lr, a.alpha, a.grid)
        print(json.dumps(rec), flush=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
        return 0
    recs = []
    with open(out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.epoch_reps, a.alpha, a.grid)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | warp, graph (us) | affine, graph (us) | shift, graph (us) | warp / affine | warp / shift | "
          "warp, eager (us) | affine, eager (us) | epoch (us) | epoch + shift (us) | epoch + affine (us) | "
          "epoch + warp (us) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['warp_graph_us']} | {r['affine_graph_us']} | "
              f"{r['shift_graph_us']} | {r['warp_over_affine']} | {r['warp_over_shift']} | {r['warp_eager_us']} | "
              f"{r['affine_eager_us']} | {r['epoch_us']} | {r['epoch_shift_us']} | {r['epoch_affine_us']} | "
              f"{r['epoch_warp_us']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
