#!/usr/bin/env python3
"""What the per-epoch augmentation costs (csrc/mlp/augment.hip, MlpEngine.enqueue_augment) next to the shuffle launch
of the same build and next to an epoch, and what it buys.

For 784-100-10 (X + XT + Xs) and 784-4096-10 (the bf16 copies Xw / XTw), fp32 (split3), batch 800, one GPU, a
60 000-sample resident training set:

  augment    the augmenting gather alone (Shift(2), shuffled order), captured once in a HIP graph and replayed (and
             enqueued eagerly): microseconds per launch between two device synchronises;
  shuffle    the shuffle launch, measured the same way in the same process, the two alternating: the yardstick;
  epoch      an epoch (the plan of 75 steps through plan_runner) alone, with the shuffle and with the augmentation
             enqueued in front.

Every figure is taken `--rounds` times, the measurements alternating, after a warm-up of each; the median is reported.
One JSON line per configuration is appended to --out, and the table rows for docs/PERFORMANCE.md are printed at the
end.

--accuracy: one measured row instead -- synthetic_mnist, 784-100-10, trained without and with Shift(2) (same seed,
same order), evaluated on a held-out set and on that set translated by a further (+-2, +-2).
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


def measure(H: int, rounds: int, reps: int, epoch_reps: int) -> dict:
    import torch

    from cme213_sp18_amd.augment import Shift, apply_shifts, epoch_shifts
    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    aug = Shift(2, seed=3)
    x, y = synthetic_mnist(N_TRAIN, seed=1)
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, shuffle_seed=SEED, augment=aug)
    tr.load(x, y)
    e = tr.engine
    N = e.num_samples
    held = {n: getattr(e, n) for n in ("X", "XT", "Xs", "Xw", "XTw", "labels") if getattr(e, n) is not None}
    plan = tr.epoch_plan()
    run_plan = tr.plan_runner(plan, LR, REG)
    run_plan()
    torch.cuda.synchronize()
    # correctness of what is timed: the kernel's rows == the host's
    e.enqueue_augment(aug, 7, SEED)
    torch.cuda.synchronize()
    perm = cpu().epoch_permutation(N, SEED, 7)
    want = apply_shifts(x[perm], epoch_shifts(N, aug, 7)[perm], 28, 28)
    assert torch.equal(e.X.cpu(), torch.from_numpy(want)), "kernel and host disagree"
    del want

    def shuffle(key):
        # the shuffle launch ALONE: after an augmentation enqueue_shuffle also zeroes the shifts (a fill launch),
        # which a run that only shuffles never has -- the buffer is set aside for the call
        kept, e._shifts = e._shifts, None
        e.enqueue_shuffle(SEED, key)
        e._shifts = kept

    graphs = {}
    for name, fn in (("augment", lambda: e.enqueue_augment(aug, 7, SEED)), ("shuffle", lambda: shuffle(7))):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    keys = iter(range(1, 1 << 30))

    def epoch_shuffled():
        shuffle(next(keys))
        run_plan()

    def epoch_augmented():
        e.enqueue_augment(aug, next(keys), SEED)
        run_plan()

    fns = {"augment_graph_us": lambda: timed(graphs["augment"].replay, reps),
           "shuffle_graph_us": lambda: timed(graphs["shuffle"].replay, reps),
           "augment_eager_us": lambda: timed(lambda: e.enqueue_augment(aug, next(keys), SEED), reps),
           "shuffle_eager_us": lambda: timed(lambda: shuffle(next(keys)), reps),
           "epoch_us": lambda: timed(run_plan, epoch_reps),
           "epoch_shuffled_us": lambda: timed(epoch_shuffled, epoch_reps),
           "epoch_augmented_us": lambda: timed(epoch_augmented, epoch_reps)}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    return {"kind": "augment_cost", "layers": [784, H, 10], "dtype": "f32", "path": e.path, "batch": BATCH,
            "train_samples": N, "layouts": sorted(held), "augment": aug.to_meta(), "rounds": rounds, "reps": reps,
            "epoch_reps": epoch_reps, "epoch_steps": len(plan.steps),
            **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            **{k: round(u, 2) for k, u in med.items()},
            "augment_over_shuffle": round(med["augment_graph_us"] / med["shuffle_graph_us"], 2),
            "augment_over_epoch": round(med["augment_graph_us"] / med["epoch_us"], 3),
            "epoch_augmented_minus_epoch_us": round(med["epoch_augmented_us"] - med["epoch_us"], 2),
            "device": torch.cuda.get_device_name(0)}


def accuracy(n_train: int, n_val: int, epochs: int, lr: float) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd.augment import Shift, apply_shifts
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.common import precision
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(n_train, seed=1)
    xv, yv = synthetic_mnist(n_val, seed=2)
    rng = np.random.default_rng(0)
    moves = rng.choice(np.array([-2, 2], np.int32), size=(n_val, 2))
    xm = apply_shifts(xv, moves, 28, 28)
    rec = {"kind": "augment_accuracy", "layers": [784, 100, 10], "dtype": "f32", "batch": 100, "lr": lr, "reg": REG,
           "train_samples": n_train, "val_samples": n_val, "epochs": epochs, "normalize": True,
           "device": torch.cuda.get_device_name(0)}
    for name, aug in (("plain", None), ("shift2", Shift(2, seed=3))):
        tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), dtype="f32", batch_size=100, shuffle_seed=SEED,
                                 augment=aug, normalize=True)
        tr.load(x, y)
        tr.train(epochs, lr, REG)
        torch.cuda.synchronize()
        rec[name + "_val_accuracy"] = round(float(precision(tr.predict(xv), yv)), 4)
        rec[name + "_val_moved_accuracy"] = round(float(precision(tr.predict(xm), yv)), 4)
        tr.engine.unshuffle()
        rec[name + "_train_accuracy"] = round(float(precision(tr.predict(x), y)), 4)
    return rec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/augment/augment_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--epoch-reps", type=int, default=20)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    ap.add_argument("--accuracy", action="store_true", help="the accuracy row instead of the timings")
    ap.add_argument("--acc-train", type=int, default=2000)
    ap.add_argument("--acc-val", type=int, default=10000)
    ap.add_argument("--acc-epochs", type=int, default=300)
    ap.add_argument("--acc-lr", type=float, default=0.1)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/augment_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.accuracy:
        rec = accuracy(a.acc_train, a.acc_val, a.acc_epochs, a.acc_lr)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
        return 0
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.epoch_reps)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | augment, graph (us) | shuffle, graph (us) | augment / shuffle | augment, eager (us) | "
          "shuffle, eager (us) | epoch (us) | epoch + shuffle (us) | epoch + augment (us) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['augment_graph_us']} | {r['shuffle_graph_us']} | "
              f"{r['augment_over_shuffle']} | {r['augment_eager_us']} | {r['shuffle_eager_us']} | {r['epoch_us']} | "
              f"{r['epoch_shuffled_us']} | {r['epoch_augmented_us']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
