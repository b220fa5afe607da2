#!/usr/bin/env python3
"""What sampling with replacement costs (csrc/mlp/sample.h inside the four gather kernels) and what it buys.

For 784-100-10 and 784-4096-10 (the second carries the bf16 copies Xw / XTw), fp32 (split3), one GPU, a 60 000-sample
resident training set with 10 Zipf-like imbalanced classes:

  (a) the shuffle launch of this build WITHOUT a table against the same launch of another build of the library
      (--parent-lib: the parent commit's _hip extension), captured once in a HIP graph and replayed: microseconds per
      launch between two device synchronises.  The libraries are measured in alternated fresh processes
      (A B A B ...) that run nothing but this one launch, so that clocks, allocator state and neighbours hit both
      alike; the spread each side shows across its own processes is reported next to the difference of the medians;
  (b) the same launch of this build with a sampling.Balanced table;
  (c) the three augmenting gathers (Shift, Affine, Warp) without and with that table.

--recall: per-class recall of the five rarest classes of a synthetic imbalanced 62-class set on a balanced test set,
784-100-62 fp32, the same epochs, rate and seeds with and without sampling.Balanced.

One JSON line per measurement is appended to --out, and the table rows for docs/PERFORMANCE.md are printed at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [100, 4096]
N_TRAIN, CLASSES, SEED = 60000, 62, 1  # (CLASSES: of --recall; the cost runs use 10)


def zipf_labels(n: int, classes: int, seed: int):
    import numpy as np

    share = 1.0 / np.arange(1, classes + 1)
    counts = 1 + np.floor(share / share.sum() * (n - classes)).astype(np.int64)
    counts[0] += n - counts.sum()
    labels = np.repeat(np.arange(classes, dtype=np.int32), counts)
    np.random.default_rng(seed).shuffle(labels)
    return labels


def use_library(path: str) -> None:
    """Load another build of the _hip extension in this build's place (before anything asks for it)."""
    import importlib.util

    import torch  # noqa: F401  -- torch's HIP runtime first (shared SONAME)

    from cme213_sp18_amd import _native

    spec = importlib.util.spec_from_file_location("cme213_sp18_amd._hip", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _native._mods["_hip"] = mod


def worker(H: int, lib: str, reps: int, rounds: int, only_shuffle: bool) -> dict:
    if lib:
        use_library(lib)
    import numpy as np
    import torch

    from cme213_sp18_amd.augment import Affine, Shift, Warp
    from cme213_sp18_amd.parallel import MlpEngine
    from cme213_sp18_amd.sampling import Balanced

    x = np.random.default_rng(0).integers(0, 256, (N_TRAIN, 784)).astype(np.uint8)
    y = zipf_labels(N_TRAIN, 10, 0)
    e = MlpEngine((784, H, 10), dtype="f32", max_cols=800)
    e.load_dataset(x, y, keep_source=True)
    smp = Balanced(SEED)
    gathers = {"shuffle": None, "shift": Shift(2, seed=4), "affine": Affine(15.0, (0.9, 1.1), 5.0, 1, seed=4),
               "warp": Warp(3.0, 3, 10.0, (0.9, 1.1), 0.0, 1, seed=4)}
    cases = {"shuffle": ("shuffle", None)}
    if not only_shuffle:  # ((a): every library runs the one table-less shuffle launch and nothing else)
        e.prepare_sampler(smp)
        cases["shuffle_sampled"] = ("shuffle", smp)
        for k in ("shift", "affine", "warp"):
            e.prepare_augment(gathers[k])
            cases[k] = (k, None)
            cases[k + "_sampled"] = (k, smp)

    def enqueue(kind, sampler):
        if kind == "shuffle":
            e.enqueue_shuffle(SEED, 7, **({"sampler": sampler} if sampler is not None else {}))
        else:
            e.enqueue_augment(gathers[kind], 7, None if sampler is not None else SEED,
                              **({"sampler": sampler} if sampler is not None else {}))

    graphs = {}
    for name, (kind, sampler) in cases.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enqueue(kind, sampler)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            enqueue(kind, sampler)
        graphs[name] = g

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    for g in graphs.values():  # warm every timed shape
        timed(g.replay, reps)
    got = {k: [] for k in graphs}
    for r in range(rounds):
        for k in (list(graphs) if r % 2 == 0 else list(graphs)[::-1]):
            got[k].append(timed(graphs[k].replay, reps))
    return {"kind": "sampler_cost_worker", "library": lib or "this build", "layers": [784, H, 10],
            "layouts": sorted(n for n in ("X", "XT", "Xs", "Xw", "XTw") if getattr(e, n) is not None),
            "train_samples": N_TRAIN, "reps": reps, "rounds": rounds,
            **{k + "_us": round(statistics.median(v), 2) for k, v in got.items()},
            **{k + "_us_rounds": [round(u, 2) for u in v] for k, v in got.items()},
            "device": torch.cuda.get_device_name(0)}


def recall(epochs: int, lr: float, n_train: int, batch: int) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.sampling import Balanced
    from cme213_sp18_amd.utils.data import synthetic_mnist

    y = zipf_labels(n_train, CLASSES, 0)
    counts = np.bincount(y, minlength=CLASSES)
    pool_x, pool_y = synthetic_mnist(int(counts.max()) * CLASSES, seed=5, num_classes=CLASSES)
    x = np.empty((n_train, 784), np.uint8)
    for c in range(CLASSES):  # class c's rows: the first counts[c] of the pool's
        x[y == c] = pool_x[pool_y == c][:counts[c]]
    xt, yt = synthetic_mnist(100 * CLASSES, seed=6, num_classes=CLASSES)
    rare = np.argsort(counts, kind="stable")[:5]
    out = {"kind": "sampler_recall", "layers": [784, 100, CLASSES], "train_samples": n_train, "epochs": epochs,
           "lr": lr, "batch": batch, "rarest_classes": rare.tolist(), "rarest_counts": counts[rare].tolist(),
           "largest_count": int(counts.max())}
    for name, smp in (("plain", None), ("balanced", Balanced(SEED))):
        tr = DataParallelTrainer(NeuralNetwork([784, 100, CLASSES]), dtype="f32", batch_size=batch, normalize=True,
                                 sampler=smp, backend="hip" if torch.cuda.is_available() else "torch",
                                 **({} if torch.cuda.is_available() else {"device": "cpu", "use_graphs": False}))
        tr.load(x, y)
        tr.train(epochs, lr, 1e-4)
        pred = np.asarray(tr.engine.predict(xt))  # (raw pixels: the engine normalises as it did the training set)
        out[name + "_recall_rarest"] = [round(float((pred[yt == c] == c).mean()), 4) for c in rare]
        out[name + "_accuracy"] = round(float((pred == yt).mean()), 4)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/sampler/sampler_cost.jsonl")
    ap.add_argument("--parent-lib", default="", help="the other build's _hip extension (a .so file) for (a)")
    ap.add_argument("--other-lib", default="", help="a third build to alternate with in (a), e.g. a variant of this one")
    ap.add_argument("--pairs", type=int, default=4, help="alternated fresh processes per library")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--lr", type=float, default=0.5)
    ap.add_argument("--recall-samples", type=int, default=8000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)  # the hidden width of a worker process
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--only-shuffle", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        print("WORKER " + json.dumps(worker(a.worker, a.lib, a.reps, a.rounds, a.only_shuffle)), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
            recs.append(rec)

        if a.recall:
            emit(recall(a.epochs, a.lr, a.recall_samples, a.batch))
            return 0
        for H in a.hidden:
            def run_worker(lib, only_shuffle):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(H), "--lib", lib,
                                    "--reps", str(a.reps), "--rounds", str(a.rounds),
                                    *(["--only-shuffle"] if only_shuffle else [])],
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("WORKER ")][-1]
                return json.loads(line[7:])

            # (a): the same worker -- the table-less shuffle launch and nothing else -- for every library, alternated
            libs = [(n, p) for n, p in (("parent", a.parent_lib), ("other", a.other_lib)) if p] + [("this", "")]
            runs = {n: [] for n, _ in libs}
            for _ in range(a.pairs):
                for side, lib in libs:
                    runs[side].append(run_worker(lib, True)["shuffle_us"])
            # (b), (c): this build's eight launches in one process each, `pairs` fresh processes
            full = [run_worker("", False) for _ in range(a.pairs)]
            med = {k: round(statistics.median(w[k] for w in full), 2) for k in full[0] if k.endswith("_us")}
            rec = {"kind": "sampler_cost", "layers": full[0]["layers"], "layouts": full[0]["layouts"],
                   "train_samples": N_TRAIN, "pairs": a.pairs, "rounds": a.rounds, "reps": a.reps, **med,
                   "device": full[0]["device"]}
            for side, v in runs.items():
                rec[f"a_{side}_shuffle_us"] = round(statistics.median(v), 2)
                rec[f"a_{side}_shuffle_us_processes"] = v
                rec[f"a_{side}_spread_us"] = round(max(v) - min(v), 2)
            for side in runs:
                if side != "this":
                    rec[f"a_this_minus_{side}_us"] = round(rec["a_this_shuffle_us"] - rec[f"a_{side}_shuffle_us"], 2)
            emit(rec)
    print("| layers | (a) shuffle, parent (us) | (a) shuffle, this build (us) | spread parent / this (us) | "
          "(b) shuffle (us) | + table | (c) Shift (us) | + table | Affine (us) | + table | Warp (us) | + table |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r.get('a_parent_shuffle_us', '-')} | {r['a_this_shuffle_us']} | "
              f"{r.get('a_parent_spread_us', '-')} / {r['a_this_spread_us']} | {r['shuffle_us']} | "
              f"{r['shuffle_sampled_us']} | {r['shift_us']} | {r['shift_sampled_us']} | {r['affine_us']} | "
              f"{r['affine_sampled_us']} | {r['warp_us']} | {r['warp_sampled_us']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
