#!/usr/bin/env python3
"""What the weight average costs on the device (csrc/mlp/ema.hip, MlpEngine.ema_update).

launch   (default) for 784-100-10, 784-1024-10 and 784-4096-10, fp32, one GPU, microseconds per launch, every launch
         chained `--chain` times in a HIP graph and the graph replayed `--reps` times between two device synchronises:
           ema    the averaging launch over the parameter arena (reads params and the average, writes the average: 12 B
                  per fp32 element);
           copy   torch.Tensor.copy_ of the arena, device to device (8 B per element);
         each taken `--rounds` times, alternating, after a warm-up; medians and every round's value.
step     `--step ema | graph | auto`: the headline step (784-100-10 fp32, batch 800, 60 000 resident samples, plain SGD),
         microseconds per step over `--epochs` epochs through plan_runner, in THIS process only -- ema: the graph
         executor with the averaging launch behind every step; graph: the graph executor without it; auto: the default
         executor without it (the native pipeline).  graph and auto measure THIS tree with averaging off, whose path
         is the parent commit's; for the parent itself, time the same loop in a checkout of it.  Alternate the forms in
         fresh processes (measuring on a warm, shared device: interleave, never back to back in one process).
curve    `--curve`: validation loss per epoch with momentum 0.9 at lr 0.2, current against averaged weights
         (784-100-10 fp32, batch 800, the synthetic set: 60 000 training / 10 000 validation samples).

One JSON line per record is appended to --out; the table rows for docs/PERFORMANCE.md are printed at the end.
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

CONFIGS = [100, 1024, 4096]
BATCH, N_TRAIN, N_VAL = 800, 60000, 10000
LR, REG = 1e-3, 1e-4


def measure_launch(H: int, rounds: int, reps: int, chain: int) -> dict:
    import torch

    from cme213_sp18_amd.optim import Ema
    from cme213_sp18_amd.parallel.engine import MlpEngine

    e = MlpEngine((784, H, 10), "f32", max_cols=BATCH)
    g0 = torch.Generator(device="cuda").manual_seed(1)
    e.params[:e.layout.status].copy_(torch.randn(e.layout.status, device="cuda", generator=g0) * 0.01)
    e.set_ema(Ema(0.999, warmup=True))
    count = e.ema_count_elems
    nrec = int(e._ema["rec"].shape[0])
    src, dst = e.params[:count], torch.empty(count, dtype=e.params.dtype, device="cuda")
    bodies = {"ema": e.ema_update, "copy": lambda: dst.copy_(src)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: lazy kernel loads
        for f in bodies.values():
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs = {}
    for k, f in bodies.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(chain):
                f()
        graphs[k] = g
    # what is timed is what is claimed: one replay advances every record by `chain`
    t0 = e.ema_count()
    graphs["ema"].replay()
    torch.cuda.synchronize()
    assert e.ema_count() == t0 + chain and e.ema_state()["t"] == t0 + chain

    def timed(fn, n, per):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e6 / (n * per)

    fns = {k + "_us": (lambda g=g: timed(g.replay, reps, chain)) for k, g in graphs.items()}
    for f in fns.values():
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    esz = e.params.element_size()
    return {"kind": "ema_launch", "layers": [784, H, 10], "dtype": "f32", "parameters": count, "workgroups": nrec,
            "bytes_moved": 3 * esz * count, "rounds": rounds, "reps": reps, "chain": chain,
            **{k + "_rounds": [round(u, 3) for u in v] for k, v in got.items()},
            **{k: round(u, 3) for k, u in med.items()},
            "ema_GBps": round(3 * esz * count / med["ema_us"] / 1e3, 1),
            "copy_GBps": round(2 * esz * count / med["copy_us"] / 1e3, 1),
            "ema_over_copy": round(med["ema_us"] / med["copy_us"], 3),
            "copy_spread": round((max(got["copy_us"]) - min(got["copy_us"])) / med["copy_us"], 3),
            "device": torch.cuda.get_device_name(0)}


def _trainer(H, ema=None, executor="auto", optimizer=None):
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N_TRAIN, seed=1)
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, ema=ema, executor=executor,
                             optimizer=optimizer)
    tr.load(x, y)
    return tr


def measure_step(mode: str, epochs: int, rounds: int) -> dict:
    import torch

    from cme213_sp18_amd.optim import Ema

    tr = _trainer(100, Ema(0.999, warmup=True) if mode == "ema" else None, "auto" if mode == "auto" else "graph")
    plan = tr.epoch_plan()
    run = tr.plan_runner(plan, LR, REG)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    got = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(epochs):
            run()
        torch.cuda.synchronize()
        got.append((time.perf_counter() - t) * 1e6 / (epochs * len(plan.steps)))
    native = tr.native_plan(plan) is not None
    return {"kind": "ema_step", "mode": mode, "layers": [784, 100, 10], "dtype": "f32", "batch": BATCH,
            "steps_per_epoch": len(plan.steps), "epochs": epochs, "native_loop": native,
            "native_reason": tr.native_reason, "step_us_rounds": [round(u, 3) for u in got],
            "step_us": round(statistics.median(got), 3),
            "averaged_updates": tr.engine.ema_count() if mode == "ema" else None,
            "device": torch.cuda.get_device_name(0)}


def measure_curve(epochs: int) -> dict:
    from cme213_sp18_amd.optim import Ema, Optimizer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    xv, yv = synthetic_mnist(N_VAL, seed=2)
    out = {}
    for w in ("current", "ema"):
        tr = _trainer(100, Ema(0.999, warmup=True), "graph", Optimizer("momentum", momentum=0.9))
        tr.load_eval(xv, yv)
        st = tr.train(epochs, 0.2, REG, eval_every=1, eval_weights=w)
        out[w] = [round(e["loss"], 6) for e in st.evals]
        out[w + "_accuracy"] = [round(e["accuracy"], 4) for e in st.evals]
    return {"kind": "ema_curve", "layers": [784, 100, 10], "dtype": "f32", "batch": BATCH, "optimizer": "momentum 0.9",
            "lr": 0.2, "reg": REG, "decay": 0.999, "warmup": True, "epochs": epochs, **out}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/ema/ema_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    ap.add_argument("--step", choices=["ema", "graph", "auto"])
    ap.add_argument("--curve", action="store_true")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/ema_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        if a.step:
            recs.append(measure_step(a.step, a.epochs, a.rounds))
        elif a.curve:
            recs.append(measure_curve(a.epochs))
        else:
            recs += [measure_launch(H, a.rounds, a.reps, a.chain) for H in a.hidden]
        for rec in recs:
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
    if not a.step and not a.curve:
        print("| layers | parameters | workgroups | averaging launch (us) | copy_ of the arena (us) | launch GB/s (12 B "
              "per element) | copy GB/s (8 B) | launch / copy | spread of the copy |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in recs:
            print(f"| {'-'.join(map(str, r['layers']))} | {r['parameters']} | {r['workgroups']} | {r['ema_us']} | "
                  f"{r['copy_us']} | {r['ema_GBps']} | {r['copy_GBps']} | {r['ema_over_copy']} | {r['copy_spread']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
