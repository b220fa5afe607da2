#!/usr/bin/env python3
"""What a learning-rate schedule and gradient-norm clipping cost on the device (csrc/mlp/clip.hip, the extended apply
launch of csrc/mlp/optim.hip, MlpEngine.set_update_policy), graph-replayed like bench/optim_cost.py.

For 784-100-10 (79,510 parameters) and 784-4096-10 (3.2 M parameters), fp32 (split3), one GPU, every launch captured
`--chain` times in one HIP graph and replayed, microseconds per launch:

  (a) apply       the momentum and the Adam apply launch with no schedule and no clipping -- the code as it stood.  Run
                  with CME_PKG_ROOT pointing at a copy of the parent commit's package, the same script measures that
                  library (it then stops here): alternate the two in fresh processes and compare (a) across them; the
                  spread of the parent's own figures over the processes is the noise floor.
  (b) scheduled   the same launches with a schedule window: no launch is added.
  (c) clipped     the sum-of-squares launch alone, a device-to-device copy of the bytes it reads, and the whole clipped
                  update (sum of squares + apply with a schedule and a threshold that clips) against (a); and the
                  stateless kSgd rule that scheduled plain SGD runs.

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

# (CME_PKG_ROOT: a variant copy of the package -- here the parent commit's, for (a))
sys.path.insert(0, os.environ.get("CME_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [100, 4096]
BATCH, N_TRAIN = 800, 1600


def measure(H: int, rounds: int, reps: int, chain: int) -> dict:
    import torch

    import cme213_sp18_amd.optim as optim
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    extended = hasattr(optim, "Schedule")
    x, y = synthetic_mnist(N_TRAIN, seed=1)
    rules = {"momentum": optim.Optimizer.momentum(0.9, True), "adam": optim.Optimizer.adam()}

    def engine(opt, **kw):
        tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH, optimizer=opt,
                                 executor="graph", **kw)
        tr.load(x, y)
        e = tr.engine
        e.run(0, BATCH, 1.0 / BATCH, 1e-4, 0.0, sgd=False)  # a real gradient in the bucket
        torch.cuda.synchronize()
        return e

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

    keep, graphs = [], {}
    for k, o in rules.items():
        e = engine(o)
        keep.append(e)
        graphs[f"apply_{k}"] = chained(lambda e=e: e.apply(0.0))
    count = keep[0].layout.total
    read_bytes = 0
    if extended:
        sch = optim.Schedule.cosine(1000, 0.1, warmup=10)
        for k, o in rules.items():
            e = engine(o, schedule=sch)
            e.set_schedule_window(0, sch.factors(0, 200))
            keep.append(e)
            graphs[f"sched_{k}"] = chained(lambda e=e: e.apply(0.0))
        norm = float(keep[0].grads[:keep[0].status_index].double().norm())
        for k, o in list(rules.items()) + [("sgd", None)]:
            e = engine(o, schedule=sch, clip_norm=0.5 * norm)  # half the norm: every element is scaled
            keep.append(e)
            graphs[f"clipped_{k}"] = chained(lambda e=e: e.apply(0.0))
        e = keep[-1]
        segs = e.clip_segments()
        read_bytes = 4 * sum(s for _, s in segs)
        from cme213_sp18_amd._native import hip

        npart = int(hip().clip_grid(sum(s for _, s in segs)))
        graphs["sumsq"] = chained(lambda: hip().grad_sumsq(0, e.grads.data_ptr(), e.layout.total, segs,
                                                           e.clip_partials.data_ptr(), npart,
                                                           torch.cuda.current_stream().cuda_stream))
        src = torch.empty(read_bytes // 2, dtype=torch.uint8, device="cuda")  # (a copy reads and writes: half each)
        dst = torch.empty_like(src)
        graphs["copy_sumsq_bytes"] = chained(lambda: dst.copy_(src))

    def timed(fn, n, per=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (n * per)

    fns = {f"{k}_us": (lambda g=g: timed(g.replay, reps, chain)) for k, g in graphs.items()}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    rec = {"kind": "clip_cost", "library": "extended" if extended else "parent", "layers": [784, H, 10], "dtype": "f32",
           "parameters": count, "rounds": rounds, "reps": reps, "chain": chain, "sumsq_bytes_read": read_bytes,
           **{k + "_rounds": [round(u, 2) for u in v] for k, v in got.items()},
           **{k: round(u, 2) for k, u in med.items()}, "device": torch.cuda.get_device_name(0)}
    if extended:
        last = keep[-1].last_update()
        rec.update(clip_grid=npart, clipped_coef=round(last["clip_coef"], 4),
                   sumsq_GBps=round(read_bytes / med["sumsq_us"] / 1e3, 1),
                   copy_GBps=round(read_bytes / med["copy_sumsq_bytes_us"] / 1e3, 1),
                   **{f"sched_minus_apply_{k}_us": round(med[f"sched_{k}_us"] - med[f"apply_{k}_us"], 2) for k in rules},
                   **{f"clipped_minus_apply_{k}_us": round(med[f"clipped_{k}_us"] - med[f"apply_{k}_us"], 2)
                      for k in rules})
    return rec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/sched_clip/clip_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/clip_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.chain)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | library | apply: momentum / adam (us) | scheduled: momentum / adam (us) | sum of squares (us) | "
          "copy of its bytes (us) | clipped update: sgd / momentum / adam (us) |")
    print("|---|---|---|---|---|---|---|")
    for r in recs:
        g = lambda k: r.get(k, "-")  # noqa: E731
        print(f"| {'-'.join(map(str, r['layers']))} | {r['library']} | {g('apply_momentum_us')} / {g('apply_adam_us')} | "
              f"{g('sched_momentum_us')} / {g('sched_adam_us')} | {g('sumsq_us')} | {g('copy_sumsq_bytes_us')} | "
              f"{g('clipped_sgd_us')} / {g('clipped_momentum_us')} / {g('clipped_adam_us')} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
