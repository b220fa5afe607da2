#!/usr/bin/env python3
"""What keeping the best validation weights costs on the device (csrc/mlp/best.hip, MlpEngine.enqueue_keep_best) next
to a copy of the same bytes, an evaluation and an epoch.

For 784-100-10 and 784-4096-10, fp32 (split3), batch 800, one GPU, a 60 000-sample resident training set and a
10 000-sample resident validation set, microseconds per launch, every launch chained `--chain` times in a HIP graph
and the graph replayed `--reps` times between two device synchronises:

  not improved  (a) the decision launch when the evaluation does not improve on the best (the common case: every
                workgroup reads its record and the stats slot, advances the record and returns);
  improved      (b) the decision launch when every evaluation improves: the parameter arena is copied into the best
                arena.  The stats slot's loss is made smaller before every launch by one tiny in-place multiply in the
                same graph; (b) = the chain of {multiply, launch} minus the chain of the multiply alone;
  copy          (c) torch.Tensor.copy_ of the same bytes, device to device;
  pack          (d) the one-workgroup pack kernel: what a launch that does next to nothing costs here;
  eval          (e) one evaluation of the validation set (forward GEMM + evaluation head, chunk by chunk);
  epoch         (f) one epoch (the plan of 75 steps through plan_runner).

Every figure is taken `--rounds` times, the measurements alternating, after a warm-up of each; the median is reported
with every round's value.  One JSON line per configuration is appended to --out and the table rows for
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
BATCH, N_TRAIN, N_VAL = 800, 60000, 10000
LR, REG = 1e-3, 1e-4


def measure(H: int, rounds: int, reps: int, chain: int, epoch_reps: int) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd._native import hip
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.parallel.trainer import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N_TRAIN, seed=1)
    xv, yv = synthetic_mnist(N_VAL, seed=2)
    tr = DataParallelTrainer(NeuralNetwork([784, H, 10]), dtype="f32", batch_size=BATCH)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    e = tr.engine
    e.enable_keep_best("loss")
    b = e._best
    count, nrec = e.best_count, int(b["rec"].shape[0])
    nbytes = count * e.params.element_size()
    # a stats slot of our own: n = 8, correct = 1, loss_sum as fp64 bits in word 2
    slot = torch.zeros(3, dtype=torch.int64, device="cuda")
    loss = slot.view(torch.float64)[2:3]
    st = torch.cuda.current_stream().cuda_stream
    m = hip()

    def launch():
        m.mlp_keep_best(0, 0, 0.0, -1, e.params.data_ptr(), b["arena"].data_ptr(), count, b["rec"].data_ptr(), nrec,
                        slot.data_ptr(), 0, 1, st)

    def rearm():
        slot[0], slot[1] = 8, 1
        loss.fill_(1e6)
        e.reset_best()

    rows = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    src = torch.randn(count, dtype=e.params.dtype, device="cuda")
    dst = torch.empty_like(src)
    bodies = {"decide": launch, "shrink": lambda: loss.mul_(0.999),
              "shrink_decide": lambda: (loss.mul_(0.999), launch()),
              "copy": lambda: dst.copy_(src),
              "pack": lambda: m.mlp_best_pack(slot.data_ptr(), rows.data_ptr(), 2, 0, st)}
    rearm()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: lazy kernel loads
        st = torch.cuda.current_stream().cuda_stream
        for f in bodies.values():
            f()
        e.enqueue_eval(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs = {}
    for k, f in bodies.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            for _ in range(chain):
                f()
        graphs[k] = g
    geval = torch.cuda.CUDAGraph()
    with torch.cuda.graph(geval):
        e.enqueue_eval(0)
    st = torch.cuda.current_stream().cuda_stream
    run_plan = tr.plan_runner(tr.epoch_plan(), LR, REG)
    run_plan()
    torch.cuda.synchronize()

    # what is timed is what is claimed: after a re-arm the first launch improves and later ones (same slot) do not;
    # with the shrinking loss every launch improves and the best arena follows the parameters
    rearm()
    graphs["decide"].replay()
    torch.cuda.synchronize()
    s0 = e.best_state()
    assert s0["evals"] == chain and s0["best_index"] == 0 and s0["bad"] == chain - 1, s0
    rearm()
    graphs["shrink_decide"].replay()
    torch.cuda.synchronize()
    s1 = e.best_state()
    assert s1["evals"] == chain and s1["best_index"] == chain - 1 and s1["bad"] == 0, s1
    assert torch.equal(b["arena"], e.params[:count])

    def timed(fn, n, per=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (n * per)

    def not_improved():
        rearm()
        graphs["decide"].replay()  # (the first launch of the first replay improves; 1 of reps * chain)
        return timed(graphs["decide"].replay, reps, chain)

    def shrink_decide():
        rearm()
        t = timed(graphs["shrink_decide"].replay, reps, chain)
        s = e.best_state()  # (the loss never underflowed: every timed launch improved)
        assert s["evals"] == reps * chain and s["bad"] == 0 and s["best_index"] == s["evals"] - 1, s
        return t

    fns = {"not_improved_us": not_improved,
           "shrink_decide_us": shrink_decide,
           "shrink_us": lambda: timed(graphs["shrink"].replay, reps, chain),
           "copy_us": lambda: timed(graphs["copy"].replay, reps, chain),
           "pack_us": lambda: timed(graphs["pack"].replay, reps, chain),
           "eval_us": lambda: timed(geval.replay, reps),
           "epoch_us": lambda: timed(run_plan, epoch_reps)}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    got["improved_us"] = [a - s for a, s in zip(got["shrink_decide_us"], got["shrink_us"])]
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = (max(got["copy_us"]) - min(got["copy_us"])) / med["copy_us"]
    return {"kind": "keep_best_cost", "layers": [784, H, 10], "dtype": "f32", "path": e.path, "batch": BATCH,
            "train_samples": N_TRAIN, "val_samples": N_VAL, "parameters": count, "bytes_copied": nbytes,
            "workgroups": nrec, "rounds": rounds, "reps": reps, "chain": chain, "epoch_reps": epoch_reps,
            "epoch_steps": len(tr.epoch_plan().steps),
            **{k + "_rounds": [round(u, 3) for u in v] for k, v in got.items()},
            **{k: round(u, 3) for k, u in med.items()},
            "improved_GBps": round(2 * nbytes / med["improved_us"] / 1e3, 1),
            "copy_GBps": round(2 * nbytes / med["copy_us"] / 1e3, 1),
            "not_improved_over_pack": round(med["not_improved_us"] / med["pack_us"], 3),
            "improved_over_copy": round(med["improved_us"] / med["copy_us"], 3),
            "copy_spread": round(spread, 3),
            "not_improved_over_eval": round(med["not_improved_us"] / med["eval_us"], 4),
            "improved_over_eval": round(med["improved_us"] / med["eval_us"], 4),
            "improved_over_epoch": round(med["improved_us"] / med["epoch_us"], 5),
            "device": torch.cuda.get_device_name(0), "numpy": np.__version__}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/keep_best/keep_best_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--epoch-reps", type=int, default=10)
    ap.add_argument("--hidden", type=int, nargs="*", default=CONFIGS)
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/keep_best_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.chain, a.epoch_reps)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | parameters | not improved (us) | improved (us) | copy_ of the same bytes (us) | pack (us) | "
          "evaluation (us) | epoch (us) | (a)/(d) | (b)/(c) | spread of (c) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['parameters']} | {r['not_improved_us']} | {r['improved_us']} | "
              f"{r['copy_us']} | {r['pack_us']} | {r['eval_us']} | {r['epoch_us']} | {r['not_improved_over_pack']} | "
              f"{r['improved_over_copy']} | {r['copy_spread']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
