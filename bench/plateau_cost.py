#!/usr/bin/env python3
"""What reducing the rate on a validation plateau costs on the device (csrc/mlp/plateau.hip, the scale word of the apply
launch in csrc/mlp/optim.hip).

For 784-100-10, fp32 (split3), one GPU, microseconds per launch, every launch chained `--chain` times in a HIP graph and
the graph replayed `--reps` times between two device synchronises:

  decide        (a) the decision launch alone (one workgroup of 64 threads; thread 0 reads the record and a stats slot,
                runs the rule and stores the record);
  pack          (b) the one-workgroup pack kernel of keep-best: what a launch that does next to nothing costs here;
  apply         (c) the apply launch (momentum) over the parameter arena WITHOUT the scale pointer: the parent commit's
                launch -- a null pointer takes the code path as it stood;
  apply_scale   (d) the same launch WITH the scale pointer: one more 8-byte load on thread 0 of every workgroup.

Every figure is taken `--rounds` times, the measurements alternating within one process, after a warm-up of each; the
median is reported with every round's value.  One JSON line is appended to --out and the table row for
docs/PERFORMANCE.md is printed at the end.
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

LR = 1e-3


def measure(H: int, rounds: int, reps: int, chain: int) -> dict:
    import numpy as np
    import torch

    from cme213_sp18_amd._native import cpu, hip
    from cme213_sp18_amd.models.mlp import NeuralNetwork
    from cme213_sp18_amd.optim import Optimizer, Plateau
    from cme213_sp18_amd.parallel.engine import MlpEngine

    rule = Plateau(factor=0.5, patience=2)
    opt = Optimizer("momentum", momentum=0.9)
    e = MlpEngine(NeuralNetwork([784, H, 10]).H, dtype="f32", max_cols=800, device="cuda", backend="hip")
    e.set_optimizer(opt)
    total = e.layout.total
    m = hip()
    rec = torch.from_numpy(cpu().plateau_start(0)).cuda()
    word = rec.data_ptr() + 8 * int(m.plateau_scale_word)
    slot = torch.zeros(3, dtype=torch.int64, device="cuda")
    slot[0], slot[1] = 8, 1
    slot.view(torch.float64)[2:3].fill_(16.0)
    rows = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    e.grads.normal_()
    e.grads[e.status_index:].zero_()
    last = torch.zeros(4, dtype=torch.float64, device="cuda")
    planes, np_ = (e.W1p, e.np) if e.np else (None, 0)

    def apply(ptr):
        def f():
            m.optim_apply(0, opt.code, *opt.hyper(LR), e.params.data_ptr(), e.grads.data_ptr(),
                          e.opt_bufs[0].data_ptr(), 0, total, planes.data_ptr() if planes is not None else 0, np_,
                          e.H * e.P if np_ else 0, e.grads[e.status_index:].data_ptr(), e.opt_rec.data_ptr(),
                          int(e.opt_rec.shape[0]), 0, 0, 0, 0, 0.0, last.data_ptr(),
                          torch.cuda.current_stream().cuda_stream, ptr)
        return f

    bodies = {
        "decide": lambda: m.mlp_plateau(*rule.native(), rec.data_ptr(), slot.data_ptr(), 0, 1,
                                        torch.cuda.current_stream().cuda_stream),
        "pack": lambda: m.mlp_best_pack(slot.data_ptr(), rows.data_ptr(), 2, 0,
                                        torch.cuda.current_stream().cuda_stream),
        "apply": apply(0),
        "apply_scale": apply(word),
    }
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
    torch.cuda.synchronize()
    # what is timed is what is claimed: a replay of the decision graph advances the record by `chain` decisions
    n0 = float(rec[0])
    graphs["decide"].replay()
    torch.cuda.synchronize()
    assert float(rec[0]) == n0 + chain and float(rec[4]) < 1.0, rec.tolist()

    def timed(fn, n, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / (n * per)

    fns = {k + "_us": (lambda g=g: timed(g.replay, reps, chain)) for k, g in graphs.items()}
    for f in fns.values():  # warm every timed shape
        f()
    got = {k: [] for k in fns}
    for r in range(rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            got[k].append(fns[k]())
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = (max(got["apply_us"]) - min(got["apply_us"])) / med["apply_us"]
    return {"kind": "plateau_cost", "layers": [784, H, 10], "dtype": "f32", "path": e.path, "optimizer": "momentum",
            "arena_elements": int(total), "apply_workgroups": int(e.opt_rec.shape[0]), "rounds": rounds, "reps": reps,
            "chain": chain, **{k + "_rounds": [round(u, 3) for u in v] for k, v in got.items()},
            **{k: round(u, 3) for k, u in med.items()},
            "decide_over_pack": round(med["decide_us"] / med["pack_us"], 3),
            "apply_scale_minus_apply_us": round(med["apply_scale_us"] - med["apply_us"], 3),
            "apply_scale_over_apply": round(med["apply_scale_us"] / med["apply_us"], 4),
            "apply_spread": round(spread, 4), "device": torch.cuda.get_device_name(0), "numpy": np.__version__}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/plateau/plateau_cost.jsonl")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--hidden", type=int, nargs="*", default=[100])
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench/plateau_cost.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    recs = []
    with open(a.out, "a") as fh:
        for H in a.hidden:
            rec = measure(H, a.rounds, a.reps, a.chain)
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            recs.append(rec)
    print("| layers | decision (us) | pack (us) | apply (us) | apply + scale (us) | difference (us) | ratio | "
          "spread of apply |")
    print("|---|---|---|---|---|---|---|---|")
    for r in recs:
        print(f"| {'-'.join(map(str, r['layers']))} | {r['decide_us']} | {r['pack_us']} | {r['apply_us']} | "
              f"{r['apply_scale_us']} | {r['apply_scale_minus_apply_us']} | {r['apply_scale_over_apply']} | "
              f"{r['apply_spread']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
