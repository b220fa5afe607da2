#!/usr/bin/env python3
"""One form of the XCD-local step pipeline's dW1 pixel operand (MlpStep.xstep_pix), alone, for a counters-only
profiler pass (scripts/gpu_pmc_xstep_pix.sh): a 20-step plan to warm up, then ONE plan of --steps walking steps at
n = --cols, i.e. one kernel dispatch whose counters divide by --steps.

    python bench/xstep_pix_run.py --pix 1 [--cols 800] [--steps 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.environ.get("CME_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pix", type=int, default=0)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--cols", type=int, default=800)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args(argv)
    import torch

    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import MlpEngine
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(54000, seed=0)
    n = a.cols
    nn = NeuralNetwork([784, a.hidden, 10])
    e = MlpEngine(nn.H, dtype="f32", max_cols=n, device="cuda", path="split3")
    e.set_params(*nn.params)
    e.load_dataset(x, y)
    e.set_store_a1(False)
    st = e._hip_step()
    st.xstep, st.xstep_pix = 1, a.pix
    stream = torch.cuda.current_stream().cuda_stream
    for count, g0 in ((20, 0), (a.steps, 8 * n)):
        st.run_steps(g0, count, n, 0, n, e.num_samples, 1.0 / n, 1e-4, 1e-3, 1, stream)
        torch.cuda.synchronize()
    print(json.dumps({"n": n, "H": a.hidden, "pix": a.pix, "steps": a.steps, "xstep_used": int(st.xstep_used),
                      "kernel_error": bool(e.kernel_error())}))


if __name__ == "__main__":
    main()
