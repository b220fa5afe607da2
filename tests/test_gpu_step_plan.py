"""MlpStep.plan / plan_steps (csrc/mlp/mlp_step.hip): the one decision of how a step runs.

* The decision is the one the step took before it became a function: tests/fixtures/step_forms.json was dumped from the
  locals of the former run() / run_xstep() at their launch points (every field of every case below), and plan() /
  plan_steps() must reproduce it.  Marked gpu because the predicates read the CU count and the buffers' alignment; no
  step kernel is launched.
* Plan and execution agree: after a step, what it left behind is what its plan said, and two engines stepped the same
  way hold bitwise equal parameters (the apply path is deterministic)."""
import json
import os

import pytest
import torch

from cme213_sp18_amd.models.mlp import NeuralNetwork
from cme213_sp18_amd.parallel.engine import MlpEngine
from cme213_sp18_amd.utils.data import synthetic_mnist

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 1e-4
PATHS = (("f32", "split3"), ("bf16", "split1"))
SHAPES = ([(H, n) for H in (64, 100, 128) for n in (100, 104, 200, 256, 272, 400, 512, 784, 800, 960)]
          + [(300, 800)] + [(H, n) for H in (512, 1024) for n in (64, 800)] + [(3072, 1024), (4096, 800)])

with open(os.path.join(os.path.dirname(__file__), "fixtures", "step_forms.json")) as _f:
    _table = json.load(_f)
GOLDEN = {k: _table["forms"][i] for k, i in _table["cases"].items()}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _engine(H, n, dtype, path, store_a1=True):
    """max_cols = n, N = 2 n + 48 samples (a partial batch at the end), lazy planes on."""
    x, y = synthetic_mnist(2 * n + 48, seed=0)
    nn = NeuralNetwork([784, H, 10])
    e = MlpEngine(nn.H, dtype, max_cols=n, device="cuda", path=path)
    e.set_params(*nn.params)
    e.load_dataset(x, y)
    e.set_lazy_planes(True)
    e.set_store_a1(store_a1)
    return e


def _same(got, want, what):
    assert {k: got.get(k) for k in want} == want, what


@pytest.mark.parametrize("H,n", SHAPES)
def test_plan_is_the_recorded_decision(H, n):
    N = 2 * n + 48
    for dtype, path in PATHS:
        e = _engine(H, n, dtype, path)
        for a1 in (1, 0):
            e.set_store_a1(bool(a1))
            st = e._hip_step()
            for off in (0, 8):
                for sgd, parts in ((1, 3), (0, 1)):
                    key = f"run/H{H}/n{n}/{path}/a1_{a1}/off{off}/sgd{sgd}/parts{parts}"
                    _same(st.plan(off, n, sgd, parts), GOLDEN[key], key)
            for g0 in (0, 2, 8):
                key = f"steps/H{H}/n{n}/{path}/a1_{a1}/g{g0}"
                _same(st.plan_steps(g0, 3, n, 0, n, N), GOLDEN[key], key)
            assert st.xstep_used == 0 and st.dz_left_swz == 0  # (planning ran nothing)


@pytest.mark.parametrize("H,n,dtype,path,store_a1", [
    (64, 100, "f32", "split3", False),     # dZ1 planes; the pipeline's row-major form
    (64, 272, "f32", "split3", False),     # fragment-ordered dZ1
    (512, 64, "bf16", "split1", False),    # the 64-tile fused wide head
    (512, 64, "f32", "split3", False),
    (3072, 1024, "f32", "split3", True),   # the 128-tile fused head (its dW1 has too few tiles for the rega engine)
    (4096, 800, "f32", "split3", True),    # ... with dz_swz 2 and the W1 planes left stale (lazy planes)
])
def test_step_leaves_what_its_plan_says(H, n, dtype, path, store_a1):
    N = 2 * n + 48
    engines = [_engine(H, n, dtype, path, store_a1) for _ in range(2)]
    for e in engines:
        st = e._hip_step()
        st.refresh_planes(_stream())  # (a new step object assumes stale planes)
        plan = st.plan(0, n, 1, 3)
        st.run(0, n, 1.0 / n, REG, LR, 1, 0, _stream())
        assert st.dz_left_swz == plan["dz_swz"]
        assert st.planes_stale == bool(plan["planes_left_stale"])
        steps = st.plan_steps(0, 3, n, 0, n, N)
        st.run_steps(0, 3, n, 0, n, N, 1.0 / n, REG, LR, 1, _stream())
        assert st.xstep_used == steps["xstep"], st.xstep_reason
        assert st.xstep_reason == steps["why_not"]
        if steps["xstep"]:
            assert st.dz_left_swz == steps["dz_swz"]
    torch.cuda.synchronize()
    assert torch.equal(engines[0].params, engines[1].params)
    assert torch.isfinite(engines[0].params).all()
    for e in engines:
        assert not e.kernel_error()
