"""Evaluation of a resident validation set on the GPU (csrc/mlp/eval.hip, MlpStep::evaluate, MlpEngine.load_eval /
enqueue_eval / read_eval, DataParallelTrainer.train(eval_every)) against the fp64 host oracle of tests/eval_oracle.py.

bound = TOL[(dtype, path)] . max|z2| (the TOL table of tests/test_gpu_few_classes.py): the mean loss is within bound of
the oracle's, and the confusion matrices differ by at most 2 u in L1, u = the samples whose fp64 top-2 margin is below
2 . bound (u <= 2 % of n).  bf16 mode: the oracle takes the W1 the kernels multiply (the sum of the planes) and the f32
tolerance -- a1, W2, b2 and the head are fp32 there (csrc/mlp/mlp_kernels.h)."""
import json

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import hip
from cme213_sp18_amd.parallel import DataParallelTrainer, MlpEngine

from .eval_oracle import TOL, check_against_oracle, eval_data, eval_params, head_oracle, oracle

pytestmark = pytest.mark.gpu

DT = {"f32": (0, torch.float32), "f64": (1, torch.float64)}
SENTINEL = 12345
EPS64 = 2.0 ** -53


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _unpack(words, C):
    w = words.cpu()
    return dict(n=int(w[0]), correct=int(w[1]), loss_sum=float(w[2:3].view(torch.float64)[0]),
                confusion=w[3:3 + C * C].view(C, C).numpy().copy())


def _run_head(dt, a1, lda, W2, b2, lab, H, C, n):
    """mlp_eval_head alone into a sentinel-filled slot with guard words behind it."""
    words = 3 + C * C
    stats = torch.full((words + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    partials = torch.zeros(256, dtype=torch.float64, device="cuda")
    hip().mlp_eval_head(DT[dt][0], a1.data_ptr(), lda, W2.data_ptr(), b2.data_ptr(), lab.data_ptr(), H, C, n,
                        stats.data_ptr(), partials.data_ptr(), 1, _stream())
    torch.cuda.synchronize()
    assert (stats[words:] == SENTINEL).all()
    return _unpack(stats, C)


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("C", [2, 10, 16, 17, 32, 33, 48, 49, 64])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_eval_head_alone_matches_fp64(dt, C):
    """Class-tile edges (C), H % 4 != 0 and H % 16 != 0 (22), the n % 16 tail (37, 200); a1 past column n holds a
    sentinel that must not be read."""
    tdt = DT[dt][1]
    for H in (22, 100, 512):
        for n in (37, 200):
            g = np.random.default_rng((C, H, n, 1))
            lda = n + 11
            a1 = np.full((H, lda), 7.0)
            a1[:, :n] = g.uniform(0.05, 0.95, (H, n))
            W2, b2 = g.normal(0.0, 1.0, (C, H)), g.normal(0.0, 1.0, C)
            lab = g.integers(0, C, n).astype(np.int32)
            lab[0] = lab[n - 1] = C - 1
            dev = [torch.as_tensor(t).to(tdt).cuda().contiguous() for t in (a1, W2, b2)]
            got = _run_head(dt, dev[0], lda, dev[1], dev[2], torch.as_tensor(lab).cuda(), H, C, n)
            # the oracle on the operands the kernel holds (their values in the parameter dtype)
            ref = head_oracle(dev[0][:, :n].double().cpu().numpy().T, dev[1].double().cpu().numpy(),
                              dev[2].double().cpu().numpy(), lab)
            check_against_oracle(got, ref, lab, TOL[(dt, "mfma")], f"head {dt} C={C} H={H} n={n}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("C,tied",
                         [(10, (3, 4)), (33, (5, 21)), (64, (17, 50, 63)), (49, (0, 16, 32, 48)), (2, (0, 1))])
def test_first_maximum_wins_exact_ties(dt, C, tied):
    """a1 = 0: z2 = b2 exactly, so equal b2 entries tie -- within a lane's registers, across lane groups and across
    class tiles.  pred is the lowest tied class for every sample, and the matrix shows it."""
    tdt = DT[dt][1]
    H, n, lda = 20, 50, 64
    b2 = np.linspace(-1.0, 0.5, C)
    b2[list(tied)] = 0.75
    lab = (np.arange(n) * 3 % C).astype(np.int32)
    a1 = torch.zeros(H, lda, dtype=tdt, device="cuda")
    W2 = torch.as_tensor(np.random.default_rng(C).normal(0, 1, (C, H))).to(tdt).cuda()
    b2d = torch.as_tensor(b2).to(tdt).cuda()
    got = _run_head(dt, a1, lda, W2, b2d, torch.as_tensor(lab).cuda(), H, C, n)
    want = np.zeros((C, C), np.int64)
    np.add.at(want, (lab, np.full(n, min(tied))), 1)
    np.testing.assert_array_equal(got["confusion"], want)
    assert got["n"] == n and got["correct"] == int((lab == min(tied)).sum())
    b = b2d.double().cpu().numpy()
    nll = np.log(np.exp(b - b.max()).sum()) - (b[lab] - b.max())
    assert abs(got["loss_sum"] - nll.sum()) <= TOL[(dt, "mfma")] * np.abs(b).max() * n


# ------------------------------------------------------------------------------------------------ the engine
def _engine(dt, path, shape, chunk, slots=1, max_cols=256, train=None):
    P, H, C = shape
    e = MlpEngine(shape, dtype=dt, max_cols=max_cols, device="cuda", path=path)
    e.set_params(*eval_params(P, H, C))
    if train is not None:
        e.load_dataset(*train)
    e.load_eval(*eval_data(1000, C, int(round(P ** 0.5))), eval_chunk=chunk, eval_slots=slots)
    return e


def _engine_oracle(e, x, y):
    """The fp64 oracle on the weights the engine's kernels multiply: bf16 mode -> the sum of the W1 planes."""
    W1, b1, W2, b2 = e.get_params()
    if e.dtype == "bf16":
        W1 = e.W1p.double().sum(0).cpu().numpy() if e.np else e.W1g.double().cpu().numpy()
    return oracle(x, y, W1, b1, W2, b2, e.xscale)


ENGINE_CASES = [("f32", "split3", (784, 100, 10)), ("bf16", "split1", (784, 100, 10)), ("f64", "mfma", (784, 100, 10)),
                ("f32", "split3", (196, 64, 5)), ("f32", "split3", (784, 100, 47)), ("f32", "split3", (784, 512, 10))]


@pytest.mark.parametrize("dt,path,shape", ENGINE_CASES)
def test_engine_evaluate_matches_the_oracle_and_a_single_chunk(dt, path, shape):
    """1000 samples in chunks of 256 (four chunks, the last of 232 columns) against the oracle; a single-chunk run has
    bitwise the same counts, and its loss differs by fp64 association only: both sum the same 63 block partials, one
    in a chain of 63 adds, the other in four chains joined by 4 -- at most (62 + 66) roundings of 2^-53 . loss_sum."""
    C = shape[2]
    x, y = eval_data(1000, C, int(round(shape[0] ** 0.5)))
    e = _engine(dt, path, shape, 256)
    assert e.path == path
    got = e.evaluate()
    tol = TOL[("f32", "split3")] if dt == "bf16" else TOL[(dt, path)]
    check_against_oracle(got, _engine_oracle(e, x, y), y, tol, f"engine {dt} {path} {shape}")
    one = _engine(dt, path, shape, 1000).evaluate()
    l1 = int(np.abs(one["confusion"] - got["confusion"]).sum())
    print("NUMERICS " + json.dumps(dict(test="single chunk", shape=shape, dt=dt, loss4=got["loss_sum"],
                                        loss1=one["loss_sum"], l1=l1)))
    assert one["n"] == got["n"] == 1000 and one["correct"] == got["correct"]
    np.testing.assert_array_equal(one["confusion"], got["confusion"])
    assert abs(one["loss_sum"] - got["loss_sum"]) <= 128 * EPS64 * abs(got["loss_sum"])


def test_two_slots_and_a_fresh_engine_are_bitwise_equal():
    shape = (784, 100, 47)
    e = _engine("f32", "split3", shape, 256, slots=2)
    e.enqueue_eval(0)
    e.enqueue_eval(1)
    e.enqueue_eval(0)  # (re-enqueueing overwrites: not twice the counts)
    w = e.eval_words()
    assert int(w[0, 0]) == 1000 and torch.equal(w[0], w[1])
    f = _engine("f32", "split3", shape, 256)
    f.enqueue_eval(0)
    assert torch.equal(f.eval_words()[0], w[0])


@pytest.mark.parametrize("H,n", [(100, 256), (512, 256), (4096, 800)])
def test_evaluate_sees_the_weights_a_step_just_updated(H, n):
    """One training step updates W1 in place (at H = 4096 and 800 columns the wide update leaves the W1 planes stale:
    MlpStep.lazy_planes), then the evaluation: against the oracle on get_params(), and bitwise what the engine that
    refreshes the planes eagerly gives."""
    shape = (784, H, 10)
    x, y = eval_data(1000, 10)
    words = []
    for lazy in (True, False):
        e = _engine("f32", "split3", shape, 256, max_cols=n, train=eval_data(n, 10, 28, 7))
        e.set_lazy_planes(lazy)
        before = e.params.clone()
        e.run(0, n, 1.0 / n, 1e-4, 0.01, sgd=True)
        if lazy and H == 4096:
            assert e._hip_step().planes_stale
        got = e.evaluate()
        assert not torch.equal(before, e.params)
        check_against_oracle(got, _engine_oracle(e, x, y), y, TOL[("f32", "split3")], f"after a step H={H} lazy={lazy}")
        words.append(e.eval_words()[0])
        assert not e.kernel_error()
    assert torch.equal(words[0], words[1])


@pytest.mark.parametrize("H", [100, 512])
def test_captured_evaluation_replays_against_the_current_weights(H):
    n = 256
    e = _engine("f32", "split3", (784, H, 10), 256, slots=2, max_cols=n, train=eval_data(n, 10, 28, 7))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: lazy kernel loads
        e.enqueue_eval(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e.enqueue_eval(0)
    torch.cuda.synchronize()
    seen = []
    for k in range(2):
        g.replay()
        e.enqueue_eval(1)  # eager, the same weights
        w = e.eval_words()
        assert int(w[0, 0]) == 1000 and torch.equal(w[0], w[1]), k
        seen.append(w[0])
        e.run(0, n, 1.0 / n, 1e-4, 0.01, sgd=True)
    assert not torch.equal(seen[0], seen[1])  # (the step in between changed the weights, and the replay saw it)


# ------------------------------------------------------------------------------------------------ train(eval_every)
def _trainer():
    nn = NeuralNetwork([784, 100, 10])
    _, _, W2, b2 = eval_params(784, 100, 10)
    nn.W[1][...], nn.b[1][...] = W2, b2
    tr = DataParallelTrainer(nn, dtype="f32", batch_size=800)
    tr.load(*eval_data(1600, 10, 28, 7))
    tr.load_eval(*eval_data(500, 10))
    return tr


def test_train_eval_every_equals_twins_stopped_after_each_epoch():
    lr, reg = 0.001, 1e-4
    tr = _trainer()
    st = tr.train(3, lr, reg, eval_every=1)
    assert [(r["epoch"], r["iter"], r["n"]) for r in st.evals] == [(0, 2, 500), (1, 4, 500), (2, 6, 500)]
    for k, rec in enumerate(st.evals):
        twin = _trainer()
        twin.train(k + 1, lr, reg)
        want = twin.evaluate()
        assert rec["loss"] == want["loss"] and rec["accuracy"] == want["accuracy"], k
        np.testing.assert_array_equal(rec["confusion"], want["confusion"])
    plain = _trainer()
    assert plain.train(3, lr, reg).evals == []
    assert torch.equal(plain.engine.params, tr.engine.params)  # nothing existing changed
    x, y = eval_data(500, 10)
    got = tr.evaluate()
    ref = _engine_oracle(tr.engine, x, y)
    check_against_oracle(dict(n=got["n"], correct=int(np.trace(got["confusion"])), loss_sum=got["loss"] * got["n"],
                              confusion=got["confusion"]), ref, y, TOL[("f32", "split3")], "trained")
