"""Shared by tests/test_eval.py and tests/test_gpu_eval.py: the evaluation tests' inputs, their fp64 host oracle, the
comparison every one of them makes, and the worker of the gloo test (importable by spawn)."""
import functools
import json
import os

import numpy as np

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd.models.mlp import feedforward
from cme213_sp18_amd.utils.data import synthetic_mnist

# tests/test_gpu_few_classes.py TOL (a test module does not import another test module)
TOL = {("f64", "mfma"): 1e-11, ("f32", "split3"): 2e-5, ("f32", "mfma"): 2e-5, ("bf16", "split1"): 3e-2,
       ("bf16", "mfma"): 3e-2}
UNDECIDED_CAP = 0.02  # of n: samples whose fp64 top-2 margin is below 2 . bound


@functools.lru_cache(maxsize=None)
def eval_data(N, C, side=28, seed=3):
    """Raw-pixel samples and labels: synthetic_mnist(N, seed=3, num_classes=C, side=side)."""
    return synthetic_mnist(N, seed=seed, num_classes=C, side=side)


def eval_params(P, H, C):
    """The seeded W1 / b1 of the network and W2, b2 ~ N(0, 1) from default_rng(11): most classes get predicted, so the
    confusion matrix fills (at the initial W2 the oracle predicts one to five classes)."""
    nn = NeuralNetwork([P, H, C])
    g = np.random.default_rng(11)
    return nn.W[0].copy(), nn.b[0].copy(), g.normal(0.0, 1.0, (C, H)), g.normal(0.0, 1.0, C)


def head_oracle(a1, W2, b2, lab):
    """fp64 numpy: a1 [n][H] -> dict(z2 [n][C], pred (first maximum), nll [n], n, correct, loss_sum, confusion)."""
    a1, W2, b2 = (np.asarray(t, np.float64) for t in (a1, W2, b2))
    lab = np.asarray(lab, np.int64)
    n, C = a1.shape[0], W2.shape[0]
    z2 = a1 @ W2.T + b2.reshape(1, -1)
    m = z2.max(1)
    pred = z2.argmax(1)  # (numpy: the first maximum)
    nll = np.log(np.exp(z2 - m[:, None]).sum(1)) - (z2[np.arange(n), lab] - m)
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (lab, pred), 1)
    return dict(z2=z2, pred=pred, nll=nll, n=n, correct=int((pred == lab).sum()), loss_sum=float(nll.sum()),
                confusion=conf)


def oracle(x, lab, W1, b1, W2, b2, xscale=1.0):
    """The fp64 host oracle: models.mlp.feedforward for a1, then z2, nll and argmax in numpy."""
    W1, b1, W2, b2 = (np.asarray(t, np.float64) for t in (W1, b1, W2, b2))
    nn = NeuralNetwork([W1.shape[1], W1.shape[0], W2.shape[0]], init=False)
    nn.W[0][...], nn.b[0][...], nn.W[1][...], nn.b[1][...] = W1, b1, W2, b2
    a1 = feedforward(nn, np.asarray(x, np.float64) * xscale).a1
    return head_oracle(a1, W2, b2, lab)


def check_against_oracle(got, ref, lab, tol, tag=""):
    """got: dict(n, correct, loss_sum, confusion) of the code under test; ref: head_oracle's.  The assertions every
    evaluation test makes: n exact, the confusion row sums equal the label histogram, trace == correct, the mean loss
    within bound = tol . max|z2| of the oracle's, the L1 distance between the matrices <= 2 u, where u counts the
    samples whose fp64 top-2 z2 margin is below 2 . bound, and u <= 2 % of n."""
    n, C = ref["n"], ref["confusion"].shape[0]
    z2 = ref["z2"]
    bound = tol * float(np.abs(z2).max())
    if C > 1:
        top = np.sort(z2, axis=1)
        u = int(((top[:, -1] - top[:, -2]) < 2 * bound).sum())
    else:
        u = 0
    conf = np.asarray(got["confusion"], np.int64)
    l1 = int(np.abs(conf - ref["confusion"]).sum())
    dloss = abs(got["loss_sum"] / n - ref["loss_sum"] / n)
    print("NUMERICS " + json.dumps(dict(test=tag, n=n, C=C, bound=bound, undecided=u, l1=l1, mean_loss_err=dloss,
                                        mean_loss=ref["loss_sum"] / n, classes_predicted=int((conf.sum(0) > 0).sum()),
                                        accuracy=ref["correct"] / n)))
    assert got["n"] == n
    assert conf.shape == (C, C)
    np.testing.assert_array_equal(conf.sum(1), np.bincount(np.asarray(lab, np.int64), minlength=C))
    assert int(np.trace(conf)) == got["correct"]
    assert u <= UNDECIDED_CAP * n, (u, n)
    assert l1 <= 2 * u, (l1, u)
    assert dloss <= bound, (dloss, bound)


def eval_dp_worker(rank, world, comm, device, out_dir, H, C, N, Nval):
    """gloo data-parallel evaluate() and train(eval_every=1) on the torch backend; every rank saves its records."""
    import torch

    torch.set_num_threads(2)
    from cme213_sp18_amd.parallel import DataParallelTrainer

    x, y = eval_data(N, C)
    xv, yv = eval_data(Nval, C, 28, 5)
    nn = NeuralNetwork([784, H, C])
    W1, b1, W2, b2 = eval_params(784, H, C)
    nn.W[1][...], nn.b[1][...] = W2, b2
    tr = DataParallelTrainer(nn, comm=comm, device=device, dtype="f64", batch_size=800, backend="torch",
                             use_graphs=False)
    tr.load(x, y)
    tr.load_eval(xv, yv)
    r = tr.evaluate()
    st = tr.train(2, 0.001, 1e-4, eval_every=1)
    np.savez(os.path.join(out_dir, f"eval{rank}.npz"), n=r["n"], loss=r["loss"], accuracy=r["accuracy"],
             confusion=r["confusion"], shard=tr.engine.eval_samples,
             t_loss=np.array([e["loss"] for e in st.evals]), t_conf=np.stack([e["confusion"] for e in st.evals]),
             t_iter=np.array([e["iter"] for e in st.evals]))
