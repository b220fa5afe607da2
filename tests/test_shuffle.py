"""The per-epoch shuffle above the kernel: the keyed permutation (csrc/mlp/shuffle.h through _cpu.epoch_permutation),
the torch-backend engine and trainers, the shuffled fp64 oracle, two gloo ranks and the CLI's --shuffle-seed."""
import json
import math
import os
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.parallel import DataParallelTrainer, MlpEngine
from cme213_sp18_amd.parallel.launcher import spawn
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist

from .shuffle_workers import dp_shuffle_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 4099, 60000)


def perm_of(n, seed, key):
    return cpu().epoch_permutation(n, seed, key)


@pytest.mark.parametrize("n", SIZES)
def test_epoch_permutation_is_a_bijection(n):
    for seed in (0, 1, 12345, 2**32 - 1):
        for key in (0, 1, 75, 10**6, 2**32 - 1):
            p = perm_of(n, seed, key)
            assert p.dtype == np.int32 and p.shape == (n,)
            assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, key)
            assert np.array_equal(p, perm_of(n, seed, key))  # deterministic
            if n >= 16 and key + 1 < 2**32:
                assert not np.array_equal(p, perm_of(n, seed, key + 1)), (n, seed, key)
    if n >= 16:
        assert not np.array_equal(perm_of(n, 1, 0), perm_of(n, 2, 0))  # the seed matters too


def test_epoch_permutation_is_uniform_over_keys():
    """n = 64, keys 0..4095 at a fixed seed: where element 0 lands, and where position 0 draws from, against the
    uniform law -- chi-square under the 1 - 1e-6 quantile for 63 degrees of freedom (Wilson-Hilferty)."""
    n, keys, df = 64, 4096, 63
    z = NormalDist().inv_cdf(1 - 1e-6)
    bound = df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3
    lands, draws = np.zeros(n), np.zeros(n)
    for key in range(keys):
        p = perm_of(n, 7, key)
        draws[p[0]] += 1
        lands[int(np.flatnonzero(p == 0)[0])] += 1
    e = keys / n
    for name, cnt in (("element 0 lands", lands), ("position 0 draws", draws)):
        chi2 = float(((cnt - e) ** 2 / e).sum())
        print(f"{name}: chi2 = {chi2:.2f} (bound {bound:.2f})")
        assert chi2 < bound, (name, chi2, bound)


def _engine(x, y, dtype="f32", path="auto", keep=False, H=16):
    e = MlpEngine((x.shape[1], H, 10), dtype=dtype, max_cols=64, device="cpu", backend="torch", path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


@pytest.mark.parametrize("dtype,path", [("f32", "split3"), ("f64", "mfma")])
def test_torch_engine_shuffle_equals_a_fresh_load(dtype, path):
    x, y = synthetic_mnist(203, seed=2)
    e = _engine(x, y, dtype, path, keep=True)
    ptrs = [t.data_ptr() for t in (e.X, e.XT, e.labels)]
    assert np.array_equal(e.permutation().numpy(), np.arange(203))
    for key in (0, 9):  # the second is a fresh load of x[perm2]: not composed with the first
        e.enqueue_shuffle(5, key)
        perm = perm_of(203, 5, key)
        f = _engine(x[perm], y[perm], dtype, path)
        assert np.array_equal(e.permutation().numpy(), perm)
        for name in ("X", "XT", "labels"):
            assert torch.equal(getattr(e, name), getattr(f, name)), (name, key)
    e.unshuffle()
    f = _engine(x, y, dtype, path)
    for name in ("X", "XT", "labels"):
        assert torch.equal(getattr(e, name), getattr(f, name)), name
    assert np.array_equal(e.permutation().numpy(), np.arange(203))
    assert ptrs == [t.data_ptr() for t in (e.X, e.XT, e.labels)]  # rewritten in place


def test_engine_without_the_source_raises_and_keeps_nothing():
    x, y = synthetic_mnist(64, seed=2)
    e = _engine(x, y)
    assert e.X0 is None and e.labels0 is None and e.shuffle_launches == 0
    with pytest.raises(RuntimeError):
        e.enqueue_shuffle(1, 0)
    with pytest.raises(RuntimeError):
        e.unshuffle()
    assert np.array_equal(e.permutation().numpy(), np.arange(64))
    k = _engine(x, y, keep=True)
    with pytest.raises(ValueError):
        k.enqueue_shuffle(1, 2**32)


def _trainer(seed=None, H=16, B=64, dtype="f64", cls=DataParallelTrainer):
    nn = NeuralNetwork([784, H, 10])
    kw = dict(use_graphs=False) if cls is DataParallelTrainer else {}
    return cls(nn, device="cpu", dtype=dtype, batch_size=B, backend="torch", shuffle_seed=seed, **kw)


def _twin_epochs(twin, x, y, seed, epochs, lr, reg, **kw):
    """The reload-per-epoch twin: load(x[perm_e], y[perm_e]) and train(1) per epoch, ``iter`` carried."""
    out = []
    for _ in range(epochs):
        perm = perm_of(x.shape[0], seed, twin.iter)
        twin.load(x[perm], y[perm])
        out.append(twin.train(1, lr, reg, **kw))
    return out


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
def test_torch_trainer_equals_the_reload_per_epoch_twin(cls):
    x, y = synthetic_mnist(200, seed=3)  # batch 64: three full batches and a remainder of 8
    tr = _trainer(4, cls=cls)
    tr.load(x, y)
    assert tr.engine.X0 is not None
    tr.train(3, 0.05, 1e-4)
    twin = _trainer(None, cls=cls)
    _twin_epochs(twin, x, y, 4, 3, 0.05, 1e-4)
    assert tr.iter == twin.iter == 12
    assert torch.equal(tr.engine.params, twin.engine.params)
    last = perm_of(200, 4, 8)  # the set stays in the last epoch's order
    assert torch.equal(tr.engine.X, torch.from_numpy(x[last]))
    plain = _trainer(None, cls=cls)
    plain.load(x, y)
    plain.train(3, 0.05, 1e-4)
    assert not torch.equal(plain.engine.params, tr.engine.params)  # the order matters


def test_train_2_plus_2_equals_train_4_and_the_per_step_path():
    x, y = synthetic_mnist(200, seed=3)
    a, b, c = _trainer(4), _trainer(4), _trainer(None)
    for t in (a, b, c):
        t.load(x, y)
    a.train(4, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4, print_every=3, log=lambda *_: None)  # the host-in-the-loop path shuffles too
    assert torch.equal(a.engine.params, b.engine.params)
    assert c.engine.X0 is None  # shuffle_seed=None: no source copy
    with pytest.raises(RuntimeError):
        c.train(1, 0.05, 1e-4, shuffle_seed=4)


def test_shuffled_oracle_matches_the_f64_trainer():
    """mlp.train(shuffle_seed=s) against the f64 torch-backend trainer with the same seed, at the bound
    tests/test_dist.py holds the f64 engine to for the same 6 steps (2 epochs of 3 batches): 1e-12 max-norm relative."""
    H, N, B, E, lr, reg, seed = 24, 2400, 800, 2, 0.05, 1e-4, 6
    x, y = synthetic_mnist(N, seed=11)
    seq = NeuralNetwork([784, H, 10])
    mlp.train(seq, x, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed)
    tr = _trainer(seed, H=H, B=B)
    tr.load(x, y)
    tr.train(E, lr, reg)
    for i in range(2):
        assert np.abs(tr.nn.W[i] - seq.W[i]).max() / np.abs(seq.W[i]).max() < 1e-12
        assert np.abs(tr.nn.b[i] - seq.b[i]).max() <= 1e-12 * max(1.0, np.abs(seq.b[i]).max())
    plain = NeuralNetwork([784, H, 10])
    mlp.train(plain, x, y, lr, reg, epochs=E, batch_size=B)
    assert np.abs(plain.W[0] - seq.W[0]).max() / np.abs(seq.W[0]).max() > 1e-6


def test_gloo_world2_shuffled_equals_single_process(tmp_path):
    H, N, B, E, lr, reg, seed = 24, 2400, 800, 2, 0.05, 1e-4, 6
    spawn(dp_shuffle_worker, 2, args=(str(tmp_path), H, N, B, E, lr, reg, seed), backend="gloo")
    x, y = synthetic_mnist(N, seed=11)
    ref = _trainer(seed, H=H, B=B)
    ref.load(x, y)
    st = ref.train(E, lr, reg)
    r0, r1 = (np.load(tmp_path / f"shuffle{r}.npz") for r in range(2))
    np.testing.assert_array_equal(r0["perm"], perm_of(N, seed, 3))
    for k, i in (("W0", 0), ("W1", 1)):
        np.testing.assert_array_equal(r0[k], r1[k])  # replicas stay bit-identical
        assert np.abs(r0[k] - ref.nn.W[i]).max() / np.abs(ref.nn.W[i]).max() < 1e-12
    for k, i in (("b0", 0), ("b1", 1)):
        np.testing.assert_array_equal(r0[k], r1[k])
        assert np.abs(r0[k] - ref.nn.b[i]).max() <= 1e-12 * max(1.0, np.abs(ref.nn.b[i]).max())
    assert int(r0["images"]) == st.images


def _cli(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "1600", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_shuffle_seed_checkpoint_and_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    _cli(tmp_path, "--shuffle-seed", "3", "-e", "4", "--ckpt-dir", whole)
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert meta["shuffle_seed"] == 3 and meta["epochs"] == 4
    _cli(tmp_path, "--shuffle-seed", "3", "-e", "2", "--ckpt-dir", half)
    assert json.loads((tmp_path / "half" / "meta.json").read_text())["shuffle_seed"] == 3
    r = _cli(tmp_path, "--shuffle-seed", "3", "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with --shuffle-seed" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])  # 2 of 4 epochs, resumed == the unbroken run
    assert json.loads((tmp_path / "rest" / "meta.json").read_text())["iter"] == meta["iter"]
    plain = _cli(tmp_path, "-e", "1", "--resume", half, "--ckpt-dir", str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with --shuffle-seed 3, this run uses None" in plain.stdout
    assert json.loads((tmp_path / "other" / "meta.json").read_text())["shuffle_seed"] is None
