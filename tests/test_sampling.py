"""Sampling with replacement on the CPU (csrc/mlp/sample.h through _cpu.alias_table / _cpu.epoch_draws, the
sampling policies, the torch-backend engine and trainers, the fp64 oracle and the CLI).

The table is checked exactly: from the integer table alone every row's implied probability p[i] is formed with Python
integers (units of 2^-32 / N), and |p[i] - 2^32 N w[i] / sum(w)|, a rational, must lie within the bound that the
header derives.  Each case prints a NUMERICS line with its worst |error| / bound (pytest -s; the recorded lines are
profiles/sampler/table_error.jsonl: the worst absolute error is 16 units, at a row with 603 aliasing columns; the
ratio comes close to 1 only at rows that no column aliases to, whose whole error is their own threshold's rounding
of up to half a unit)."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cme213_sp18_amd import NeuralNetwork
from cme213_sp18_amd._native import cpu
from cme213_sp18_amd.augment import Shift, apply_shifts, epoch_shifts
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.optim import Optimizer, Schedule
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, MlpEngine, TensorParallelTrainer
from cme213_sp18_amd.parallel.launcher import spawn
from cme213_sp18_amd.sampling import Balanced, Weighted, from_meta
from cme213_sp18_amd.utils.data import synthetic_mnist
from tests import sampling_cases as sc
from tests.sampling_workers import dp_sampling_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, REG = 0.05, 1e-4


@pytest.mark.parametrize("N", [1, 2, 63, 1000, 60000])
@pytest.mark.parametrize("name", sc.SETS)
def test_table_implies_the_weights_within_the_derived_bound(name, N):
    case = sc.policy_of(name, N)
    if case is None:  # (no positive weight at this size: the refusal is tested below)
        with pytest.raises(ValueError):
            cpu().alias_table(np.zeros(N))
        return
    policy, labels = case
    w = policy.weights(labels)
    table = policy.table(labels)
    assert table.dtype == np.uint32 and table.shape == (N, 2) and int(table[:, 1].max()) < N
    assert np.array_equal(table, cpu().alias_table(w))  # a pure function of the weights
    p, a = sc.implied(table)
    assert sum(p) == N * sc.U
    W, S = sc.exact_weights(w)
    bnd = sc.bound(w, table, a)
    worst_ratio, worst_err = 0.0, 0.0
    for i in range(N):
        if W[i] == 0:
            assert p[i] == 0 and table[i, 0] == 0 and a[i] == 0, i  # never drawn, nobody's alias
        num = abs(p[i] * S - sc.U * N * W[i])  # |p[i] - U N w[i] / sum(w)| * S
        # (the bound floored to a multiple of 2^-40 unit: an integer comparison, never looser than the bound)
        assert num << 40 <= int(bnd[i] * 2.0 ** 40) * S, (i, num / S, bnd[i])
        worst_ratio, worst_err = max(worst_ratio, num / S / bnd[i]), max(worst_err, num / S)
    print("NUMERICS " + json.dumps({"case": name, "N": N, "worst_error_units": worst_err,
                                    "worst_error_over_bound": worst_ratio, "max_aliasing_columns": max(a)}))


def test_table_refuses_bad_weights():
    for bad in ([1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [0.0, 0.0], [], [1e308, 1e308]):
        with pytest.raises(ValueError):
            cpu().alias_table(np.asarray(bad, np.float64))
    with pytest.raises(ValueError):
        cpu().alias_table(np.ones((2, 2)))
    with pytest.raises(ValueError):
        Weighted(np.ones(5)).table(np.zeros(6, np.int32))  # len(w) != N
    with pytest.raises(ValueError):
        cpu().epoch_draws(3, 0, 0, cpu().alias_table(np.ones(4)))
    with pytest.raises(ValueError):
        Balanced(seed=1 << 32)
    # a column that always yields itself is stored as alias == own index
    assert np.array_equal(cpu().alias_table(np.ones(3))[:, 1], np.arange(3))


def test_policies_meta_and_checksum():
    labels = sc.zipf_labels(1000)
    b = Balanced(3)
    w = b.weights(labels)
    assert np.array_equal(w, 1.0 / np.bincount(labels)[labels])
    assert from_meta(json.loads(json.dumps(b.to_meta()))) == b and from_meta(None) is None
    wp = Weighted(w, 3)
    assert wp.checksum(labels) == b.checksum(labels) and 0 <= b.checksum(labels) < 1 << 64
    assert from_meta(json.loads(json.dumps(wp.to_meta())), weights=w) == wp
    assert Weighted(w * 2.0 + 1.0, 3).checksum(labels) != b.checksum(labels)
    with pytest.raises(ValueError):
        from_meta(wp.to_meta())  # (the record does not hold the weights)
    # equal policies hash alike; where the weights were read from is recorded and never compared
    assert hash(Balanced(3)) == hash(b) and len({b, Balanced(3), Balanced(4)}) == 2
    moved = Weighted(w.copy(), 3, source="elsewhere.npy")
    assert moved == wp and hash(moved) == hash(wp) and moved.to_meta()["source"] == "elsewhere.npy"
    assert Weighted(w, 4) != wp and Weighted(w * 2.0, 3) != wp and wp != b
    # a class absent from the data gets nothing: no row carries it
    gap = np.array([0, 0, 5, 5, 5, 9], np.int32)
    assert np.array_equal(Balanced().weights(gap), [1 / 2, 1 / 2, 1 / 3, 1 / 3, 1 / 3, 1.0])


@pytest.mark.parametrize("name,N", [("lognormal", 1000), ("seventh_zero", 63), ("zipf62_balanced", 200),
                                    ("one_nonzero", 65), ("uniform", 1)])
def test_epoch_draws_equal_the_python_restatement(name, N):
    policy, labels = sc.policy_of(name, N)
    table = policy.table(labels)
    for seed, it in ((0, 0), (9, 4), (2**32 - 1, 2**32 - 1)):
        got = cpu().epoch_draws(N, seed, it, table)
        assert got.dtype == np.int32
        key = sc.sample_key(seed, it)
        assert got.tolist() == [sc.draw(d, N, key, table) for d in range(N)]
        assert np.array_equal(got, cpu().epoch_draws(N, seed, it, table))
        assert policy.weights(labels)[got].min() > 0.0  # a zero-weight row is never drawn


def test_draws_are_keyed_and_a_stream_of_their_own():
    N = 1000
    policy, labels = sc.policy_of("uniform", N)
    table = policy.table(labels)
    base = cpu().epoch_draws(N, 5, 7, table)
    assert np.array_equal(base, Weighted(np.ones(N), 5).draws(labels, 7))
    assert (base != cpu().epoch_draws(N, 5, 8, table)).mean() > 0.9
    assert (base != cpu().epoch_draws(N, 6, 7, table)).mean() > 0.9
    assert (base != cpu().epoch_permutation(N, 5, 7)).mean() > 0.9
    assert len(np.unique(base)) < N  # with replacement: no permutation
    # the augmentation's hash of the same (seed, iter, index), used as a draw, gives other rows
    akey = sc.mix64(((5 << 32) ^ 7) ^ sc.AUGMENT_STREAM)
    as_aug = np.array([sc.draw(d, N, akey, table) for d in range(N)])
    assert sc.sample_key(5, 7) not in (akey, (5 << 32) ^ 7) and (base != as_aug).mean() > 0.9


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_balanced_draws_are_uniform_over_the_classes(seed):
    """Chi-square of the drawn class histogram against N / 62 below dof + 6 sqrt(2 dof): a cap a correct sampler
    exceeds with probability below about 1e-7 (measured: 51.3, 67.0, 47.9 at 61 degrees of freedom)."""
    N = 60000
    labels = sc.zipf_labels(N)
    hist = np.bincount(labels[Balanced(seed).draws(labels, 0)], minlength=62)
    chi2 = float(((hist - N / 62) ** 2 / (N / 62)).sum())
    print("NUMERICS " + json.dumps({"case": "balanced_chi2", "seed": seed, "chi2": chi2}))
    assert chi2 < 61 + 6 * np.sqrt(2 * 61)


# ------------------------------------------------------------------------------------------------ torch backend
def _trainer(sampler=None, H=16, B=64, cls=DataParallelTrainer, **kw):
    nn = NeuralNetwork([784, H, 10])
    if cls is DataParallelTrainer:
        kw.setdefault("use_graphs", False)
    return cls(nn, device="cpu", dtype="f64", batch_size=B, backend="torch", sampler=sampler, **kw)


def _twin_epochs(twin, x, y, sampler, epochs, lr=LR, reg=REG):
    """The reload-per-epoch twin: load the host-drawn set and train(1) per epoch, ``iter`` carried."""
    for _ in range(epochs):
        d = sampler.draws(y, twin.iter)
        twin.load(x[d], y[d])
        twin.train(1, lr, reg)


def _imbalanced(n, seed=3):
    x, _ = synthetic_mnist(n, seed=seed)
    y = np.sort(sc.zipf_labels(n, classes=10, seed=seed))
    return x, y.astype(np.int32)


@pytest.mark.parametrize("cls,kw", [
    (DataParallelTrainer, {}),
    (DataParallelTrainer, {"optimizer": "adam", "schedule": "cosine"}),
    (TensorParallelTrainer, {})])
def test_torch_trainer_equals_the_reload_per_epoch_twin(cls, kw):
    kw = dict(kw)
    if "optimizer" in kw:
        kw["optimizer"], kw["schedule"] = Optimizer.adam(), Schedule.cosine(3, 0.05)
    lr = 0.001 if kw else LR
    x, y = _imbalanced(200)
    smp = Balanced(4)
    tr = _trainer(smp, cls=cls, **kw)
    tr.load(x, y)
    assert tr.engine.X0 is not None and tr.engine._sampler is not None
    tr.train(3, lr, REG)
    twin = _trainer(None, cls=cls, **kw)
    _twin_epochs(twin, x, y, smp, 3, lr)
    assert tr.iter == twin.iter == 12
    assert torch.equal(tr.engine.params, twin.engine.params)
    last = smp.draws(y, 8)  # the set stays in the last epoch's state, and permutation() holds its draws
    assert np.array_equal(tr.engine.permutation().numpy(), last)
    assert torch.equal(tr.engine.X, torch.from_numpy(x[last]))
    assert np.array_equal(tr.engine.labels.numpy(), y[last])
    tr.engine.unshuffle()
    assert torch.equal(tr.engine.X, torch.from_numpy(x)) and np.array_equal(tr.engine.labels.numpy(), y)
    plain = _trainer(None, cls=cls, **kw)
    plain.load(x, y)
    plain.train(3, lr, REG)
    assert not torch.equal(plain.engine.params, tr.engine.params)
    assert plain.engine.X0 is None and plain.engine._sampler is None  # sampler=None: nothing kept


def test_train_2_plus_2_equals_train_4_and_the_per_step_path():
    x, y = _imbalanced(200)
    a, b = _trainer(Balanced(4)), _trainer(Balanced(4))
    for t in (a, b):
        t.load(x, y)
    a.train(4, LR, REG)
    b.train(2, LR, REG)
    b.train(2, LR, REG, print_every=3, log=lambda *_: None)  # the host-in-the-loop path samples too
    assert torch.equal(a.engine.params, b.engine.params)
    assert torch.equal(a.engine.permutation(), b.engine.permutation())


def test_sampler_with_a_shuffle_seed_raises():
    x, y = _imbalanced(100)
    for cls in (DataParallelTrainer, TensorParallelTrainer):
        with pytest.raises(ValueError):
            _trainer(Balanced(), cls=cls, shuffle_seed=3)
        t = _trainer(Balanced(), cls=cls)
        t.load(x, y)
        with pytest.raises(ValueError):
            t.train(1, LR, REG, shuffle_seed=3)
    with pytest.raises(ValueError):
        mlp.train(NeuralNetwork([784, 16, 10]), x, y, LR, REG, epochs=1, batch_size=64, shuffle_seed=3,
                  sampler=Balanced())
    with pytest.raises(TypeError):
        _trainer("balanced")
    e = MlpEngine((784, 16, 10), dtype="f64", device="cpu", backend="torch")
    e.load_dataset(x, y, keep_source=True)
    with pytest.raises(ValueError):
        e.enqueue_augment(Shift(2), 0, shuffle_seed=3, sampler=Balanced())
    with pytest.raises(ValueError):
        e.enqueue_shuffle(0, 0, sampler=Weighted(np.ones(99)))  # len(w) != N
    bare = MlpEngine((784, 16, 10), dtype="f64", device="cpu", backend="torch")
    bare.load_dataset(x, y)
    with pytest.raises(RuntimeError):
        bare.enqueue_shuffle(0, 0, sampler=Balanced())


def test_an_engine_serves_one_policy_per_load():
    x, y = _imbalanced(100)
    e = MlpEngine((784, 16, 10), dtype="f64", device="cpu", backend="torch")
    e.load_dataset(x, y, keep_source=True)
    e.enqueue_shuffle(0, 0, sampler=Balanced(1))
    table = e._sampler[2]
    e.enqueue_shuffle(0, 5, sampler=Balanced(1))  # an equal policy: the table stays where it is
    assert e._sampler[2] is table and np.array_equal(e.permutation().numpy(), Balanced(1).draws(y, 5))
    for other in (Balanced(2), Weighted(np.ones(100), 1)):
        with pytest.raises(RuntimeError):
            e.enqueue_shuffle(0, 0, sampler=other)
        with pytest.raises(RuntimeError):
            e.prepare_sampler(other)
    assert e._sampler[2] is table
    e.load_dataset(x, y, keep_source=True)  # a new load: a new policy
    e.enqueue_shuffle(0, 0, sampler=Balanced(2))
    assert np.array_equal(e.permutation().numpy(), Balanced(2).draws(y, 0))


def test_copies_of_one_row_get_their_own_shifts():
    """Every destination holds source row 7 (one non-zero weight): with the shifts keyed by the destination they differ
    from place to place, and the pixels are apply_shifts with the shifts indexed by destination."""
    N = 96
    x, y = _imbalanced(N)
    w = np.zeros(N)
    w[7] = 1.0
    smp, aug = Weighted(w, 2), Shift(2, seed=4)
    tr = _trainer(smp, augment=aug)
    tr.load(x, y)
    tr.train(1, LR, REG)
    e = tr.engine
    assert np.array_equal(e.permutation().numpy(), np.full(N, 7))
    sh = epoch_shifts(N, aug, 0)  # row d: the shift of destination d
    assert np.array_equal(e.shifts().numpy(), sh)
    assert len({tuple(s) for s in sh.tolist()}) > 10  # 25 possible shifts over 96 places
    assert torch.equal(e.X, torch.from_numpy(apply_shifts(x[np.full(N, 7)], sh, 28, 28)))
    assert not all(torch.equal(e.X[0], e.X[d]) for d in range(1, N))
    # without a sampler the shift belongs to the source row, as before
    plain = _trainer(None, augment=aug)
    plain.load(x, y)
    plain.train(1, LR, REG)
    assert torch.equal(plain.engine.X, torch.from_numpy(apply_shifts(x, sh, 28, 28)))


def test_sampled_oracle_matches_the_f64_trainer():
    """mlp.train(sampler=) against the f64 torch-backend trainer, at the bound tests/test_shuffle.py holds the shuffled
    oracle to for the same 6 steps: 1e-12 max-norm relative.  With a Shift on top as well."""
    H, N, B, E = 24, 2400, 800, 2
    x, y = _imbalanced(N, seed=11)
    for aug in (None, Shift(2, seed=4)):
        smp = Balanced(6)
        seq = NeuralNetwork([784, H, 10])
        mlp.train(seq, x, y, LR, REG, epochs=E, batch_size=B, sampler=smp, augment=aug)
        tr = _trainer(smp, H=H, B=B, augment=aug)
        tr.load(x, y)
        tr.train(E, LR, REG)
        for i in range(2):
            assert np.abs(tr.nn.W[i] - seq.W[i]).max() / np.abs(seq.W[i]).max() < 1e-12
            assert np.abs(tr.nn.b[i] - seq.b[i]).max() <= 1e-12 * max(1.0, np.abs(seq.b[i]).max())
    plain = NeuralNetwork([784, H, 10])
    mlp.train(plain, x, y, LR, REG, epochs=E, batch_size=B)
    assert np.abs(plain.W[0] - seq.W[0]).max() / np.abs(seq.W[0]).max() > 1e-6


def _loopback(world, cls, x, y, B, epochs, sampler, twin):
    comms = LoopbackComm.create(world)
    out = [None] * world

    def work(r):
        torch.set_num_threads(1)
        tr = _trainer(None if twin else sampler, H=24, B=B, cls=cls, comm=comms[r])
        if twin:
            _twin_epochs(tr, x, y, sampler, epochs)
        else:
            tr.load(x, y)
            tr.train(epochs, LR, REG)
        out[r] = (tr.engine.params.clone(), tr.engine.X.clone(), tr.engine.labels.clone())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
def test_loopback_ranks_with_uneven_shards_equal_their_twin(cls):
    """Three ranks, batches of 200 and a last one of 100: shards of 66 and 33 columns (the remainder is dropped, as
    in the reference).  Every rank holds the whole set and forms the same draws, and the run is bitwise the
    reload-per-epoch twin's, rank by rank."""
    x, y = _imbalanced(500, seed=11)
    smp = Balanced(6)
    got = _loopback(3, cls, x, y, 200, 2, smp, twin=False)
    want = _loopback(3, cls, x, y, 200, 2, smp, twin=True)
    last = smp.draws(y, 3)  # the second epoch starts at iteration counter 3
    for r in range(3):
        assert torch.equal(got[r][1], got[0][1]) and torch.equal(got[r][2], got[0][2])  # the same set on every rank
        assert np.array_equal(got[r][2].numpy(), y[last])
        assert torch.equal(got[r][0], want[r][0]), r
        if cls is DataParallelTrainer:
            assert torch.equal(got[r][0], got[0][0])  # replicas bitwise equal


def test_gloo_world2_sampled_equals_single_process(tmp_path):
    H, N, B, E, seed = 24, 2400, 800, 2, 6
    spawn(dp_sampling_worker, 2, args=(str(tmp_path), H, N, B, E, LR, REG, seed), backend="gloo")
    x, y = _imbalanced(N, seed=11)
    ref = _trainer(Balanced(seed), H=H, B=B)
    ref.load(x, y)
    st = ref.train(E, LR, REG)
    r0, r1 = (np.load(tmp_path / f"sampling{r}.npz") for r in range(2))
    np.testing.assert_array_equal(r0["perm"], Balanced(seed).draws(y, 3))
    for k, i in (("W0", 0), ("W1", 1)):
        np.testing.assert_array_equal(r0[k], r1[k])  # replicas stay bit-identical
        assert np.abs(r0[k] - ref.nn.W[i]).max() / np.abs(ref.nn.W[i]).max() < 1e-12
    for k, i in (("b0", 0), ("b1", 1)):
        np.testing.assert_array_equal(r0[k], r1[k])
        assert np.abs(r0[k] - ref.nn.b[i]).max() <= 1e-12 * max(1.0, np.abs(ref.nn.b[i]).max())
    assert int(r0["images"]) == st.images


# ----------------------------------------------------------------------------------------------------------- CLI
def _cli(tmp_path, *args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "cme213_sp18_amd.train", "--preset", "cpu_plumbing", "-n", "16", "-b",
                        "400", "--num-train", "1600", "--num-test", "100", "--outdir", str(tmp_path / "Outputs"),
                        *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_cli_balance_classes_checkpoint_and_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--balance-classes", "--sampler-seed", "3")
    _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "--log-json", str(tmp_path / "run.jsonl"))
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert meta["sampler"]["kind"] == "balanced" and meta["sampler"]["seed"] == 3
    assert len(meta["sampler"]["table_checksum"]) == 16 and meta["epochs"] == 4
    head = json.loads((tmp_path / "run.jsonl").read_text().splitlines()[0])
    assert head["event"] == "config" and head["sampler"] == {"kind": "balanced", "seed": 3}
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with sampler" not in r.stdout
    assert "sampling table has checksum" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])  # 2 of 4 epochs, resumed == the unbroken run
    plain = _cli(tmp_path, "-e", "1", "--resume", half, "--ckpt-dir", str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with sampler {'kind': 'balanced', 'seed': 3}" in plain.stdout
    assert "sampler" not in json.loads((tmp_path / "other" / "meta.json").read_text())
    # the same flags over another training split: the policy agrees, the table does not
    moved = _cli(tmp_path, *flags, "-e", "1", "--resume", half, "--seed", "77", "--ckpt-dir", str(tmp_path / "moved"))
    assert "warning: the checkpoint's sampling table has checksum" in moved.stdout


def test_cli_sample_weights_and_refusals(tmp_path):
    w = np.linspace(0.0, 1.0, 1440)  # (--num-train 1600: 1440 training samples and a dev split of 160)
    np.save(tmp_path / "w.npy", w)
    _cli(tmp_path, "--sample-weights", str(tmp_path / "w.npy"), "-e", "1", "--ckpt-dir", str(tmp_path / "ck"))
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["sampler"]["kind"] == "weighted" and meta["sampler"]["n"] == 1440
    assert meta["sampler"]["table_checksum"] == f"{Weighted(w).checksum(np.zeros(1440)):016x}"
    # the same weights file at another path is the same sampler: --resume does not warn
    np.save(tmp_path / "copy.npy", w)
    r = _cli(tmp_path, "--sample-weights", str(tmp_path / "copy.npy"), "-e", "1", "--resume", str(tmp_path / "ck"))
    assert "warning: the checkpoint was trained with sampler" not in r.stdout
    assert "sampling table has checksum" not in r.stdout
    r = _cli(tmp_path, "--balance-classes", "--shuffle-seed", "3", "-e", "1", ok=False)
    assert "not with --shuffle-seed" in r.stderr
    r = _cli(tmp_path, "--sampler-seed", "3", "-e", "1", ok=False)
    assert "--sampler-seed needs" in r.stderr
    np.save(tmp_path / "short.npy", np.ones(5))
    r = _cli(tmp_path, "--sample-weights", str(tmp_path / "short.npy"), "-e", "1", ok=False)
    assert "5 weights for 1440 training samples" in r.stdout + r.stderr
