"""Random-shift augmentation above the kernel: the rule of csrc/mlp/augment.h through _cpu.epoch_shifts /
_cpu.augment_rows, the torch-backend engine and trainers, the augmented fp64 oracle, loopback and gloo ranks and the
CLI's --augment-shift."""
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
from cme213_sp18_amd.config import parse_config
from cme213_sp18_amd.models import mlp
from cme213_sp18_amd.parallel import DataParallelTrainer, LoopbackComm, MlpEngine
from cme213_sp18_amd.parallel.launcher import spawn
from cme213_sp18_amd.parallel.tensor_parallel import TensorParallelTrainer
from cme213_sp18_amd.utils.data import synthetic_mnist

from .augment_workers import dp_augment_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def perm_of(n, seed, key):
    return np.arange(n, dtype=np.int32) if seed is None else cpu().epoch_permutation(n, seed, key)


def shifted_numpy(x, shifts, h, w):
    """The restatement: out[i, y, x] = in[i, y - dy, x - dx], or 0 outside the image."""
    n = x.shape[0]
    src = x.reshape(n, h, w)
    out = np.zeros_like(src)
    for i, (dx, dy) in enumerate(shifts):
        ys = slice(max(0, dy), min(h, h + dy))
        xs = slice(max(0, dx), min(w, w + dx))
        out[i, ys, xs] = src[i, ys.start - dy:ys.stop - dy, xs.start - dx:xs.stop - dx]
    return out.reshape(n, h * w)


def augmented(x, y, aug, seed, key):
    """The host's epoch: (x[perm] shifted by shifts[perm], y[perm], perm, shifts[perm])."""
    n = x.shape[0]
    h, w = aug.shape(x.shape[1])
    perm = perm_of(n, seed, key)
    sh = epoch_shifts(n, aug, key)[perm]
    return apply_shifts(x[perm], sh, h, w), y[perm], perm, sh


@pytest.mark.parametrize("h,w", [(28, 28), (5, 6), (21, 37)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_augment_rows_equals_the_numpy_restatement(h, w, dtype):
    rng = np.random.default_rng(h * 100 + w)
    n = 40
    x = (rng.integers(1, 256, (n, h * w)).astype(dtype) if dtype is np.uint8 else rng.random((n, h * w)) + 0.5)
    # every corner of the range, zero, and random shifts in between
    sh = np.stack([rng.integers(-(w - 1), w, n), rng.integers(-(h - 1), h, n)], axis=1).astype(np.int32)
    sh[:5] = [(0, 0), (w - 1, h - 1), (-(w - 1), -(h - 1)), (w - 1, -(h - 1)), (-(w - 1), h - 1)]
    got = apply_shifts(x, sh, h, w)
    assert got.dtype == x.dtype and got.shape == x.shape
    assert np.array_equal(got, shifted_numpy(x, sh, h, w))
    assert np.array_equal(got[0], x[0])  # (0, 0) is the identity
    one = apply_shifts(x[:1], np.array([[1, 2]], np.int32) if h > 2 else np.array([[1, 0]], np.int32), h, w)
    img, src = one.reshape(h, w), x[:1].reshape(h, w)
    assert img[h - 1, w - 1] == src[h - 1 - (2 if h > 2 else 0), w - 2]  # positive dx: right, positive dy: down
    with pytest.raises(ValueError):
        apply_shifts(x, sh, h, w + 1)
    with pytest.raises(ValueError):
        apply_shifts(x, sh[:-1], h, w)


def test_augment_rows_float32():
    rng = np.random.default_rng(5)
    x = rng.random((9, 30)).astype(np.float32)
    sh = np.stack([rng.integers(-5, 6, 9), rng.integers(-4, 5, 9)], axis=1).astype(np.int32)
    got = apply_shifts(x, sh, 5, 6)
    assert got.dtype == np.float32 and np.array_equal(got, shifted_numpy(x, sh, 5, 6))


def test_epoch_shifts_are_uniform_and_differ_between_epochs():
    """100 000 samples over the 25 cells of Shift(2): each count within 6 binomial standard deviations of N / 25 --
    4000 +- 6 sqrt(N * (1/25) * (24/25)) = 4000 +- 372.  The hash is deterministic: a fixed fact, not a flaky bound."""
    n = 100000
    a = cpu().epoch_shifts(n, 7, 150, 2, 2)
    assert a.dtype == np.int32 and a.shape == (n, 2)
    assert a.min() == -2 and a.max() == 2
    cells = np.bincount((a[:, 0] + 2) * 5 + (a[:, 1] + 2), minlength=25)
    bound = 6 * np.sqrt(n * (1 / 25) * (24 / 25))
    print(f"cell counts {cells.min()} .. {cells.max()} (4000 +- {bound:.0f})")
    assert bound < 372.5 and np.all(np.abs(cells - n / 25) <= bound)
    b = cpu().epoch_shifts(n, 7, 225, 2, 2)
    differ = float(np.mean(np.any(a != b, axis=1)))
    print(f"two epochs differ for {differ:.4f} of the samples")
    assert differ > 0.90
    assert np.array_equal(a, cpu().epoch_shifts(n, 7, 150, 2, 2))  # deterministic
    assert np.array_equal(a[:1000], cpu().epoch_shifts(1000, 7, 150, 2, 2))  # by source index, whatever N
    assert not np.array_equal(a, cpu().epoch_shifts(n, 8, 150, 2, 2))  # the seed matters
    z = cpu().epoch_shifts(1000, 7, 150, 0, 3)
    assert np.all(z[:, 0] == 0) and z[:, 1].min() == -3 and z[:, 1].max() == 3
    assert np.array_equal(z[:, 1], cpu().epoch_shifts(1000, 7, 150, 5, 3)[:, 1])  # one half of the hash per axis


def test_shift_validates_and_round_trips():
    s = Shift(2, seed=4)
    assert (s.max_dx, s.max_dy, s.seed) == (2, 2, 4) and s.shape(784) == (28, 28)
    assert Shift.from_meta(s.to_meta()) == s and Shift.from_meta(None) is None
    assert Shift.from_meta(json.loads(json.dumps(Shift(3, 0, 21, 37, 9).to_meta()))) == Shift(3, 0, 21, 37, 9)
    assert Shift(1, height=5, width=6).shape(30) == (5, 6)
    assert s != Shift(2, seed=5)
    for bad in (lambda: Shift(-1), lambda: Shift(2, height=5), lambda: Shift(2, seed=2**32),
                lambda: Shift(6, height=5, width=6), lambda: s.shape(30), lambda: Shift(28).shape(784),
                lambda: Shift(1, height=5, width=6).shape(784)):
        with pytest.raises(ValueError):
            bad()


def _engine(x, y, dtype="f32", path="auto", keep=False, H=16):
    e = MlpEngine((x.shape[1], H, 10), dtype=dtype, max_cols=64, device="cpu", backend="torch", path=path)
    e.load_dataset(x, y, keep_source=keep)
    return e


@pytest.mark.parametrize("dtype,path", [("f32", "split3"), ("f64", "mfma"), ("bf16", "mfma")])
@pytest.mark.parametrize("seed", [None, 5])
def test_torch_engine_augment_equals_a_fresh_load(dtype, path, seed):
    x, y = synthetic_mnist(203, seed=2)
    aug = Shift(2, seed=4)
    e = _engine(x, y, dtype, path, keep=True)
    names = [n for n in ("X", "XT", "labels") if getattr(e, n) is not None]
    ptrs = [getattr(e, n).data_ptr() for n in names]
    assert not e.shifts().any() and e.shifts().shape == (203, 2) and e.shifts().dtype == torch.int32
    for key in (0, 9):  # the second is a fresh load of the second epoch's set: not composed with the first
        e.enqueue_augment(aug, key, seed)
        xa, ya, perm, sh = augmented(x, y, aug, seed, key)
        assert sh.any()
        f = _engine(xa, ya, dtype, path)
        assert np.array_equal(e.permutation().numpy(), perm) and np.array_equal(e.shifts().numpy(), sh)
        for name in names:
            assert torch.equal(getattr(e, name), getattr(f, name)), (name, key)
    e.unshuffle()
    f = _engine(x, y, dtype, path)
    for name in names:
        assert torch.equal(getattr(e, name), getattr(f, name)), name
    assert np.array_equal(e.permutation().numpy(), np.arange(203)) and not e.shifts().any()
    assert ptrs == [getattr(e, n).data_ptr() for n in names]  # rewritten in place
    assert e.augment_launches == 0 and e.shuffle_launches == 0  # (the kernels' counters: the hip backend's)


def test_engine_without_the_source_raises_and_keeps_nothing():
    x, y = synthetic_mnist(64, seed=2)
    e = _engine(x, y)
    assert e.X0 is None and e._shifts is None and e.augment_launches == 0
    with pytest.raises(RuntimeError):
        e.enqueue_augment(Shift(2), 0)
    assert not e.shifts().any()
    k = _engine(x, y, keep=True)
    assert k._shifts is None  # nothing allocated before the first augmentation
    with pytest.raises(ValueError):
        k.enqueue_augment(Shift(2), 2**32)
    with pytest.raises(ValueError):
        k.enqueue_augment(Shift(2, height=5, width=6), 0)
    k.enqueue_augment(Shift(2), 3)
    assert k.shifts().any()
    k.enqueue_shuffle(1, 3)  # the plain gather restores the loaded pixels
    assert not k.shifts().any() and torch.equal(k.X, torch.from_numpy(x[perm_of(64, 1, 3)]))


def _trainer(seed=None, aug=None, H=16, B=64, dtype="f64", cls=DataParallelTrainer, comm=None):
    nn = NeuralNetwork([784, H, 10])
    kw = dict(use_graphs=False) if cls is DataParallelTrainer else {}
    if comm is not None:
        kw["comm"] = comm
    return cls(nn, device="cpu", dtype=dtype, batch_size=B, backend="torch", shuffle_seed=seed, augment=aug, **kw)


def _twin_epochs(twin, x, y, aug, seed, epochs, lr, reg):
    """The reload-per-epoch twin: load the host's augmented epoch and train(1), ``iter`` carried."""
    for _ in range(epochs):
        xa, ya, _, _ = augmented(x, y, aug, seed, twin.iter)
        twin.load(xa, ya)
        twin.train(1, lr, reg)


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
@pytest.mark.parametrize("seed", [None, 6])
def test_torch_trainer_equals_the_reload_per_epoch_twin(cls, seed):
    x, y = synthetic_mnist(200, seed=3)  # batch 64: three full batches and a remainder of 8
    aug = Shift(2, seed=4)
    tr = _trainer(seed, aug, cls=cls)
    tr.load(x, y)
    assert tr.engine.X0 is not None
    tr.train(3, 0.05, 1e-4)
    twin = _trainer(None, None, cls=cls)
    _twin_epochs(twin, x, y, aug, seed, 3, 0.05, 1e-4)
    assert tr.iter == twin.iter == 12
    assert torch.equal(tr.engine.params, twin.engine.params)
    xa, _, perm, sh = augmented(x, y, aug, seed, 8)  # the set stays in the last epoch's state
    assert torch.equal(tr.engine.X, torch.from_numpy(xa).to(tr.engine.X.dtype))
    assert np.array_equal(tr.engine.permutation().numpy(), perm) and np.array_equal(tr.engine.shifts().numpy(), sh)
    plain = _trainer(seed, None, cls=cls)
    plain.load(x, y)
    plain.train(3, 0.05, 1e-4)
    assert not torch.equal(plain.engine.params, tr.engine.params)  # the shifts matter
    assert np.array_equal(tr.predict(x[:50]), twin.predict(x[:50]))  # predict() is never augmented


def test_train_2_plus_2_equals_train_4_and_the_per_step_path():
    x, y = synthetic_mnist(200, seed=3)
    aug = Shift(2, seed=4)
    a, b, c = _trainer(6, aug), _trainer(6, aug), _trainer(None, None)
    for t in (a, b, c):
        t.load(x, y)
    a.train(4, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4)
    b.train(2, 0.05, 1e-4, print_every=3, log=lambda *_: None)  # the host-in-the-loop path augments too
    assert torch.equal(a.engine.params, b.engine.params)
    assert c.engine.X0 is None and c.engine._shifts is None and c.engine.augment_launches == 0  # augment=None
    with pytest.raises(ValueError):
        _trainer(None, Shift(2, height=5, width=6)).load(x, y)  # validated against the engine's P at load()


@pytest.mark.parametrize("seed", [None, 6])
def test_augmented_oracle_equals_the_manual_per_epoch_loop(seed):
    H, N, B, E, lr, reg = 24, 600, 200, 2, 0.05, 1e-4
    x, y = synthetic_mnist(N, seed=11)
    aug = Shift(2, 1, seed=3)
    seq = NeuralNetwork([784, H, 10])
    mlp.train(seq, x, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed, augment=aug)
    man = NeuralNetwork([784, H, 10])
    it = 0
    for _ in range(E):
        xa, ya, _, _ = augmented(x, y, aug, seed, it)
        mlp.train(man, xa, ya, lr, reg, epochs=1, batch_size=B, iter0=it)
        it += 3
    for i in range(2):
        assert np.array_equal(seq.W[i], man.W[i]) and np.array_equal(seq.b[i], man.b[i])
    # ... and the f64 torch-backend trainer agrees with it at the bound tests/test_dist.py holds the f64 engine to
    tr = _trainer(seed, aug, H=H, B=B)
    tr.load(x, y)
    tr.train(E, lr, reg)
    for i in range(2):
        assert np.abs(tr.nn.W[i] - seq.W[i]).max() / np.abs(seq.W[i]).max() < 1e-12
    plain = NeuralNetwork([784, H, 10])
    mlp.train(plain, x, y, lr, reg, epochs=E, batch_size=B, shuffle_seed=seed)
    assert np.abs(plain.W[0] - seq.W[0]).max() / np.abs(seq.W[0]).max() > 1e-6


def _loopback(world, cls, x, y, B, epochs, seed, aug, twin):
    comms = LoopbackComm.create(world)
    out = [None] * world

    def work(r):
        torch.set_num_threads(1)
        tr = _trainer(None if twin else seed, None if twin else aug, H=24, B=B, cls=cls, comm=comms[r])
        if twin:
            _twin_epochs(tr, x, y, aug, seed, epochs, 0.05, 1e-4)
        else:
            tr.load(x, y)
            tr.train(epochs, 0.05, 1e-4)
        out[r] = (tr.engine.params.clone(), tr.engine.X.clone())

    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


@pytest.mark.parametrize("cls", [DataParallelTrainer, TensorParallelTrainer])
def test_loopback_ranks_with_uneven_shards_equal_their_twin(cls):
    """Three ranks, batches of 200 and a last one of 100: shards of 66 and 33 columns (the remainder is dropped, as
    in the reference).  Every rank forms the same pixels, and the run is bitwise the reload-per-epoch twin's."""
    x, y = synthetic_mnist(500, seed=11)
    aug = Shift(2, seed=4)
    got = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=False)
    want = _loopback(3, cls, x, y, 200, 2, 6, aug, twin=True)
    for r in range(3):
        assert torch.equal(got[r][1], got[0][1])  # the same pixels on every rank
        assert torch.equal(got[r][0], want[r][0]), r


def test_gloo_world2_augmented_equals_single_process(tmp_path):
    H, N, B, E, lr, reg, seed = 24, 2400, 800, 2, 0.05, 1e-4, 6
    aug = Shift(2, seed=4)
    spawn(dp_augment_worker, 2, args=(str(tmp_path), H, N, B, E, lr, reg, seed, aug.to_meta()), backend="gloo")
    x, y = synthetic_mnist(N, seed=11)
    ref = _trainer(seed, aug, H=H, B=B)
    ref.load(x, y)
    st = ref.train(E, lr, reg)
    r0, r1 = (np.load(tmp_path / f"augment{r}.npz") for r in range(2))
    xa, _, perm, sh = augmented(x, y, aug, seed, 3)
    for r in (r0, r1):
        np.testing.assert_array_equal(r["perm"], perm)
        np.testing.assert_array_equal(r["shifts"], sh)
        np.testing.assert_array_equal(r["X"], xa.astype(np.float64))
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


def test_cli_augment_checkpoint_and_resume(tmp_path):
    whole, half, rest = (str(tmp_path / d) for d in ("whole", "half", "rest"))
    flags = ("--augment-shift", "2", "--augment-seed", "1")
    log = tmp_path / "run.jsonl"
    _cli(tmp_path, *flags, "-e", "4", "--ckpt-dir", whole, "--log-json", str(log))
    meta = json.loads((tmp_path / "whole" / "meta.json").read_text())
    assert Shift.from_meta(meta["augment"]) == Shift(2, seed=1) and meta["epochs"] == 4
    head = json.loads(log.read_text().splitlines()[0])
    assert head["event"] == "config" and head["augment"] == Shift(2, seed=1).to_meta()
    _cli(tmp_path, *flags, "-e", "2", "--ckpt-dir", half)
    r = _cli(tmp_path, *flags, "-e", "2", "--resume", half, "--ckpt-dir", rest)
    assert "warning: the checkpoint was trained with augmentation" not in r.stdout
    a, b = np.load(tmp_path / "whole" / "params.npz"), np.load(tmp_path / "rest" / "params.npz")
    for k in ("W0", "W1", "b0", "b1"):
        np.testing.assert_array_equal(a[k], b[k])  # 2 of 4 epochs, resumed == the unbroken run
    assert json.loads((tmp_path / "rest" / "meta.json").read_text())["iter"] == meta["iter"]
    other = _cli(tmp_path, "--augment-shift", "2", "--augment-seed", "2", "-e", "1", "--resume", half, "--ckpt-dir",
                 str(tmp_path / "other"))
    assert "warning: the checkpoint was trained with augmentation" in other.stdout
    assert json.loads((tmp_path / "other" / "meta.json").read_text())["augment"]["seed"] == 2
    plain = _cli(tmp_path, "-e", "1", "--ckpt-dir", str(tmp_path / "plain"))
    assert json.loads((tmp_path / "plain" / "meta.json").read_text())["augment"] is None
    unaug = np.load(tmp_path / "plain" / "params.npz")
    assert not np.array_equal(unaug["W0"], np.load(tmp_path / "other" / "params.npz")["W0"])


@pytest.mark.parametrize("argv", [("--augment-shift", "2", "--image-shape", "28x27"),
                                  ("--augment-shift", "2", "--image-shape", "28by28"),
                                  ("--augment-shift", "2", "--image-shape", "0x784"),
                                  ("--augment-shift", "28"),
                                  ("--augment-shift", "2", "--augment-shift-y", "4", "--image-shape", "4x196"),
                                  ("--augment-seed", "1"),
                                  ("--image-shape", "28x28")])
def test_cli_refuses_bad_flags_at_parse_time(argv, capsys):
    with pytest.raises(SystemExit) as ex:
        parse_config(list(argv))
    assert ex.value.code == 2
    assert "error:" in capsys.readouterr().err


def test_cli_flags_make_the_shift():
    assert parse_config([]).augment is None
    assert parse_config(["--augment-shift", "2", "--augment-seed", "9"]).augment == Shift(2, seed=9)
    cfg = parse_config(["--augment-shift", "3", "--augment-shift-y", "1", "--image-shape", "16x49"])
    assert cfg.augment == Shift(3, 1, 16, 49)
