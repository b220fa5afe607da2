"""Workers of the sampling tests (tests/test_sampling.py, tests/test_gpu_sampling.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch


def _imbalanced(n, seed):
    from cme213_sp18_amd.utils.data import synthetic_mnist
    from tests.sampling_cases import zipf_labels

    x, _ = synthetic_mnist(n, seed=seed)
    return x, np.sort(zipf_labels(n, classes=10, seed=seed)).astype(np.int32)


def dp_sampling_worker(rank, world, comm, device, out_dir, H, N, batch, epochs, lr, reg, seed):
    """tests/shuffle_workers.py dp_shuffle_worker with a Balanced sampler: f64 torch backend over gloo."""
    torch.set_num_threads(2)
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.sampling import Balanced

    x, y = _imbalanced(N, 11)
    nn = NeuralNetwork([784, H, 10])
    tr = DataParallelTrainer(nn, comm=comm, device=device, dtype="f64", batch_size=batch, backend="torch",
                             use_graphs=False, sampler=Balanced(seed))
    tr.load(x, y)
    st = tr.train(epochs, lr, reg)
    np.savez(os.path.join(out_dir, f"sampling{rank}.npz"), W0=nn.W[0], W1=nn.W[1], b0=nn.b[0], b1=nn.b[1],
             images=st.images, perm=tr.engine.permutation().numpy())


def gpu_shared_sampling_worker(rank, world, comm, device, out_dir, N, batch, seed):
    """Two processes sharing GPU 0 (gloo group, hip backend): every rank holds the whole set and forms the same draws;
    after one sampled epoch its X is the host-drawn set, after two the replicas agree bitwise."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.sampling import Balanced

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x, y = _imbalanced(N, 11)
    smp = Balanced(seed)
    tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), comm=comm, device=dev, batch_size=batch, sampler=smp)
    tr.load(x, y)
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    d = smp.draws(y, 0)
    res = {"x_equal": float(torch.equal(tr.engine.X.cpu(), torch.from_numpy(x[d]))),
           "y_equal": float(np.array_equal(tr.engine.labels.cpu().numpy(), y[d])),
           "launches_1": float(tr.engine.shuffle_launches)}
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    res["agree"] = float(tr.replicas_agree())
    res["iter"] = float(tr.iter)
    res["perm2_equal"] = float(np.array_equal(tr.engine.permutation().cpu().numpy(), smp.draws(y, tr.iter // 2)))
    res["impl"] = tr.allreduce_impl
    tr.close()
    np.savez(os.path.join(out_dir, f"gpu_sampling{rank}.npz"), **{k: np.array(v) for k, v in res.items()})


def gpu_shared_sampling_main(out_dir, N, batch, seed):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_sampling_worker, 2, (out_dir, N, batch, seed), backend="gloo")
