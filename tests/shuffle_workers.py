"""Workers of the per-epoch shuffle tests (tests/test_shuffle.py, tests/test_gpu_shuffle.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch


def dp_shuffle_worker(rank, world, comm, device, out_dir, H, N, batch, epochs, lr, reg, seed):
    """tests/dist_workers.py dp_train_worker with a shuffle seed: f64 torch backend over gloo."""
    torch.set_num_threads(2)
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N, seed=11)
    nn = NeuralNetwork([784, H, 10])
    tr = DataParallelTrainer(nn, comm=comm, device=device, dtype="f64", batch_size=batch, backend="torch",
                             use_graphs=False, shuffle_seed=seed)
    tr.load(x, y)
    st = tr.train(epochs, lr, reg)
    np.savez(os.path.join(out_dir, f"shuffle{rank}.npz"), W0=nn.W[0], W1=nn.W[1], b0=nn.b[0], b1=nn.b[1],
             images=st.images, perm=tr.engine.permutation().numpy())


def gpu_shared_shuffle_worker(rank, world, comm, device, out_dir, N, batch, seed):
    """Two processes sharing GPU 0 (gloo group, hip backend): every rank holds the whole set and forms the same
    order; after one shuffled epoch its X is the host-permuted set, after two the replicas agree bitwise."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x, y = synthetic_mnist(N, seed=11)
    tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), comm=comm, device=dev, batch_size=batch,
                             shuffle_seed=seed)
    tr.load(x, y)
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    perm = cpu().epoch_permutation(N, seed, 0)
    res = {"x_equal": float(torch.equal(tr.engine.X.cpu(), torch.from_numpy(x[perm]))),
           "y_equal": float(np.array_equal(tr.engine.labels.cpu().numpy(), y[perm].astype(np.int32))),
           "launches_1": float(tr.engine.shuffle_launches)}
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    res["agree"] = float(tr.replicas_agree())
    res["iter"] = float(tr.iter)
    res["perm2_equal"] = float(np.array_equal(tr.engine.permutation().cpu().numpy(),
                                              cpu().epoch_permutation(N, seed, tr.iter // 2)))
    res["impl"] = tr.allreduce_impl
    tr.close()
    np.savez(os.path.join(out_dir, f"gpu_shuffle{rank}.npz"), **{k: np.array(v) for k, v in res.items()})


def gpu_shared_shuffle_main(out_dir, N, batch, seed):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_shuffle_worker, 2, (out_dir, N, batch, seed), backend="gloo")
