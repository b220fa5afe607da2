"""Workers of the affine augmentation tests (tests/test_affine.py, tests/test_gpu_affine.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch


def dp_affine_worker(rank, world, comm, device, out_dir, H, N, batch, epochs, lr, reg, seed, aug_meta):
    """tests/augment_workers.py dp_augment_worker with an affine policy: f64 torch backend over gloo."""
    torch.set_num_threads(2)
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.augment import from_meta
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N, seed=11)
    nn = NeuralNetwork([784, H, 10])
    tr = DataParallelTrainer(nn, comm=comm, device=device, dtype="f64", batch_size=batch, backend="torch",
                             use_graphs=False, shuffle_seed=seed, augment=from_meta(aug_meta))
    tr.load(x, y)
    st = tr.train(epochs, lr, reg)
    np.savez(os.path.join(out_dir, f"affine{rank}.npz"), W0=nn.W[0], W1=nn.W[1], b0=nn.b[0], b1=nn.b[1],
             images=st.images, perm=tr.engine.permutation().numpy(), shifts=tr.engine.shifts().numpy(),
             transforms=tr.engine.transforms().numpy(), X=tr.engine.X.numpy())


def dp_affine_main(out_dir, world, H, N, batch, epochs, lr, reg, seed, aug_meta):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(dp_affine_worker, world, (out_dir, H, N, batch, epochs, lr, reg, seed, aug_meta), backend="gloo")


def gpu_shared_affine_worker(rank, world, comm, device, out_dir, N, batch, seed, aug_meta):
    """Two processes sharing GPU 0 (gloo group, hip backend): every rank holds the whole set and forms the same order
    and the same pixels; after one augmented epoch its X is the host-transformed permuted set, after two the replicas
    agree bitwise."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.augment import apply_affine, epoch_shifts, epoch_transforms, from_meta
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    aug = from_meta(aug_meta)
    x, y = synthetic_mnist(N, seed=11)
    tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), comm=comm, device=dev, batch_size=batch,
                             shuffle_seed=seed, augment=aug)
    tr.load(x, y)
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    perm = cpu().epoch_permutation(N, seed, 0)
    want = apply_affine(x[perm], epoch_shifts(N, aug, 0)[perm], aug.table()[epoch_transforms(N, aug, 0)[perm]], 28, 28)
    res = {"x_equal": float(torch.equal(tr.engine.X.cpu(), torch.from_numpy(want))),
           "y_equal": float(np.array_equal(tr.engine.labels.cpu().numpy(), y[perm].astype(np.int32))),
           "launches_1": float(tr.engine.affine_launches), "shuffle_launches": float(tr.engine.shuffle_launches)}
    tr.train(1, 0.05, 1e-4)
    torch.cuda.synchronize()
    res["agree"] = float(tr.replicas_agree())
    res["iter"] = float(tr.iter)
    k2 = tr.iter // 2
    perm2 = cpu().epoch_permutation(N, seed, k2)
    res["perm2_equal"] = float(np.array_equal(tr.engine.permutation().cpu().numpy(), perm2))
    res["shifts2_equal"] = float(np.array_equal(tr.engine.shifts().cpu().numpy(), epoch_shifts(N, aug, k2)[perm2]))
    res["transforms2_equal"] = float(np.array_equal(tr.engine.transforms().cpu().numpy(),
                                                    epoch_transforms(N, aug, k2)[perm2]))
    res["impl"] = tr.allreduce_impl
    tr.close()
    np.savez(os.path.join(out_dir, f"gpu_affine{rank}.npz"), **{k: np.array(v) for k, v in res.items()})


def gpu_shared_affine_main(out_dir, N, batch, seed, aug_meta):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_affine_worker, 2, (out_dir, N, batch, seed, aug_meta), backend="gloo")
