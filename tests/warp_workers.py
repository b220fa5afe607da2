"""Workers of the elastic distortion tests (tests/test_warp.py, tests/test_gpu_warp.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch


def dp_warp_worker(rank, world, comm, device, out_dir, H, N, batch, epochs, lr, reg, seed, aug_meta):
    """tests/affine_workers.py dp_affine_worker with a warp policy: f64 torch backend over gloo."""
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
    np.savez(os.path.join(out_dir, f"warp{rank}.npz"), W0=nn.W[0], W1=nn.W[1], b0=nn.b[0], b1=nn.b[1],
             images=st.images, perm=tr.engine.permutation().numpy(), shifts=tr.engine.shifts().numpy(),
             transforms=tr.engine.transforms().numpy(), X=tr.engine.X.numpy())


def dp_warp_main(out_dir, world, H, N, batch, epochs, lr, reg, seed, aug_meta):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(dp_warp_worker, world, (out_dir, H, N, batch, epochs, lr, reg, seed, aug_meta), backend="gloo")


def host_warped(x, aug, perm, key, h=28, w=28):
    """x[perm] through the host's rule in the epoch that starts at iteration counter ``key``."""
    from cme213_sp18_amd.augment import apply_warp, epoch_nodes, epoch_shifts, epoch_transforms

    n = x.shape[0]
    return apply_warp(x[perm], epoch_shifts(n, aug, key)[perm], aug.table()[epoch_transforms(n, aug, key)[perm]],
                      epoch_nodes(n, aug, key)[perm], aug, h, w)


def gpu_shared_warp_worker(rank, world, comm, device, out_dir, N, batch, seed, aug_meta):
    """Two processes sharing GPU 0 (gloo group, hip backend): every rank holds the whole set and forms the same order
    and the same pixels; after one warped epoch its X is the host-warped permuted set, after two the replicas agree
    bitwise and X is the second epoch's."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd._native import cpu
    from cme213_sp18_amd.augment import epoch_shifts, epoch_transforms, from_meta
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
    res = {"x_equal": float(torch.equal(tr.engine.X.cpu(), torch.from_numpy(host_warped(x, aug, perm, 0)))),
           "y_equal": float(np.array_equal(tr.engine.labels.cpu().numpy(), y[perm].astype(np.int32))),
           "launches_1": float(tr.engine.warp_launches), "shuffle_launches": float(tr.engine.shuffle_launches),
           "other_launches": float(tr.engine.affine_launches + tr.engine.augment_launches)}
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
    res["x2_equal"] = float(torch.equal(tr.engine.X.cpu(), torch.from_numpy(host_warped(x, aug, perm2, k2))))
    res["impl"] = tr.allreduce_impl
    tr.close()
    np.savez(os.path.join(out_dir, f"gpu_warp{rank}.npz"), **{k: np.array(v) for k, v in res.items()})


def gpu_shared_warp_main(out_dir, N, batch, seed, aug_meta):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_warp_worker, 2, (out_dir, N, batch, seed, aug_meta), backend="gloo")
