"""Workers of the stateful-optimizer tests (tests/test_optim.py, tests/test_gpu_optim.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch

LR, REG = 1e-3, 1e-4  # (tests/test_optim.py ORACLE_LR: the runs compared with another summation order)


# ---- what binds two Adam runs that see slightly different gradients (docs/PERFORMANCE.md "Stateful optimizers") ----
# A tolerance on the gradient relative to max|g| (the project's TOL table) does not carry over to Adam's parameters: the
# rule divides by sqrt(s), so an element whose gradient is far below max|g| -- about which that tolerance says nothing --
# moves as far as every other.  Two bounds are derived instead.
#   * first update: from zero state m_1 = (1 - b1) g and s_1 = (1 - b2) g^2 are linear and quadratic in the gradient,
#     so per tensor max|m - m'| <= tol max|m'| and max|s - s'| <= (2 tol + tol^2) max|s'| whenever the gradients agree to
#     tol relative to max|g|.  This is where a wrong scale, regulariser or a missed all-reduce contribution shows.
#   * drift: by Cauchy-Schwarz |m_t| <= (1 - b1) sqrt(sum_{k<t} (b1^2 / b2)^k) sqrt(s_t / (1 - b2)), so update t moves
#     an element by at most lr c_t, c_t = (1 - b1) / (1 - b1^t) sqrt((1 - b2^t) / (1 - b2)) sqrt(sum_{k<t} (b1^2 / b2)^k)
#     (c_1 = 1; 1.03 at t = 8 for 0.9 / 0.999), whatever the gradients are.  Two runs from the same start therefore
#     differ elementwise by at most 2 lr sum_t c_t; runs that share their first d updates' directions exactly gain
#     nothing from that here, so the bound is loose, but it holds for every element and catches a wrong t or bias
#     correction (c_t is what the bias corrections make it).


def adam_step_cap(opt, t: int) -> float:
    b1, b2 = opt.beta1, opt.beta2
    geo = sum((b1 * b1 / b2) ** k for k in range(t)) if b2 > 0 else float(t)
    return (1 - b1) / (1 - b1 ** t) * ((1 - b2 ** t) / (1 - b2)) ** 0.5 * geo ** 0.5


def adam_drift_bound(opt, lr: float, steps: int) -> float:
    """max |p - p'| elementwise after `steps` updates of two Adam runs from the same parameters and zero state."""
    return 2.0 * lr * sum(adam_step_cap(opt, t) for t in range(1, steps + 1))


def split_params(H, flat):
    """[W1|b1|W2|b2] unpadded (MlpEngine.optim_state's layout) -> the four tensors' flat pieces."""
    P, Hd, C = H
    sizes = [Hd * P, Hd, C * Hd, C]
    out, o = [], 0
    for n in sizes:
        out.append(np.asarray(flat[o:o + n], np.float64))
        o += n
    assert o == len(flat)
    return out


def check_adam_first_update(H, got_state, want_state, tol, tag=""):
    """got / want: [m, s] after ONE update from zero state (unpadded flat arrays); asserts the first-update bound."""
    for name, g, w, bound in (("m", got_state[0], want_state[0], tol), ("s", got_state[1], want_state[1],
                                                                       2 * tol + tol * tol)):
        for part, a, b in zip(("W1", "b1", "W2", "b2"), split_params(H, g), split_params(H, w)):
            rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
            print(f"NUMERICS adam first update {tag} {name}[{part}] rel {rel:.3e} (bound {bound:.3e})")
            assert np.abs(b).max() > 0, (tag, name, part)
            assert rel <= bound, (tag, name, part, rel, bound)


def check_adam_drift(opt, lr, steps, got, want, tag=""):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    bound = adam_drift_bound(opt, lr, steps)
    print(f"NUMERICS adam drift {tag} max|dp| {d:.3e} (bound {bound:.3e}, {steps} updates)")
    assert d <= bound, (tag, d, bound)


def _optimizers():
    from cme213_sp18_amd.optim import Optimizer

    return {"nesterov": Optimizer.momentum(0.8, True), "adam": Optimizer.adam(0.9, 0.999, 1e-8)}


def first_update_state(tr, lr, reg):
    """One update from the initial parameters and zero state -> its [m, s] (or [v]) as optim_state() lays them out;
    then parameters, state and count are put back, so the trainer is as constructed."""
    from cme213_sp18_amd import NeuralNetwork

    tr.step(*tr.epoch_plan().steps[0], lr, reg)
    st = tr.engine.optim_state()
    assert st["t"] == 1
    tr.engine.reset_optimizer()
    tr.engine.set_params(*NeuralNetwork(list(tr.nn.H)).params)
    return st["state"]


def dp_optim_worker(rank, world, comm, device, out_dir, H, N, batch, epochs, dtype):
    """tests/dist_workers.py dp_train_worker with a stateful optimizer: the torch backend over loopback or gloo."""
    torch.set_num_threads(2)
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    x, y = synthetic_mnist(N, seed=11)
    out = {}
    for kind, opt in _optimizers().items():
        nn = NeuralNetwork([784, H, 10])
        tr = DataParallelTrainer(nn, comm=comm, device=device, dtype=dtype, batch_size=batch, backend="torch",
                                 use_graphs=False, optimizer=opt)
        tr.load(x, y)
        out[f"{kind}_first"] = np.concatenate(first_update_state(tr, LR, REG))
        tr.train(epochs, LR, REG)
        st = tr.engine.optim_state()
        out[f"{kind}_params"] = np.concatenate([p.ravel() for p in tr.engine.get_params()])
        out[f"{kind}_state"] = np.concatenate(st["state"])
        out[f"{kind}_t"] = np.array(st["t"])
    np.savez(os.path.join(out_dir, f"optim{rank}.npz"), **out)


def gpu_shared_optim_worker(rank, world, comm, device, out_dir, mode):
    """Two processes sharing GPU 0 (gloo group, hip backend): gradient mode, the all-reduce of ``mode`` (rccl = the
    communicator's, host = staged through host memory, xgmi = the separate peer-to-peer kernel), then the optimizer
    launch.  Every rank saves its arena and state; replicas_agree() covers both."""
    from cme213_sp18_amd import NeuralNetwork
    from cme213_sp18_amd.parallel import DataParallelTrainer
    from cme213_sp18_amd.utils.data import synthetic_mnist

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x, y = synthetic_mnist(384, seed=11)
    res = {}
    for kind, opt in _optimizers().items():
        tr = DataParallelTrainer(NeuralNetwork([784, 100, 10]), comm=comm, device=dev, batch_size=128, allreduce=mode,
                                 optimizer=opt)
        assert (tr.xgmi is not None) == (mode == "xgmi")
        tr.load(x, y)
        res[f"{kind}_first"] = np.concatenate(first_update_state(tr, LR, REG))
        tr.train(2, LR, REG)
        torch.cuda.synchronize()
        res[f"{kind}_agree"] = float(tr.replicas_agree())
        res[f"{kind}_fused"] = float(tr.fused_allreduce or tr._xgmi_fused is not None)
        res[f"{kind}_t"] = float(tr.engine.optim_state()["t"])
        res[f"{kind}_params"] = tr.engine.params.cpu().numpy()
        res[f"{kind}_state"] = torch.cat(tr.engine.opt_bufs).cpu().numpy()
        res["impl"] = tr.allreduce_impl
        tr.close()
    if mode == "rccl":  # the bucketed, overlapped backward against one bucket (H = 300: three 128-row chunks)
        import cme213_sp18_amd.parallel.trainer as trmod

        trmod.BUCKET_BYTES = 256 << 10
        outs = {}
        for overlap in (True, False):
            tr = DataParallelTrainer(NeuralNetwork([784, 300, 10]), comm=comm, device=dev, batch_size=128,
                                     allreduce="rccl", overlap=overlap, optimizer=_optimizers()["nesterov"])
            assert tr._bucketed == overlap and len(tr._buckets()) > 1
            tr.load(x, y)
            tr.train(2, LR, REG)
            torch.cuda.synchronize()
            res[f"bucketed_agree_{int(overlap)}"] = float(tr.replicas_agree())
            outs[overlap] = tr.engine.params.cpu().double()
            tr.close()
        res["bucketed_rel"] = float((outs[True] - outs[False]).abs().max() / outs[False].abs().max())
    np.savez(os.path.join(out_dir, f"optim_{mode}_{rank}.npz"), **{k: np.asarray(v) for k, v in res.items()})


def gpu_shared_optim_main(out_dir, mode):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_optim_worker, 2, (out_dir, mode), backend="gloo")
