"""Workers of the plateau tests on the GPU (tests/test_gpu_plateau.py): started by
cme213_sp18_amd.parallel.launcher.spawn as fn(rank, world, comm, device, *args)."""
import os

import numpy as np
import torch

EPOCHS = 4


def gpu_shared_plateau_worker(rank, world, comm, device, out_dir, mode, keep_best):
    """Two processes sharing GPU 0 (gloo group, hip backend): train(eval_every=1) one epoch at a time under the plateau
    rule with the all-reduce of ``mode`` (rccl = the communicator's, host = staged through host memory), with and
    without keep-best (whose gathered rows the decision then shares).  Every rank saves its own triple and its record
    after every epoch, the gathered rows, its parameters and replicas_agree()."""
    from tests.plateau_oracle import CONFIGS, REG, make_trainer, rule_for

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    kw, lr, _ = CONFIGS["sgd"]
    tr = make_trainer(rule_for("sgd", threshold=0.5), dtype="f32", H=100, device=dev, backend="hip", comm=comm, nval=255,
                      allreduce=mode, use_graphs=True, **kw)
    e = tr.engine
    triples, recs = [], []
    for _ in range(EPOCHS):
        tr.train(1, lr, REG, eval_every=1, keep_best="loss" if keep_best else None)
        torch.cuda.synchronize()
        triples.append(e._slot_triple(e._eval, 0)[0])
        recs.append(e.plateau_record())
    rows = e.best_rows if keep_best else e.plateau_rows
    np.savez(os.path.join(out_dir, f"plateau_{mode}_{int(keep_best)}_{rank}.npz"), triples=np.asarray(triples),
             recs=np.asarray(recs), rows=rows.cpu().numpy(), shard=e.eval_samples, agree=float(tr.replicas_agree()),
             params=e.params.cpu().numpy(), last=e.opt_last.cpu().numpy(), impl=tr.allreduce_impl)
    tr.close()


def gpu_shared_plateau_main(out_dir, mode, keep_best):
    from cme213_sp18_amd.parallel.launcher import spawn

    spawn(gpu_shared_plateau_worker, 2, (out_dir, mode, bool(keep_best)), backend="gloo")
