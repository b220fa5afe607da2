"""CLI driver -- the reference's ``main()`` (fpcode/main.cpp:34-276).

    python -m cme213_sp18_amd.train -g 1                      # grade preset 1 (fp64 parity)
    python -m cme213_sp18_amd.train -n 100 -e 5 -p 10         # f32 split-bf16 engine, print loss
    python -m cme213_sp18_amd.train --preset 8gpu_wide --gpus 8   # 8 ranks, one per GPU, RCCL/xGMI
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m cme213_sp18_amd.train --preset 8gpu_wide           # the same under an external launcher

Flow: bootstrap (one process per GPU, device = LOCAL_RANK) -> data (identical on
every rank, uploaded once per GPU) -> optional sequential fp64 CPU training on
rank 0 (-s) -> data-parallel GPU training -> rank 0 evaluates on the dev split,
writes test-set predictions, and with -g/-d compares against the CPU run.
Grade 4 runs the GEMM benchmark instead.
"""
from __future__ import annotations

import copy
import json
import os
import sys
import time

import numpy as np

from .config import TrainConfig, parse_config


def log0(rank: int, *a):
    if rank == 0:
        print(*a, flush=True)


class JsonLog:
    """Rank-0 JSON-lines event log: config, losses, epochs, summary."""

    def __init__(self, path: str, rank: int):
        self.fh = open(path, "a") if path and rank == 0 else None
        self.t0 = time.time()

    def __call__(self, rec: dict) -> None:
        if self.fh is not None:
            rec = {"t": round(time.time() - self.t0, 6), **rec}
            self.fh.write(json.dumps(rec, default=float) + "\n")
            self.fh.flush()

    def close(self):
        if self.fh is not None:
            self.fh.close()


def parse_fault(spec: str):
    if not spec:
        return None
    r, s = spec.split(":")
    return int(r), int(s)


def run(cfg: TrainConfig) -> dict:
    import torch

    from .models import mlp
    from .models.mlp import NeuralNetwork
    from .optim import Optimizer
    from .parallel.launcher import PlacementError, init_distributed, shutdown, verify_placement
    from .parallel.trainer import DataParallelTrainer
    from .utils.checkpoint import (checkNNErrors, load_best_state, load_checkpoint, load_ema_state,
                                   load_optim_state, save_checkpoint)
    from .utils.common import precision, save_label
    from .utils.data import load_dataset

    backend = cfg.backend
    if backend == "hip" and not torch.cuda.is_available():
        backend = "torch"
    comm, device = init_distributed("gloo" if backend == "torch" else None, timeout_s=cfg.comm_timeout)
    rank, world = comm.rank, comm.world_size
    try:  # exactly --gpus ranks, on distinct GPUs (CME_SHARED_GPU=1: the shared-GPU rehearsal)
        placement = verify_placement(comm, device, cfg.gpus)
    except PlacementError as ex:
        print(f"[rank {rank}] error: {ex}", file=sys.stderr, flush=True)
        shutdown()
        raise SystemExit(2)
    jlog = JsonLog(cfg.log_json, rank)
    try:
        aug = cfg.augment  # an augment.Shift, an augment.Affine, an augment.Warp or None
        # what meta.json and the run header record: the policy and, for an Affine, a checksum of its table (the table
        # goes through libm: another libm must not silently change a resumed run)
        aug_meta = aug.to_meta() if aug is not None else None
        if aug_meta is not None and aug_meta["kind"] == "affine":
            aug_meta["table_checksum"] = f"{aug.table_checksum():016x}"
        elif aug_meta is not None and aug_meta["kind"] == "warp":  # (its axis tables are built in fp64 too)
            aug_meta["table_checksum"] = f"{aug.table_checksum(*aug.shape(cfg.H[0])):016x}"
        smp = cfg.sampler  # a sampling.Balanced, a sampling.Weighted or None
        jlog({"event": "config", "world": world, "device": str(device), **placement, **{
            k: v for k, v in vars(cfg).items() if isinstance(v, (int, float, str, bool))},
            "augment": aug_meta,
            "sampler": smp.to_meta() if smp is not None else None,
            "ema": cfg.ema_rule.as_meta() if cfg.ema_rule is not None else None,
            "plateau": cfg.plateau.as_meta() if cfg.plateau is not None else None})
        log0(rank, f"Number of processes = {world}")
        log0(rank, f"Device = {device} ({torch.cuda.get_device_name(device) if device.type == 'cuda' else 'cpu'})")
        if cfg.grade == 4:
            if rank == 0:
                from .ops.gemm import benchmark_gemm

                # the reference's fp64 benchmark first, then the MI355X dtypes (fp32, bf16)
                benchmark_gemm(device=device, dtypes=(torch.float64, torch.float32, torch.bfloat16))
            return {}
        log0(rank, f"num_neuron={cfg.num_neuron}, reg={cfg.reg}, learning_rate={cfg.learning_rate}, "
                   f"num_epochs={cfg.num_epochs}, batch_size={cfg.batch_size}, dtype={cfg.dtype}")
        t = time.perf_counter()
        ds = load_dataset(cfg.data, cfg.data_dir, cfg.num_train, cfg.num_test, cfg.seed, cfg.num_classes)
        log0(rank, f"Loaded {ds.source}: train {ds.x_train.shape[0]}, dev {ds.x_dev.shape[0]}, "
                   f"test {ds.x_test.shape[0]} ({time.perf_counter() - t:.2f}s)")
        os.makedirs(cfg.outdir, exist_ok=True)
        # what meta.json records of the sampler: the policy and a checksum of its alias table (built in fp64 on the
        # host from this training split: other weights or another split must not silently change a resumed run)
        smp_meta = None
        if smp is not None:
            try:
                smp_meta = {**smp.to_meta(), "table_checksum": f"{smp.checksum(ds.y_train):016x}"}
            except ValueError as ex:
                raise SystemExit(f"error: {ex}")
        meta = {}
        opt = cfg.optim
        sched, clip = cfg.schedule, cfg.clip_norm
        plateau = cfg.plateau  # an optim.Plateau or None
        plateau_saved = None  # the checkpoint's plateau record (continued when the flags agree)
        # (plain SGD then keeps an update count too: optim_t)
        policy = sched is not None or clip is not None or plateau is not None
        keeps_state = opt.stateful or policy
        opt_state = None  # the checkpoint's optimizer state (both runs continue it)
        best_rule = ({"monitor": cfg.keep_best, "min_delta": float(cfg.min_delta), "patience": cfg.patience}
                     if cfg.keep_best else None)
        best_saved = None  # the checkpoint's keep-best state (continued when the flags agree)
        ema = cfg.ema_rule  # an optim.Ema or None
        ema_saved = None  # the checkpoint's averaged weights and count (continued when the flags agree)
        seq_ema = None  # the sequential run's average (optim.new_ema_state)
        if cfg.resume:
            nn, meta = load_checkpoint(cfg.resume)
            log0(rank, f"Resumed from {cfg.resume}: {meta}")
            saved = Optimizer.from_meta(meta.get("optimizer"))  # (no record: plain SGD)
            same = saved == opt if opt.stateful else not saved.stateful
            if keeps_state and same:
                opt_state = load_optim_state(cfg.resume, meta)
            from .optim import Schedule

            if Schedule.from_meta(meta.get("schedule")) != sched or meta.get("clip_norm") != clip:
                log0(rank, f"warning: the checkpoint was trained with schedule {meta.get('schedule')} and clip norm "
                           f"{meta.get('clip_norm')}, this run uses {sched.as_meta() if sched else None} and {clip}: "
                           "the rates do not continue the checkpoint's")
            if not same:
                log0(rank, f"warning: the checkpoint was trained with optimizer {saved}, this run uses {opt}: the "
                           "optimizer state starts fresh")
            elif opt.stateful and opt_state is None:
                log0(rank, "warning: the checkpoint holds no optimizer state (optim.npz): it starts fresh")
            saved_best = load_best_state(cfg.resume, meta)
            saved_rule = ({k: saved_best[k] for k in ("monitor", "min_delta", "patience")}
                          if saved_best is not None else None)
            if saved_rule != best_rule:
                log0(rank, f"warning: the checkpoint was trained with keep-best {saved_rule}, this run uses "
                           f"{best_rule}: the best weights and the patience count do not continue the checkpoint's")
            elif saved_best is not None:
                best_saved = saved_best
            saved_ema = load_ema_state(cfg.resume, meta)
            saved_ema_rule = {k: saved_ema[k] for k in ("decay", "warmup")} if saved_ema is not None else None
            if saved_ema_rule != (ema.as_meta() if ema is not None else None):
                log0(rank, f"warning: the checkpoint was trained with weight averaging {saved_ema_rule}, this run uses "
                           f"{ema.as_meta() if ema is not None else None}: the average does not continue the "
                           "checkpoint's" + (" (it starts from the resumed weights)" if ema is not None else ""))
            elif saved_ema is not None:
                ema_saved = saved_ema
            from .optim import Plateau

            saved_plateau = meta.get("plateau")
            saved_plateau_rule = Plateau.from_meta(saved_plateau["rule"]) if saved_plateau else None
            if saved_plateau_rule != plateau:
                log0(rank, f"warning: the checkpoint was trained with the plateau rule "
                           f"{saved_plateau['rule'] if saved_plateau else None}, this run uses "
                           f"{plateau.as_meta() if plateau is not None else None}: the rate's scale does not continue "
                           "the checkpoint's" + (" (it starts at 1)" if plateau is not None else ""))
            elif saved_plateau:
                plateau_saved = saved_plateau["record"]
            if meta.get("shuffle_seed") != cfg.shuffle_seed:
                log0(rank, f"warning: the checkpoint was trained with --shuffle-seed {meta.get('shuffle_seed')}, this "
                           f"run uses {cfg.shuffle_seed}: the epochs' orders do not continue the checkpoint's")
            from .augment import from_meta as augment_from_meta

            if augment_from_meta(meta.get("augment")) != aug:
                log0(rank, f"warning: the checkpoint was trained with augmentation {meta.get('augment')}, this run "
                           f"uses {aug.to_meta() if aug is not None else None}: the epochs' shifts do not continue "
                           "the checkpoint's")
            elif aug_meta is not None and meta["augment"].get("table_checksum") != aug_meta.get("table_checksum"):
                log0(rank, f"warning: the checkpoint's transform table has checksum "
                           f"{meta['augment'].get('table_checksum')}, this run's has "
                           f"{aug_meta.get('table_checksum')} (another math library?): the epochs' transforms do not "
                           "continue the checkpoint's")
            saved_smp = meta.get("sampler")
            # (the checksum is compared apart; `source` is where the weights were read from, weights_checksum says
            # which they are: the same file at another path is the same sampler)
            strip = lambda m: ({k: v for k, v in m.items() if k not in ("table_checksum", "source")}  # noqa: E731
                               if m else None)
            if strip(saved_smp) != strip(smp_meta):
                log0(rank, f"warning: the checkpoint was trained with sampler {strip(saved_smp)}, this run uses "
                           f"{strip(smp_meta)}: the epochs' draws do not continue the checkpoint's")
            elif smp_meta is not None and saved_smp.get("table_checksum") != smp_meta["table_checksum"]:
                log0(rank, f"warning: the checkpoint's sampling table has checksum {saved_smp.get('table_checksum')}, "
                           f"this run's has {smp_meta['table_checksum']} (other labels or weights?): the epochs' "
                           "draws do not continue the checkpoint's")
        else:
            nn = NeuralNetwork(cfg.H)
        seq_nn = nn.copy()
        xs = ds.x_train / 255.0 if cfg.normalize else ds.x_train
        xd = ds.x_dev / 255.0 if cfg.normalize else ds.x_dev
        out = {}
        if rank == 0 and cfg.run_seq:
            log0(rank, "Start Sequential Training")
            t = time.perf_counter()
            if ema is not None:
                from .optim import new_ema_state

                seq_ema = new_ema_state(seq_nn)
                if ema_saved is not None:
                    W1a, b1a, W2a, b2a = ema_saved["params"]
                    seq_ema = {"t": ema_saved["t"], "avg": np.concatenate(
                        [np.asarray(a, np.float64).reshape(-1) for a in (W1a, b1a, W2a, b2a)])}
            seq_kw = dict(shuffle_seed=cfg.shuffle_seed, optimizer=opt, schedule=sched, clip_norm=clip, augment=aug,
                          ema=ema, ema_state=seq_ema, sampler=smp)
            if plateau is None:
                mlp.train(seq_nn, xs, ds.y_train, cfg.learning_rate, cfg.reg, cfg.num_epochs, cfg.batch_size,
                          False, cfg.print_every, cfg.debug, cfg.outdir, cfg.softmax_shift, cfg.ckpt_precision,
                          iter0=int(meta.get("iter", 0)), optim_state=copy.deepcopy(opt_state), **seq_kw)
            else:
                # the oracle evaluates no validation set: it runs --eval-every epochs at a time at the scale the rule
                # holds, the dev split is evaluated on the host in fp64 and the rule (csrc/mlp/plateau.h) decides
                from ._native import cpu
                from .optim import new_state, plateau_record_array, plateau_record_dict

                seq_state = copy.deepcopy(opt_state) if opt_state is not None else new_state(
                    opt, seq_nn.num_params(), policy=True)
                seq_rec = (plateau_record_array(plateau_saved) if plateau_saved is not None
                           else cpu().plateau_start(plateau.monitor_code))
                nb = (xs.shape[0] + cfg.batch_size - 1) // cfg.batch_size
                it, left = int(meta.get("iter", 0)), cfg.num_epochs
                while left > 0:
                    k = min(cfg.eval_every, left)
                    mlp.train(seq_nn, xs, ds.y_train, cfg.learning_rate, cfg.reg, k, cfg.batch_size, False,
                              cfg.print_every, cfg.debug, cfg.outdir, cfg.softmax_shift, cfg.ckpt_precision, iter0=it,
                              optim_state=seq_state, lr_scale=float(seq_rec[cpu().plateau_scale_word]), **seq_kw)
                    it, left = it + k * nb, left - k
                    if k == cfg.eval_every:
                        triple = mlp.eval_triple(seq_nn, xd, ds.y_dev, cfg.softmax_shift)
                        seq_rec, _ = cpu().plateau_decide(seq_rec, plateau.native(), np.asarray([triple], np.float64))
                seq_ps = plateau_record_dict(seq_rec)
                out.update(seq_lr_scale=seq_ps["scale"], seq_lr_reductions=seq_ps["reductions"])
                log0(rank, f"Sequential plateau rule: scale {seq_ps['scale']:.10g} after {seq_ps['reductions']} "
                           "reduction(s)")
            out["seq_seconds"] = time.perf_counter() - t
            log0(rank, f"Time for Sequential Training: {out['seq_seconds']:.6f} seconds")
            if cfg.use_ema:  # the sequential run's final weights are its average too
                o = 0
                for dst in seq_nn.params:
                    dst[...] = seq_ema["avg"][o:o + dst.size].reshape(dst.shape)
                    o += dst.size
            out["seq_dev_precision"] = precision(mlp.predict(seq_nn, xd, cfg.softmax_shift), ds.y_dev)
            log0(rank, f"Precision on validation set for sequential training = {out['seq_dev_precision']}")
        comm.barrier()  # the parallel run's debug diff reads the CPU snapshots
        log0(rank, "\nStart Parallel Training")
        if cfg.parallel == "tp":
            from .parallel.tensor_parallel import TensorParallelTrainer, tp_allreduce_mode

            if cfg.debug:
                log0(rank, "note: -d (per-iteration CPU diff) is data-parallel only; ignored with --parallel tp")
                cfg.debug = False
            tr = TensorParallelTrainer(nn, comm=comm, device=device, dtype=cfg.dtype, batch_size=cfg.batch_size,
                                       backend=backend, shift=cfg.softmax_shift, normalize=cfg.normalize,
                                       path=cfg.path,
                                       allreduce=tp_allreduce_mode(cfg.allreduce), shuffle_seed=cfg.shuffle_seed,
                                       optimizer=opt, schedule=sched, clip_norm=clip, augment=aug, ema=ema,
                                       plateau=plateau, sampler=smp)
            tr.use_graphs = cfg.use_graphs
        else:
            tr = DataParallelTrainer(nn, comm=comm, device=device, dtype=cfg.dtype, batch_size=cfg.batch_size,
                                     backend=backend, shift=cfg.softmax_shift, use_graphs=cfg.use_graphs,
                                     normalize=cfg.normalize, path=cfg.path, allreduce=cfg.allreduce,
                                     overlap_chunks=cfg.overlap_chunks, shuffle_seed=cfg.shuffle_seed, optimizer=opt,
                                     schedule=sched, clip_norm=clip, augment=aug, ema=ema, plateau=plateau,
                                     sampler=smp)
            if opt_state is not None:
                tr.engine.set_optim_state(opt_state)
            if plateau_saved is not None:
                tr.set_plateau_state(plateau_saved)
            if ema_saved is not None:
                tr.set_ema_state(ema_saved["t"], ema_saved["params"])
        tr.load(ds.x_train, ds.y_train)
        eval_every = cfg.eval_every if cfg.parallel != "tp" else 0
        if cfg.eval_every > 0 and not eval_every:
            log0(rank, "note: --eval-every is data-parallel only; ignored with --parallel tp")
        if eval_every > 0:
            tr.load_eval(ds.x_dev, ds.y_dev)
        train_kw = {"eval_every": eval_every} if eval_every > 0 else {}
        if ema is not None and cfg.eval_weights:
            train_kw["eval_weights"] = cfg.eval_weights
        if cfg.keep_best:
            train_kw.update(keep_best=cfg.keep_best, patience=cfg.patience, min_delta=cfg.min_delta,
                            stop_check_every=cfg.stop_check_every)
            if best_saved is not None:
                tr.enable_keep_best(cfg.keep_best, cfg.min_delta, cfg.patience)
                tr.set_best_state(best_saved["record"], best_saved["params"], best_saved.get("iters"))
        # a resumed run continues the iteration counter (loss lines, -d diff rows and the print_flag
        # schedule pick up where the checkpoint left off; CpuGpuDiff.txt is appended to, not truncated)
        tr.iter = int(meta.get("iter", 0))
        if cfg.profile:
            tr.enable_profiling()
        fault = parse_fault(cfg.fault_inject)
        ckpt_meta = lambda done: {"epochs": done + meta.get("epochs", 0), "lr": cfg.learning_rate, "reg": cfg.reg,
                                  "seed": cfg.seed, "dtype": cfg.dtype, "iter": tr.iter,
                                  "shuffle_seed": cfg.shuffle_seed,
                                  "augment": aug_meta,
                                  **({"sampler": smp_meta} if smp_meta is not None else {}),
                                  **({"optimizer": opt.as_meta()} if opt.stateful else {}),
                                  **({"schedule": sched.as_meta()} if sched is not None else {}),
                                  **({"clip_norm": clip} if clip is not None else {}),
                                  **({"plateau": {"rule": plateau.as_meta(),
                                                  "record": tr.engine.plateau_record().tolist()}}
                                     if plateau is not None else {})}

        def ckpt_ema():
            if ema is None:
                return None
            return {**ema.as_meta(), "t": tr.engine.ema_count(), "params": tr.ema_params()}
        ckpt_optim = lambda: tr.engine.optim_state() if keeps_state else None  # noqa: E731

        def ckpt_best():
            if not cfg.keep_best:
                return None
            return {**best_rule, "record": tr.engine.best_records()[0].tolist(), "iter": tr.best_state()["iter"],
                    "iters": list(tr._best_iters), "params": tr.engine.best_params()}
        seg = cfg.ckpt_every if (cfg.ckpt_every > 0 and cfg.ckpt_dir) else cfg.num_epochs
        done, st = 0, None
        while done < cfg.num_epochs or st is None:  # train in checkpoint segments
            k = min(seg, cfg.num_epochs - done)
            s1 = tr.train(k, cfg.learning_rate, cfg.reg, print_every=cfg.print_every, debug=cfg.debug,
                          outdir=cfg.outdir, log=lambda m: log0(rank, m), on_event=jlog, fault=fault, **train_kw)
            st = s1 if st is None else st
            if st is not s1:
                st.seconds += s1.seconds
                st.steps += s1.steps
                st.images += s1.images
                st.losses += s1.losses
                st.evals += s1.evals
                st.best, st.stopped, st.stop_index = s1.best, s1.stopped, s1.stop_index
                st.plateau = s1.plateau
            done += k
            if cfg.keep_best and s1.stopped:  # the device's rule stopped and the host has seen it
                done += s1.steps // max(1, tr.steps_per_epoch()) - k  # (the epochs this segment really ran)
                break
            if cfg.ckpt_dir and done < cfg.num_epochs:
                if rank == 0:
                    save_checkpoint(nn, cfg.ckpt_dir, meta=ckpt_meta(done), optim_state=ckpt_optim(),
                                    best=ckpt_best(), ema=ckpt_ema())
                    jlog({"event": "checkpoint", "dir": cfg.ckpt_dir, "epochs": done})
                comm.barrier()
            if k == 0:
                break
        out.update(par_seconds=st.seconds, images_per_sec=st.images_per_sec, engine_path=tr.engine.path,
                   allreduce=tr.allreduce_impl)
        if cfg.keep_best:
            epochs_run = st.steps // max(1, tr.steps_per_epoch())
            bs = tr.best_state()
            if bs["stopped"]:
                log0(rank, f"Early stop: evaluation {bs['stop_index']} was non-improving number "
                           f"{bs['patience'] + 1} in a row; {epochs_run} epoch(s) run in this call")
                jlog({"event": "early_stop", "stop_index": bs["stop_index"], "patience": bs["patience"],
                      "epochs_run": epochs_run, "iter": tr.iter})
            if cfg.restore_best and bs["best_index"] >= 0:
                tr.restore_best()  # every rank: before the precision, the predictions and the final checkpoint
            log0(rank, f"Best evaluation: index {bs['best_index']} (iteration {bs['iter']}), {bs['monitor']} = "
                       f"{bs['best_metric']:.10g}" + (" -- restored" if cfg.restore_best and bs['best_index'] >= 0
                                                     else ""))
            jlog({"event": "best", "index": bs["best_index"], "iter": bs["iter"], "metric": bs["best_metric"],
                  "monitor": bs["monitor"], "evals": bs["evals"], "stopped": bs["stopped"],
                  "restored": bool(cfg.restore_best and bs["best_index"] >= 0),
                  **({k: st.best[k] for k in ("epoch", "loss", "accuracy")} if st.best else {})})
            out.update(best_index=bs["best_index"], best_metric=bs["best_metric"], stopped=bs["stopped"])
        if ema is not None:
            es = tr.ema_state()
            if cfg.use_ema:
                tr.adopt_ema()  # every rank: before the precision, the predictions and the final checkpoint
            log0(rank, f"Weight averaging: decay {es['decay']:.10g}" + (" with warmup" if es["warmup"] else "")
                 + f", {es['t']} update(s) averaged" + (" -- adopted" if cfg.use_ema else ""))
            jlog({"event": "ema", "decay": es["decay"], "warmup": es["warmup"], "t": es["t"],
                  "adopted": bool(cfg.use_ema)})
            out.update(ema_t=es["t"])
        if plateau is not None:
            ps = tr.plateau_state()
            log0(rank, f"Plateau rule ({plateau.monitor}): scale {ps['scale']:.10g} after {ps['reductions']} "
                       f"reduction(s) in {ps['evals']} evaluation(s), best {ps['best']:.10g}")
            jlog({"event": "plateau", "scale": ps["scale"], "reductions": ps["reductions"], "evals": ps["evals"],
                  "best": ps["best"], "last_reduced_index": ps["last_reduced_index"], "monitor": plateau.monitor})
            out.update(lr_scale=ps["scale"], lr_reductions=ps["reductions"])
        if tr.profiler is not None:
            phases = tr.profiler.summary()
            out["profile"] = phases
            log0(rank, f"Per-step phases (eager, mean): {tr.profiler.format()}")
            jlog({"event": "profile", "phases": phases})
        log0(rank, f"Time for Parallel Training: {st.seconds:.6f} seconds ({st.images_per_sec:,.0f} images/s, "
                   f"engine path {tr.engine.path})")
        if rank == 0:
            out["par_dev_precision"] = precision(tr.predict(ds.x_dev), ds.y_dev)
            log0(rank, f"Precision on validation set for parallel training = {out['par_dev_precision']}")
            pred = tr.predict(ds.x_test)
            if cfg.num_classes <= 10:
                save_label(os.path.join(cfg.outdir, "Pred_testset.txt"), pred)
            else:  # (the reference's format concatenates single digits: one label per line instead)
                np.savetxt(os.path.join(cfg.outdir, "Pred_testset.txt"), np.asarray(pred, np.int64), fmt="%d")
            if ds.y_test is not None:
                out["par_test_precision"] = precision(pred, ds.y_test)
            if cfg.ckpt_dir:
                save_checkpoint(nn, cfg.ckpt_dir, meta=ckpt_meta(done), optim_state=ckpt_optim(), best=ckpt_best(),
                                ema=ckpt_ema())
            if (cfg.grade or cfg.debug) and cfg.run_seq:
                log0(rank, "\nGrading mode on. Checking for correctness")
                out["correct"] = checkNNErrors(seq_nn, nn, os.path.join(cfg.outdir, "NNErrors.txt"))
        jlog({"event": "summary", **{k: v for k, v in out.items() if isinstance(v, (int, float, str, bool))}})
        comm.barrier()
        return out
    except BaseException as ex:
        # failure detection: report, then leave without waiting on peers -- torchrun's agent (or the
        # collective timeout) takes the rest of the job down instead of leaving it hung
        import traceback

        traceback.print_exc()
        print(f"[rank {rank}] FATAL: {type(ex).__name__}: {ex}", file=sys.stderr, flush=True)
        jlog({"event": "fatal", "rank": rank, "error": f"{type(ex).__name__}: {ex}"})
        jlog.close()
        sys.stderr.flush()
        sys.stdout.flush()
        os._exit(3)
    finally:
        jlog.close()
        shutdown()


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = parse_config(argv)
    from .parallel.launcher import PlacementError, self_launch

    try:  # --gpus N and no launcher: run the N ranks (a child launcher) and return their status
        rc = self_launch(cfg.gpus, argv, module="cme213_sp18_amd.train", need_gpus=False)
    except PlacementError as ex:
        print(f"error: {ex}", file=sys.stderr, flush=True)
        return 2
    if rc is not None:
        return rc
    out = run(cfg)
    if out and int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps({k: (float(v) if isinstance(v, (np.floating,)) else v) for k, v in out.items()}))
    return 0 if out.get("correct", True) else 1


if __name__ == "__main__":
    sys.exit(main())
