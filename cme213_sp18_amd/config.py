"""Training configuration: the reference's getopt flags, grade presets and the
BASELINE configs as named presets.

Reference flags (fpcode/main.cpp:58-109): ``-n num_neuron -r reg -l lr -e epochs
-b batch -g grade -p print_every -s (run sequential) -d (debug)``; grade presets
1-3 override them (fpcode/main.cpp:113-152) and grade 4 runs the GEMM benchmark
(fpcode/main.cpp:154-161).
"""
from __future__ import annotations

import argparse
import dataclasses


@dataclasses.dataclass
class TrainConfig:
    num_neuron: int = 1000      # -n  (main.cpp:63)
    reg: float = 1e-4           # -r
    learning_rate: float = 1e-3  # -l
    num_epochs: int = 20        # -e
    batch_size: int = 800       # -b
    grade: int = 0              # -g
    print_every: int = 0        # -p
    run_seq: bool = False       # -s
    debug: bool = False         # -d
    # --- MI355X engine options (not in the reference)
    dtype: str = "f32"          # f32 | f64 | bf16
    path: str = "auto"          # auto | split3 | split1 | mfma
    backend: str = "hip"        # hip (gfx950 kernels) | torch (plain PyTorch ops; CPU capable)
    data: str = "synthetic"     # synthetic | mnist
    data_dir: str = "data"
    normalize: bool = False     # reference feeds raw 0..255 pixels (mnist.cpp:26-31)
    num_train: int = 60000
    num_test: int = 10000
    seed: int = 0
    outdir: str = "Outputs"
    ckpt_dir: str = ""
    resume: str = ""
    use_graphs: bool = True
    softmax_shift: bool = True
    ckpt_precision: int = 12
    allreduce: str = "auto"     # auto | xgmi (one-shot peer kernel, SGD fused) | xgmi2 (two-shot, sharded SGD) | rccl
    comm_timeout: float = 300.0  # seconds before a stuck collective fails the job
    fault_inject: str = ""      # "rank:step" -- raise on that rank at that step (failure-detection test hook)
    log_json: str = ""          # rank-0 JSON-lines event log
    ckpt_every: int = 0         # epochs between checkpoints (needs --ckpt-dir); 0 = only at the end
    profile: bool = False       # per-phase event timing + roctx ranges (eager steps), summary at the end
    overlap_chunks: int = 0     # RCCL path: dW1 all-reduce row chunks overlapped with the backward (0 = auto)
    parallel: str = "dp"        # dp (reference scheme) | tp (hidden-dimension tensor parallel, wide layers)
    num_classes: int = 10       # --classes: output classes (up to 64); labels must lie in [0, classes)
    eval_every: int = 0         # --eval-every N: evaluate the resident dev split on the device every N epochs (dp)
    shuffle_seed: int | None = None  # --shuffle-seed S: reshuffle the resident training set on the device every epoch
    balance_classes: bool = False  # --balance-classes: draw every epoch with replacement, every class equally often
    sample_weights: str = ""    # --sample-weights FILE.npy: ... with per-sample weights (sampling.Weighted)
    sampler_seed: int = 0       # --sampler-seed S
    augment_shift: int | None = None    # --augment-shift M: move every training image by up to M pixels per epoch
    augment_shift_y: int | None = None  # --augment-shift-y: the vertical bound (default: M)
    augment_seed: int = 0       # --augment-seed S
    augment_rotate: float | None = None  # --augment-rotate DEG: rotate every training image by up to DEG per epoch
    augment_scale: str = ""     # --augment-scale LO[:HI]: scale it by a factor in [LO, HI]
    augment_shear: float | None = None   # --augment-shear DEG: shear it by up to DEG
    augment_table: int = 1024   # --augment-table T: the number of distinct transforms (augment.Affine)
    augment_warp: float | None = None    # --augment-warp ALPHA: elastic distortion, nodes moved by up to ALPHA pixels
    augment_warp_grid: str = ""  # --augment-warp-grid G or GYxGX: the cells per axis of its lattice (augment.Warp)
    image_shape: str = ""       # --image-shape HxW: the images' rows x columns (default: 28x28, the square of 784)
    gpus: int = 0               # ranks (one per GPU); 0 = WORLD_SIZE of the launcher, else 1.  N > 1 without a
                                # launcher: the CLI starts the N ranks itself (parallel/launcher.self_launch)
    optimizer: str = "sgd"      # --optimizer sgd | momentum | adam (optim.Optimizer; sequential and parallel run alike)
    momentum: float = 0.9       # --momentum
    nesterov: bool = False      # --nesterov
    beta1: float = 0.9          # --beta1
    beta2: float = 0.999        # --beta2
    adam_eps: float = 1e-8      # --adam-eps
    lr_schedule: str = ""       # --lr-schedule constant | step | exp | linear | cosine (optim.Schedule); "": none
    lr_gamma: float = 1.0       # --lr-gamma (step, exp)
    lr_step_size: int = 1       # --lr-step-size (step)
    lr_total: int = 1           # --lr-total (linear, cosine)
    lr_end_factor: float = 1.0  # --lr-end-factor (linear)
    lr_min_factor: float = 0.0  # --lr-min-factor (cosine)
    lr_unit: str = "step"       # --lr-unit step | epoch
    warmup: int = 0             # --warmup: linear warm-up over that many units (needs --lr-schedule)
    warmup_start: float = 0.0   # --warmup-start: the factor of the first unit
    clip_norm: float | None = None  # --clip-norm: clip the gradient's global norm (torch's clip_grad_norm_)
    keep_best: str = ""         # --keep-best loss | accuracy: keep the best evaluation's weights on the device (dp)
    patience: int | None = None  # --patience N: stop after N + 1 non-improving evaluations in a row (needs --keep-best)
    min_delta: float = 0.0      # --min-delta D: an evaluation improves only by more than D
    stop_check_every: int = 0   # --stop-check-every K: the host looks at the stop flag after every K-th evaluated epoch
    restore_best: bool = False  # --restore-best: the best weights become the final ones (outputs and checkpoint)
    ema: float | None = None    # --ema DECAY: keep an exponential moving average of the weights (csrc/mlp/ema.h; dp)
    ema_warmup: bool = False    # --ema-warmup: the decay of update t is min(DECAY, (1 + t) / (10 + t))
    eval_weights: str = ""      # --eval-weights ema | current: the weights --eval-every reads ("": ema when averaging)
    use_ema: bool = False       # --use-ema: the averaged weights become the final ones (outputs and checkpoint)
    lr_plateau: float | None = None  # --lr-plateau FACTOR: reduce the rate on a validation plateau (optim.Plateau; dp)
    plateau_patience: int = 10  # --plateau-patience: non-improving evaluations tolerated before a reduction
    plateau_threshold: float = 1e-4   # --plateau-threshold
    plateau_threshold_mode: str = "rel"  # --plateau-threshold-mode rel | abs
    plateau_cooldown: int = 0   # --plateau-cooldown: evaluations not counted after a reduction
    plateau_min_factor: float = 0.0   # --plateau-min-factor: the scale's lower bound
    plateau_monitor: str = "loss"     # --plateau-monitor loss | accuracy

    @property
    def schedule(self):
        """The optim.Schedule of the --lr-* flags, or None."""
        from .optim import Schedule

        if not self.lr_schedule:
            return None
        kind = {"exp": "exponential"}.get(self.lr_schedule, self.lr_schedule)
        return Schedule(kind, unit=self.lr_unit, warmup=self.warmup, warmup_start=self.warmup_start,
                        size=self.lr_step_size, gamma=self.lr_gamma, total=self.lr_total,
                        end_factor=self.lr_end_factor, min_factor=self.lr_min_factor)

    @property
    def plateau(self):
        """The optim.Plateau of the --lr-plateau / --plateau-* flags, or None."""
        from .optim import Plateau

        if self.lr_plateau is None:
            return None
        return Plateau(float(self.lr_plateau), self.plateau_patience, self.plateau_threshold,
                       self.plateau_threshold_mode, self.plateau_cooldown, self.plateau_min_factor,
                       monitor=self.plateau_monitor)

    @property
    def ema_rule(self):
        """The optim.Ema of the --ema flags, or None."""
        from .optim import Ema

        return Ema(float(self.ema), bool(self.ema_warmup)) if self.ema is not None else None

    @property
    def augment(self):
        """The augment.Shift of the --augment-* flags -- with a transform flag (--augment-rotate / -scale / -shear) the
        augment.Affine, with a warp flag (--augment-warp / --augment-warp-grid) the augment.Warp over that map -- or
        None."""
        from .augment import Affine, Shift, Warp

        if self.augment_shift is None and not self.augment_affine and not self.augment_elastic:
            return None
        h, w = parse_image_shape(self.image_shape) if self.image_shape else (None, None)
        if self.augment_elastic:
            aug = Warp(4.0 if self.augment_warp is None else self.augment_warp,
                       parse_warp_grid(self.augment_warp_grid) if self.augment_warp_grid else 3,
                       self.augment_rotate or 0.0, parse_scale(self.augment_scale) if self.augment_scale else 1.0,
                       self.augment_shear or 0.0, self.augment_shift or 0, self.augment_shift_y, h, w,
                       self.augment_seed, self.augment_table)
            aug.shape(self.H[0])
            return aug
        if self.augment_affine:
            aug = Affine(self.augment_rotate or 0.0, parse_scale(self.augment_scale) if self.augment_scale else 1.0,
                         self.augment_shear or 0.0, self.augment_shift or 0, self.augment_shift_y, h, w,
                         self.augment_seed, self.augment_table)
            aug.shape(self.H[0])
            return aug
        aug = Shift(self.augment_shift, self.augment_shift_y, h, w, self.augment_seed)
        aug.shape(self.H[0])
        return aug

    @property
    def sampler(self):
        """The sampling.Balanced of --balance-classes or the sampling.Weighted of --sample-weights, or None."""
        from .sampling import Balanced, Weighted

        if self.balance_classes:
            return Balanced(self.sampler_seed)
        if self.sample_weights:
            import numpy as np

            return Weighted(np.load(self.sample_weights, allow_pickle=False), self.sampler_seed,
                            source=self.sample_weights)
        return None

    @property
    def augment_affine(self) -> bool:
        """Whether a transform flag makes the policy an augment.Affine."""
        return self.augment_rotate is not None or bool(self.augment_scale) or self.augment_shear is not None

    @property
    def augment_elastic(self) -> bool:
        """Whether a warp flag makes the policy an augment.Warp."""
        return self.augment_warp is not None or bool(self.augment_warp_grid)

    @property
    def optim(self):
        from .optim import Optimizer

        return Optimizer(self.optimizer, momentum=self.momentum, nesterov=self.nesterov, beta1=self.beta1,
                         beta2=self.beta2, eps=self.adam_eps)

    @property
    def H(self):
        return [784, self.num_neuron, self.num_classes]


def parse_image_shape(spec: str) -> tuple[int, int]:
    """'HxW' -> (H, W), both >= 1."""
    parts = spec.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts) or int(parts[0]) < 1 or int(parts[1]) < 1:
        raise ValueError(f"--image-shape must be HxW with positive integers (got {spec!r})")
    return int(parts[0]), int(parts[1])


def parse_scale(spec: str) -> tuple[float, float]:
    """'LO' or 'LO:HI' -> (lo, hi)."""
    parts = spec.split(":")
    try:
        vals = [float(p) for p in parts]
    except ValueError:
        vals = []
    if len(vals) not in (1, 2):
        raise ValueError(f"--augment-scale must be LO or LO:HI (got {spec!r})")
    return vals[0], vals[-1]


def parse_warp_grid(spec: str):
    """'G' or 'GYxGX' -> G or (gy, gx)."""
    parts = spec.lower().split("x")
    if len(parts) not in (1, 2) or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"--augment-warp-grid must be G or GYxGX (got {spec!r})")
    return int(parts[0]) if len(parts) == 1 else (int(parts[0]), int(parts[1]))


# fpcode/main.cpp:113-152 -- "DO NOT change the following parameters"
GRADE_PRESETS = {
    1: dict(reg=1e-4, learning_rate=0.001, num_epochs=40, batch_size=800, num_neuron=100, run_seq=True,
            debug=True, print_every=0),
    2: dict(reg=1e-4, learning_rate=0.01, num_epochs=10, batch_size=800, num_neuron=100, run_seq=True,
            debug=True, print_every=0),
    3: dict(reg=1e-4, learning_rate=0.025, num_epochs=1, batch_size=800, num_neuron=100, run_seq=True,
            debug=True, print_every=1),
}

# BASELINE.json configs
NAMED_PRESETS = {
    "cpu_plumbing": dict(num_neuron=100, batch_size=800, backend="torch", dtype="f64", run_seq=True),
    "1gpu_fp32": dict(num_neuron=100, batch_size=800, dtype="f32"),
    "4gpu_rccl": dict(num_neuron=100, batch_size=800, dtype="f32", allreduce="rccl"),
    "8gpu_wide": dict(num_neuron=4096, batch_size=6400, dtype="f32"),
    "8gpu_bf16": dict(num_neuron=1024, batch_size=800, dtype="bf16"),
}


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cme213_sp18_amd.train",
                                 description="2-layer MLP training on MI355X (CME213 final-project CLI)")
    ap.add_argument("-n", "--hidden", dest="num_neuron", type=int)
    ap.add_argument("-r", dest="reg", type=float)
    ap.add_argument("-l", dest="learning_rate", type=float)
    ap.add_argument("-e", dest="num_epochs", type=int)
    ap.add_argument("-b", dest="batch_size", type=int)
    ap.add_argument("-g", dest="grade", type=int)
    ap.add_argument("-p", dest="print_every", type=int)
    ap.add_argument("-s", dest="run_seq", action="store_true", default=None)
    ap.add_argument("-d", dest="debug", action="store_true", default=None)
    ap.add_argument("--preset", choices=sorted(NAMED_PRESETS))
    ap.add_argument("--dtype", choices=["f32", "f64", "bf16"])
    ap.add_argument("--path", choices=["auto", "split3", "split1", "mfma"])
    ap.add_argument("--backend", choices=["hip", "torch"])
    ap.add_argument("--data", choices=["synthetic", "mnist"])
    ap.add_argument("--data-dir")
    ap.add_argument("--normalize", action="store_true", default=None)
    ap.add_argument("--num-train", type=int)
    ap.add_argument("--num-test", type=int)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--outdir")
    ap.add_argument("--ckpt-dir")
    ap.add_argument("--resume")
    ap.add_argument("--no-graphs", dest="use_graphs", action="store_false", default=None)
    ap.add_argument("--no-softmax-shift", dest="softmax_shift", action="store_false", default=None)
    ap.add_argument("--ckpt-precision", type=int)
    ap.add_argument("--allreduce", choices=["auto", "xgmi", "xgmi2", "rccl", "host"])
    ap.add_argument("--comm-timeout", type=float)
    ap.add_argument("--fault-inject", help="rank:step")
    ap.add_argument("--log-json")
    ap.add_argument("--ckpt-every", type=int)
    ap.add_argument("--profile", action="store_true", default=None,
                    help="time forward+head / weight gradients / all-reduce / SGD per step (eager) and emit roctx "
                         "ranges for rocprofv3 --marker-trace")
    ap.add_argument("--parallel", choices=["dp", "tp"],
                    help="dp: data parallel (default); tp: shard the hidden layer over the ranks (one z2 all-reduce "
                         "per step, every rank runs the whole global batch)")
    ap.add_argument("--classes", dest="num_classes", type=int,
                    help="output classes, 1..64 (default 10; e.g. 26 / 47 / 62 for the EMNIST splits): the layer sizes "
                         "become 784-H-N, synthetic data gets N classes, and labels read with --data must lie in "
                         "[0, N)")
    ap.add_argument("--eval-every", type=int,
                    help="keep the dev split resident on the device and evaluate it there after every N epochs "
                         "(loss, accuracy, confusion matrix; `eval` events in --log-json); 0 = never (default)")
    ap.add_argument("--shuffle-seed", type=int,
                    help="reshuffle the resident training set on the device before every epoch (sequential and "
                         "parallel run alike; the order depends on the seed and the iteration counter only, so "
                         "--resume continues the sequence); default: the loaded order every epoch")
    ap.add_argument("--balance-classes", action="store_true", default=None,
                    help="draw every epoch's N training samples with replacement on the device, each with weight "
                         "1 / (its class's count), so that every class is seen equally often (sequential and parallel "
                         "run alike; the draws depend on --sampler-seed and the iteration counter only, so --resume "
                         "continues the sequence); not with --shuffle-seed")
    ap.add_argument("--sample-weights", metavar="FILE.npy",
                    help="the same with per-sample weights: a vector of one non-negative weight per training sample")
    ap.add_argument("--sampler-seed", type=int, help="seed of the draws (default 0)")
    ap.add_argument("--augment-shift", type=int,
                    help="before every epoch move each training image by its own random (dx, dy), |dx| and |dy| <= M, "
                         "on the device (zeros move in; sequential and parallel run alike; the shifts depend on the "
                         "seed, the iteration counter and the sample only, so --resume continues the sequence); "
                         "default: no augmentation")
    ap.add_argument("--augment-shift-y", type=int, help="the vertical bound of --augment-shift (default: M)")
    ap.add_argument("--augment-seed", type=int, help="seed of the shifts (default 0)")
    ap.add_argument("--augment-rotate", type=float,
                    help="before every epoch rotate each training image about its centre by its own random angle, "
                         "|angle| <= DEG (0..180), resampled bilinearly on the device; alone or with --augment-scale / "
                         "--augment-shear / --augment-shift (any of the three makes the policy an affine one)")
    ap.add_argument("--augment-scale", help="LO[:HI]: scale each training image by its own factor in [LO, HI] "
                                            "(1/16 <= LO <= HI <= 16)")
    ap.add_argument("--augment-shear", type=float, help="shear each training image by up to DEG (0..60) per epoch")
    ap.add_argument("--augment-table", type=int,
                    help="the number of distinct transforms the affine policy draws from (default 1024, up to 65536)")
    ap.add_argument("--augment-warp", type=float,
                    help="before every epoch distort each training image elastically: its own smooth random "
                         "displacement field, control nodes moved by up to ALPHA pixels (0..8), on top of whatever "
                         "--augment-rotate / -scale / -shear / -shift give")
    ap.add_argument("--augment-warp-grid",
                    help="G or GYxGX: the cells per axis (1..5) of the elastic distortion's control lattice (default 3)")
    ap.add_argument("--image-shape", help="HxW: rows x columns of the images, H * W = 784 (default 28x28)")
    ap.add_argument("--optimizer", choices=["sgd", "momentum", "adam"],
                    help="the update rule (default sgd, the reference's w -= lr g); momentum and adam keep their state "
                         "on the device and cost one extra launch per step (data parallel only)")
    ap.add_argument("--momentum", type=float, help="momentum coefficient in [0, 1) (default 0.9)")
    ap.add_argument("--nesterov", action="store_true", default=None, help="Nesterov momentum")
    ap.add_argument("--beta1", type=float, help="Adam's first-moment decay (default 0.9)")
    ap.add_argument("--beta2", type=float, help="Adam's second-moment decay (default 0.999)")
    ap.add_argument("--adam-eps", type=float, help="Adam's epsilon (default 1e-8)")
    ap.add_argument("--lr-schedule", choices=["constant", "step", "exp", "linear", "cosine"],
                    help="learning-rate schedule: the rate of applied update t is -l times the schedule's factor "
                         "(sequential and parallel run alike; the device reads the factors, so graphs replay across "
                         "rates; --resume continues the sequence; data parallel only)")
    ap.add_argument("--lr-gamma", type=float, help="decay factor in (0, 1] of step / exp (default 1)")
    ap.add_argument("--lr-step-size", type=int, help="units between two decays of step (default 1)")
    ap.add_argument("--lr-total", type=int, help="units over which linear / cosine run (default 1)")
    ap.add_argument("--lr-end-factor", type=float, help="final factor of linear (default 1)")
    ap.add_argument("--lr-min-factor", type=float, help="final factor of cosine (default 0)")
    ap.add_argument("--lr-unit", choices=["step", "epoch"], help="what the schedule counts (default step)")
    ap.add_argument("--warmup", type=int, help="linear warm-up over that many units before the schedule starts")
    ap.add_argument("--warmup-start", type=float, help="the factor of the first warm-up unit (default 0)")
    ap.add_argument("--clip-norm", type=float,
                    help="clip the gradient's global L2 norm at this value before the update (torch's "
                         "clip_grad_norm_, the regulariser included; formed on the device; data parallel only)")
    ap.add_argument("--keep-best", choices=["loss", "accuracy"],
                    help="behind every --eval-every evaluation decide on the device whether it is the best so far "
                         "(validation loss or accuracy) and keep those weights there; `best` event in --log-json, "
                         "<ckpt>/best/ in checkpoints (data parallel only)")
    ap.add_argument("--patience", type=int,
                    help="early stopping: tolerate N non-improving evaluations in a row and stop on number N + 1 "
                         "(0: the first one); needs --keep-best")
    ap.add_argument("--min-delta", type=float,
                    help="an evaluation counts as an improvement only when it beats the best by more than D (default 0)")
    ap.add_argument("--stop-check-every", type=int,
                    help="the host reads the device's stop flag after every K-th evaluated epoch (a sync and a 64-byte "
                         "read) and ends the run when it is set; 0 = only where the host syncs on the epoch anyway")
    ap.add_argument("--restore-best", action="store_true", default=None,
                    help="after training, make the best weights the current ones: the precision, the predictions and "
                         "the final checkpoint are those of the best evaluation")
    ap.add_argument("--ema", type=float, metavar="DECAY",
                    help="keep an exponential moving average of the weights on the device, folded in after every "
                         "update: e += (1 - DECAY)(p - e), 0 <= DECAY < 1 (torch's get_ema_multi_avg_fn); the "
                         "sequential run (-s) keeps one too; data parallel only")
    ap.add_argument("--ema-warmup", action="store_true", default=None,
                    help="the decay of update t is min(DECAY, (1 + t) / (10 + t)): the early average follows the "
                         "weights instead of their starting point; needs --ema")
    ap.add_argument("--eval-weights", choices=["ema", "current"],
                    help="the weights the --eval-every evaluations (and --keep-best) read: the averaged ones "
                         "(default with --ema) or the current ones")
    ap.add_argument("--use-ema", action="store_true", default=None,
                    help="after training, make the averaged weights the current ones: the precision, the predictions "
                         "and the final checkpoint are those of the average; needs --ema")
    ap.add_argument("--lr-plateau", type=float, metavar="FACTOR",
                    help="reduce the learning rate on a validation plateau (torch's ReduceLROnPlateau), decided on the "
                         "device behind every --eval-every evaluation: after more than --plateau-patience evaluations "
                         "that do not improve, every later update's rate is multiplied by FACTOR (0 < FACTOR < 1), on "
                         "top of --lr-schedule; sequential and parallel run alike; `plateau` event in --log-json; data "
                         "parallel only")
    ap.add_argument("--plateau-patience", type=int, help="non-improving evaluations tolerated (default 10)")
    ap.add_argument("--plateau-threshold", type=float,
                    help="an evaluation improves only when it beats the best by more than this (default 1e-4)")
    ap.add_argument("--plateau-threshold-mode", choices=["rel", "abs"],
                    help="the threshold as a fraction of the best (rel, default) or as a difference (abs)")
    ap.add_argument("--plateau-cooldown", type=int,
                    help="evaluations after a reduction that are not counted (default 0)")
    ap.add_argument("--plateau-min-factor", type=float,
                    help="the lower bound of the accumulated factor, in [0, 1] (default 0)")
    ap.add_argument("--plateau-monitor", choices=["loss", "accuracy"],
                    help="the validation metric the rule watches (default loss)")
    ap.add_argument("--gpus", type=int,
                    help="number of ranks, one per GPU (the reference's mpirun -np N); started here when no "
                         "launcher started this process")
    ap.add_argument("--overlap-chunks", type=int,
                    help="RCCL path: number of dW1 row chunks all-reduced while the backward runs (0 = auto)")
    return ap


def parse_config(argv=None) -> TrainConfig:
    ap = build_parser()
    a = ap.parse_args(argv)
    cfg = TrainConfig()
    explicit = {k: v for k, v in vars(a).items() if v is not None and k != "preset"}
    if a.preset:
        for k, v in NAMED_PRESETS[a.preset].items():
            setattr(cfg, k, v)
    for k, v in explicit.items():
        setattr(cfg, k.replace("-", "_"), v)
    if cfg.gpus <= 0:
        import os

        cfg.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if cfg.grade in GRADE_PRESETS:
        for k, v in GRADE_PRESETS[cfg.grade].items():
            setattr(cfg, k, v)
        # the grading gate is fp64-tight (max-norm rel <= 1e-7, utils/tests.cpp:39): run the
        # fp64 engine unless a dtype was requested explicitly
        if "dtype" not in explicit:
            cfg.dtype = "f64"
    # refused here, before any data is loaded or the sequential run starts: TensorParallelTrainer applies plain SGD only
    if cfg.parallel == "tp" and cfg.optimizer != "sgd":
        ap.error(f"--parallel tp applies plain SGD only; --optimizer {cfg.optimizer} needs --parallel dp")
    if cfg.parallel == "tp" and (cfg.lr_schedule or cfg.clip_norm is not None):
        ap.error("--parallel tp applies plain SGD at one rate only; --lr-schedule / --clip-norm need --parallel dp")
    if not cfg.lr_schedule and any(k.startswith("lr_") or k.startswith("warmup") for k in explicit
                                   if k not in ("lr_schedule", "lr_plateau")):
        ap.error("--lr-gamma, --lr-step-size, --lr-total, --lr-end-factor, --lr-min-factor, --lr-unit, --warmup and "
                 "--warmup-start need --lr-schedule")
    # keeping the best weights acts on the device-side evaluations of the data-parallel trainer
    best_flags = [f for f, on in (("--patience", cfg.patience is not None), ("--min-delta", "min_delta" in explicit),
                                  ("--stop-check-every", "stop_check_every" in explicit),
                                  ("--restore-best", cfg.restore_best)) if on]
    if best_flags and not cfg.keep_best:
        ap.error(f"{', '.join(best_flags)} need(s) --keep-best loss | accuracy")
    if cfg.keep_best and cfg.parallel == "tp":
        ap.error("--keep-best acts on the device-side evaluation, which is data-parallel only; it needs --parallel dp")
    if cfg.keep_best and not cfg.eval_every > 0:
        ap.error("--keep-best acts on the evaluations: it needs --eval-every N > 0")
    if cfg.keep_best and ((cfg.patience is not None and cfg.patience < 0) or cfg.min_delta < 0
                          or cfg.stop_check_every < 0):
        ap.error("--patience, --min-delta and --stop-check-every must be >= 0")
    # weight averaging runs over the whole parameter arena of the data-parallel trainer
    if cfg.ema is not None and cfg.parallel == "tp":
        ap.error("--ema averages the whole parameter arena, which --parallel tp shards; it needs --parallel dp")
    ema_flags = [f for f, on in (("--ema-warmup", cfg.ema_warmup), ("--use-ema", cfg.use_ema),
                                 ("--eval-weights ema", cfg.eval_weights == "ema")) if on]
    if ema_flags and cfg.ema is None:
        ap.error(f"{', '.join(ema_flags)} need(s) --ema DECAY")
    if cfg.use_ema and cfg.restore_best:
        ap.error("--use-ema and --restore-best both choose the final weights: give one of them")
    # the plateau rule acts on the device-side evaluations of the data-parallel trainer
    plateau_flags = sorted("--" + k.replace("_", "-") for k in explicit if k.startswith("plateau_"))
    if plateau_flags and cfg.lr_plateau is None:
        ap.error(f"{', '.join(plateau_flags)} need(s) --lr-plateau FACTOR")
    if cfg.lr_plateau is not None and cfg.parallel == "tp":
        ap.error("--lr-plateau acts on the device-side evaluation and the apply launch, which are data-parallel only; "
                 "it needs --parallel dp")
    if cfg.lr_plateau is not None and not cfg.eval_every > 0:
        ap.error("--lr-plateau acts on the evaluations: it needs --eval-every N > 0")
    if cfg.balance_classes and cfg.sample_weights:
        ap.error("--balance-classes and --sample-weights both choose the sampling weights: give one of them")
    if (cfg.balance_classes or cfg.sample_weights) and cfg.shuffle_seed is not None:
        ap.error("--balance-classes / --sample-weights draw in random order already: not with --shuffle-seed")
    if "sampler_seed" in explicit and not (cfg.balance_classes or cfg.sample_weights):
        ap.error("--sampler-seed needs --balance-classes or --sample-weights")
    if cfg.augment_shift is None and not cfg.augment_affine and not cfg.augment_elastic and any(
            k in explicit for k in ("augment_shift_y", "augment_seed", "image_shape")):
        ap.error("--augment-shift-y, --augment-seed and --image-shape need --augment-shift")
    if "augment_table" in explicit and not cfg.augment_affine and not cfg.augment_elastic:
        ap.error("--augment-table needs --augment-rotate, --augment-scale or --augment-shear")
    try:
        cfg.augment  # the image shape and the bounds (augment.Shift validates)
        cfg.sampler  # (the weights file is read; sampling validates the seed)
        cfg.optim  # the hyper-parameters' ranges (optim.Optimizer validates)
        cfg.schedule
        cfg.ema_rule  # (optim.Ema validates the decay)
        cfg.plateau  # (optim.Plateau validates the ranges)
        from .optim import resolve_policy

        resolve_policy(None, cfg.clip_norm)
    except (ValueError, OSError) as ex:
        ap.error(str(ex))
    return cfg
