"""Device-resident MLP training engine (one per rank).

Replaces the reference's per-batch host<->device shuffle
(fpcode/neural_network.cpp:484-499: X, y and ALL weights uploaded every batch,
all gradients downloaded) and its ``device_cache`` of 18 separate cudaMallocs
(fpcode/inc/gpu_func.h:49-101) with:

* the WHOLE training set uploaded once per GPU in the GEMM dtype (54,000 x 784
  fp32 = 169 MB, a rounding error of 288 GB of HBM), so a batch is a pointer
  offset -- no scatter, no H2D copies;
* one flat parameter arena ``[W1|b1|W2|b2]`` and a gradient bucket with the same
  layout, so a single all-reduce and a single fused SGD kernel cover every
  parameter;
* activations ``a1, dZ1 [H][ld]``, ``D [C][ld]`` sized once for the per-rank
  batch.

Two interchangeable compute backends execute a step:
* ``"hip"``   -- the hand-written gfx950 kernels (csrc/mlp): 3 launches per step.
* ``"torch"`` -- the same math in plain PyTorch ops; the numerics reference for
  the kernels and the backend for CPU-only (gloo) data-parallel tests.
"""
from __future__ import annotations

import types

import numpy as np
import torch

from .._native import DTYPE_CODES, cpu, hip

_ALIGN = 64  # elements; keeps every arena segment 256-byte aligned for f32


def _round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def fragment_order_pixels(x: torch.Tensor) -> torch.Tensor:
    """[N][P] uint8 -> the forward's fragment-ordered copy (csrc/mlp/mma_tile.h ``xs_off``): sample tile s // 16,
    64-k pair k // 64, lane ((k % 64) // 16) * 16 + s % 16, byte k % 16; zero-padded to whole tiles and pairs."""
    n, p = x.shape
    ns, npair = _round_up(n, 16), (p + 63) // 64
    xp = torch.zeros(ns, npair * 64, dtype=torch.uint8, device=x.device)
    xp[:n, :p] = x
    return xp.view(ns // 16, 16, npair, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def fragment_rows_to_rowmajor(buf: torch.Tensor, rows: int, cols: int, kblock: int = 64) -> torch.Tensor:
    """Inverse of the fp32 fragment orders -> a [rows][cols] view.  kblock 64: csrc/mlp/mma_tile.h ``w1s_off`` (row
    tile r // 16, 64-column pair c // 64, load i = (c % 16) // 4, lane ((c % 64) // 16) * 16 + r % 16, element c % 4);
    kblock 32: csrc/mlp/rega_gemm.h ``dzr_off`` (32-column stage c // 32, load h = (c % 8) // 4, lane
    ((c % 32) // 8) * 16 + r % 16, element c % 4)."""
    rt, nb = (rows + 15) // 16, (cols + kblock - 1) // kblock
    v = buf[: rt * 16 * nb * kblock].view(rt, nb, kblock // 16, 4, 16, 4)  # [row tile][block][load][lane grp][r][e]
    return v.permute(0, 4, 1, 3, 2, 5).reshape(rt * 16, nb * kblock)[:rows, :cols]


def param_dtype(dtype: str) -> torch.dtype:
    return torch.float64 if dtype == "f64" else torch.float32


def gemm_dtype(dtype: str) -> torch.dtype:
    return {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}[dtype]


class FlatLayout:
    """Offsets of W1, b1, W2, b2 inside the flat arena (each 64-element aligned), then one STATUS element:
    in the gradient bucket it is 0 for a trusted step and 1 when this rank's forward + head launch timed out
    (csrc/mlp/mlp_split.h SplitStepArgs::gstatus); the all-reduce sums it with the gradients and the SGD
    kernels apply nothing when it is non-zero.  The parameter arena's copy stays 0."""

    def __init__(self, P: int, H: int, C: int):
        self.P, self.H, self.C = P, H, C
        sizes = [H * P, H, C * H, C, 1]
        self.offsets = []
        o = 0
        for s in sizes:
            self.offsets.append(o)
            o += _round_up(s, _ALIGN)
        self.sizes = sizes
        self.total = o
        self.status = self.offsets[4]

    def views(self, flat: torch.Tensor):
        P, H, C = self.P, self.H, self.C
        o = self.offsets
        return (flat[o[0]:o[0] + H * P].view(H, P), flat[o[1]:o[1] + H], flat[o[2]:o[2] + C * H].view(C, H),
                flat[o[3]:o[3] + C])


PATHS = ("auto", "split3", "split1", "mfma")


def fused_allreduce_eligible(backend: str, planes: int, H: int, C: int, device_type: str,
                             bias_feature: bool) -> bool:
    """The all-reduce fused into the weight-gradient launch (MlpEngine.fused_allreduce_slots) applies: HIP split
    path on a GPU, H <= 128, the all-ones XT feature, and at most 16 classes -- its dW2 / db2 exchange tiles are
    16-class, so above that DataParallelTrainer takes the separate xGMI / RCCL / host all-reduce."""
    return bool(backend == "hip" and planes and H <= 128 and C <= 16 and device_type == "cuda" and bias_feature)


def resolve_path(dtype: str, path: str = "auto") -> str:
    """Compute path for a dtype.

    * ``split3`` (f32 default): fp32 parameters, GEMMs on bf16 MFMA over an EXACT
      3-plane bf16 split of the fp32 operands (csrc/mlp/mlp_split.h); needs inputs
      that are exact in bf16 (raw 0..255 pixels).  2 kernels per step.
    * ``split1`` (bf16 default): the same kernels with single bf16 planes (mixed precision).
    * ``mfma``: plain f32 / f64 MFMA kernels (csrc/mlp/mlp_kernels.hip); the f64 parity
      path and the f32 path for non-integer (normalised) inputs.  3 kernels per step.
    """
    if path not in PATHS:
        raise ValueError(f"path must be one of {PATHS}")
    if path == "auto":
        return {"f32": "split3", "bf16": "split1", "f64": "mfma"}[dtype]
    if path.startswith("split") and dtype == "f64":
        raise ValueError("the split-bf16 path has fp32 parameters; use path='mfma' for f64")
    return path


class MlpEngine:
    def __init__(self, H=(784, 100, 10), dtype: str = "f32", max_cols: int = 800, device=None,
                 backend: str = "hip", shift: bool = True, feature_major_copy: bool = True, path: str = "auto"):
        if dtype not in DTYPE_CODES:
            raise ValueError(f"dtype must be one of {list(DTYPE_CODES)}")
        self.P, self.H, self.C = (int(h) for h in H)
        self.dtype = dtype
        self.path = resolve_path(dtype, path)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        if backend == "hip" and self.device.type != "cuda":
            raise RuntimeError("the 'hip' backend needs a GPU; use backend='torch' on CPU")
        self.backend = backend
        self.shift = bool(shift)
        self.pdt = param_dtype(dtype)
        self.layout = FlatLayout(self.P, self.H, self.C)
        dev = self.device
        self.params = torch.zeros(self.layout.total, dtype=self.pdt, device=dev)
        self.grads = torch.zeros(self.layout.total, dtype=self.pdt, device=dev)
        self.W1, self.b1, self.W2, self.b2 = self.layout.views(self.params)
        self.gW1, self.gb1, self.gW2, self.gb2 = self.layout.views(self.grads)
        self.status_index = self.layout.status  # the gradient bucket's status element (FlatLayout)
        self.X = None
        self.Xw = self.XTw = None  # wide-layer bf16 copies (load_dataset)
        self.XT = None
        self.Xs = None  # the pixels in the forward's fragment order (load_dataset)
        self.labels = None
        # the pristine rows as loaded (load_dataset(keep_source=True)): what enqueue_shuffle gathers from
        self.X0 = self.labels0 = self._perm = None
        self.shuffle_launches = 0  # shuffle kernel launches enqueued (0: the kernel was never loaded)
        # the augmenting gather (enqueue_augment): its launches, and the (dx, dy) of every resident sample -- allocated
        # by the first augmentation, so a run without one holds nothing
        self.augment_launches = 0
        self._shifts = None
        # the affine gather (enqueue_augment with an augment.Affine): its launches, the table index of every resident
        # sample and the uploaded table {policy, device int32 [T][4]} -- allocated by prepare_augment / the first use
        self.affine_launches = 0
        self._transforms = self._affine_table = None
        # the warping gather (enqueue_augment with an augment.Warp): its launches and the uploaded axis tables
        # {(grid, h, w), device int32 [h + w][5]} -- it shares the shifts, the transforms and the table above
        self.warp_launches = 0
        self._warp_axes = None
        # sampling with replacement (enqueue_shuffle / enqueue_augment with a sampling policy): the uploaded alias table
        # {policy, host uint32 [N][2], its device copy} -- None without a sampler: nothing allocated, nothing changed
        self._sampler = None
        self._eval = None  # the resident validation set and its evaluation buffers (load_eval)
        self._normalize = False
        self.xscale = 1.0
        # keep a second, feature-major copy of the dataset ([P][N]) so the dW1 GEMM
        # reads its B operand K-contiguous (16-byte loads); +1x dataset bytes, which
        # is nothing next to 288 GB of HBM.
        self.feature_major_copy = bool(feature_major_copy) or self.path.startswith("split")
        self._configure_path()
        self._alloc_acts(max_cols)
        self._step = None
        self._xgmi_fuse = None
        # H <= 128 split path: the forward + head launch in its all-gather form (every workgroup of the
        # launch must be resident at once; DataParallelTrainer turns it off when processes share a GPU)
        self.fh_allgather = True
        self.store_a1 = True
        # wide split3 layers: the in-place W1 update skips the W1-plane refresh when no forward reads the planes
        # (MlpStep.lazy_planes; they are re-split before one that does)
        # (measured at 784-4096-10 fp32: step 58.0 -> 55.2 us, profiles/wide_ag_ab_lazy_planes_r3.jsonl)
        self.lazy_planes = True
        self._ag_test_skip, self._ag_wait_us = -1, 50_000  # inject_handoff_timeout (tests); 50 ms default
        self.kpart = None  # split-K dW1 slabs (enable_splitk)
        # the update rule of apply() (set_optimizer): None = plain SGD, no state; else the state buffers and the
        # device-resident counter records of a stateful optimizer
        self.optimizer, self.opt_bufs, self.opt_rec = None, [], None
        # the update policy of apply() (set_update_policy): a learning-rate schedule (optim.Schedule) and / or a
        # gradient-norm threshold.  With either set, every update -- plain SGD's too, as the stateless kSgd rule -- goes
        # through the apply launch: the schedule window {t0, n, f[0 .. n)} and its host copy, the sum-of-squares
        # partials (csrc/mlp/clip.h) and the last-update record {t, lr_t, grad_norm, clip_coef}
        self.schedule, self.clip_norm = None, 0.0
        self.sched_win = self._win_host = self.clip_partials = self.opt_last = None
        # keeping the best validation weights (enable_keep_best): None = nothing allocated, nothing launched; else the
        # rule, the best arena, the per-workgroup records (csrc/mlp/best.h) and, for data parallel, the [R][3] rows
        self._best = None
        # reducing the rate on a validation plateau (set_plateau): None = nothing allocated, nothing launched; else the
        # rule (optim.Plateau), the ONE record of 8 doubles (csrc/mlp/plateau.h) whose scale word the apply launch reads
        # and, for data parallel, the [R][3] rows of a decision
        self._plateau = None
        # an exponential moving average of the parameters (set_ema): None = nothing allocated, nothing launched; else
        # the rule, the averaged arena, the per-workgroup records (csrc/mlp/ema.h) and, once an evaluation has read the
        # average, its own derived copies of W1 and (split paths) the MlpStep bound to them
        self._ema = None

    def _configure_path(self):
        dev = self.device
        self.np = {"split3": 3, "split1": 1}.get(self.path, 0)
        if self.np:
            self.gdt = torch.bfloat16
            self.W1p = torch.zeros(self.np, self.H, self.P, dtype=torch.bfloat16, device=dev)
            self.W1g = self.W1  # the torch backend reads the (exact) fp32 master
        else:
            self.gdt = gemm_dtype(self.dtype)
            self.W1p = None
            self.W1g = (torch.zeros(self.H, self.P, dtype=torch.bfloat16, device=dev)
                        if self.dtype == "bf16" else self.W1)

    # ------------------------------------------------------------------ setup
    def _alloc_acts(self, max_cols: int):
        self.ld = _round_up(max(int(max_cols), 1), 16)
        dev, H, C, ld = self.device, self.H, self.C, self.ld
        self.a1 = torch.zeros(H, ld, dtype=self.pdt, device=dev)
        self.dZ1 = torch.zeros(H, ld, dtype=self.pdt, device=dev)
        self.D = torch.zeros(C, ld, dtype=self.pdt, device=dev)
        if self.np:
            self.dZ1p = torch.zeros(self.np, H, ld, dtype=torch.bfloat16, device=dev)
            self.dZ1g = self.dZ1
        else:
            self.dZ1p = None
            self.dZ1g = torch.zeros(H, ld, dtype=torch.bfloat16, device=dev) if self.dtype == "bf16" else self.dZ1
        # wide layers: scratch for the split-H z2 partial sums of the two-kernel head
        self.z2buf = self.dw2buf = None
        # (both are 16-class layouts: above 16 classes the many-class head forms z2 itself, csrc/mlp/head_mc.hip)
        if self.backend == "hip" and H >= 512 and self.pdt == torch.float32 and C <= 16:
            self.z2buf = torch.zeros(int(hip().head_big_scratch_floats(H, ld)), dtype=torch.float32, device=dev)
            # dW2 partials the wide head leaves per 32-column tile ([tile][16][H]) for the weight-gradient launch
            self.dw2buf = torch.zeros((ld + 31) // 32 * 16 * H, dtype=torch.float32, device=dev)
        elif self.backend == "hip" and self.np and H <= 128 and C <= 16:
            # ... and the H <= 128 all-gather forward + head (MlpStep.head_dw2: two 16-column partials per tile)
            self.dw2buf = torch.zeros((ld + 31) // 32 * 2 * 16 * H, dtype=torch.float32, device=dev)
        nblk = (ld + 15) // 16
        self.loss_buf = torch.zeros(max(nblk, 1), dtype=torch.float32, device=dev)
        # split path, H <= 128: forward GEMM + head in one launch (mlp_fwd1_head); one uint32
        # counter per 32-column a1 tile tells the last row-tile workgroup to run the head
        self.fh_counters = None
        self.ag_counters = self.ag_slabs = self.ag_err = self.ag_gran = self.W1s = self.dZ1s = None
        if self.backend == "hip" and self.np and H <= 128 and C <= 16:
            tiles = (ld + 31) // 32
            self.fh_counters = torch.zeros(tiles, dtype=torch.int32, device=dev)
            # all-gather form (mlp_fwd1_head_ag): monotonic uint64 tile counters (the launch epoch), z2 partial
            # granules {value, epoch} [tile][8 row tiles][16 classes][32 columns], and the timed-out-poll word
            self.ag_counters = torch.zeros(tiles * 32, dtype=torch.int64, device=dev)  # one 256-B line each
            self.ag_slabs = torch.zeros(tiles * 8 * 16 * 32, dtype=torch.int64, device=dev)
            self.ag_err = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.np == 3:  # the forward's fragment-ordered fp32 copy of W1 (MlpStep.w1_swz)
                self.W1s = torch.zeros(int(hip().mlp_split_w1s_floats(H, self.P)), dtype=torch.float32, device=dev)
                # ... and dZ1 in the weight-gradient GEMM's fragment order (MlpStep.dz_swz)
                self.dZ1s = torch.zeros(int(hip().mlp_split_w1s_floats(H, ld)), dtype=torch.float32, device=dev)
        elif self.backend == "hip" and self.np and H >= 512 and C <= 16 and self.dw2buf is not None:
            # wide layers: the all-gather head fused into the forward launch (mlp_fwd1_wide_ag) uses one
            # monotonic counter per column tile -- a separate array per tiling (128 x 128 / 64 x 64) -- and
            # the timed-out-wait word
            tiles = (ld + 31) // 32
            if self.np == 3:  # fp32 dZ1 in the A-in-registers dW1 K loop's fragment order (MlpStep.dz_swz)
                self.dZ1s = torch.zeros((H + 15) // 16 * 16 * ((ld + 31) // 32 * 32), dtype=torch.float32, device=dev)
            self.ag_counters = torch.zeros(2 * tiles * 32, dtype=torch.int64, device=dev)
            self.ag_err = torch.zeros(1, dtype=torch.int32, device=dev)
            # its hand-off granules: 8-byte {value, epoch} z2 partials [H/64][16][ld] and D [16][ld] (tags only
            # grow, so the buffer is never re-zeroed)
            self.ag_gran = torch.zeros(((H + 63) // 64 * 16 + 16) * ld, dtype=torch.int64, device=dev)
        self._step = None

    def load_dataset(self, x, labels, normalize: bool = False, keep_source: bool = False):
        """Upload the training set once ([N][P] uint8 or float) and keep it resident.

        ``keep_source``: also keep a pristine copy of the rows and labels as loaded (``X0`` / ``labels0``, in the
        resident dtype) and an int32 order buffer, so that enqueue_shuffle can rewrite the layouts in another order.

        Split paths keep the RAW uint8 pixels (1 byte/element; widened to bf16
        exactly inside the GEMM kernels, normalisation folded into the epilogues
        as ``xscale``), plus a feature-major uint8 copy for the dW1 GEMM.  The
        mfma path stores the (optionally normalised) values in the GEMM dtype.
        """
        x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        if x.ndim != 2 or x.shape[1] != self.P:
            raise ValueError(f"expected [N][{self.P}] samples, got {tuple(x.shape)}")
        xd = x.to(self.device)
        self._normalize = bool(normalize)
        if self.np:
            raw = xd.to(torch.float32)
            exact = bool(((raw == raw.round()) & (raw >= 0) & (raw <= 255)).all().item())
            if not exact:  # the split kernels need raw 0..255 pixels; fall back to the plain MFMA path
                self.path = "mfma"
                self._configure_path()
                self._alloc_acts(self.ld)
        if self.np:
            self.xscale = 1.0 / 255.0 if normalize else 1.0
            self.X = raw.to(torch.uint8).contiguous()
        else:
            self.xscale = 1.0
            xd = xd.to(torch.float64 if self.dtype == "f64" else torch.float32)
            if normalize:
                xd = xd / 255.0
            self.X = xd.to(self.gdt).contiguous()
        if self.feature_major_copy and self.np:
            # + an all-ones feature row: the dW1 GEMM's extra column is db1 (no separate bias reduction)
            self.XT = torch.cat([self.X.t(), torch.ones(1, self.X.shape[0], dtype=self.X.dtype, device=self.device)])
            self.XT = self.XT.contiguous()
        else:
            self.XT = self.X.t().contiguous() if self.feature_major_copy else None
        # wide layers on the hip backend: bf16 copies of both layouts for the direct-to-LDS GEMM engine
        # (csrc/mlp/glds_gemm.h streams operands global -> LDS unconverted; 2 B/pixel, ~170 MB for the
        # 54k-image training split -- nothing next to 288 GB of HBM)
        self.Xw = self.XTw = None
        # H <= 128 split3: the pixels again, in the forward's fragment order (MlpStep.x_swz; mma_tile.h xs_off):
        # [cdiv(N, 16)][cdiv(P, 64)][4 lane groups][16 samples][16 B], zero-padded -- a wave's 16-byte load
        # instruction reads 1 KB of contiguous memory instead of 16 rows x 64 B (~47 MB for 60k images)
        self.Xs = None
        if self.np == 3 and self.backend == "hip" and self.H <= 128 and self.XT is not None:
            self.Xs = fragment_order_pixels(self.X)
        if self.np and self.backend == "hip" and self.H >= 512 and self.XT is not None:
            self.Xw = self.X.to(torch.bfloat16).contiguous()
            self.XTw = self.XT.to(torch.bfloat16).contiguous()
        self.labels = torch.as_tensor(np.asarray(labels, dtype=np.int32)).to(self.device).contiguous()
        self.num_samples = int(self.X.shape[0])
        self.X0 = self.labels0 = self._perm = self._shifts = self._transforms = self._sampler = None
        if keep_source:
            # the loaded tensors become the (never written) source and the step reads fresh copies: on the CPU the
            # loaded ones may share memory with the caller's arrays, which a shuffle must not rewrite
            self.X0, self.labels0 = self.X, self.labels
            self.X, self.labels = self.X0.clone(), self.labels0.clone()
            if self.XT is not None and self.XT.data_ptr() == self.X0.data_ptr():  # (N == 1: the transpose is a view)
                self.XT = self.XT.clone()
            self._perm = torch.arange(self.num_samples, dtype=torch.int32, device=self.device)
        self._step = None
        self.refresh_shadow()

    # ------------------------------------------------------- per-epoch shuffle
    def enqueue_shuffle(self, seed: int, key: int, sampler=None) -> None:
        """Rewrite every resident layout (X, labels, XT, Xs, Xw, XTw) in place so that sample i is SOURCE sample
        perm[i], perm = epoch_permutation(N, seed, key) (csrc/mlp/shuffle.h; seed and key are unsigned 32-bit, packed
        as (seed << 32) ^ key).  Always gathers from the pristine copy, never from the previous order, so the order
        depends on (seed, key) alone.  On the current stream; no sync, no read-back, no allocation on the hip backend:
        the buffers keep their addresses, so a bound MlpStep and every captured graph stay valid.

        With ``sampler`` (a sampling.Balanced / Weighted; ``seed`` is then not used) perm[i] is a draw with replacement
        instead: perm = sampler.draws(loaded labels, key) (csrc/mlp/sample.h), by the same one launch with the alias
        table's address; the table is uploaded on first use (prepare_sampler: before a capture begins)."""
        self._shuffle(int(seed), int(key), False, sampler)

    def prepare_sampler(self, sampler) -> None:
        """What a gather with ``sampler`` needs on the device, now: the alias table of the policy's weights for the
        loaded labels (never rewritten).  The trainers call it from load(), so that no allocation and no upload happens
        inside a capture.  An engine serves ONE policy per load_dataset(): a captured graph holds the table's address,
        so another policy is refused (RuntimeError) rather than the table replaced under it; load the set again to
        change it.  Raises ValueError for weights the rule refuses."""
        if sampler is None or self.X is None or self.num_samples == 0:
            return
        if self.labels0 is None:
            raise RuntimeError("no pristine copy of the training set: load_dataset(..., keep_source=True) first")
        if self._sampler is not None:
            if self._sampler[0] is sampler or self._sampler[0] == sampler:
                return
            raise RuntimeError(f"this engine already samples with {self._sampler[0]!r}: one policy per "
                               "load_dataset() (a captured graph holds its table's address); load the set again "
                               f"to sample with {sampler!r}")
        table = sampler.table(self.labels0.cpu().numpy())
        if table.shape != (self.num_samples, 2):
            raise ValueError(f"the sampler's table is {table.shape}, the training set has {self.num_samples} samples")
        dev = torch.from_numpy(table.view(np.int32).copy()).to(self.device).contiguous()  # (the bits of the uint32 pairs)
        self._sampler = (sampler, table, dev)

    def _sampler_kw(self, sampler) -> dict:
        """The gather launchers' trailing arguments for ``sampler`` (nothing without one: the call is today's)."""
        if sampler is None:
            return {}
        self.prepare_sampler(sampler)
        return {"sample_table": self._sampler[2].data_ptr(), "sample_seed": sampler.seed}

    def _host_order(self, key: int, shuffle_seed, sampler):
        """(perm, ids) of the torch backend's gathers: the source row of every resident sample, and the index the
        augmentation rules hash for it -- the source row, or with a sampler the destination."""
        N = self.num_samples
        if sampler is not None:
            self.prepare_sampler(sampler)
            return cpu().epoch_draws(N, sampler.seed, key, self._sampler[1]), np.arange(N)
        perm = (np.arange(N, dtype=np.int32) if shuffle_seed is None
                else cpu().epoch_permutation(N, int(shuffle_seed), key))
        return perm, perm

    def unshuffle(self) -> None:
        """The order of load_dataset() again -- and, after an augmentation, its pixels: shifts() is zero again."""
        self._shuffle(0, 0, True)

    # ------------------------------------------------ per-epoch augmentation
    def enqueue_augment(self, aug, key: int, shuffle_seed: int | None = None, sampler=None) -> None:
        """enqueue_shuffle with the images moved on the way (augment.Shift; csrc/mlp/augment.h): every resident layout
        is rewritten in place from the pristine rows so that sample i is SOURCE sample perm[i] -- perm =
        epoch_permutation(N, shuffle_seed, key), or the loaded order without a seed -- shifted by
        epoch_shifts(N, aug.seed, key, ...)[perm[i]].  The shift belongs to the source sample, so the order does not
        change it.  Never composed with the previous state.  On the hip backend one launch of the augmenting gather
        (csrc/mlp/augment.hip) on the current stream: no sync, no read-back, and the buffers keep their addresses.

        With an augment.Affine the image is also resampled through table entry epoch_transforms(...)[perm[i]] of
        aug.table() (csrc/mlp/affine.h) by one launch of the affine gather (csrc/mlp/affine.hip) instead; the table is
        uploaded on first use (prepare_augment: before a capture begins).

        With an augment.Warp every source position of that resampling is moved by the field of the sample's lattice
        epoch_nodes(...)[perm[i]] (csrc/mlp/warp.h) by one launch of the warping gather (csrc/mlp/warp.hip) instead;
        its axis tables are uploaded next to the table.

        With ``sampler`` (a sampling policy; no ``shuffle_seed`` then) perm is the epoch's draws with replacement
        (enqueue_shuffle), and the shift, the table entry and the lattice are those of index i, the DESTINATION, not of
        perm[i]: a row drawn many times gets a different augmentation at each of its places."""
        from ..augment import Affine, Warp

        if sampler is not None and shuffle_seed is not None:
            raise ValueError("sampler and shuffle_seed together: two orders would be ambiguous")
        if isinstance(aug, Warp):
            return self._enqueue_warp(aug, int(key), shuffle_seed, sampler)
        if isinstance(aug, Affine):
            return self._enqueue_affine(aug, int(key), shuffle_seed, sampler)
        key, seed = int(key), 0 if shuffle_seed is None else int(shuffle_seed)
        ready = self._gather_ready(seed, key)
        N, P = self.num_samples, self.P
        h, w = aug.shape(P)
        if not ready:
            return
        if self._shifts is None:
            self._shifts = torch.zeros(N, 2, dtype=torch.int32, device=self.device)
        if self._transforms is not None:  # (only after an affine augmentation: this gather takes no transform)
            self._transforms.zero_()
        if self.backend == "hip":
            self._gather_launch(hip().mlp_augment, self._shifts.data_ptr(), N, P, self.X.element_size(), h, w,
                                aug.max_dx, aug.max_dy, aug.seed, key, int(shuffle_seed is not None), seed,
                                **self._sampler_kw(sampler))
            self.augment_launches += 1
            return
        with torch.no_grad():
            perm, ids = self._host_order(key, shuffle_seed, sampler)
            shifts = cpu().epoch_shifts(N, aug.seed, key, aug.max_dx, aug.max_dy)[ids]
            self._perm.copy_(torch.from_numpy(perm))
            self._shifts.copy_(torch.from_numpy(shifts))
            # the rule moves bytes (zero fill = all-zero bits): the rows go through the host as same-size integers
            bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.X0.element_size()]
            rows = self.X0.index_select(0, self._perm.long()).view(bits).cpu().numpy()
            moved = torch.from_numpy(cpu().augment_rows(rows, shifts, h, w)).view(self.X.dtype)
            self.X.copy_(moved)
            self.labels.copy_(self.labels0.index_select(0, self._perm.long()))
            self._rebuild_from_rows()

    def prepare_augment(self, aug) -> None:
        """What enqueue_augment(aug, ...) would allocate, now: the shifts, for an augment.Affine the transforms and
        the table on the device, and for an augment.Warp those of its Affine and the axis tables (once per policy;
        never rewritten).  The trainers call it from load(), so that no allocation and no upload happens inside a
        capture."""
        from ..augment import Affine, Warp

        if aug is None or self.X is None or self.num_samples == 0:
            return
        aug.shape(self.P)
        N = self.num_samples
        if self._shifts is None:
            self._shifts = torch.zeros(N, 2, dtype=torch.int32, device=self.device)
        if isinstance(aug, Affine):
            if self._transforms is None:
                self._transforms = torch.zeros(N, dtype=torch.int32, device=self.device)
            if self._affine_table is None or self._affine_table[0] != aug:
                self._affine_table = (aug, torch.from_numpy(aug.table().copy()).to(self.device).contiguous())
        if isinstance(aug, Warp):
            self.prepare_augment(aug.affine)
            h, w = aug.shape(self.P)
            if self._warp_axes is None or self._warp_axes[0] != (aug.grid, h, w):
                self._warp_axes = ((aug.grid, h, w),
                                   torch.from_numpy(aug.axes(h, w).copy()).to(self.device).contiguous())

    def _enqueue_warp(self, aug, key: int, shuffle_seed: int | None, sampler=None) -> None:
        seed = 0 if shuffle_seed is None else int(shuffle_seed)
        ready = self._gather_ready(seed, key)
        N, P = self.num_samples, self.P
        h, w = aug.shape(P)
        if not ready:
            return
        self.prepare_augment(aug)
        kind = {torch.uint8: 0, torch.bfloat16: 1, torch.float32: 2, torch.float64: 3}.get(self.X0.dtype)
        if kind is None:
            raise RuntimeError(f"the elastic distortion takes uint8, bf16, f32 or f64 pixels, not {self.X0.dtype}")
        if self.backend == "hip":
            table, axes = self._affine_table[1], self._warp_axes[1]
            self._gather_launch(hip().mlp_warp, self._shifts.data_ptr(), self._transforms.data_ptr(),
                                table.data_ptr(), int(table.shape[0]), kind, axes.data_ptr(), aug.grid[0], aug.grid[1],
                                aug.bound, N, P, self.X.element_size(), h, w, aug.max_dx, aug.max_dy, aug.seed, key,
                                int(shuffle_seed is not None), seed, **self._sampler_kw(sampler))
            self.warp_launches += 1
            return
        with torch.no_grad():
            perm, ids = self._host_order(key, shuffle_seed, sampler)
            shifts = cpu().epoch_shifts(N, aug.seed, key, aug.max_dx, aug.max_dy)[ids]
            index = cpu().epoch_transforms(N, aug.seed, key, aug.table_size)[ids]
            nodes = np.ascontiguousarray(cpu().epoch_nodes(N, aug.seed, key, aug.nodes, aug.bound)[ids])
            self._perm.copy_(torch.from_numpy(perm))
            self._shifts.copy_(torch.from_numpy(shifts))
            self._transforms.copy_(torch.from_numpy(index))
            rows = self.X0.index_select(0, self._perm.long())
            rows = (rows.view(torch.int16) if kind == 1 else rows).cpu().numpy()
            moved = cpu().warp_rows(rows, shifts, np.ascontiguousarray(aug.table()[index]), nodes, aug.axes(h, w), h,
                                    w, aug.grid[0], aug.grid[1], kind)
            self.X.copy_(torch.from_numpy(moved).view(self.X.dtype))
            self.labels.copy_(self.labels0.index_select(0, self._perm.long()))
            self._rebuild_from_rows()

    def _enqueue_affine(self, aug, key: int, shuffle_seed: int | None, sampler=None) -> None:
        seed = 0 if shuffle_seed is None else int(shuffle_seed)
        ready = self._gather_ready(seed, key)
        N, P = self.num_samples, self.P
        h, w = aug.shape(P)
        if not ready:
            return
        self.prepare_augment(aug)
        kind = {torch.uint8: 0, torch.bfloat16: 1, torch.float32: 2, torch.float64: 3}.get(self.X0.dtype)
        if kind is None:
            raise RuntimeError(f"the affine augmentation takes uint8, bf16, f32 or f64 pixels, not {self.X0.dtype}")
        if self.backend == "hip":
            table = self._affine_table[1]
            self._gather_launch(hip().mlp_affine, self._shifts.data_ptr(), self._transforms.data_ptr(),
                                table.data_ptr(), int(table.shape[0]), kind, N, P, self.X.element_size(), h, w,
                                aug.max_dx, aug.max_dy, aug.seed, key, int(shuffle_seed is not None), seed,
                                **self._sampler_kw(sampler))
            self.affine_launches += 1
            return
        with torch.no_grad():
            perm, ids = self._host_order(key, shuffle_seed, sampler)
            shifts = cpu().epoch_shifts(N, aug.seed, key, aug.max_dx, aug.max_dy)[ids]
            index = cpu().epoch_transforms(N, aug.seed, key, aug.table_size)[ids]
            self._perm.copy_(torch.from_numpy(perm))
            self._shifts.copy_(torch.from_numpy(shifts))
            self._transforms.copy_(torch.from_numpy(index))
            rows = self.X0.index_select(0, self._perm.long())
            rows = (rows.view(torch.int16) if kind == 1 else rows).cpu().numpy()
            moved = cpu().affine_rows(rows, shifts, np.ascontiguousarray(aug.table()[index]), h, w, kind)
            self.X.copy_(torch.from_numpy(moved).view(self.X.dtype))
            self.labels.copy_(self.labels0.index_select(0, self._perm.long()))
            self._rebuild_from_rows()

    def transforms(self) -> torch.Tensor:
        """The current affine augmentation as a device int32 [N]: resident sample i went through table entry
        transforms()[i] (zeros before any augmentation, and after unshuffle(), a plain shuffle or a Shift)."""
        if self._transforms is not None:
            return self._transforms
        if self.X is None:
            raise RuntimeError("load_dataset() first")
        return torch.zeros(self.num_samples, dtype=torch.int32, device=self.device)

    def shifts(self) -> torch.Tensor:
        """The current augmentation as a device int32 [N][2]: resident sample i is its source image moved by
        (dx, dy) = shifts()[i] (zeros before any augmentation, and after unshuffle() or a plain shuffle)."""
        if self._shifts is not None:
            return self._shifts
        if self.X is None:
            raise RuntimeError("load_dataset() first")
        return torch.zeros(self.num_samples, 2, dtype=torch.int32, device=self.device)

    def _rebuild_from_rows(self) -> None:
        """XT, Xs, Xw, XTw again from X (torch backend)."""
        P = self.P
        if self.XT is not None:
            self.XT[:P].copy_(self.X.t())
        if self.Xs is not None:
            self.Xs.copy_(fragment_order_pixels(self.X))
        if self.Xw is not None:
            self.Xw.copy_(self.X.to(torch.bfloat16))
            self.XTw[:P].copy_(self.X.t().to(torch.bfloat16))

    def permutation(self) -> torch.Tensor:
        """The current order as a device int32 tensor: resident sample i is loaded sample permutation()[i] (the
        identity before any shuffle).  After a gather with a sampler these are the epoch's draws -- the source row of
        every resident sample -- and no permutation: rows may repeat and rows may be missing."""
        if self._perm is not None:
            return self._perm
        if self.X is None:
            raise RuntimeError("load_dataset() first")
        return torch.arange(self.num_samples, dtype=torch.int32, device=self.device)

    def _gather_ready(self, seed: int, key: int) -> bool:
        """What the shuffle and the augmentation need before they rewrite the resident set; False: the set is empty,
        there is nothing to do."""
        if self.X is None:
            raise RuntimeError("load_dataset() first")
        if self.X0 is None:
            raise RuntimeError("no pristine copy of the training set: load_dataset(..., keep_source=True) first")
        if not (0 <= seed < 1 << 32 and 0 <= key < 1 << 32):
            raise ValueError("shuffle seed and key must be in [0, 2^32)")
        return self.num_samples != 0

    def _gather_launch(self, launch, *rest, **sampler_kw) -> None:
        """hip().mlp_shuffle / mlp_augment on the current stream: the pristine source, the resident layouts and the
        order as device addresses (0: a layout this engine does not hold), then ``rest`` (and a sampler's table)."""
        held = (self.X0, self.labels0, self.X, self.labels, self.XT, self.Xs, self.Xw, self.XTw, self._perm)
        launch(*(t.data_ptr() if t is not None else 0 for t in held), *rest,
               stream=torch.cuda.current_stream(self.device).cuda_stream, **sampler_kw)

    def _shuffle(self, seed: int, key: int, identity: bool, sampler=None) -> None:
        if not self._gather_ready(seed, key):
            return
        N, P = self.num_samples, self.P
        if self._shifts is not None:  # (only after an augmentation: the plain gather restores the loaded pixels)
            self._shifts.zero_()
        if self._transforms is not None:
            self._transforms.zero_()
        if self.backend == "hip":
            self._gather_launch(hip().mlp_shuffle, N, P, self.X.element_size(), seed, key, int(identity),
                                **self._sampler_kw(sampler))
            self.shuffle_launches += 1
            return
        with torch.no_grad():
            perm = self._host_order(key, None if identity else seed, sampler)[0]
            self._perm.copy_(torch.from_numpy(perm))
            idx = self._perm.long()
            self.X.copy_(self.X0.index_select(0, idx))
            self.labels.copy_(self.labels0.index_select(0, idx))
            self._rebuild_from_rows()

    def set_params(self, W1, b1, W2, b2):
        self.join()
        with torch.no_grad():
            for dst, src in ((self.W1, W1), (self.b1, b1), (self.W2, W2), (self.b2, b2)):
                dst.copy_(torch.as_tensor(np.asarray(src)).to(dst.dtype))
            self.refresh_shadow()
        if self._ema is not None:
            self.reset_ema()

    def dz1(self) -> torch.Tensor:
        """The last step's dZ1 as [H][ld] row-major.  A whole hip step with fp32 dZ1 leaves it only in the
        weight-gradient GEMM's fragment order (MlpStep.dz_swz, csrc/mlp/mma_tile.h w1s_off over [H][ld]); this view
        undoes that order (diagnostics and tests; the training step never reads dZ1 back)."""
        st = self._step
        if self.backend != "hip" or st is None or not st.dz_left_swz:
            return self.dZ1
        return fragment_rows_to_rowmajor(self.dZ1s, self.H, self.ld, 64 if st.dz_left_swz == 1 else 32)

    def _w1_written(self) -> None:
        """W1 changed outside the step's own in-place update: the forward's fragment-ordered copy (MlpStep.w1_swz)
        is rebuilt before the next forward that reads it."""
        if self._step is not None:
            self._step.swz_stale = True

    def refresh_shadow(self):
        """Re-derive the low-precision copies of W1 (bf16 shadow or bf16 planes)."""
        self.join()
        self._w1_written()
        with torch.no_grad():
            if self.np:
                if self.backend == "hip":
                    hip().split_planes(self.W1.data_ptr(), self.W1p.data_ptr(), self.H * self.P, self.np,
                                       torch.cuda.current_stream(self.device).cuda_stream)
                else:
                    r = self.W1.clone()
                    for p in range(self.np):
                        self.W1p[p] = r.to(torch.bfloat16)
                        r -= self.W1p[p].to(torch.float32)
            elif self.dtype == "bf16":
                self.W1g.copy_(self.W1.to(torch.bfloat16))

    def set_fh_allgather(self, on: bool) -> None:
        self.fh_allgather = bool(on)
        if self._step is not None:
            self._step.fh_allgather = int(self.fh_allgather)

    def enable_splitk(self, max_split: int = 8) -> None:
        """Let the wide weight-gradient launch split K (the batch) over up to ``max_split`` slices when its output
        tiles alone cannot fill the chip and K is long -- the tensor-parallel shard at a large global batch
        (784-4096-10 at global batch 6400 on 8 GPUs: 512 x 785 outputs, K = 6400).  Allocates the fp32 partial
        slabs [max_split][H][P + 1]; a second kernel sums them in slab order and applies the update."""
        if self.backend != "hip" or not self.np or max_split < 2:
            return
        self.kpart = torch.zeros(int(max_split) * self.H * (self.P + 1), dtype=torch.float32, device=self.device)
        self._step = None

    def set_store_a1(self, on: bool) -> None:
        """Split layers with the head fused into the forward launch: False skips the a1 store whenever that launch
        also leaves the dW2 partials (no kernel of the training step reads a1 then: dZ1 and the partials come out
        of the same launch).  Wide layers: always; H <= 128: from n = 768 columns (MlpStep.head_dw2 auto), where
        the weight-gradient launch's dW2 GEMM over the whole batch was that launch's critical path
        (bench/stamps_roles.py: roles end 5.99 -> 3.74 us at n = 800; below, the partials cost the forward more
        than they save -- profiles/r5/)."""
        self.store_a1 = bool(on)
        if self._step is not None:
            self._step.store_a1 = int(self.store_a1)

    def w1_planes_maintained(self) -> bool:
        """True when the W1 bf16 planes track the fp32 master after every update.  Below H = 512 the split3
        forward kernels read fp32 W1 and split it in registers, so the update stops refreshing the planes
        (csrc/mlp/mlp_split.hip mlp_split_w1_planes_read); at H = 4096 the 128 x 128 forward does too, and with
        lazy_planes the in-place update leaves them stale until a forward that reads them (MlpStep.planes_stale).
        refresh_w1_planes() rebuilds them on demand."""
        if not (self.np and self.backend == "hip"):
            return False
        s = self._hip_step()
        return bool(s.w1_planes_read()) and not s.lazy_planes_apply()

    def refresh_w1_planes(self) -> None:
        """Rebuild the W1 planes from the fp32 master (exact split3 / rounded split1)."""
        if self.np and self.backend == "hip":
            hip().split_planes(self.W1.data_ptr(), self.W1p.data_ptr(), self.W1.numel(), self.np,
                               torch.cuda.current_stream(self.device).cuda_stream)
            if self._step is not None:
                self._step.planes_stale = False

    def inject_handoff_timeout(self, row_tile: int = 0, wait_us: int = 2000) -> None:
        """TEST HOOK: from the next step on, row tile ``row_tile`` of column tile 0 withholds its hand-off
        granules in every all-gather forward + head launch, so that tile's wait really times out (after
        ``wait_us`` microseconds of wall time; the production bound is 50 ms).  ``row_tile=-1`` turns the
        withholding off (the bound stays).  A timed-out launch sets the sticky error word: this engine then
        applies no further update (kernel_error(), KernelHandoffTimeout) -- make a new engine afterwards."""
        self._ag_test_skip, self._ag_wait_us = int(row_tile), int(wait_us)
        if self._step is not None:
            self._step.ag_test_skip, self._step.ag_wait_us = self._ag_test_skip, self._ag_wait_us

    def kernel_error(self) -> bool:
        """True if a forward + head launch's wait for the workgroups of its column tile timed out (the
        all-gather form; its outputs were then not trusted).  Reads a device word: synchronises."""
        return self.ag_err is not None and bool(self.ag_err.item())

    def join(self):
        """Kept for API stability: every kernel of a step runs on the caller's stream, nothing to join."""

    def get_params(self):
        """Host float64 copies (W1, b1, W2, b2)."""
        self.join()
        return tuple(t.detach().to("cpu", torch.float64).numpy().copy()
                     for t in (self.W1, self.b1, self.W2, self.b2))

    # -------------------------------------------------------------- one step
    def set_lazy_planes(self, on: bool) -> None:
        self.lazy_planes = bool(on)
        if self._step is not None:
            self._step.lazy_planes = int(self.lazy_planes)

    def mark_planes_stale(self) -> None:
        """W1 / the W1 planes were overwritten from outside the step (a snapshot restore): the next forward that
        reads the planes re-splits W1 first (MlpStep.lazy_planes: the wide in-place update skips the refresh)."""
        if self._step is not None and self.W1p is not None:
            self._step.planes_stale = True
        self._w1_written()

    def _hip_step(self):
        if self._step is None:
            self._step = self._new_step()
        return self._step

    def _new_step(self, weights=None):
        """An MlpStep bound to the engine's buffers.  ``weights`` = (W1, b1, W2, b2, W1g, W1p): another set of
        weights with its own derived copies of W1 (the averaged evaluation: it never runs a training step, so it
        gets no fragment-ordered copy and no xGMI attachment); None: the engine's own."""
        own = weights is None
        W1, b1, W2, b2, W1g, W1p = (self.W1, self.b1, self.W2, self.b2, self.W1g, self.W1p) if own else weights
        m = hip()
        s = m.MlpStep()
        loaded = self.X is not None
        ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        b = dict(dt=DTYPE_CODES[self.dtype], P=self.P, H=self.H, C=self.C, ld=self.ld,
                 X=ptr(self.X), labels=ptr(self.labels), XT=ptr(self.XT), Xw=ptr(self.Xw), XTw=ptr(self.XTw),
                 N=self.num_samples if loaded else 0,
                 W1=ptr(W1), b1=ptr(b1), W2=ptr(W2), b2=ptr(b2), W1g=ptr(W1g),
                 gW1=ptr(self.gW1), gb1=ptr(self.gb1), gW2=ptr(self.gW2), gb2=ptr(self.gb2),
                 gstatus=self.grads[self.status_index:].data_ptr(),
                 a1=ptr(self.a1), D=ptr(self.D), dZ1=ptr(self.dZ1), dZ1g=ptr(self.dZ1g), loss=ptr(self.loss_buf),
                 act=1, z2p=ptr(self.z2buf))
        if self.np:
            b.update(split=1, xscale=float(self.xscale), npw=self.np, npz=self.np, W1p=ptr(W1p),
                     dZ1p=ptr(self.dZ1p))
        if self.fh_counters is not None:
            b.update(fh_counters=ptr(self.fh_counters), fh_tiles=int(self.fh_counters.numel()),
                     ag_counters=ptr(self.ag_counters), ag_slabs=ptr(self.ag_slabs),
                     w1s=ptr(self.W1s) if own else 0, xs=ptr(self.Xs), dz1s=ptr(self.dZ1s))
        elif self.ag_gran is not None:  # the wide fused head
            b.update(fh_tiles=int(self.ag_counters.numel()) // 64,  # [2 tilings][tiles][32]
                     ag_gran=ptr(self.ag_gran), ag_gran_count=int(self.ag_gran.numel()),
                     ag_counters=ptr(self.ag_counters), dz1s=ptr(self.dZ1s))
        if self.kpart is not None:
            b.update(kpart=ptr(self.kpart), kpart_cap=int(self.kpart.numel()))
        bias_col = bool(self.np and self.XT is not None and self.XT.shape[0] == self.P + 1)
        b.update(bias_col=int(bias_col))
        s.bind(b)
        s.shift = int(self.shift)
        s.dw2p = ptr(self.dw2buf)
        if self.ag_err is not None and (self.fh_counters is not None or self.ag_gran is not None):
            s.ag_err = self.ag_err.data_ptr()
            s.fh_allgather = int(self.fh_allgather)
        if self.np:
            # a new step cannot know whether an earlier one left the planes stale: re-split once
            s.planes_stale = True
            s.lazy_planes = int(self.lazy_planes)
        s.store_a1 = int(self.store_a1)
        s.ag_test_skip, s.ag_wait_us = self._ag_test_skip, self._ag_wait_us
        if own and self._xgmi_fuse is not None and bias_col:
            s.set_xgmi(*self._xgmi_fuse)
        return s

    # ------------------------------------------------ xGMI all-reduce fused into the wgrad launch
    def fused_allreduce_slots(self) -> int:
        """Flag slots (one per wgrad workgroup tile) the fused data-parallel step needs; 0 when this
        engine cannot run it (split path, H <= 128, at most 16 classes, all-ones XT feature, no head partials)."""
        bias_feature = (self.XT.shape[0] == self.P + 1 if self.XT is not None   # loaded, or will be
                        else self.feature_major_copy)
        if not fused_allreduce_eligible(self.backend, self.np, self.H, self.C, self.device.type, bias_feature):
            return 0
        return max(0, int(hip().mlp_split_fused_tiles(self.P, self.H, 1 << 30)))

    def attach_xgmi(self, bucket, push: bool = False) -> None:
        """Bind an open XgmiBucket (created with flag_slots >= fused_allreduce_slots()) to the step;
        ``None`` detaches.  run(..., sgd=2) then all-reduces and applies SGD inside the wgrad launch: the one-shot
        pull (every rank reads every peer's tile), or with ``push`` the owner-tile form (XgmiFuse::push: tile t
        reduced and applied by rank t % world, pushed both ways as tagged granules; the bucket needs
        slab_tiles >= fused_allreduce_slots())."""
        if bucket is None:
            self._xgmi_fuse = None
            if self._step is not None:
                self._step.set_xgmi(0, 0, 0, 0, 0)
            return
        o = self.layout.offsets
        self._xgmi_fuse = (int(bucket.c.desc_address), int(bucket.c.nblocks), int(o[1]), int(o[2]), int(o[3]),
                           int(bool(push)))
        self._hip_step().set_xgmi(*self._xgmi_fuse)

    def run(self, off: int, n: int, scale: float, reg: float, lr: float, sgd, with_loss: bool = False,
            parts: int = 3, pf_next: int = -1):
        """Forward + backward on samples [off, off+n).  sgd=True: update params in
        place; False: write pre-scaled gradients into ``self.grads``; 2: all-reduce over the attached
        xGMI bucket and update inside the wgrad launch (attach_xgmi).  parts (hip backend): bit0 forward +
        head, bit1 weight gradients / update -- the per-phase profiler runs the two halves separately.
        pf_next >= 0: the next step's first sample, whose pixels this step's prefetch workgroups pull into L2."""
        if self.X is None:
            raise RuntimeError("load_dataset() first")
        if n > self.ld:
            raise ValueError(f"batch slice {n} exceeds activation capacity {self.ld}")
        if off < 0 or off + n > self.num_samples:
            raise IndexError("batch slice outside the resident dataset")
        if self.backend == "hip":
            st = self._hip_step()
            st.run(int(off), int(n), float(scale), float(reg), float(lr), 2 if sgd == 2 else int(bool(sgd)),
                   int(bool(with_loss)),
                   torch.cuda.current_stream(self.device).cuda_stream, int(parts), int(pf_next))
        elif parts & 1:  # the torch backend always runs the whole step
            self._torch_step(off, n, scale, reg, lr, sgd, with_loss)

    def run_forward_head(self, off: int, n: int, scale: float, with_loss: bool = False):
        """Forward + head only (a1, D, dZ1 and its planes); the weight gradients follow via run_wgrad."""
        self._hip_step().run(int(off), int(n), float(scale), 0.0, 0.0, 0, int(bool(with_loss)),
                             torch.cuda.current_stream(self.device).cuda_stream, 1)

    def run_wgrad(self, off: int, n: int, scale: float, reg: float, parts: int, row0: int = 0, rows: int = -1):
        """Gradient pieces into ``self.grads`` (split paths): parts bit0 = dW1 rows [row0, row0+rows),
        bit1 = dW2 + bias gradients."""
        self._hip_step().run_wgrad(int(off), int(n), float(scale), float(reg), 0.0, 0, int(parts), int(row0),
                                   int(rows), torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def supports_bucketed_wgrad(self) -> bool:
        return self.backend == "hip" and bool(self.np)

    def _torch_step(self, off, n, scale, reg, lr, sgd, with_loss):
        """Same math as the HIP step in PyTorch ops (param dtype accumulation)."""
        with torch.no_grad():
            Xb = self.X[off:off + n].to(self.pdt) * self.xscale
            # the weights the kernels actually multiply: sum of the bf16 planes (== W1 for split3)
            W1g = self.W1p.to(self.pdt).sum(0) if self.np else self.W1g.to(self.pdt)
            z1 = Xb @ W1g.t() + self.b1
            a1 = torch.sigmoid(z1)
            z2 = a1 @ self.W2.t() + self.b2
            if self.shift:
                z2 = z2 - z2.max(dim=1, keepdim=True).values
            e = torch.exp(z2)
            p = e / e.sum(dim=1, keepdim=True)
            lab = self.labels[off:off + n].long()
            if with_loss:
                self.loss_buf.zero_()
                # log(sum) - (z_label - m), the HIP heads' form (csrc/mlp/head_math.h head_nll): finite where the
                # label's probability underflows
                self.loss_buf[0] = (torch.log(e.sum(dim=1)) - z2.gather(1, lab[:, None])[:, 0]).sum().float()
            onehot = torch.zeros_like(p)
            onehot[torch.arange(n, device=p.device), lab] = 1.0
            D = (p - onehot) * scale
            dZ1 = (D @ self.W2) * a1 * (1 - a1)
            self.a1[:, :n] = a1.t()
            self.D[:, :n] = D.t()
            self.dZ1[:, :n] = dZ1.t()
            gW1 = dZ1.t() @ Xb + reg * self.W1
            gW2 = D.t() @ a1 + reg * self.W2
            gb1 = dZ1.sum(0)
            gb2 = D.sum(0)
            if sgd:
                self.W1.sub_(lr * gW1)
                self.W2.sub_(lr * gW2)
                self.b1.sub_(lr * gb1)
                self.b2.sub_(lr * gb2)
                self.refresh_shadow()
            else:
                self.gW1.copy_(gW1)
                self.gW2.copy_(gW2)
                self.gb1.copy_(gb1)
                self.gb2.copy_(gb2)

    def sgd(self, lr: float):
        """params -= lr * grads over the whole flat arena (one fused kernel)."""
        self.join()
        self._w1_written()
        if self.backend == "hip" and self.np:
            hip().split_sgd(self.params.data_ptr(), self.grads.data_ptr(), self.layout.total, float(lr),
                            self.W1p.data_ptr(), self.H * self.P, self.np,
                            torch.cuda.current_stream(self.device).cuda_stream,
                            self.grads[self.status_index:].data_ptr())
        elif self.backend == "hip":
            stream = torch.cuda.current_stream(self.device).cuda_stream
            shadow = self.W1g.data_ptr() if self.dtype == "bf16" else 0
            hip().sgd_flat(DTYPE_CODES[self.dtype], self.params.data_ptr(), self.grads.data_ptr(),
                           self.layout.total, float(lr), shadow, self.H * self.P if shadow else 0, stream)
        else:
            with torch.no_grad():
                self.params.sub_(lr * self.grads)
                self.refresh_shadow()

    # ------------------------------------------------- stateful optimizers
    def set_optimizer(self, opt) -> None:
        """Select the update rule of apply().  None / Optimizer.sgd(): plain SGD, nothing allocated.  Momentum
        allocates one arena-sized state buffer in the parameter dtype and Adam two, plus the counter records
        {t, b1^t, b2^t, 0} (fp64; one per workgroup of the kernel's fixed grid on the hip backend, one otherwise) --
        all zeroed / reset."""
        from ..optim import resolve

        self.optimizer = resolve(opt)
        self._alloc_update_state()

    def _alloc_update_state(self) -> None:
        if not self.uses_apply_launch:
            self.opt_bufs, self.opt_rec = [], None
            return
        dev = self.device
        self.opt_bufs = [torch.zeros(self.layout.total, dtype=self.pdt, device=dev)
                         for _ in range(self.optimizer.num_state if self.optimizer is not None else 0)]
        nrec = int(hip().optim_grid(self.layout.total)) if self.backend == "hip" else 1
        self.opt_rec = torch.zeros(nrec, 4, dtype=torch.float64, device=dev)
        self.reset_optimizer()

    WINDOW_MIN_CAP = 256  # factors the schedule window holds before it has to grow

    @property
    def policy_set(self) -> bool:
        return self.schedule is not None or self.clip_norm > 0.0 or self._plateau is not None

    @property
    def uses_apply_launch(self) -> bool:
        """apply() is the one launch of csrc/mlp/optim.hip (a stateful rule, or plain SGD under a schedule, clipping
        or a plateau rule) rather than sgd(lr)."""
        return self.optimizer is not None or self.policy_set

    def set_update_policy(self, schedule=None, clip_norm=None) -> None:
        """A learning-rate schedule (optim.Schedule) and / or gradient-norm clipping at ``clip_norm`` for apply().
        With neither, nothing changes and nothing is allocated.  With either, plain SGD becomes the stateless kSgd rule
        through the apply launch (counter records allocated, update count reset to 0); a stateful optimizer keeps its
        state.  The clipped gradient is the one the step leaves -- scaled, regulariser included: torch's
        clip_grad_norm_ with the L2 term in the loss; a non-finite norm propagates as torch's default does.  The window
        starts as the single factor of update 0: set_schedule_window() (DataParallelTrainer does) fills it."""
        from ..optim import resolve_policy

        had = self.uses_apply_launch
        self.schedule, self.clip_norm = resolve_policy(schedule, clip_norm)
        dev = self.device
        if not self.policy_set:
            self.sched_win = self._win_host = self.clip_partials = self.opt_last = None
            if had and self.optimizer is None:
                self._alloc_update_state()
            return
        if not had:
            self._alloc_update_state()
        self.opt_last = torch.tensor([-1.0, float("nan"), float("nan"), 1.0], dtype=torch.float64, device=dev)
        self.clip_partials = None
        if self.clip_norm > 0.0:
            self.clip_partials = torch.zeros(64, dtype=torch.float64, device=dev)  # (clip.h kClipMaxGrid)
        self.sched_win = self._win_host = None
        if self.schedule is not None:
            self.sched_win = torch.zeros(2 + self.WINDOW_MIN_CAP, dtype=torch.float64, device=dev)
            self.set_schedule_window(0, self.schedule.factors(0, 1))

    def clip_segments(self) -> list:
        """The (offset, size) pairs of [W1|b1|W2|b2] in the arena: what enters the gradient norm (never a segment's
        padding, never the status element)."""
        return [(int(o), int(s)) for o, s in zip(self.layout.offsets[:4], self.layout.sizes[:4])]

    def set_schedule_window(self, t0: int, factors) -> bool:
        """Fill the schedule window: update t0 + i gets factors[i]; an update outside [t0, t0 + n) takes the nearest
        end's factor.  A copy into the resident buffer, in place -- captured graphs stay valid -- unless the factors
        outgrow its capacity: then the buffer is reallocated and True is returned (graphs captured against the old one
        must be dropped).  Never call it during a capture."""
        if self.schedule is None:
            raise RuntimeError("set_update_policy() with a schedule first")
        f = np.ascontiguousarray(factors, dtype=np.float64).reshape(-1)
        t0, n = int(t0), int(f.size)
        if t0 < 0 or n < 1:
            raise ValueError("a schedule window needs t0 >= 0 and at least one factor")
        if not bool(np.all(f >= 0.0)):
            raise ValueError("schedule factors must be >= 0")
        grew = False
        if n > self.sched_win.numel() - 2:
            cap = max(n, 2 * (self.sched_win.numel() - 2))
            self.sched_win = torch.zeros(2 + cap, dtype=torch.float64, device=self.device)
            grew = True
        host = np.concatenate([[float(t0), float(n)], f])
        with torch.no_grad():
            self.sched_win[:host.size].copy_(torch.from_numpy(host))
        self._win_host = (t0, f.copy())
        return grew

    def update_count(self) -> int:
        """The count of applied updates (the device-resident record).  Synchronises."""
        if self.opt_rec is None:
            raise RuntimeError("plain SGD without a schedule or clipping keeps no update count")
        return int(self.opt_rec[0, 0].item())

    def last_update(self) -> dict | None:
        """{t, lr, grad_norm, clip_coef} of the last applied update under a schedule or clipping (grad_norm None
        without clipping; None before the first update).  Synchronises."""
        if self.opt_last is None:
            raise RuntimeError("set_update_policy() first")
        t, lr, norm, coef = self.opt_last.cpu().tolist()
        if t < 0:
            return None
        return {"t": int(t), "lr": lr, "grad_norm": None if self.clip_norm <= 0.0 else norm, "clip_coef": coef}

    def reset_optimizer(self) -> None:
        """Zero the optimizer state and the update count."""
        if self.opt_rec is None:
            return
        with torch.no_grad():
            for b in self.opt_bufs:
                b.zero_()
            self.opt_rec.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).expand_as(self.opt_rec))

    def _unpadded(self, flat: torch.Tensor) -> np.ndarray:
        return torch.cat([v.reshape(-1) for v in self.layout.views(flat)]).to("cpu", torch.float64).numpy().copy()

    def optim_state(self) -> dict | None:
        """Host copy of the optimizer state: {kind, t, b1p, b2p, state: [fp64 arrays over [W1|b1|W2|b2], unpadded]}
        (the layout of optim.new_state and models.mlp.train); None for plain SGD.  Checks that every workgroup's
        counter record agrees.  Synchronises."""
        if self.opt_rec is None:
            return None
        rec = self.opt_rec.cpu()
        if not bool((rec == rec[0]).all()):
            raise RuntimeError("optimizer counter records disagree: " + str(rec[:, :3].unique(dim=0).tolist()))
        return {"kind": self._rule_kind, "t": int(rec[0, 0]), "b1p": float(rec[0, 1]), "b2p": float(rec[0, 2]),
                "state": [self._unpadded(b) for b in self.opt_bufs]}

    @property
    def _rule_kind(self) -> str:
        return self.optimizer.kind if self.optimizer is not None else "sgd"

    def set_optim_state(self, st: dict) -> None:
        if self.opt_rec is None:
            raise RuntimeError("set_optimizer() with a stateful optimizer (or set_update_policy()) first")
        if st["kind"] != self._rule_kind or len(st["state"]) != len(self.opt_bufs):
            raise ValueError(f"the state is a {st['kind']} state, the optimizer is {self._rule_kind}")
        srcs = [torch.as_tensor(np.asarray(s, np.float64)).reshape(-1) for s in st["state"]]
        count = sum(v.numel() for v in self.layout.views(self.params))
        if any(s.numel() != count for s in srcs):  # (before anything is copied)
            raise ValueError(f"the state must hold one value per parameter ({count}), got "
                             f"{[int(s.numel()) for s in srcs]}")
        with torch.no_grad():
            for buf, src in zip(self.opt_bufs, srcs):
                o = 0
                for v in self.layout.views(buf):
                    v.copy_(src[o:o + v.numel()].view(v.shape).to(v.dtype))
                    o += v.numel()
            rec = torch.tensor([float(st["t"]), float(st["b1p"]), float(st["b2p"]), 0.0], dtype=torch.float64)
            self.opt_rec.copy_(rec.expand_as(self.opt_rec))

    def apply(self, lr: float) -> None:
        """Apply the gradient bucket to the arena with the engine's update rule: sgd(lr) for plain SGD, else ONE
        launch of the stateful kernel (csrc/mlp/optim.hip), which also refreshes the bf16 planes / shadow of W1,
        advances the device-resident update count and applies nothing when the bucket's status element is non-zero.
        No host sync: legal under stream capture."""
        if not self.uses_apply_launch:
            self.sgd(lr)
            return
        if self.policy_set:
            self._apply_policy(lr)
            return
        o = self.optimizer
        self._w1_written()
        if self.backend == "hip":
            planes, np_ = (self.W1p, self.np) if self.np else ((self.W1g, 1) if self.dtype == "bf16" else (None, 0))
            hip().optim_step(0 if self.pdt == torch.float32 else 1, o.code, *o.hyper(lr), self.params.data_ptr(),
                             self.grads.data_ptr(), self.opt_bufs[0].data_ptr(),
                             self.opt_bufs[1].data_ptr() if len(self.opt_bufs) > 1 else 0, self.layout.total,
                             planes.data_ptr() if planes is not None else 0, np_, self.H * self.P if np_ else 0,
                             self.grads[self.status_index:].data_ptr(), self.opt_rec.data_ptr(),
                             int(self.opt_rec.shape[0]), torch.cuda.current_stream(self.device).cuda_stream)
            return
        with torch.no_grad():
            if float(self.grads[self.status_index]) != 0.0:
                return
            host = self.device.type == "cpu"
            arrs = [t if host else t.cpu() for t in (self.params, self.grads, *self.opt_bufs)]
            rec = self.opt_rec[0].cpu()
            t, b1p, b2p = cpu().optim_step(o.code, o.hyper(lr), *(a.numpy() for a in arrs[:3]),
                                           arrs[3].numpy() if len(arrs) > 3 else None, int(rec[0]), float(rec[1]),
                                           float(rec[2]))
            if not host:
                for dst, src in zip((self.params, None, *self.opt_bufs), arrs):
                    if dst is not None:
                        dst.copy_(src)
            self.opt_rec.copy_(torch.tensor([float(t), b1p, b2p, 0.0], dtype=torch.float64).expand_as(self.opt_rec))
            self.refresh_shadow()

    def _apply_policy(self, lr: float) -> None:
        """apply() under a schedule and / or clipping: (clipping) the sum-of-squares launch over the four parameter
        segments, then the ONE apply launch, which combines the partials, reads the update's factor from the window and
        leaves the last-update record.  The torch backend evaluates the same header on the host (_cpu.grad_clip,
        _cpu.window_rate, _cpu.optim_step)."""
        from ..optim import SGD_CODE, Optimizer

        o = self.optimizer
        code = o.code if o is not None else SGD_CODE
        hyper = (o if o is not None else Optimizer.sgd()).hyper
        self._w1_written()
        if self.backend == "hip":
            m = hip()
            st = torch.cuda.current_stream(self.device).cuda_stream
            dt = 0 if self.pdt == torch.float32 else 1
            npart = 0
            if self.clip_norm > 0.0:
                segs = self.clip_segments()
                npart = int(m.clip_grid(sum(s for _, s in segs)))
                m.grad_sumsq(dt, self.grads.data_ptr(), self.layout.total, segs, self.clip_partials.data_ptr(), npart,
                             st)
            planes, np_ = (self.W1p, self.np) if self.np else ((self.W1g, 1) if self.dtype == "bf16" else (None, 0))
            win = self.sched_win
            m.optim_apply(dt, code, *hyper(lr), self.params.data_ptr(), self.grads.data_ptr(),
                          self.opt_bufs[0].data_ptr() if self.opt_bufs else 0,
                          self.opt_bufs[1].data_ptr() if len(self.opt_bufs) > 1 else 0, self.layout.total,
                          planes.data_ptr() if planes is not None else 0, np_, self.H * self.P if np_ else 0,
                          self.grads[self.status_index:].data_ptr(), self.opt_rec.data_ptr(),
                          int(self.opt_rec.shape[0]), win.data_ptr() if win is not None else 0,
                          int(win.numel()) - 2 if win is not None else 0,
                          self.clip_partials.data_ptr() if npart else 0, npart, self.clip_norm,
                          self.opt_last.data_ptr(), st, self._plateau_word())
            return
        with torch.no_grad():
            if float(self.grads[self.status_index]) != 0.0:
                return
            host = self.device.type == "cpu"
            arrs = [t if host else t.cpu() for t in (self.params, self.grads, *self.opt_bufs)]
            g = arrs[1].numpy().copy()  # (the bucket itself stays as the step left it, as on the device)
            rec = self.opt_rec[0].cpu()
            t = int(rec[0])
            lr_t = float(lr)
            if self._win_host is not None:
                lr_t = float(cpu().window_rate(float(lr), float(self._win_host[0]), self._win_host[1], t))
            if self._plateau is not None:  # (lr * f) * scale, as the apply launch forms it
                lr_t = float(cpu().plateau_rate(lr_t, float(self._plateau["rec"][cpu().plateau_scale_word])))
            norm, coef = float("nan"), 1.0
            if self.clip_norm > 0.0:
                norm, coef = cpu().grad_clip(g, self.clip_segments(), self.clip_norm)
            state = [a.numpy() for a in arrs[2:]]
            t1, b1p, b2p = cpu().optim_step(code, hyper(lr_t), arrs[0].numpy(), g, state[0] if state else None,
                                            state[1] if len(state) > 1 else None, t, float(rec[1]), float(rec[2]))
            if not host:
                self.params.copy_(arrs[0])
                for dst, src in zip(self.opt_bufs, arrs[2:]):
                    dst.copy_(src)
            self.opt_rec.copy_(torch.tensor([float(t1), b1p, b2p, 0.0], dtype=torch.float64).expand_as(self.opt_rec))
            self.opt_last.copy_(torch.tensor([float(t), lr_t, norm, coef], dtype=torch.float64))
            self.refresh_shadow()

    def reg_only_grads(self, reg: float):
        """Gradient of an EMPTY shard: reg*W for weights, 0 for biases (the
        reference's in_proc == 0 case, neural_network.cpp:458)."""
        with torch.no_grad():
            self.grads.zero_()
            self.gW1.copy_(reg * self.W1)
            self.gW2.copy_(reg * self.W2)

    def loss_sum(self) -> float:
        """Sum of -log(yhat[label]) over the last step's local samples (if requested)."""
        return float(self.loss_buf.double().sum().item())

    # --------------------------------------------------------------- predict
    def predict(self, x, chunk: int | None = None, weights: str = "current") -> np.ndarray:
        """argmax labels for samples ``x`` ([N][P], host or device); GPU forward.  ``weights="ema"``: with the
        averaged weights (set_ema), their derived copies of W1 rebuilt first; the live parameters are not touched."""
        self.join()
        w = self._weights_for(weights)
        W1g, b1, W2, b2 = (self.W1g, self.b1, self.W2, self.b2) if w is None else (w["W1g"], w["b1"], w["W2"], w["b2"])
        step = None
        if self.backend == "hip" and self.np:
            step = self._hip_step() if w is None else self._ema_step()
        xt = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        n = int(xt.shape[0])
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        chunk = chunk or max(self.ld, 4096)
        a1 = torch.empty(self.H, _round_up(chunk, 16), dtype=self.pdt, device=self.device)
        if self.backend == "hip":
            self._hip_step()
        if w is not None:
            self._ema_derive()
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            if self.np:  # raw uint8 pixels, scaled inside the kernel
                raw = xt[s:e].to(self.device).to(torch.float32)
                if not bool(((raw == raw.round()) & (raw >= 0) & (raw <= 255)).all().item()):
                    raise ValueError("split-path predict needs raw 0..255 pixel inputs")
                xb = raw.to(torch.uint8).contiguous()
            else:
                xb = xt[s:e].to(self.device).to(torch.float64 if self.dtype == "f64" else torch.float32)
                if self._normalize:
                    xb = xb / 255.0
                xb = xb.to(self.gdt).contiguous()
            if self.backend == "hip" and self.np:
                step.predict(xb.data_ptr(), e - s, a1.data_ptr(), a1.shape[1], out[s:e].data_ptr(),
                             torch.cuda.current_stream(self.device).cuda_stream)
            elif self.backend == "hip":
                m = hip()
                st = torch.cuda.current_stream(self.device).cuda_stream
                dt = DTYPE_CODES[self.dtype]
                m.mlp_forward1(dt, W1g.data_ptr(), b1.data_ptr(), xb.data_ptr(), self.P, self.H, e - s,
                               a1.data_ptr(), a1.shape[1], 1, st)
                m.mlp_head(dt if self.dtype != "bf16" else 0, 1, a1.data_ptr(), a1.shape[1], W2.data_ptr(),
                           b2.data_ptr(), H=self.H, C=self.C, n=e - s, pred=out[s:e].data_ptr(), stream=st)
            else:
                with torch.no_grad():
                    W1p = self.W1p if w is None else w["W1p"]
                    W1e = W1p.to(self.pdt).sum(0) if self.np else W1g.to(self.pdt)
                    z1 = (xb.to(self.pdt) * self.xscale) @ W1e.t() + b1
                    z2 = torch.sigmoid(z1) @ W2.t() + b2
                    out[s:e] = z2.argmax(dim=1).to(torch.int32)
        return out.cpu().numpy()

    # -------------------------------------------------------------- evaluate
    def load_eval(self, x, labels, eval_chunk: int | None = None, eval_slots: int = 1):
        """Upload a validation set once ([N][P]) and keep it resident next to the training set, with everything an
        evaluation needs: the a1 scratch for ``eval_chunk`` columns (default as predict: max(ld, 4096)), the loss
        partials and ``eval_slots`` stats slots (csrc/mlp/eval.h: n, correct, loss_sum, C x C confusion counts, rows
        = labels).  Split paths keep raw uint8 pixels, range-checked once here; the others the GEMM dtype with the
        training set's ``normalize``.  No evaluation allocates anything afterwards."""
        xt = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        if xt.ndim != 2 or xt.shape[1] != self.P:
            raise ValueError(f"expected [N][{self.P}] samples, got {tuple(xt.shape)}")
        lab = torch.as_tensor(np.asarray(labels, dtype=np.int64)).reshape(-1)
        n = int(xt.shape[0])
        if int(lab.numel()) != n:
            raise ValueError("one label per sample expected")
        if n and (int(lab.min()) < 0 or int(lab.max()) >= self.C):
            raise ValueError(f"labels must be in [0, {self.C})")
        if int(eval_slots) < 1:
            raise ValueError("eval_slots must be >= 1")
        xd = xt.to(self.device)
        if self.np:
            raw = xd.to(torch.float32)
            if not bool(((raw == raw.round()) & (raw >= 0) & (raw <= 255)).all().item()):
                raise ValueError("split-path evaluation needs raw 0..255 pixel inputs")
            X = raw.to(torch.uint8).contiguous()
        else:
            xd = xd.to(torch.float64 if self.dtype == "f64" else torch.float32)
            if self._normalize:
                xd = xd / 255.0
            X = xd.to(self.gdt).contiguous()
        chunk = int(eval_chunk or max(self.ld, 4096))
        if chunk < 1:
            raise ValueError("eval_chunk must be >= 1")
        cols = _round_up(max(1, min(chunk, n)), 16)
        words = 3 + self.C * self.C
        self._eval = dict(
            X=X, labels=lab.to(torch.int32).to(self.device).contiguous(), n=n, chunk=chunk, path=self.path,
            a1=torch.zeros(self.H, cols, dtype=self.pdt, device=self.device),
            partials=torch.zeros(256, dtype=torch.float64, device=self.device),  # (eval.h kEvalMaxWgs)
            stats=torch.zeros(int(eval_slots), words, dtype=torch.int64, device=self.device))

    @property
    def eval_samples(self) -> int:
        return self._eval["n"] if self._eval is not None else 0

    @property
    def eval_slots(self) -> int:
        return int(self._eval["stats"].shape[0]) if self._eval is not None else 0

    def reserve_eval_slots(self, slots: int) -> None:
        """At least ``slots`` stats slots (allocates; call before the evaluations are enqueued, never between an
        enqueue and its read, and not while a captured evaluation is to be replayed)."""
        ev = self._eval
        if ev is None:
            raise RuntimeError("load_eval() first")
        if int(slots) > ev["stats"].shape[0]:
            ev["stats"] = torch.zeros(int(slots), ev["stats"].shape[1], dtype=torch.int64, device=self.device)

    def _eval_set(self, slot: int):
        ev = self._eval
        if ev is None:
            raise RuntimeError("load_eval() first")
        if ev["path"] != self.path:
            raise RuntimeError("the compute path changed after load_eval(): load the validation set again")
        if not 0 <= int(slot) < ev["stats"].shape[0]:
            raise IndexError(f"evaluation slot {slot} outside [0, {ev['stats'].shape[0]})")
        return ev

    def enqueue_eval(self, slot: int, first: int = 0, count: int | None = None, weights: str = "current") -> None:
        """Enqueue the evaluation of validation samples [first, first + count) into stats slot ``slot`` on the
        current stream, chunk by chunk: forward GEMM into the a1 scratch, then the evaluation head.  The first chunk
        clears the slot.  No host read, no sync, no allocation: legal under stream capture.  ``weights="ema"``
        evaluates the averaged weights (set_ema) through their own derived copies of W1, rebuilt on the stream ahead of
        the first chunk; the live parameters are never overwritten."""
        ev = self._eval_set(slot)
        count = ev["n"] - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > ev["n"]:
            raise IndexError("evaluation range outside the resident validation set")
        if self._weights_for(weights) is not None:
            self._enqueue_eval_ema(ev, int(slot), int(first), count)
            return
        if self.backend != "hip":
            self._torch_eval(ev, int(slot), int(first), count)
            return
        m = hip()
        st = torch.cuda.current_stream(self.device).cuda_stream
        a1, lda = ev["a1"].data_ptr(), int(ev["a1"].shape[1])
        stats = ev["stats"].data_ptr() + int(slot) * ev["stats"].shape[1] * 8
        part = ev["partials"].data_ptr()
        x0, l0, xrow = ev["X"].data_ptr(), ev["labels"].data_ptr(), self.P * ev["X"].element_size()
        step = min(ev["chunk"], lda)
        dt = DTYPE_CODES[self.dtype]
        if count == 0:  # an empty shard still clears its slot
            m.mlp_eval_head(0 if self.dtype == "bf16" else dt, 0, lda, self.W2.data_ptr(), self.b2.data_ptr(), 0,
                            self.H, self.C, 0, stats, part, 1, st)
            return
        for s in range(first, first + count, step):
            nb = min(step, first + count - s)
            zero = int(s == first)
            if self.np:
                self._hip_step().evaluate(x0 + s * xrow, l0 + 4 * s, nb, a1, lda, stats, part, st, zero)
            else:
                m.mlp_forward1(dt, self.W1g.data_ptr(), self.b1.data_ptr(), x0 + s * xrow, self.P, self.H, nb, a1,
                               lda, 1, st)
                m.mlp_eval_head(0 if self.dtype == "bf16" else dt, a1, lda, self.W2.data_ptr(), self.b2.data_ptr(),
                                l0 + 4 * s, self.H, self.C, nb, stats, part, zero, st)

    def _torch_eval(self, ev, slot: int, first: int, count: int, w: dict | None = None) -> None:
        """The evaluation head's math in torch ops (param dtype z2 and nll, fp64 loss accumulation).  ``w``: another
        set of weights (the averaged ones) with their derived copies of W1; None: the engine's own."""
        C = self.C
        src = self if w is None else types.SimpleNamespace(**w)
        with torch.no_grad():
            row = ev["stats"][slot]
            row.zero_()
            loss = row[2:3].view(torch.float64)
            cls = torch.arange(C, device=self.device)
            step = ev["chunk"]
            for s in range(first, first + count, step):
                e = min(first + count, s + step)
                W1e = src.W1p.to(self.pdt).sum(0) if self.np else src.W1g.to(self.pdt)
                z1 = (ev["X"][s:e].to(self.pdt) * self.xscale) @ W1e.t() + src.b1
                z2 = torch.sigmoid(z1) @ src.W2.t() + src.b2
                lab = ev["labels"][s:e].long()
                mx = z2.max(dim=1, keepdim=True).values
                pred = torch.where(z2 == mx, cls, C).min(dim=1).values  # the first maximum
                nll = torch.log(torch.exp(z2 - mx).sum(1)) - (z2.gather(1, lab[:, None])[:, 0] - mx[:, 0])
                row[0] += e - s
                row[1] += (pred == lab).sum()
                loss += nll.double().sum()
                row[3:] += torch.bincount(lab * C + pred, minlength=C * C)

    def eval_words(self, slots: int | None = None, first: int = 0) -> torch.Tensor:
        """Host copy of stats slots [first, first + slots) as raw 8-byte words [slots][3 + C * C] (word 2 is the fp64
        loss_sum's bits): the one sync and copy of an evaluation."""
        ev = self._eval_set(first)
        k = ev["stats"].shape[0] - first if slots is None else int(slots)
        self._eval_set(first + max(k, 1) - 1)
        return ev["stats"][first:first + k].cpu()

    def unpack_eval(self, words: torch.Tensor) -> dict:
        """One slot's words -> dict(n, correct, loss_sum, confusion [C][C] int64, rows = labels)."""
        C = self.C
        return dict(n=int(words[0]), correct=int(words[1]), loss_sum=float(words[2:3].view(torch.float64)[0]),
                    confusion=words[3:].view(C, C).numpy().copy())

    def read_eval(self, slot: int = 0) -> dict:
        ev = self._eval_set(slot)
        return self.unpack_eval(ev["stats"][int(slot)].cpu())

    def evaluate(self, slot: int = 0, first: int = 0, count: int | None = None, weights: str = "current") -> dict:
        self.enqueue_eval(slot, first, count, weights=weights)
        return self.read_eval(slot)

    # ------------------------------------------------------- keep the best weights
    BEST_MONITORS = {"loss": 0, "accuracy": 1}
    BEST_FIELDS = ("evals", "best_index", "best_metric", "bad", "stopped", "stop_index", "last_metric")

    @staticmethod
    def _best_rule(monitor, min_delta, patience) -> tuple:
        if monitor not in MlpEngine.BEST_MONITORS:
            raise ValueError(f"monitor must be one of {list(MlpEngine.BEST_MONITORS)}")
        min_delta = float(min_delta)
        if not min_delta >= 0.0:
            raise ValueError("min_delta must be >= 0")
        if patience is not None and int(patience) < 0:
            raise ValueError("patience must be >= 0 (None: never stop)")
        return monitor, min_delta, -1 if patience is None else int(patience)

    @property
    def best_count(self) -> int:
        """Elements of the best arena: the parameter arena [W1|b1|W2|b2] without the status element."""
        return int(self.layout.status)

    def enable_keep_best(self, monitor: str = "loss", min_delta: float = 0.0, patience: int | None = None,
                         ranks: int = 1) -> None:
        """Keep the parameters of the best evaluation on the device (csrc/mlp/best.h): allocates the best arena (the
        parameter dtype; bf16 mode's masters are fp32, the bf16 planes are derived state and not kept), the records
        (one per workgroup of the kernel's fixed grid on the hip backend, one otherwise) and, for ``ranks`` > 1, the
        [ranks][3] rows of a data-parallel decision; nothing else ever allocates.  ``patience`` = p tolerates p
        non-improving evaluations and stops on number p + 1 (0: the first one; None: never).  Calling it again with
        the same rule is a no-op; a different rule raises unless reset_best() was called first."""
        rule = self._best_rule(monitor, min_delta, patience)
        ranks = int(ranks)
        if ranks < 1:
            raise ValueError("ranks must be >= 1")
        b = self._best
        if b is not None:
            if b["rule"] == rule and b["ranks"] == ranks:
                return
            if not b["fresh"]:
                raise RuntimeError(f"keep-best is enabled with the rule {b['rule']}; reset_best() before changing it "
                                   f"to {rule}")
        dev = self.device
        nrec = int(hip().best_grid(self.best_count)) if self.backend == "hip" else 1
        self._best = dict(rule=rule, ranks=ranks, fresh=True,
                          arena=torch.zeros(self.best_count, dtype=self.pdt, device=dev),
                          rec=torch.zeros(nrec, 8, dtype=torch.float64, device=dev),
                          rows=torch.zeros(ranks, 3, dtype=torch.float64, device=dev) if ranks > 1 else None)
        self.reset_best()

    def _best_set(self) -> dict:
        if self._best is None:
            raise RuntimeError("enable_keep_best() first")
        return self._best

    @property
    def best_rows(self):
        """The [ranks][3] device buffer of a data-parallel decision (None for one rank)."""
        return self._best_set()["rows"]

    def reset_best(self) -> None:
        """Forget the best: the records back to the start state {0, -1, NaN, 0, 0, -1, NaN, 0}, the best arena zeroed.
        The rule may be changed afterwards."""
        b = self._best_set()
        with torch.no_grad():
            b["arena"].zero_()
            b["rec"].copy_(torch.from_numpy(cpu().best_start()).expand_as(b["rec"]))
        b["fresh"] = True

    def _slot_triple(self, ev, slot: int) -> np.ndarray:
        w = ev["stats"][int(slot), :3].cpu()
        return np.array([[float(int(w[0])), float(int(w[1])), float(w[2:3].view(torch.float64)[0])]], np.float64)

    def pack_best_rows(self, slot: int, rank: int) -> None:
        """This rank's {n, correct, loss_sum} of stats slot ``slot`` into row ``rank`` of best_rows, zero into every
        other row: a SUM all-reduce of the buffer is then an exact all-gather.  On the current stream; no host read on
        the hip backend."""
        rows = self._best_set()["rows"]
        if rows is None:
            raise RuntimeError("enable_keep_best(ranks=R) with R > 1 first")
        self.pack_rows(slot, rank, rows)

    def pack_rows(self, slot: int, rank: int, rows) -> None:
        """pack_best_rows into any [R][3] float64 buffer on the engine's device (the plateau rule's, when keep-best is
        off)."""
        ev = self._eval_set(slot)
        if rows is None or rows.dtype != torch.float64 or rows.ndim != 2 or rows.shape[1] != 3 \
                or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous [R][3] float64 tensor")
        if not 0 <= int(rank) < rows.shape[0]:
            raise IndexError(f"rank {rank} outside [0, {rows.shape[0]})")
        if self.backend == "hip":
            hip().mlp_best_pack(ev["stats"].data_ptr() + int(slot) * ev["stats"].shape[1] * 8, rows.data_ptr(),
                                int(rows.shape[0]), int(rank), torch.cuda.current_stream(self.device).cuda_stream)
            return
        with torch.no_grad():
            rows.zero_()
            rows[int(rank)].copy_(torch.from_numpy(self._slot_triple(ev, slot)[0]))

    def enqueue_keep_best(self, slot: int, rows=None, weights: str = "current") -> None:
        """One decision on the current stream, behind enqueue_eval(slot): from stats slot ``slot`` (one process) or from
        ``rows`` (a [R][3] float64 tensor of {n, correct, loss_sum} per rank, summed in rank order; on the hip backend
        a device tensor that stays alive until the launch has run -- best_rows is the resident one).  When the metric
        improves on the best so far, the parameter arena is copied into the best arena; every record advances.  No host
        read, no sync, no allocation on the hip backend: legal under stream capture."""
        b = self._best_set()
        ev = self._eval_set(slot)
        monitor, min_delta, patience = b["rule"]
        code = self.BEST_MONITORS[monitor]
        b["fresh"] = False
        # (weights="ema": the evaluation behind this decision read the averaged weights, so those are the ones kept)
        w = self._weights_for(weights)
        params = self.params if w is None else w["arena"]
        if rows is not None and (rows.dtype != torch.float64 or rows.ndim != 2 or rows.shape[1] != 3
                                 or rows.shape[0] < 1 or not rows.is_contiguous()):
            raise ValueError("rows must be a contiguous [R][3] float64 tensor, R >= 1")
        if self.backend == "hip":
            if rows is not None and rows.device != self.device:
                raise ValueError("rows must live on the engine's device")
            hip().mlp_keep_best(0 if self.pdt == torch.float32 else 1, code, min_delta, patience,
                                params.data_ptr(), b["arena"].data_ptr(), self.best_count, b["rec"].data_ptr(),
                                int(b["rec"].shape[0]),
                                0 if rows is not None else
                                ev["stats"].data_ptr() + int(slot) * ev["stats"].shape[1] * 8,
                                rows.data_ptr() if rows is not None else 0,
                                int(rows.shape[0]) if rows is not None else 1,
                                torch.cuda.current_stream(self.device).cuda_stream)
            return
        with torch.no_grad():
            triples = rows.cpu().numpy() if rows is not None else self._slot_triple(ev, slot)
            rec, improved = cpu().best_decide(b["rec"][0].cpu().numpy(), code, min_delta, patience, triples)
            b["rec"].copy_(torch.from_numpy(rec).expand_as(b["rec"]))
            if improved:
                b["arena"].copy_(params[:self.best_count])

    def best_state(self) -> dict:
        """Record 0 as a dict: evals, best_index, best_metric, bad, stopped, stop_index, last_metric (+ the rule:
        monitor, min_delta, patience).  The one sync: a 64-byte read."""
        b = self._best_set()
        r = b["rec"][0].cpu().tolist()
        monitor, min_delta, patience = b["rule"]
        return {"evals": int(r[0]), "best_index": int(r[1]), "best_metric": r[2], "bad": int(r[3]),
                "stopped": bool(r[4]), "stop_index": int(r[5]), "last_metric": r[6], "monitor": monitor,
                "min_delta": min_delta, "patience": None if patience < 0 else patience}

    def best_records(self) -> np.ndarray:
        """Every workgroup's record as raw doubles [nrec][8] (tests and diagnostics).  Synchronises."""
        return self._best_set()["rec"].cpu().numpy().copy()

    def best_params(self):
        """Host float64 copies (W1, b1, W2, b2) of the best weights, as get_params(); None before any best."""
        b = self._best_set()
        if float(b["rec"][0, 1].item()) < 0:
            return None
        return tuple(t.detach().to("cpu", torch.float64).numpy().copy() for t in self.layout.views(b["arena"]))

    def restore_best(self) -> dict:
        """Copy the best weights back into the parameter arena (a device copy) and re-derive the bf16 planes / shadow
        of W1, as set_params does.  Raises when there is no best yet.  Returns best_state()."""
        b = self._best_set()
        st = self.best_state()
        if st["best_index"] < 0:
            raise RuntimeError("restore_best(): no evaluation has been accepted as the best yet")
        with torch.no_grad():
            self.params[:self.best_count].copy_(b["arena"])
            self.refresh_shadow()
        self.mark_planes_stale()
        return st

    def set_best_state(self, record, params=None) -> None:
        """Resume: ``record`` = the 8 doubles of a record (or a best_state() dict), ``params`` = (W1, b1, W2, b2) of the
        best weights (None: the arena is left as it is; required when the record holds a best)."""
        b = self._best_set()
        if isinstance(record, dict):
            record = [record[k] for k in self.BEST_FIELDS] + [0.0]
        rec = np.asarray([float(v) for v in record], np.float64).reshape(-1)
        if rec.size != 8:
            raise ValueError("a record is 8 doubles")
        if rec[1] >= 0 and params is None:
            raise ValueError("the record holds a best: its weights are required")
        with torch.no_grad():
            if params is not None:
                for dst, src in zip(self.layout.views(b["arena"]), params):
                    src = torch.as_tensor(np.asarray(src))
                    if src.numel() != dst.numel():
                        raise ValueError("best weights of another shape")
                    dst.copy_(src.reshape(dst.shape).to(dst.dtype))
            b["rec"].copy_(torch.from_numpy(rec).expand_as(b["rec"]))
        b["fresh"] = False

    # ------------------------------------------------------- reduce the rate on a plateau
    def set_plateau(self, rule, ranks: int = 1) -> None:
        """Reduce the learning rate when the validation metric stops improving (optim.Plateau; csrc/mlp/plateau.h).
        None: nothing allocated, nothing launched, apply() as it stands.  A rule allocates the one record of 8 doubles
        (reset to the start state) and, for ``ranks`` > 1, the [ranks][3] rows of a data-parallel decision; from then
        on every update -- plain SGD's too, as the stateless kSgd rule -- goes through the apply launch, which
        multiplies its rate by the record's scale word: ``(lr * f) * scale``.  enqueue_plateau() behind an evaluation
        advances the record.  Setting the rule it already has keeps the record."""
        from ..optim import resolve_plateau

        rule = resolve_plateau(rule)
        ranks = int(ranks)
        if ranks < 1:
            raise ValueError("ranks must be >= 1")
        p = self._plateau
        if rule is not None and p is not None and p["rule"] == rule and p["ranks"] == ranks:
            return
        had, had_policy = self.uses_apply_launch, self.policy_set
        dev = self.device
        if rule is None:
            self._plateau = None
            if had_policy and not self.policy_set:
                self.opt_last = None
                if self.optimizer is None:
                    self._alloc_update_state()
            return
        self._plateau = dict(rule=rule, ranks=ranks, rec=torch.zeros(8, dtype=torch.float64, device=dev),
                             rows=torch.zeros(ranks, 3, dtype=torch.float64, device=dev) if ranks > 1 else None)
        if not had:
            self._alloc_update_state()
        if not had_policy:
            self.opt_last = torch.tensor([-1.0, float("nan"), float("nan"), 1.0], dtype=torch.float64, device=dev)
        self.reset_plateau()

    def _plateau_set(self) -> dict:
        if self._plateau is None:
            raise RuntimeError("set_plateau() first")
        return self._plateau

    def _plateau_word(self) -> int:
        """The address of the record's scale word for the apply launch (0 without a rule)."""
        p = self._plateau
        return 0 if p is None else p["rec"].data_ptr() + 8 * int(hip().plateau_scale_word)

    @property
    def plateau_rows(self):
        """The [ranks][3] device buffer of a data-parallel decision (None for one rank)."""
        return self._plateau_set()["rows"]

    def reset_plateau(self) -> None:
        """The record back to its start state {0, +inf | -inf, 0, 0, 1.0, 0, NaN, -1}: the scale is 1 again."""
        p = self._plateau_set()
        with torch.no_grad():
            p["rec"].copy_(torch.from_numpy(cpu().plateau_start(p["rule"].monitor_code)))

    def enqueue_plateau(self, slot: int, rows=None) -> None:
        """One decision on the current stream, behind enqueue_eval(slot): from stats slot ``slot`` (one process) or from
        ``rows`` (a contiguous [R][3] float64 tensor of {n, correct, loss_sum} per rank, summed in rank order; on the
        hip backend a device tensor that stays alive until the launch has run).  One workgroup advances the record; the
        updates enqueued behind it use the new scale.  No host read, no sync, no allocation on the hip backend: legal
        under stream capture."""
        p = self._plateau_set()
        ev = self._eval_set(slot)
        if rows is not None and (rows.dtype != torch.float64 or rows.ndim != 2 or rows.shape[1] != 3
                                 or rows.shape[0] < 1 or not rows.is_contiguous()):
            raise ValueError("rows must be a contiguous [R][3] float64 tensor, R >= 1")
        if self.backend == "hip":
            if rows is not None and rows.device != self.device:
                raise ValueError("rows must live on the engine's device")
            hip().mlp_plateau(*p["rule"].native(), p["rec"].data_ptr(),
                              0 if rows is not None else ev["stats"].data_ptr() + int(slot) * ev["stats"].shape[1] * 8,
                              rows.data_ptr() if rows is not None else 0,
                              int(rows.shape[0]) if rows is not None else 1,
                              torch.cuda.current_stream(self.device).cuda_stream)
            return
        with torch.no_grad():
            triples = rows.cpu().numpy() if rows is not None else self._slot_triple(ev, slot)
            rec, _ = cpu().plateau_decide(p["rec"].cpu().numpy(), p["rule"].native(), triples)
            p["rec"].copy_(torch.from_numpy(rec))

    def plateau_record(self) -> np.ndarray:
        """The record as raw doubles [8].  Synchronises."""
        return self._plateau_set()["rec"].cpu().numpy().copy()

    def plateau_state(self) -> dict:
        """The record as a dict: evals, best, bad, cooldown_left, scale, reductions, last_metric, last_reduced_index.
        The one sync: a 64-byte read."""
        from ..optim import plateau_record_dict

        return plateau_record_dict(self.plateau_record())

    def set_plateau_state(self, record) -> None:
        """Resume: ``record`` = the 8 doubles of a record, or a plateau_state() dict."""
        from ..optim import plateau_record_array

        p = self._plateau_set()
        with torch.no_grad():
            p["rec"].copy_(torch.from_numpy(plateau_record_array(record)))

    # ------------------------------------------------------- an average of the weights
    @property
    def ema_count_elems(self) -> int:
        """Elements the averaging launch covers: the arena [W1|b1|W2|b2] without the status element."""
        return int(self.layout.status)

    def set_ema(self, rule) -> None:
        """Keep an exponential moving average of the parameters on the device (optim.Ema, csrc/mlp/ema.h): allocates the
        averaged arena (the parameter dtype, the layout of the parameter arena; bf16 mode's masters are fp32) and the
        records {t, d of the last update, 0, 0} (one per workgroup of the kernel's fixed grid on the hip backend, one
        otherwise), and starts the average as a copy of the parameters with t = 0.  ``None`` releases everything: then
        nothing is allocated and nothing is launched."""
        from ..optim import resolve_ema

        rule = resolve_ema(rule)
        if rule is None:
            self._ema = None
            return
        dev = self.device
        nrec = int(hip().ema_grid(self.ema_count_elems)) if self.backend == "hip" else 1
        arena = torch.zeros(self.layout.total, dtype=self.pdt, device=dev)
        W1, b1, W2, b2 = self.layout.views(arena)
        # (W1g / W1p / step: the average's own derived copies of W1, made by the first evaluation that reads it)
        self._ema = dict(rule=rule, arena=arena, rec=torch.zeros(nrec, 4, dtype=torch.float64, device=dev),
                         W1=W1, b1=b1, W2=W2, b2=b2, W1g=None, W1p=None, step=None, step_for=None)
        self.reset_ema()

    def _ema_set(self) -> dict:
        if self._ema is None:
            raise RuntimeError("set_ema() first")
        return self._ema

    def reset_ema(self) -> None:
        """The average becomes a copy of the current parameters and the count 0 (set_ema and set_params do this)."""
        a = self._ema_set()
        with torch.no_grad():
            n = self.ema_count_elems
            a["arena"][:n].copy_(self.params[:n])
            a["rec"].zero_()

    def ema_update(self, status: bool = False) -> None:
        """Fold the parameters into the average: ONE launch (csrc/mlp/ema.hip) behind an applied update, on the current
        stream, no host sync, legal under stream capture.  ``status``: the update came from the gradient bucket
        (gradient mode + apply), whose status element, when non-zero, says that it was not applied -- the launch then
        changes nothing; the sticky hand-off word of the all-gather forward + head is passed wherever the engine has
        one, for the same reason.  Without set_ema() this is a no-op."""
        a = self._ema
        if a is None:
            return
        r = a["rule"]
        n = self.ema_count_elems
        if self.backend == "hip":
            hip().mlp_ema_step(0 if self.pdt == torch.float32 else 1, float(r.decay), int(bool(r.warmup)),
                               self.params.data_ptr(), a["arena"].data_ptr(), n, a["rec"].data_ptr(),
                               int(a["rec"].shape[0]),
                               self.grads[self.status_index:].data_ptr() if status else 0,
                               self.ag_err.data_ptr() if self.ag_err is not None else 0,
                               torch.cuda.current_stream(self.device).cuda_stream)
            return
        with torch.no_grad():
            if status and float(self.grads[self.status_index]) != 0.0:
                return
            host = self.device.type == "cpu"
            e, p = a["arena"][:n], self.params[:n]
            ea, pa = (e, p) if host else (e.cpu(), p.cpu())
            t = int(a["rec"][0, 0].item())
            t1 = cpu().ema_step(ea.numpy(), pa.numpy(), float(r.decay), bool(r.warmup), t)
            if not host:
                e.copy_(ea)
            d = float(cpu().ema_decay(float(r.decay), bool(r.warmup), t))
            a["rec"].copy_(torch.tensor([float(t1), d, 0.0, 0.0], dtype=torch.float64).expand_as(a["rec"]))

    def ema_count(self) -> int:
        """The count of averaged updates (the device-resident record).  Synchronises."""
        return int(self._ema_set()["rec"][0, 0].item())

    def ema_records(self) -> np.ndarray:
        """Every workgroup's record as raw doubles [nrec][4] (tests and diagnostics).  Synchronises."""
        return self._ema_set()["rec"].cpu().numpy().copy()

    def ema_state(self) -> dict:
        """{decay, warmup, t, last_decay}: the rule and record 0.  Checks that every workgroup's record agrees.
        Synchronises."""
        a = self._ema_set()
        rec = a["rec"].cpu()
        if not bool((rec == rec[0]).all()):
            raise RuntimeError("averaging records disagree: " + str(rec[:, :2].unique(dim=0).tolist()))
        return {"decay": float(a["rule"].decay), "warmup": bool(a["rule"].warmup), "t": int(rec[0, 0]),
                "last_decay": float(rec[0, 1])}

    def ema_params(self):
        """Host float64 copies (W1, b1, W2, b2) of the averaged weights, unpadded, as get_params()."""
        a = self._ema_set()
        return tuple(a[k].detach().to("cpu", torch.float64).numpy().copy() for k in ("W1", "b1", "W2", "b2"))

    def set_ema_state(self, t: int, params=None, last_decay: float = 0.0) -> None:
        """Resume: the count of averaged updates and (W1, b1, W2, b2) of the average (None: the arena is left as it
        is)."""
        a = self._ema_set()
        if int(t) < 0:
            raise ValueError("t must be >= 0")
        with torch.no_grad():
            if params is not None:
                for k, src in zip(("W1", "b1", "W2", "b2"), params):
                    src = torch.as_tensor(np.asarray(src))
                    if src.numel() != a[k].numel():
                        raise ValueError("averaged weights of another shape")
                    a[k].copy_(src.reshape(a[k].shape).to(a[k].dtype))
            rec = torch.tensor([float(int(t)), float(last_decay), 0.0, 0.0], dtype=torch.float64)
            a["rec"].copy_(rec.expand_as(a["rec"]))

    def adopt_ema(self) -> None:
        """Make the average the current weights: a device copy into the parameter arena, then the bf16 planes / shadow
        of W1 re-derived, as restore_best() does.  The average and its count stay as they are."""
        a = self._ema_set()
        with torch.no_grad():
            n = self.ema_count_elems
            self.params[:n].copy_(a["arena"][:n])
            self.refresh_shadow()
        self.mark_planes_stale()

    def _weights_for(self, weights: str) -> dict | None:
        """None for "current"; the averaging state for "ema" (with its derived copies of W1 allocated)."""
        if weights == "current":
            return None
        if weights != "ema":
            raise ValueError('weights must be "current" or "ema"')
        a = self._ema_set()
        if self.np and a["W1p"] is None:
            a["W1p"] = torch.zeros(self.np, self.H, self.P, dtype=torch.bfloat16, device=self.device)
        if a["W1g"] is None:
            if self.np or self.dtype != "bf16":
                a["W1g"] = a["W1"]
            else:
                a["W1g"] = torch.zeros(self.H, self.P, dtype=torch.bfloat16, device=self.device)
        if self.backend == "hip" and self.np:
            self._ema_step()
        return a

    def _ema_step(self):
        """The second MlpStep: the engine's buffers with the averaged weights and their own bf16 planes.  Created on
        first use, and again when the engine's own step was rebuilt (its buffers changed)."""
        a = self._ema_set()
        main = self._hip_step()
        if a["step"] is None or a["step_for"] is not main:
            a["step"] = self._new_step((a["W1"], a["b1"], a["W2"], a["b2"], a["W1g"], a["W1p"]))
            a["step_for"] = main
        return a["step"]

    def _ema_derive(self) -> None:
        """Ahead of the first chunk of an averaged evaluation: the derived copies of the averaged W1 are stale (the
        averaging launch maintains none).  Split paths on the hip backend mark the second step's planes stale, so its
        existing re-split runs -- inside a capture too, where the replay cannot decide; the bf16 path converts the
        shadow on the stream; the torch backend re-derives them as refresh_shadow() does."""
        a = self._ema_set()
        with torch.no_grad():
            if self.np and self.backend == "hip":
                a["step"].planes_stale = True
            elif self.np:
                r = a["W1"].clone()
                for p in range(self.np):
                    a["W1p"][p] = r.to(torch.bfloat16)
                    r -= a["W1p"][p].to(torch.float32)
            elif self.dtype == "bf16":
                a["W1g"].copy_(a["W1"])

    def _enqueue_eval_ema(self, ev, slot: int, first: int, count: int) -> None:
        """enqueue_eval() with the averaged weights: the same launches, the weight pointers those of the averaged
        arena and its derived copies."""
        a = self._weights_for("ema")
        self._ema_derive()
        if self.backend != "hip":
            self._torch_eval(ev, slot, first, count, w=a)
            return
        m = hip()
        st = torch.cuda.current_stream(self.device).cuda_stream
        a1, lda = ev["a1"].data_ptr(), int(ev["a1"].shape[1])
        stats = ev["stats"].data_ptr() + slot * ev["stats"].shape[1] * 8
        part = ev["partials"].data_ptr()
        x0, l0, xrow = ev["X"].data_ptr(), ev["labels"].data_ptr(), self.P * ev["X"].element_size()
        step = min(ev["chunk"], lda)
        dt = DTYPE_CODES[self.dtype]
        hdt = 0 if self.dtype == "bf16" else dt
        if count == 0:  # an empty shard still clears its slot
            m.mlp_eval_head(hdt, 0, lda, a["W2"].data_ptr(), a["b2"].data_ptr(), 0, self.H, self.C, 0, stats, part, 1,
                            st)
            return
        for s in range(first, first + count, step):
            nb = min(step, first + count - s)
            zero = int(s == first)
            if self.np:
                a["step"].evaluate(x0 + s * xrow, l0 + 4 * s, nb, a1, lda, stats, part, st, zero)
            else:
                m.mlp_forward1(dt, a["W1g"].data_ptr(), a["b1"].data_ptr(), x0 + s * xrow, self.P, self.H, nb, a1, lda,
                               1, st)
                m.mlp_eval_head(hdt, a1, lda, a["W2"].data_ptr(), a["b2"].data_ptr(), l0 + 4 * s, self.H, self.C, nb,
                                stats, part, zero, st)
