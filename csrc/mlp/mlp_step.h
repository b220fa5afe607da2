// The host object behind every training step (Python: _hip.MlpStep, bound in csrc/bindings_hip.cpp): everything a
// step needs, bound once, the measured policies, and -- MlpStep::plan -- the ONE decision of how a step runs.
#pragma once

#include <algorithm>
#include <string>

#include "eval.h"
#include "mlp_kernels.h"
#include "mlp_split.h"

namespace cme {

// How one step runs: the finished launch arguments and the host actions around them.  MlpStep::plan decides,
// MlpStep::run executes; the XCD-local pipeline qualifies a plan of steps by reading the same decision.
struct StepForm {
  enum Fwd { kNone, kAllGather, kLastArriver, kWide, kSeparate };
  Fwd fwd = kNone;       // kAllGather / kLastArriver: the H <= 128 forward + head launch; kWide: the wide fused head
  bool run_fwd = false, run_head = false;  // kSeparate: mlp_split_fwd1 and / or mlp_head (parts & 8, parts & 4 skip one)
  bool run_wgrad = false;
  int store_a1 = 1;      // kWide: the fused head also stores a1 (MlpStep::store_a1)
  SplitStepArgs f, w;    // the forward (+ head) launch's arguments, the weight-gradient launch's
  HeadArgs h{};
  // host actions before the launches: rebuild the fragment-ordered W1 copy if stale / this step's update does not
  // maintain it; re-split the W1 planes if stale (a forward kernel of this step reads them)
  bool refresh_swz = false, mark_swz_stale = false, refresh_planes = false;
  bool planes_left_stale = false;  // ... and after: the weight-gradient launch's update skips the W1-plane refresh
  // what the forward + head leaves for the rest of the step's backward (run_wgrad, run(parts = 2))
  struct Left {
    int dw2 = 0;         // dW2 partials in dw2p (the H <= 128 all-gather head or the wide heads) ...
    int dw2_cols = 32;   // ... per 128 / 64 columns (the fused wide head), 32 (head_wide_kernel), 16 (fha_body step 4a)
    int dz_swz = 0;      // dZ1 in dz1s (fragment order), not in dZ1 (MlpEngine.dz1())
  } left;
};

// The XCD-local pipeline's two departures from the two-launch step's policy (MlpStep::plan_steps): the two-launch
// step that takes the same choices computes the same bits.
struct StepOverrides {
  // the head's dW2 partials at every n, not only from 768 (head_dw2 auto: the pipeline's role workgroup sums them;
  // below 768 columns the two-launch form forms dW2 in its own role instead, so the bits there match head_dw2 = 1)
  bool dw2_every_n = false;
  // unless pixels AND dZ1 take their fragment orders (grid16: every step of the plan starts a 16-sample tile; dZ1 has
  // no fragment order below 257 columns): row-major pixels and fp32 dZ1 row-major, a_fp32 |= 2 (n = 100 takes dZ1
  // planes by default there: the pipeline has no plane form)
  bool rm_unless_frag = false, grid16 = false;
};

// Hot-path step object: everything a training step needs, bound once.  One
// Python call launches the whole fused step (3 kernels), keeping host overhead
// out of eager-mode steps; graph capture records the same launches.
struct MlpStep {
  int dt = 0;
  int P = 784, H = 100, C = 10, ld = 0;
  uintptr_t X = 0, labels = 0;            // device-resident dataset (gemm dtype) + int32 labels
  uintptr_t XT = 0;                       // optional feature-major copy [P][N]
  uintptr_t Xw = 0, XTw = 0;              // wide layers: bf16 copies of X [N][P] / XT [P+1][N] (0: none)
  int64_t N = 0;                          // samples in the resident dataset (ld of XT)
  uintptr_t W1 = 0, b1 = 0, W2 = 0, b2 = 0, W1g = 0;  // params (+ bf16 shadow of W1)
  uintptr_t gW1 = 0, gb1 = 0, gW2 = 0, gb2 = 0;       // gradient bucket views
  uintptr_t a1 = 0, D = 0, dZ1 = 0, dZ1g = 0;         // activations [rows][ld]
  uintptr_t loss = 0;                                 // float partials, >= head blocks
  int shift = 1, act = 1;
  // split-bf16 path (mlp_split.h): X/XT are bf16, W1p/dZ1p hold npw/npz bf16 planes
  int split = 0, npw = 3, npz = 3;
  uintptr_t stamps = 0;  // diagnostics only
  uintptr_t hstamps = 0;  // diagnostics only: head-block stamps
  uintptr_t wstamps = 0;  // diagnostics only: weight-gradient workgroup stamps (SplitStepArgs::wstamps)
  uintptr_t z2p = 0;     // wide-layer head scratch (head_big_scratch_floats), 0: column head
  uintptr_t dw2p = 0;    // wide layers: dW2 partials [cdiv(ld, 32)][16][H] left by the head (0: the dW2 GEMM)
  int bias_col = 0;      // XT has an all-ones feature row P: db1 comes out of the dW1 GEMM
  // split path, H <= 128: uint32 tile counters (>= fh_tiles, zeroed) enable the single-launch forward +
  // head (mlp_fwd1_head); 0: separate fwd1 + head kernels
  uintptr_t fh_counters = 0;
  int fh_tiles = 0;
  // the all-gather form of that launch (mlp_fwd1_head_ag): uint64 counters, z2 partial slabs and an error
  // word (>= fh_tiles each); fh_allgather = 1 selects it when all three are set
  uintptr_t ag_counters = 0, ag_slabs = 0, ag_err = 0;
  int fh_allgather = 0;
  // the gradient bucket's status element (float, after b2): written by the wgrad launch in gradient mode
  uintptr_t gstatus = 0;
  // the all-gather hand-offs' wait bound (microseconds of wall time) and the forced-timeout test hook
  // (SplitStepArgs::ag_test_skip; -1 off)
  int ag_wait_us = (int)kHandoffWaitUs, ag_test_skip = -1;
  // what the last run(parts & 1) left for run_wgrad / run(parts = 2).  Wide split layers: the all-gather head fused
  // into the forward launch (fh_allgather, ag_counters, ag_err; mlp_fwd1_wide_ag) leaves dW2 partials per 128 / 64
  // columns (32 from head_wide_kernel): what run_wgrad sums
  StepForm::Left left;
  int store_a1 = 1;  // the fused wide head: 0 skips the a1 store (nothing in the step reads it)
  // the fused wide head's hand-off granules ([cdiv(H, 64)][16][ld] z2 partials, then [16][ld] D; uint64)
  uintptr_t ag_gran = 0;
  int64_t ag_gran_count = 0;
  // the fused wide head on the 64 x 64 tiling (H = 512-1024): -1 = when a1 is not stored (measured faster only
  // then: profiles/wide_fused_head_r2.md), 1 = always, 0 = never
  int ag_tiles64 = -1;
  // H <= 128: the XCD-row placement of the forward + head and dW1 launches (SplitStepArgs::xcd_rows; on: the W1
  // rows and dZ1 rows each launch writes are read back by the next one from the same XCD's L2 -- step 14.0 ->
  // 13.1-13.2 us at n = 800, 12.3 -> 11.7 us at n = 100, profiles/kbench_xcd_rows_r4.jsonl; 0 for A/B)
  int xcd_rows = 1;
  // SplitStepArgs::xcd_rows == 2 for the forward + head when it fits (small batches): the first four XCDs start a
  // launch up to ~1 us before the other four (profiles/r5/stamps_fha_per_xcd.jsonl), but two row tiles per XCD
  // measured SLOWER, off: walking step +0.3-0.7 us at n = 100-512 (profiles/r5/kbench_xcd_pack.jsonl, alternated
  // twice) -- each XCD then pulls twice the W1 rows and pixels through its L2
  int xcd_pack = 0;
  // SplitStepArgs::w1_swz / W1s: the forward (H <= 128 split3, 16-byte pixel pairs) reads fp32 W1 from its
  // fragment-ordered copy w1s; the in-place update keeps the copy fresh, every other W1 write marks it stale
  // (swz_stale: MlpEngine.refresh_shadow / sgd / mark_planes_stale, run_wgrad with an update) and run() rebuilds it
  // before the next forward that reads it
  int w1_swz = 1;
  uintptr_t w1s = 0;
  int a_fp32 = -1;  // SplitStepArgs::a_fp32 (-1: the measured policy in split_args; A/B knob)
  // SplitStepArgs::dz_swz: with fp32 dZ1 (a_fp32 bit1) and the W1 copy's forward, the all-gather head writes dZ1 in
  // the weight-gradient GEMM's fragment order into dz1s and that GEMM reads it from there (whole steps only: a
  // bucketed run_wgrad reads the row-major dZ1)
  int dz_swz = 1;
  uintptr_t dz1s = 0;
  // SplitStepArgs::x_swz / Xs: with w1_swz, the forward also reads the pixels from their fragment-ordered copy xs
  // (MlpEngine.load_dataset builds it once; a step whose first sample is not a multiple of 16 reads the row-major X)
  int x_swz = 1;
  uintptr_t xs = 0;
  bool swz_stale = true;
  void refresh_swz(uintptr_t stream) {
    if (!swz_stale || !w1s) return;
    mlp_split_w1s_refresh(P_<float>(W1), P_<float>(w1s), H, P, S(stream));
    swz_stale = false;
  }
  // SplitStepArgs::pf_wgs, prefetch workgroups per XCD (0: off).  Walking-batch step (kbench step_walk_us, A/B twice):
  // 0 -> 4: 14.55-14.63 -> 14.11-14.14 us at n = 800, 13.0-13.1 -> 12.64-12.66 at n = 100; 2 and 6 slower at n = 800
  // (profiles/kbench_prefetch_wgs_r4.jsonl)
  int prefetch = 4;
  // SplitStepArgs::pf_wgs_xt (this step's XT pulled by extra workgroups of the forward + head launch): on in round 4,
  // OFF since the end of round 5 -- with the fragment-ordered forward operands and fp32 dZ1 they cost the forward more
  // than they save the weight-gradient launch: walking step 14.01-14.06 -> 13.73-13.85 us at n = 800, -0.13 at 512,
  // -0.15 at 400, -0.03 to -0.1 at 100-200 (profiles/r5/kbench_prefetch_xt_r5.jsonl, alternated three times)
  int prefetch_xt = 0;
  int wide_eng = -1;    // SplitStepArgs::wide_eng: the 128 x 128 wide K loop's engine (0 rega, 1 g64; -1: g64 for bf16
                        // A, rega for fp32 -- 784-4096-10 step bf16 39.1 -> 38.1 us, fp32 55.4 -> 58.0 with g64,
                        // profiles/r5/kbench_wide_engines.jsonl)
  // H <= 128, the all-gather forward + head: it also leaves the dW2 partials per 32 columns (fha_body step 4a) for
  // the weight-gradient launch's dW2 role (needs dw2p); 0: the role forms D . a1^T over the batch itself; -1 (auto):
  // from n = 768 columns (it was 512 when it went in; re-measured on the final round-5 forms, walking step: n = 512
  // h0 12.90-13.04 vs h1 13.24-13.25 us, n = 800 equal, 13.76-13.91 either way -- profiles/r5/kbench_head_dw2_r5end.jsonl)
  int head_dw2 = -1;
  int xp_dbg = 0;       // SplitStepArgs::xp_dbg (diagnostics)
  int g64_touch = 0;    // SplitStepArgs::g64_touch (measured slower: 784-4096-10 bf16 38.1 -> 41.7 us,
                        // fp32 57.5 -> 62.6, profiles/r5/kbench_wide_touch.jsonl)
  int ag64() const { return ag_tiles64 >= 0 ? ag_tiles64 : (store_a1 ? 0 : 1); }
  // data-parallel step with the xGMI gradient all-reduce + SGD fused into the wgrad launch (run(sgd=2))
  XgmiFuse xf;
  // push != 0: the owner-tile push form (XgmiFuse::push; the bucket must have slab_tiles >= the launch's tiles)
  XgmiFuse* xf_dev = nullptr;  // its device copy (SplitStepArgs::xf): allocated once, so captured graphs stay valid
  // The XCD-local step pipeline (mlp_xstep, csrc/mlp/xstep.hip): run_steps runs the whole plan in ONE persistent
  // launch when the plan's step has the pipeline's shape (H <= 128 split3, fragment-ordered operands, the head's dW2
  // partials, fused SGD, one process, steps on the 16-sample grid); -1 auto (on), 0 off, 1 required (an error if
  // the plan does not qualify).
  int xstep = -1;
  int xstep_pix = 1;      // XStepPlan::pix: the dW1 tiles' pixel operand (0 XT, 1 the forward's copy through LDS)
  int xstep_used = 0;     // the last run_steps ran as one xstep launch (tests, bench records)
  std::string xstep_reason = "";  // why the last run_steps did not take the pipeline ("" when it did)
  unsigned xs_ep = 1, xs_launch = 0;  // the next step's granule tag; launches so far (control bank)
  unsigned long long *xs_gran = nullptr, *xs_ctl = nullptr;
  float *xs_dx = nullptr, *xs_b2x = nullptr;
  uintptr_t xs_stamps = 0;  // diagnostics: [xs_stamp_steps][8][32][4] uint64 (bench/stamps_xstep.py)
  int xs_stamp_steps = 0;
  uintptr_t xs_w1stamps = 0;  // diagnostics: XStepPlan::w1stamps, kXstepW1Stamps uint64 (bench/xstep_ab.py --w1-stamps)
  float xscale = 1.f;    // split path: inputs are uint8 * xscale
  uintptr_t W1p = 0, dZ1p = 0;
  // wide split3 layers: the in-place dW1 update skips the W1-plane refresh (SplitStepArgs::w1_planes_lazy) and
  // planes_stale records it; refresh_planes() re-splits W1 before any forward that reads the planes
  int lazy_planes = 0;
  bool planes_stale = false;
  void refresh_planes(uintptr_t stream) {
    if (!planes_stale) return;
    mlp_split_planes(P_<float>(W1), reinterpret_cast<void*>(W1p), (int64_t)H * P, npw, S(stream));
    planes_stale = false;
  }
  uintptr_t kpart = 0;  // split-K dW1 partial slabs (SplitStepArgs::kpart), kpart_cap floats; 0: no split-K
  int64_t kpart_cap = 0;

  ~MlpStep() {
    if (xf_dev) (void)hipFree(xf_dev);
    for (void* q : {(void*)xs_gran, (void*)xs_ctl, (void*)xs_dx, (void*)xs_b2x})
      if (q) (void)hipFree(q);
  }
  void set_xgmi(uintptr_t desc, int64_t slots, int64_t off_b1, int64_t off_W2, int64_t off_b2, int push = 0);
  // the step's buffers, shapes and the policies that depend on the shape alone, for samples [off, off + n)
  SplitStepArgs split_args(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss) const;

  // The decision (split paths): how run() with these arguments runs the step.  Enqueues nothing, changes no state.
  StepForm plan(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss, int parts = 3,
                int64_t pf_next = -1, StepOverrides ov = {}) const;
  // The native step loop's plan as ONE XCD-local pipeline launch: nullptr and the plan's step in `p` (p.w and p.h: the
  // launch's arguments), or why it does not qualify -- its step as the two-launch form would run it under the
  // pipeline's StepOverrides is not the all-gather forward + head reading fp32 W1 from its copy, or not the pipeline's
  // shape (mlp_xstep_ok).  stream: also refuses a stream that is capturing a graph (nullptr: not looked at).
  const char* plan_steps(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end,
                         double scale, double reg, double lr, const hipStream_t* stream, StepForm& p) const;

  // Forward + backward for samples [off, off+n) of the resident dataset.
  // sgd=1 applies the update in place (single process); sgd=0 writes the
  // pre-scaled gradients into the bucket for the all-reduce; sgd=2 all-reduces over xGMI and applies
  // the update inside the wgrad launch (set_xgmi, split path).
  // parts: bit0 = forward + head, bit1 = weight gradients / update (profiling hook; default both);
  //        with bit0: +4 skips the head (forward GEMM only), +8 skips the forward GEMM (head only)
  // pf_next: the next step's first sample (the native step loop knows it): its pixels are prefetched by this step's
  // weight-gradient launch (SplitStepArgs::pf_X)
  void run(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss, uintptr_t stream,
           int parts = 3, int64_t pf_next = -1);
  // the whole plan as one XCD-local pipeline launch; false (nothing enqueued) when the plan does not qualify
  bool run_xstep(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end, double scale,
                 double reg, double lr, uintptr_t stream);
  // Native step loop: `count` consecutive global batches of B samples starting at gstart0 (wrapping to 0
  // when a batch would pass N_end), this rank's shard [gstart + shard_off, +n) of each, every kernel
  // launched from here with no Python between steps.  sgd = 1: single process, SGD fused into wgrad;
  // sgd = 2: the xGMI all-reduce + SGD fused into wgrad (set_xgmi).  The eager counterpart of a captured
  // epoch graph: the first kernel starts one launch after the call instead of after a whole-graph
  // submission (bench/launch_overhead.py: ~7 us less fixed cost per timed run, equal per-step cost).
  void run_steps(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end, double scale,
                 double reg, double lr, int sgd, uintptr_t stream);
  // Weight-gradient pieces of a step whose forward + head already ran (parts=1): used by the
  // trainer to overlap per-bucket all-reduces with the rest of the backward pass.
  // parts bit0 = dW1 rows [row0, row0+rows), bit1 = dW2 + bias gradients.  Split paths only.
  void run_wgrad(int64_t off, int n, double scale, double reg, double lr, int sgd, int parts, int row0, int rows,
                 uintptr_t stream);
  // ---- tensor parallel over the hidden dimension (split paths; parallel/tensor_parallel.py)
  // forward GEMM of this rank's hidden shard only; with z2p != 0 the LDS GEMM also leaves the z2 row-tile
  // partials there.  Returns how many it wrote (0: the caller forms W2_s . a1_s itself).
  int tp_forward(int64_t off, int n, uintptr_t z2p_, uintptr_t stream);
  // head on the all-reduced pre-activation z2 ([16][ld], without b2): softmax / loss / D for every
  // column, dZ1 (+ planes) for this rank's hidden rows
  void tp_head(int64_t off, int n, double scale, int with_loss, uintptr_t z2full, uintptr_t stream);
  // split path forward + argmax for n samples at x (uint8 [n][P]); a1buf: [H][lda] scratch.  The
  // tiled forward (wave-split-K: the wide engines' bf16 copies are of the training set, not of x)
  // into a1buf, then the column head in predict mode
  void predict(uintptr_t x, int n, uintptr_t a1buf, int lda, uintptr_t pred, uintptr_t stream);
  // split path forward + evaluation head (eval.h) for n samples at x (uint8 [n][P]) with labels (int32 [n]): the same
  // forward as predict into a1buf, then loss / hits / confusion counts into the slot `stats` (partials: the head's
  // loss scratch).  zero = 1 on an evaluation's first chunk.  Enqueues only (legal under stream capture; there the
  // first chunk re-splits the W1 planes whenever a step's in-place update may leave them stale -- the replay cannot
  // decide -- and the later chunks of the captured evaluation rely on it)
  void evaluate(uintptr_t x, uintptr_t labels_, int n, uintptr_t a1buf, int lda, uintptr_t stats, uintptr_t partials,
                uintptr_t stream, int zero = 0);
  bool w1_planes_read() const {  // a forward kernel of this step reads the W1 planes (else: not refreshed)
    return split != 0 && mlp_split_w1_planes_read(split_args(0, ld, 1.0, 0.0, 0.0, 1, 0));
  }
  bool lazy_planes_apply() const {  // this step's in-place W1 update leaves the planes stale (lazy_planes on)
    if (!split || !lazy_planes) return false;
    SplitStepArgs a = split_args(0, ld, 1.0, 0.0, 0.0, 1, 0);
    a.w1_planes_lazy = 1;
    return mlp_split_wgrad_leaves_planes_stale(a);
  }
  // the f64 / plain MFMA step (mlp_kernels.h): three launches
  void run_plain(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss, uintptr_t stream,
                 int parts);

  template <typename T>
  static T* P_(uintptr_t p) { return reinterpret_cast<T*>(p); }
  static hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
};

}  // namespace cme
