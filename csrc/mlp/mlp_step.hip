// MlpStep (mlp_step.h): host code only -- the step's decision (plan), its execution (run) and the native step loop.
#include "mlp_step.h"

#include "../comm/xgmi_allreduce.h"

namespace cme {
namespace {

// the head over the buffers of `a`; a predict / probs head reads the forward's side only (the caller sets its output)
HeadArgs head_args(const SplitStepArgs& a, int mode) {
  HeadArgs h{};
  h.a1 = a.a1; h.lda = a.ld; h.W2 = a.W2; h.b2 = a.b2; h.H = a.H; h.C = a.C; h.n = a.n; h.shift = a.shift;
  h.mode = mode;
  if (mode != HEAD_TRAIN) return h;
  h.labels = a.labels; h.scale = a.scale; h.D = a.D; h.ldd = a.ld; h.dZ1 = a.dZ1; h.ldz = a.ld;
  h.dZ1_planes = a.dZ1p; h.npz = a.npz; h.loss_partial = a.loss_partial;
  return h;
}

}  // namespace

void MlpStep::set_xgmi(uintptr_t desc, int64_t slots, int64_t off_b1, int64_t off_W2, int64_t off_b2, int push) {
  if (!desc) {
    xf = XgmiFuse{};  // (the device copy is read only by sgd = 2 launches, which now refuse to run)
    return;
  }
  CME_REQUIRE(split && bias_col && XT, "MlpStep.set_xgmi: split path with the all-ones XT feature only");
  CME_REQUIRE(mlp_split_fused_tiles(P, H, (int)std::min<int64_t>(slots, 1 << 30)) > 0,
              "MlpStep.set_xgmi: the bucket has fewer flag slots than the wgrad launch has tiles");
  const auto* d = reinterpret_cast<const comm::XgmiDesc*>(desc);
  CME_REQUIRE(d->world >= 1 && d->world <= 8 && d->mybuf && d->n >= off_b2 + C,
              "MlpStep.set_xgmi: bucket not open or smaller than the flat gradient");
  XgmiFuse f;
  f.mybuf = d->mybuf;
  for (int r = 0; r < d->world; ++r) {
    CME_REQUIRE(d->peers[r] && d->peerflags[r], "MlpStep.set_xgmi: peer handles not opened");
    f.peers[r] = d->peers[r];
    f.peerflags[r] = d->peerflags[r];
  }
  f.myflags = d->myflags;
  f.epochs = d->epochs;
  f.err = d->err;
  f.rank = d->rank;
  f.world = d->world;
  f.npad = d->npad;
  f.off_b1 = off_b1;
  f.off_W2 = off_W2;
  f.off_b2 = off_b2;
  if (push) {
    CME_REQUIRE(d->myslab && d->slab_tiles >= mlp_split_fused_tiles(P, H, 1 << 30),
                "MlpStep.set_xgmi(push): the bucket's receive areas are missing or smaller than the launch's tiles");
    f.push = 1;
    f.myslab = d->myslab;
    f.slab_tiles = d->slab_tiles;
    for (int r = 0; r < d->world; ++r) {
      CME_REQUIRE(d->peerslabs[r], "MlpStep.set_xgmi(push): peer receive areas not mapped");
      f.peerslab[r] = d->peerslabs[r];
    }
  }
  xf = f;
  if (!xf_dev) HIP_CHECK(hipMalloc(&xf_dev, sizeof(XgmiFuse)));
  // every launch already enqueued (on any stream, or replayed from a graph) reads the device copy: it finishes
  // before the copy changes under it.  A graph captured against the old bucket must not be replayed afterwards --
  // DataParallelTrainer drops its captured graphs wherever it attaches or detaches a bucket.
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(xf_dev, &xf, sizeof(XgmiFuse), hipMemcpyHostToDevice));
}

SplitStepArgs MlpStep::split_args(int64_t off, int n, double scale, double reg, double lr, int sgd,
                                  int with_loss) const {
  SplitStepArgs a;
  a.P = P; a.H = H; a.C = C; a.n = n; a.ld = ld; a.npw = npw; a.npz = npz;
  a.X = reinterpret_cast<const char*>(X) + (size_t)off * P;  // uint8 dataset
  a.XT = reinterpret_cast<const char*>(XT) + (size_t)off;
  a.xscale = xscale;
  a.ldxt = (int)N;
  if (Xw) a.Xw = reinterpret_cast<const char*>(Xw) + (size_t)off * P * 2;
  if (XTw) a.XTw = reinterpret_cast<const char*>(XTw) + (size_t)off * 2;
  a.labels = P_<int>(labels) + off;
  a.W1 = P_<float>(W1); a.b1 = P_<float>(b1); a.W2 = P_<float>(W2); a.b2 = P_<float>(b2);
  a.W1p = reinterpret_cast<void*>(W1p);
  a.gW1 = P_<float>(gW1); a.gb1 = P_<float>(gb1); a.gW2 = P_<float>(gW2); a.gb2 = P_<float>(gb2);
  a.a1 = P_<float>(a1); a.D = P_<float>(D); a.dZ1 = P_<float>(dZ1);
  a.dZ1p = reinterpret_cast<void*>(dZ1p);
  a.loss_partial = with_loss ? P_<float>(loss) : nullptr;
  a.scale = scale; a.reg = reg; a.lr = lr; a.sgd = sgd; a.shift = shift; a.mode = 0;
  a.stamps = reinterpret_cast<unsigned long long*>(stamps);
  a.wstamps = reinterpret_cast<unsigned long long*>(wstamps);
  a.bias_col = bias_col;
  // split3 small layers, measured (bench/kbench.py): fp32 W1 split in registers always (one split per weight
  // per column tile is cheaper than pulling 6 B); fp32 dZ1 above H = 128, where the separate head's plane
  // stores cost ~2 us at H = 300, and -- since round 5 (the head's dW2 partials, the fragment-ordered forward
  // operands and dZ1, dz_swz) -- at H <= 128 from n = 200 columns: the head's three plane stores cost more than the
  // dW1 tiles' re-split (walking step at n = 800 14.24 -> 14.02-14.07 us, n = 512 14.09-14.15 -> 13.33-13.36,
  // n = 400 12.94-12.96 -> 12.67-12.76; n = 100 +0.04-0.16 us, so planes there: profiles/r5/kbench_dz_fp32_r5.jsonl).
  // The decision depends only on the step's shape, so the head and every weight-gradient call of a step agree.
  // (The wide engines always split fp32 operands.)
  a.a_fp32 = a_fp32 >= 0 ? a_fp32 : (H <= 128 ? (n >= 200 ? 3 : 1) : 3);
  a.kpart = P_<float>(kpart);
  a.kpart_cap = kpart_cap;
  // a timed-out all-gather forward + head launch (sticky word) makes every later update a no-op
  a.ag_err = P_<const int>(ag_err);
  a.gstatus = P_<float>(gstatus);
  a.ag_wait_us = ag_wait_us;
  a.ag_test_skip = ag_test_skip;
  a.xcd_rows = xcd_rows && mlp_split_xcd_rows_ok(a) ? 1 : 0;
  if (a.xcd_rows && xcd_pack && mlp_split_xcd_rows_packed_ok(a)) a.xcd_rows = 2;
  a.pf_wgs = (a.xcd_rows && bias_col) ? prefetch : 0;
  a.pf_wgs_xt = (a.xcd_rows && bias_col) ? prefetch_xt : 0;
  a.wide_eng = wide_eng >= 0 ? wide_eng : (npw == 1 ? 1 : 0);
  a.xp_dbg = xp_dbg;
  a.g64_touch = g64_touch;
  return a;
}

StepForm MlpStep::plan(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss, int parts,
                       int64_t pf_next, StepOverrides ov) const {
  CME_REQUIRE(split && n > 0 && n <= ld, "MlpStep.plan: split (bf16-plane) paths, 0 < n <= ld");
  CME_REQUIRE(XT != 0 && W1p != 0 && dZ1p != 0, "MlpStep.run: split path needs XT, W1p, dZ1p");
  StepForm p;
  SplitStepArgs& a = p.w;  // (the forward's arguments are copied from it where the two launches part)
  HeadArgs& h = p.h;
  a = split_args(off, n, scale, reg, lr, sgd == 2 ? 0 : sgd, with_loss);
  // the forward reads the fragment-ordered W1 copy (rebuilt first if anything but this step's update wrote W1)
  const bool swz = w1_swz && w1s && mlp_fwd_swz_ok(a);
  p.refresh_swz = swz;
  p.mark_swz_stale = !swz && sgd;  // (this step's update does not write the copy)
  if (swz) {
    a.w1_swz = 1;
    a.W1s = P_<float>(w1s);
  }
  // ... and the pixels from theirs when this step's samples start a 16-sample tile of it
  const int64_t xs_tile = (int64_t)((P + 63) / 64) * 1024;  // bytes per 16 samples
  const bool xsw = swz && x_swz && xs;
  const bool x_frag = xsw && (ov.rm_unless_frag ? ov.grid16 : off % 16 == 0);
  // the fragment-ordered fp32 dZ1 applies (whole steps; small: the all-gather head, else the wide fused head)
  auto dz_frag = [&](bool small) {
    if (!dz_swz || !dz1s || (parts & 3) != 3) return false;
    SplitStepArgs t = a;
    t.dZ1 = P_<float>(dz1s);
    return small ? swz && mlp_wgrad_dz_swz_ok(t) : mlp_wgrad_dzr_ok(t);
  };
  const bool rm = ov.rm_unless_frag && !(x_frag && mlp_split_wgrad_fp32_dz(a) && dz_frag(true));
  if (rm) a.a_fp32 |= 2;  // (fp32 dZ1, row-major)
  if (x_frag && !rm) {
    a.x_swz = 1;
    a.Xs = reinterpret_cast<const char*>(xs) + off / 16 * xs_tile;
  }
  // (only the rows that exist: the next step's shard may be shorter than this one, or past the dataset's end)
  if (pf_next >= 0 && pf_next < N && a.pf_wgs) {  // (the copy the next step's forward will read)
    const int64_t rows = std::min<int64_t>(n, N - pf_next);
    if (xsw && pf_next % 16 == 0) {
      a.pf_X = reinterpret_cast<const char*>(xs) + pf_next / 16 * xs_tile;
      a.pf_bytes = (rows + 15) / 16 * xs_tile;
    } else {
      a.pf_X = reinterpret_cast<const char*>(X) + (size_t)pf_next * P;
      a.pf_bytes = rows * P;
    }
  }
  if (sgd == 2) {  // all-reduce + SGD inside the wgrad launch
    CME_REQUIRE(xf.world > 0 && xf_dev, "MlpStep.run(sgd=2): set_xgmi() first");
    a.xf = xf_dev;
    a.xf_world = xf.world;
    a.xf_push = xf.push;
  }
  if (parts & 1) {  // the forward GEMM + the head (fused into one launch where the shapes allow)
    h = head_args(a, HEAD_TRAIN);
    h.z2part = P_<float>(z2p);
    h.stamps = P_<unsigned long long>(hstamps);
    // the dW1 GEMM splits fp32 dZ1 in registers: the head writes fp32 dZ1 and no planes
    const bool dz32 = mlp_split_wgrad_fp32_dz(a);
    if (dz32) h.dZ1_planes = nullptr;
    // (the small forms read the planes unless they split fp32 W1 in registers; the wide forms below decide
    // by their kernel)
    p.refresh_planes = H < 512 && !mlp_split_fwd_fp32_w(a);
    if (fh_allgather && ag_counters && ag_slabs && ag_err && !(parts & 12) && mlp_fwd1_head_ok(a, h) &&
        mlp_fwd1_head_ag_fits(a)) {
      p.fwd = StepForm::kAllGather;
      p.f = a;
      // training (store_a1 off): with the all-ones XT feature the dW1 launch reads only the dZ1 planes (db1 is
      // its column P) unless it splits fp32 dZ1 itself -- the fp32 dZ1 store is then skipped
      if (!store_a1 && bias_col && !dz32 && h.dZ1_planes) h.dZ1 = nullptr;
      // the head writes the fragment-ordered dZ1, the dW1 GEMM reads it
      if (!rm && dz32 && !h.dZ1_planes && dz_frag(true)) {
        h.dZ1 = a.dZ1 = P_<float>(dz1s);
        h.dz_swz = a.dz_swz = 1;
      }
      const int hd = ov.dw2_every_n && head_dw2 < 0 ? 1 : head_dw2;
      if ((hd > 0 || (hd < 0 && n >= 768)) && dw2p && C <= 16) {  // the head leaves the dW2 partials (fha_body step 5); then
        // nothing after this launch reads a1: not stored in training (store_a1 off)
        h.dw2part = a.dw2part = P_<float>(dw2p);
        a.dw2_cols = 16;  // (fha_body step 4a: two partials per 32-column tile)
        if (!store_a1) h.a1 = p.f.a1 = nullptr;
      }
    } else if (fh_counters && !(parts & 12) && mlp_fwd1_head_ok(a, h)) {  // one launch
      p.fwd = StepForm::kLastArriver;
      p.f = a;
    } else {
      // wide layers: the forward GEMM also leaves the head's z2 partials (unless only the head runs)
      SplitStepArgs& f = p.f;
      f = a;
      // (the partials are 16-class: with more classes the forward leaves none and the many-class head forms z2)
      f.z2part = (z2p && !(parts & 8) && C <= 16) ? P_<float>(z2p) : nullptr;
      h.z2_chunks = f.z2part ? mlp_split_fwd1_z2_chunks(f) : 0;
      // with the all-ones XT feature nothing reads dZ1 in fp32 on the wide path (db1 comes out of
      // the dW1 GEMM over the planes): skip those 4 B/element of HBM writes
      if (h.z2_chunks > 0 && bias_col) h.dZ1 = nullptr;
      // ... unless the dW1 GEMM splits fp32 dZ1 in registers: then fp32 dZ1 and no planes
      if (dz32) h.dZ1 = a.dZ1;
      // the head leaves dW2 partials for the wgrad launch
      if (h.z2_chunks > 0 && dw2p && !(parts & 4)) h.dw2part = a.dw2part = P_<float>(dw2p);
      const bool ag = fh_allgather && ag_counters && ag_err && ag_gran && h.dw2part && !(parts & 12) &&
                      mlp_fwd1_wide_ag_ok(f, h, ag64());
      if (!(parts & 8) && mlp_split_wide_fwd_reads_planes(f, ag, ag64())) p.refresh_planes = true;
      if (ag && dz32 && h.dZ1 && dz_frag(false)) {  // the wide head writes dZ1 in the dW1 K loop's fragment order
        h.dZ1 = a.dZ1 = P_<float>(dz1s);
        h.dz_swz = a.dz_swz = 2;
      }
      p.fwd = ag ? StepForm::kWide : StepForm::kSeparate;  // one launch: forward GEMM + the all-gather head
      p.store_a1 = store_a1;
      // (its tile, which mlp_fwd1_wide_ag returns: 128 where the 128 x 128 engine takes the layer without allow64)
      if (ag) a.dw2_cols = mlp_fwd1_wide_ag_ok(f, h, 0) ? 128 : 64;
      p.run_fwd = !ag && !(parts & 8);
      p.run_head = !ag && !(parts & 4);
    }
    // what run_wgrad (the rest of this step's backward) reads: did this forward leave dW2 partials
    p.left = {a.dw2part != nullptr, a.dw2_cols, a.dz_swz};
  } else if (dw2p && left.dw2) {  // the backward half alone (profiling): the partials of the last forward
    a.dw2part = P_<float>(dw2p);
    a.dw2_cols = left.dw2_cols;
  }
  if ((p.run_wgrad = parts & 2)) {
    a.w1_planes_lazy = lazy_planes;  // (what the predicate asks about; kept only where nothing reads the planes)
    a.w1_planes_lazy = mlp_split_wgrad_leaves_planes_stale(a) ? 1 : 0;
    p.planes_left_stale = a.w1_planes_lazy;
  }
  return p;
}

void MlpStep::run(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss, uintptr_t stream,
                  int parts, int64_t pf_next) {
  CME_REQUIRE(n > 0 && n <= ld, "MlpStep.run: 0 < n <= ld required");
  if (!split) return run_plain(off, n, scale, reg, lr, sgd, with_loss, stream, parts);
  const StepForm p = plan(off, n, scale, reg, lr, sgd, with_loss, parts, pf_next);
  if (p.refresh_swz) refresh_swz(stream);
  if (p.mark_swz_stale) swz_stale = true;
  if (p.refresh_planes) refresh_planes(stream);
  if (p.fwd == StepForm::kAllGather)
    mlp_fwd1_head_ag(p.f, p.h, P_<unsigned long long>(ag_counters), P_<unsigned long long>(ag_slabs),
                     P_<int>(ag_err), fh_tiles, S(stream));
  else if (p.fwd == StepForm::kLastArriver)
    mlp_fwd1_head(p.f, p.h, P_<unsigned>(fh_counters), fh_tiles, S(stream));
  else if (p.fwd == StepForm::kWide)
    CME_REQUIRE(mlp_fwd1_wide_ag(p.f, p.h, P_<unsigned long long>(ag_counters), fh_tiles,
                                 P_<unsigned long long>(ag_gran), ag_gran_count, P_<int>(ag_err), p.store_a1, ag64(),
                                 S(stream)) == p.w.dw2_cols,
                "MlpStep.run: the fused wide head ran on another tile than planned");
  if (p.run_fwd) mlp_split_fwd1(p.f, S(stream));  // (kSeparate)
  if (p.run_head) mlp_head(DType::F32, p.h, S(stream));
  if (parts & 1) left = p.left;
  if (p.run_wgrad) mlp_split_wgrad(p.w, S(stream));
  if (p.planes_left_stale) planes_stale = true;
}

void MlpStep::run_plain(int64_t off, int n, double scale, double reg, double lr, int sgd, int with_loss,
                        uintptr_t stream, int parts) {
  CME_REQUIRE(sgd != 2, "MlpStep.run(sgd=2): split paths only");
  CME_REQUIRE(dt >= 0 && dt <= 2, "dtype code must be 0 (f32), 1 (f64) or 2 (bf16)");
  const DType d = static_cast<DType>(dt);
  const size_t xe = d == DType::F64 ? 8 : (d == DType::BF16 ? 2 : 4);
  const void* Xb = reinterpret_cast<const char*>(X) + (size_t)off * P * xe;
  const int* lab = P_<int>(labels) + off;
  if (parts & 1)
    mlp_forward1(d, reinterpret_cast<void*>(W1g), reinterpret_cast<void*>(b1), Xb, P, H, n,
                 reinterpret_cast<void*>(a1), ld, act, S(stream));
  HeadArgs h{};
  h.a1 = reinterpret_cast<void*>(a1); h.lda = ld;
  h.W2 = reinterpret_cast<void*>(W2); h.b2 = reinterpret_cast<void*>(b2);
  h.labels = lab; h.H = H; h.C = C; h.n = n; h.scale = scale;
  h.D = reinterpret_cast<void*>(D); h.ldd = ld;
  h.dZ1 = reinterpret_cast<void*>(dZ1); h.ldz = ld;
  h.dZ1_bf16 = d == DType::BF16 ? reinterpret_cast<void*>(dZ1g) : nullptr;
  h.loss_partial = with_loss ? P_<float>(loss) : nullptr;
  h.shift = shift; h.mode = HEAD_TRAIN;
  h.z2part = P_<float>(z2p);
  if (parts & 1) mlp_head(d, h, S(stream));
  WgradArgs w{};
  w.roles = 7;
  w.dZ1g = reinterpret_cast<void*>(d == DType::BF16 ? dZ1g : dZ1); w.ldz = ld;
  w.X = Xb; w.P = P;
  w.XT = XT ? reinterpret_cast<const char*>(XT) + (size_t)off * xe : nullptr;
  w.ldxt = (int)N;
  w.dZ1 = reinterpret_cast<void*>(dZ1);
  w.D = reinterpret_cast<void*>(D); w.ldd = ld;
  w.a1 = reinterpret_cast<void*>(a1); w.lda = ld;
  w.H = H; w.C = C; w.n = n; w.reg = reg; w.lr = lr; w.sgd = sgd;
  w.W1 = reinterpret_cast<void*>(W1); w.b1 = reinterpret_cast<void*>(b1);
  w.W2 = reinterpret_cast<void*>(W2); w.b2 = reinterpret_cast<void*>(b2);
  w.gW1 = reinterpret_cast<void*>(gW1); w.gb1 = reinterpret_cast<void*>(gb1);
  w.gW2 = reinterpret_cast<void*>(gW2); w.gb2 = reinterpret_cast<void*>(gb2);
  w.W1_bf16 = d == DType::BF16 ? reinterpret_cast<void*>(W1g) : nullptr;
  if (parts & 2) mlp_wgrad(d, w, S(stream));
}

const char* MlpStep::plan_steps(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end,
                                double scale, double reg, double lr, const hipStream_t* stream, StepForm& p) const {
  if (xstep == 0) return "off";
  if (count <= 0 || count > (1 << 30) || gstart0 % 4 || B % 4 || shard_off % 4)
    return "the plan's steps start off 4-byte aligned pixel columns";
  if (stream) {  // (granule tags come from the host: never replayed)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_CHECK(hipStreamIsCapturing(*stream, &cap));
    if (cap != hipStreamCaptureStatusNone) return "the stream is capturing a graph";
  }
  // what the pipeline needs bound and switched on
  if (!split || !XT || !W1p || !dZ1p || !w1s || !dw2p || !bias_col) return "not the split3 H <= 128 layout";
  if (!fh_allgather || !ag_counters || !ag_slabs || !ag_err) return "the all-gather forward + head is off";
  if (!w1_swz) return "the fragment-ordered W1 is off";
  if (C > 16 || head_dw2 == 0) return "the head leaves no dW2 partials";
  // the plan's step as the two-launch form runs it (SGD fused into the weight-gradient launch)
  const int64_t g0 = gstart0 + B > N_end ? 0 : gstart0;
  StepOverrides ov;
  ov.dw2_every_n = ov.rm_unless_frag = true;
  ov.grid16 = gstart0 % 16 == 0 && B % 16 == 0 && shard_off % 16 == 0;
  p = plan(g0 + shard_off, n, scale, reg, lr, 1, 0, 3, -1, ov);
  if (!p.f.w1_swz || mlp_split_w1_planes_read(p.f)) return "the forward would not read fp32 W1";
  if (!p.w.dz_swz) {  // the pipeline's row-major form
    if (xs_stamps || xs_w1stamps || hstamps || ag_test_skip >= 0) return "the row-major form has no diagnostics build";
    if (!mlp_xstep_rm(p.w)) return "the row-major form needs n % 4 == 0 and 4-byte aligned pixel columns";
  }
  if (p.fwd != StepForm::kAllGather) return "the all-gather head does not fit";
  p.w.a1 = p.f.a1;  // (one launch runs both halves: the forward's a1, not stored once the head leaves the dW2 partials)
  return mlp_xstep_ok(p.w, p.h) ? nullptr : "mlp_xstep_ok";
}

bool MlpStep::run_xstep(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end,
                        double scale, double reg, double lr, uintptr_t stream) {
  const hipStream_t s = S(stream);
  StepForm f;
  if (const char* why = plan_steps(gstart0, count, B, shard_off, n, N_end, scale, reg, lr, &s, f)) {
    xstep_reason = why;
    return false;
  }
  xstep_reason.clear();
  refresh_swz(stream);
  if (!xs_gran) {
    HIP_CHECK(hipMalloc(&xs_gran, kXstepGranules * 8));
    HIP_CHECK(hipMemset(xs_gran, 0, kXstepGranules * 8));
    HIP_CHECK(hipMalloc(&xs_ctl, kXstepCtlWords * 8));
    HIP_CHECK(hipMemset(xs_ctl, 0, kXstepCtlWords * 8));
    HIP_CHECK(hipMalloc(&xs_dx, (size_t)8 * 16 * ld * 4));
    HIP_CHECK(hipMalloc(&xs_b2x, (size_t)8 * 16 * 4));
    HIP_CHECK(hipDeviceSynchronize());
  }
  XStepPlan p;
  p.gstart0 = gstart0; p.B = B; p.shard_off = shard_off; p.N_end = N_end; p.count = (int)count;
  p.X0 = P_<const uint8_t>(X); p.XT0 = P_<const uint8_t>(XT); p.Xs0 = P_<const uint8_t>(xs);
  p.lab0 = P_<const int>(labels);
  p.xs_tile = (int64_t)((P + 63) / 64) * 1024;
  p.ep0 = xs_ep; p.launch = xs_launch;
  p.gran = xs_gran; p.ctl = xs_ctl; p.Dx = xs_dx; p.b2x = xs_b2x; p.err = P_<int>(ag_err);
  p.nw = mlp_xstep_workers(f.w);
  p.pix = xstep_pix;
  p.stamps = reinterpret_cast<unsigned long long*>(xs_stamps);
  p.stamp_steps = xs_stamps ? xs_stamp_steps : 0;
  p.w1stamps = reinterpret_cast<unsigned long long*>(xs_w1stamps);
  mlp_xstep(f.w, f.h, p, s);
  xs_ep += (unsigned)count;
  xs_launch += 1;
  left = f.left;
  return true;
}

void MlpStep::run_steps(int64_t gstart0, int64_t count, int64_t B, int64_t shard_off, int n, int64_t N_end,
                        double scale, double reg, double lr, int sgd, uintptr_t stream) {
  CME_REQUIRE(count >= 0 && n > 0 && n <= ld && B >= n && N_end >= B && (sgd == 1 || sgd == 2),
              "MlpStep.run_steps: bad step plan");
  if (count == 0) return;
  xstep_used = sgd == 1 && run_xstep(gstart0, count, B, shard_off, n, N_end, scale, reg, lr, stream) ? 1 : 0;
  CME_REQUIRE(xstep_used || xstep != 1 || sgd != 1,
              "MlpStep.run_steps: xstep = 1 but the plan's step does not qualify: " + xstep_reason);
  if (xstep_used) return;
  int64_t gs = gstart0;
  for (int64_t i = 0; i < count; ++i) {
    if (gs + B > N_end) gs = 0;
    const int64_t nx = gs + B + B > N_end ? 0 : gs + B;  // (the next step's batch, wrap included)
    run(gs + shard_off, n, scale, reg, lr, sgd, 0, stream, 3, nx + shard_off);
    gs += B;
  }
}

void MlpStep::run_wgrad(int64_t off, int n, double scale, double reg, double lr, int sgd, int parts, int row0,
                        int rows, uintptr_t stream) {
  CME_REQUIRE(split, "MlpStep.run_wgrad: split (bf16-plane) paths only");
  CME_REQUIRE(n > 0 && n <= ld, "MlpStep.run_wgrad: 0 < n <= ld required");
  SplitStepArgs a = split_args(off, n, scale, reg, lr, sgd, 0);
  if (sgd) swz_stale = true;  // (an in-place update here does not maintain the forward's W1 copy)
  a.wg_parts = parts;
  a.w1_row0 = row0;
  a.w1_rows = rows;
  if (dw2p && left.dw2) {  // the forward + head half (run(parts=1)) of this step left dW2 partials
    a.dw2part = P_<float>(dw2p);
    a.dw2_cols = left.dw2_cols;
  }
  mlp_split_wgrad(a, S(stream));
}

int MlpStep::tp_forward(int64_t off, int n, uintptr_t z2p_, uintptr_t stream) {
  CME_REQUIRE(split && n > 0 && n <= ld, "MlpStep.tp_forward: split path, 0 < n <= ld");
  SplitStepArgs a = split_args(off, n, 1.0, 0.0, 0.0, 1, 0);
  a.z2part = z2p_ ? P_<float>(z2p_) : nullptr;
  refresh_planes(stream);
  mlp_split_fwd1(a, S(stream));
  return a.z2part ? mlp_split_fwd1_z2_chunks(a) : 0;
}

void MlpStep::tp_head(int64_t off, int n, double scale, int with_loss, uintptr_t z2full, uintptr_t stream) {
  CME_REQUIRE(split && n > 0 && n <= ld && z2full, "MlpStep.tp_head: split path, 0 < n <= ld, z2 buffer");
  HeadArgs h = head_args(split_args(off, n, scale, 0.0, 0.0, 1, with_loss), HEAD_TRAIN);
  h.z2part = P_<float>(z2full);
  h.z2_chunks = 1;
  mlp_head(DType::F32, h, S(stream));
}

void MlpStep::predict(uintptr_t x, int n, uintptr_t a1buf, int lda, uintptr_t pred, uintptr_t stream) {
  refresh_planes(stream);
  SplitStepArgs a = split_args(0, n, 1.0, 0.0, 0.0, 0, 0);
  a.X = reinterpret_cast<const void*>(x);
  a.Xw = nullptr;
  a.a1 = reinterpret_cast<float*>(a1buf);
  a.ld = lda;
  mlp_split_fwd1(a, S(stream));
  HeadArgs h = head_args(a, HEAD_PREDICT);
  h.pred = reinterpret_cast<int*>(pred);
  mlp_head(DType::F32, h, S(stream));
}

void MlpStep::evaluate(uintptr_t x, uintptr_t labels_, int n, uintptr_t a1buf, int lda, uintptr_t stats,
                       uintptr_t partials, uintptr_t stream, int zero) {
  CME_REQUIRE(split && n >= 0 && n <= lda, "MlpStep.evaluate: split path, 0 <= n <= lda");
  EvalArgs e{};
  e.a1 = reinterpret_cast<const void*>(a1buf); e.lda = lda; e.W2 = P_<float>(W2); e.b2 = P_<float>(b2);
  e.labels = P_<int>(labels_); e.H = H; e.C = C; e.n = n;
  e.stats = P_<unsigned long long>(stats); e.partials = P_<double>(partials); e.zero = zero;
  if (n > 0) {
    // a captured evaluation is replayed after steps the host does not see: where their in-place update leaves the
    // W1 planes stale and this forward reads them, the re-split is part of the capture whatever planes_stale says
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_CHECK(hipStreamIsCapturing(S(stream), &cap));
    if (cap == hipStreamCaptureStatusNone) {
      refresh_planes(stream);
    } else if (zero) {  // (the first chunk's re-split covers the later chunks of the captured evaluation)
      const bool stale = planes_stale;
      if (stale || (W1p && lazy_planes_apply())) {
        planes_stale = true;
        refresh_planes(stream);
      }
      planes_stale = stale;  // (a captured re-split has not run)
    }
    SplitStepArgs a = split_args(0, n, 1.0, 0.0, 0.0, 0, 0);
    a.X = reinterpret_cast<const void*>(x);
    a.Xw = nullptr;
    a.a1 = reinterpret_cast<float*>(a1buf);
    a.ld = lda;
    mlp_split_fwd1(a, S(stream));
  }
  mlp_eval_head(DType::F32, e, S(stream));
}

}  // namespace cme
