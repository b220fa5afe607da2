// Reducing the learning rate on a validation plateau, one header for host and device: the launch behind an evaluation
// (plateau.hip), the apply launch that reads the scale (optim.hip), the CPU bindings `_cpu.plateau_decide` /
// `_cpu.plateau_rate` (the kernel tests' bitwise oracle and the torch backend's implementation) and the trainer's twin
// tests all evaluate the functions below, so the rule is written once.
//
// One decision.  The metric is best.h's: R triples {n, correct, loss_sum} summed in rank order, loss_sum / n for
// monitor = loss (mode min) and correct / n for monitor = accuracy (mode max); every NaN metric is the one quiet NaN.
//
// The record (8 doubles; counts are exact to 2^53, so a device record is eight 8-byte words of one type):
//   [0] evals               decisions taken so far
//   [1] best                the best metric so far
//   [2] bad                 consecutive non-improving decisions
//   [3] cooldown_left       decisions still inside a cooldown
//   [4] scale               the factor on the caller's lr (what the apply launch reads)
//   [5] reductions          the reductions applied so far
//   [6] last_metric
//   [7] last_reduced_index  the decision that reduced last (-1: none)
// and starts as {0, +inf (min) | -inf (max), 0, 0, 1.0, 0, NaN, -1}.
//
// plateau_decide(rec, rule, metric) is torch.optim.lr_scheduler.ReduceLROnPlateau.step, in torch's order:
//   1. better = min, rel: metric < best * (1.0 - threshold)      min, abs: metric < best - threshold
//               max, rel: metric > best * (threshold + 1.0)      max, abs: metric > best + threshold
//      (strict comparisons: a tie is not better; NaN is never better);
//   2. better: best = metric, bad = 0; else bad += 1;
//   3. cooldown_left > 0: cooldown_left -= 1 and bad = 0;
//   4. bad > patience: new = max(scale * factor, min_factor); if scale - new > eps: scale = new, reductions += 1,
//      last_reduced_index = evals; then always cooldown_left = cooldown and bad = 0;
//   5. last_metric = metric, evals += 1.
// patience = p therefore tolerates p bad evaluations and reduces on bad evaluation number p + 1.  The scale is a factor
// on the caller's lr, as a schedule's factors are: with base lr = 1.0, min_lr = min_factor and the same eps torch's
// scheduler produces the same doubles.
//
// plateau_rate(lr_t, scale) = lr_t * scale: lr_t is the rate the apply launch has formed so far (h.lr, or window_rate
// when a schedule window is set), so the update's rate is (lr * f[i]) * scale, in that order.
//
// Host (g++) and device (hipcc) produce the same bits: only + - * /, comparisons and max, contraction off under clang.
#pragma once

#include <cstdint>

#include "best.h"

namespace cme {

enum PlateauThresholdMode { kPlateauRel = 0, kPlateauAbs = 1 };

struct PlateauRule {
  int monitor = kBestLoss;            // kBestLoss: mode min; kBestAccuracy: mode max
  double factor = 0.1;                // 0 < factor < 1
  int patience = 10;                  // >= 0
  double threshold = 1e-4;            // >= 0
  int threshold_mode = kPlateauRel;
  int cooldown = 0;                   // >= 0
  double min_factor = 0.0;            // in [0, 1]
  double eps = 1e-8;                  // >= 0
};

constexpr int kPlateauRecWords = 8;   // doubles per record (64 bytes)
constexpr int kPlateauScaleWord = 4;  // the word the apply launch reads

struct PlateauRecord {
  double evals, best, bad, cooldown_left, scale, reductions, last_metric, last_reduced_index;
};

__host__ __device__ inline PlateauRecord plateau_start(int monitor) {
  const double inf = __builtin_inf();
  return {0.0, monitor == kBestAccuracy ? -inf : inf, 0.0, 0.0, 1.0, 0.0, __builtin_nan(""), -1.0};
}

__host__ __device__ inline PlateauRecord plateau_load(const double* r) {
  return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

__host__ __device__ inline void plateau_store(double* r, const PlateauRecord& p) {
  r[0] = p.evals; r[1] = p.best; r[2] = p.bad; r[3] = p.cooldown_left;
  r[4] = p.scale; r[5] = p.reductions; r[6] = p.last_metric; r[7] = p.last_reduced_index;
}

// what the launcher and the bindings check
inline bool plateau_rule_ok(const PlateauRule& r) {
  return (r.monitor == kBestLoss || r.monitor == kBestAccuracy) && r.factor > 0.0 && r.factor < 1.0 &&
         r.patience >= 0 && r.threshold >= 0.0 &&
         (r.threshold_mode == kPlateauRel || r.threshold_mode == kPlateauAbs) && r.cooldown >= 0 &&
         r.min_factor >= 0.0 && r.min_factor <= 1.0 && r.eps >= 0.0;
}

__host__ __device__ inline double plateau_max(double a, double b) { return a > b ? a : b; }

// -> reduced (the scale changed)
__host__ __device__ inline bool plateau_decide(PlateauRecord& rec, const PlateauRule& rule, double metric) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool better;
  if (rule.monitor == kBestAccuracy) {
    better = rule.threshold_mode == kPlateauRel ? metric > rec.best * (rule.threshold + 1.0)
                                                : metric > rec.best + rule.threshold;
  } else {
    better = rule.threshold_mode == kPlateauRel ? metric < rec.best * (1.0 - rule.threshold)
                                                : metric < rec.best - rule.threshold;
  }
  if (better) {
    rec.best = metric;
    rec.bad = 0.0;
  } else {
    rec.bad = rec.bad + 1.0;
  }
  if (rec.cooldown_left > 0.0) {
    rec.cooldown_left = rec.cooldown_left - 1.0;
    rec.bad = 0.0;
  }
  bool reduced = false;
  if (rec.bad > static_cast<double>(rule.patience)) {
    const double nw = plateau_max(rec.scale * rule.factor, rule.min_factor);
    if (rec.scale - nw > rule.eps) {
      rec.scale = nw;
      rec.reductions = rec.reductions + 1.0;
      rec.last_reduced_index = rec.evals;
      reduced = true;
    }
    rec.cooldown_left = static_cast<double>(rule.cooldown);
    rec.bad = 0.0;
  }
  rec.last_metric = best_isnan(metric) ? __builtin_nan("") : metric;
  rec.evals = rec.evals + 1.0;
  return reduced;
}

__host__ __device__ inline double plateau_rate(double lr_t, double scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return lr_t * scale;
}

// ---- the launch (plateau.hip) -------------------------------------------------------------------------------------
// mlp_plateau: ONE launch behind an evaluation, one workgroup of 64 threads.  Thread 0 reads the one record and the
// decision inputs, runs plateau_decide and stores the advanced record with plain vector stores.  The launch is a single
// workgroup, launches on one stream are ordered and nothing else writes the record, so one record is race-free under
// graph replay (the apply launch only reads word kPlateauScaleWord).  No atomics, no waits, no host sync.
// The decision inputs are exactly one of
//   slot  a stats slot of eval.h, read directly (one process): words 0 and 1 are uint64 counts, word 2 the loss bits;
//   rows  [R][3] doubles (data parallel: mlp_best_pack + a SUM all-reduce).
struct PlateauArgs {
  PlateauRule rule{};
  double* rec = nullptr;
  const unsigned long long* slot = nullptr;
  const double* rows = nullptr;
  int R = 1;
};
void mlp_plateau(const PlateauArgs& a, void* stream);  // stream: a hipStream_t

}  // namespace cme
