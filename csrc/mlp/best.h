// Keeping the best validation weights and stopping on patience, one header for host and device: the launch behind an
// evaluation (best.hip), the CPU binding `_cpu.best_decide` (the kernel tests' bitwise oracle and the torch backend's
// implementation) and the trainer's twin tests all evaluate the functions below, so the rule is written once.
//
// One decision.  R triples {n, correct, loss_sum} as doubles, one per rank, are summed IN RANK ORDER (counts are exact in
// fp64; one process has R = 1).  The metric is loss_sum / n for monitor = loss and correct / n for monitor = accuracy;
// n == 0 gives 0 / 0 = NaN (every NaN metric is stored as the one quiet NaN, so records compare bitwise).
//
// The record (8 doubles; counts are exact to 2^53, so a device record is eight 8-byte words of one type):
//   [0] evals        decisions taken so far
//   [1] best_index   the decision that holds the best (-1 before any)
//   [2] best_metric
//   [3] bad          consecutive non-improving decisions
//   [4] stopped      0 or 1
//   [5] stop_index   the decision that set `stopped` (-1: none)
//   [6] last_metric
//   [7] spare
// and starts as {0, -1, NaN, 0, 0, -1, NaN, 0}.
//
// best_decide(rec, rule, metric) -> improved:
//   stopped set: only evals and last_metric advance; nothing can improve any more.
//   otherwise improved = best_index < 0 ? !isnan(metric)
//                      : loss ? metric < best_metric - min_delta : metric > best_metric + min_delta
//   (strict comparisons: a tie keeps the earlier evaluation; NaN never improves);
//   improved: best_index = evals, best_metric = metric, bad = 0;
//   else: bad += 1 and, when patience >= 0 && bad >= patience + 1, stopped = 1 and stop_index = evals.
//   evals += 1 always.
// patience = p therefore tolerates p bad evaluations and stops on bad evaluation number p + 1: patience = 0 stops at the
// first non-improving evaluation; patience < 0 never stops.
//
// Host (g++) and device (hipcc) produce the same bits: only + - * / and comparisons, contraction off under clang.
#pragma once

#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cme {

enum BestMonitor { kBestLoss = 0, kBestAccuracy = 1 };

struct BestRule {
  int monitor = kBestLoss;
  double min_delta = 0.0;  // >= 0
  int patience = -1;       // < 0: never stop
};

constexpr int kBestRecWords = 8;  // doubles per record (64 bytes)

struct BestRecord {
  double evals, best_index, best_metric, bad, stopped, stop_index, last_metric, spare;
};

__host__ __device__ inline bool best_isnan(double x) { return x != x; }

__host__ __device__ inline BestRecord best_start() {
  const double nan = __builtin_nan("");
  return {0.0, -1.0, nan, 0.0, 0.0, -1.0, nan, 0.0};
}

__host__ __device__ inline BestRecord best_load(const double* r) {
  return {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
}

__host__ __device__ inline void best_store(double* r, const BestRecord& b) {
  r[0] = b.evals; r[1] = b.best_index; r[2] = b.best_metric; r[3] = b.bad;
  r[4] = b.stopped; r[5] = b.stop_index; r[6] = b.last_metric; r[7] = b.spare;
}

// rows: [R][3] doubles {n, correct, loss_sum}, summed in rank order
__host__ __device__ inline double best_metric_of(const double* rows, int R, int monitor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double n = 0.0, correct = 0.0, loss = 0.0;
  for (int r = 0; r < R; ++r) {
    n = n + rows[3 * r];
    correct = correct + rows[3 * r + 1];
    loss = loss + rows[3 * r + 2];
  }
  const double m = (monitor == kBestAccuracy ? correct : loss) / n;
  return best_isnan(m) ? __builtin_nan("") : m;  // (one NaN on host and device: 0 / 0 differs in sign between them)
}

__host__ __device__ inline bool best_decide(BestRecord& rec, const BestRule& rule, double metric) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool improved = false;
  if (rec.stopped == 0.0) {
    if (rec.best_index < 0.0) improved = !best_isnan(metric);
    else if (rule.monitor == kBestAccuracy) improved = metric > rec.best_metric + rule.min_delta;
    else improved = metric < rec.best_metric - rule.min_delta;
    if (improved) {
      rec.best_index = rec.evals;
      rec.best_metric = metric;
      rec.bad = 0.0;
    } else {
      rec.bad = rec.bad + 1.0;
      if (rule.patience >= 0 && rec.bad >= static_cast<double>(rule.patience) + 1.0) {
        rec.stopped = 1.0;
        rec.stop_index = rec.evals;
      }
    }
  }
  rec.last_metric = metric;
  rec.evals = rec.evals + 1.0;
  return improved;
}

// ---- the launches (best.hip) --------------------------------------------------------------------------------------
// mlp_keep_best: ONE launch behind an evaluation.  best_grid(count) workgroups of 256 threads, fixed by `count` alone;
// rec = nrec = best_grid(count) records, one per workgroup: a captured graph replays the same kernel arguments, so the
// launch reads and advances the record itself, and a single shared record would race with a workgroup scheduled late.
// Thread 0 of every workgroup reads its record and the decision inputs, runs best_decide, stores the advanced record
// and broadcasts `improved` through LDS.  Not improved: the workgroup returns.  Improved: it copies its span of
// params -> best (`count` elements of dtype 0: f32 / 1: f64; the arena [W1|b1|W2|b2] without the status element),
// elements assigned to workgroups by index alone; 16-byte loads and stores when both pointers are 16-byte aligned, then
// a scalar tail, else all scalar.  Plain vector stores only; no workgroup waits for another; no atomics.
// The decision inputs are exactly one of
//   slot  a stats slot of eval.h, read directly (one process): words 0 and 1 are uint64 counts, word 2 the loss bits;
//   rows  [R][3] doubles (data parallel: mlp_best_pack + a SUM all-reduce).
struct BestArgs {
  int dtype = 0;
  BestRule rule{};
  const void* params = nullptr;
  void* best = nullptr;
  int64_t count = 0;
  double* rec = nullptr;
  int nrec = 0;
  const unsigned long long* slot = nullptr;
  const double* rows = nullptr;
  int R = 1;
};
int best_grid(int64_t count);  // workgroups (= records) of the launch over `count` elements, any dtype
void mlp_keep_best(const BestArgs& a, void* stream);  // stream: a hipStream_t
// one workgroup: this rank's triple (from `slot`) into row `rank` of rows[R][3], zero into every other row.  A SUM
// all-reduce of that buffer is then an exact all-gather (every element is x + 0 + ... + 0 in any order), so every rank
// holds the same rows bitwise and takes the same decision.
void mlp_best_pack(const unsigned long long* slot, double* rows, int R, int rank, void* stream);

}  // namespace cme
