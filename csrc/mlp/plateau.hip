// Reduce the learning rate on a validation plateau, decided on the device (MI355X, gfx950): one launch behind an
// evaluation reads the numbers the evaluation left in device memory, runs plateau.h's rule and advances the one
// record whose `scale` word the apply launch (optim.hip) multiplies into every update's rate.
//
// plateau_kernel (mlp_plateau): ONE workgroup of 64 threads (one wave).
//   thread 0 reads the record and the decision inputs (a stats slot of eval.h, or R rows of doubles summed in rank
//   order by best_metric_of), runs plateau_decide and stores the advanced record back: eight 8-byte vector stores.
//   The other 63 lanes do nothing: the launch is a decision, not a pass over memory.
// A single workgroup, launches ordered on one stream and no other writer: one record is race-free under graph replay,
// and a captured graph advances the record by replaying.  Every index is checked by the launcher (R, the pointers);
// no atomics, no waits, no host sync.  Measured: bench/plateau_cost.py, docs/PERFORMANCE.md "Reduce on plateau".
#include "plateau.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kPlateauThreads = 64;
constexpr int kPlateauMaxRanks = 1024;  // as mlp_best_pack's: a sanity bound

__global__ __launch_bounds__(kPlateauThreads) void plateau_kernel(PlateauArgs a) {
  if (threadIdx.x != 0) return;
  PlateauRecord rec = plateau_load(a.rec);
  double metric;
  if (a.slot) {
    // {n, correct, loss_sum} of a stats slot as doubles (words 0 and 1 are uint64 counts, word 2 the fp64 loss's bits)
    const double t[3] = {static_cast<double>(a.slot[0]), static_cast<double>(a.slot[1]),
                         __builtin_bit_cast(double, a.slot[2])};
    metric = best_metric_of(t, 1, a.rule.monitor);
  } else {
    metric = best_metric_of(a.rows, a.R, a.rule.monitor);
  }
  plateau_decide(rec, a.rule, metric);
  plateau_store(a.rec, rec);
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

void mlp_plateau(const PlateauArgs& a, void* stream) {
  CME_REQUIRE(a.rec && al(a.rec, 8), "mlp_plateau: an 8-byte aligned record is required");
  CME_REQUIRE((a.slot != nullptr) != (a.rows != nullptr), "mlp_plateau: exactly one of slot and rows");
  CME_REQUIRE(a.R >= 1 && a.R <= kPlateauMaxRanks, "mlp_plateau: R must be in [1, 1024]");
  CME_REQUIRE(!a.slot || a.R == 1, "mlp_plateau: a stats slot is one rank's (R = 1)");
  CME_REQUIRE(al(a.slot, 8) && al(a.rows, 8), "mlp_plateau: slot and rows must be 8-byte aligned");
  CME_REQUIRE(plateau_rule_ok(a.rule),
              "mlp_plateau: rule out of range (monitor 0 / 1, 0 < factor < 1, patience >= 0, threshold >= 0, "
              "threshold_mode 0 / 1, cooldown >= 0, 0 <= min_factor <= 1, eps >= 0)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(plateau_kernel, dim3(1), dim3(kPlateauThreads), 0, st, a);
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
