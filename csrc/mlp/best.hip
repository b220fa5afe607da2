// Keep the best validation weights on the device (MI355X, gfx950): one launch behind an evaluation decides, from the
// numbers the evaluation left in device memory, whether the parameters are the best so far (best.h) and, if so, copies
// the arena into the best arena.  It takes its form from optim.hip, which solves the same two problems: a device-held
// record under graph replay, and a streaming pass over the flat arena.
//
// keep_best_kernel<T> (mlp_keep_best): grid best_grid(count) <= 2048 workgroups of 256 threads, fixed by `count` alone.
//   record   thread 0 reads its workgroup's record and the decision inputs (a stats slot of eval.h, or R rows of
//            doubles summed in rank order), runs best_decide, stores the advanced record back and leaves `improved`
//            in LDS.  No other workgroup reads or writes that record, and launches on one stream are ordered: race-free
//            by construction.  Every workgroup reads the same inputs and the same record values, so all decide alike.
//   body     not improved: return -- the common case costs a launch and nothing else.  Improved: grid-stride over
//            16-byte groups (4 floats / 2 doubles) when both pointers are 16-byte aligned (nvec groups, else 0), then a
//            scalar grid-stride tail over [nvec * VEC, count).  An element's workgroup depends on its index alone; every
//            element is read and written by exactly one thread.
// best_pack_kernel (mlp_best_pack): one workgroup; thread i < 3 R writes element i of rows[R][3] -- this rank's triple
//   in row `rank`, zero elsewhere.
// Every index is checked against count / nrec / R by the launcher or the loop bounds; plain vector stores only; no
// workgroup waits for another; no atomics.  Measured: bench/keep_best_cost.py, docs/PERFORMANCE.md "Keeping the best
// weights".
#include "best.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kBestThreads = 256;
constexpr int kBestMaxGrid = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md: memory-bound grid cap)
constexpr int kBestMaxRanks = 1024;  // rows the pack kernel's one workgroup covers in a few passes; a sanity bound

template <typename T>
struct Vec;
template <>
struct Vec<float> {
  typedef float type __attribute__((ext_vector_type(4)));
  static constexpr int N = 4;
};
template <>
struct Vec<double> {
  typedef double type __attribute__((ext_vector_type(2)));
  static constexpr int N = 2;
};

// {n, correct, loss_sum} of a stats slot as doubles (words 0 and 1 are uint64 counts, word 2 the fp64 loss's bits)
__device__ __forceinline__ void slot_triple(const unsigned long long* slot, double* t) {
  t[0] = static_cast<double>(slot[0]);
  t[1] = static_cast<double>(slot[1]);
  t[2] = __builtin_bit_cast(double, slot[2]);
}

template <typename T>
__global__ __launch_bounds__(kBestThreads) void keep_best_kernel(BestArgs a, int64_t nvec) {
  __shared__ int s_improved;
  if (threadIdx.x == 0) {
    double* r = a.rec + static_cast<int64_t>(blockIdx.x) * kBestRecWords;
    BestRecord rec = best_load(r);
    double metric;
    if (a.slot) {
      double t[3];
      slot_triple(a.slot, t);
      metric = best_metric_of(t, 1, a.rule.monitor);
    } else {
      metric = best_metric_of(a.rows, a.R, a.rule.monitor);
    }
    s_improved = best_decide(rec, a.rule, metric) ? 1 : 0;
    best_store(r, rec);
  }
  __syncthreads();
  if (!s_improved) return;

  using V = typename Vec<T>::type;
  constexpr int VN = Vec<T>::N;
  const T* P = static_cast<const T*>(a.params);
  T* B = static_cast<T*>(a.best);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBestThreads;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBestThreads + threadIdx.x;
  for (int64_t i = tid; i < nvec; i += stride) reinterpret_cast<V*>(B)[i] = reinterpret_cast<const V*>(P)[i];
  for (int64_t i = nvec * VN + tid; i < a.count; i += stride) B[i] = P[i];
}

__global__ __launch_bounds__(kBestThreads) void best_pack_kernel(const unsigned long long* slot, double* rows, int R,
                                                                 int rank) {
  double t[3];
  slot_triple(slot, t);
  const int n = 3 * R;
  for (int i = static_cast<int>(threadIdx.x); i < n; i += kBestThreads) rows[i] = (i / 3 == rank) ? t[i % 3] : 0.0;
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <typename T>
void launch(const BestArgs& a, hipStream_t st) {
  const bool vec = al(a.params, 16) && al(a.best, 16);
  const int64_t nvec = vec ? a.count / Vec<T>::N : 0;
  hipLaunchKernelGGL((keep_best_kernel<T>), dim3(static_cast<unsigned>(a.nrec)), dim3(kBestThreads), 0, st, a, nvec);
  CME_LAUNCH_CHECK(st);
}

}  // namespace

int best_grid(int64_t count) {
  const int64_t per = static_cast<int64_t>(kBestThreads) * 4;
  const int64_t g = (count + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : (g > kBestMaxGrid ? kBestMaxGrid : g));
}

void mlp_keep_best(const BestArgs& a, void* stream) {
  CME_REQUIRE(a.dtype == 0 || a.dtype == 1, "mlp_keep_best: dtype must be 0 (f32) or 1 (f64)");
  CME_REQUIRE(a.count >= 1, "mlp_keep_best: count must be >= 1");
  CME_REQUIRE(a.params && a.best && a.rec, "mlp_keep_best: params, best and records are required");
  CME_REQUIRE(al(a.params, a.dtype ? 8 : 4) && al(a.best, a.dtype ? 8 : 4) && al(a.rec, 8),
              "mlp_keep_best: pointers must be aligned to their element size");
  CME_REQUIRE(a.nrec == best_grid(a.count), "mlp_keep_best: one record per workgroup (best_grid(count))");
  CME_REQUIRE((a.slot != nullptr) != (a.rows != nullptr), "mlp_keep_best: exactly one of slot and rows");
  CME_REQUIRE(a.R >= 1 && a.R <= kBestMaxRanks, "mlp_keep_best: R must be in [1, 1024]");
  CME_REQUIRE(!a.slot || a.R == 1, "mlp_keep_best: a stats slot is one rank's (R = 1)");
  CME_REQUIRE(al(a.slot, 8) && al(a.rows, 8), "mlp_keep_best: slot and rows must be 8-byte aligned");
  CME_REQUIRE(a.rule.monitor == kBestLoss || a.rule.monitor == kBestAccuracy,
              "mlp_keep_best: monitor must be loss (0) or accuracy (1)");
  CME_REQUIRE(a.rule.min_delta >= 0.0, "mlp_keep_best: min_delta must be >= 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.dtype == 0) launch<float>(a, st);
  else launch<double>(a, st);
}

void mlp_best_pack(const unsigned long long* slot, double* rows, int R, int rank, void* stream) {
  CME_REQUIRE(slot && rows && al(slot, 8) && al(rows, 8), "mlp_best_pack: an 8-byte aligned slot and rows are required");
  CME_REQUIRE(R >= 1 && R <= kBestMaxRanks, "mlp_best_pack: R must be in [1, 1024]");
  CME_REQUIRE(rank >= 0 && rank < R, "mlp_best_pack: rank must be in [0, R)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(best_pack_kernel, dim3(1), dim3(kBestThreads), 0, st, slot, rows, R, rank);
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
