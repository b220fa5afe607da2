// The exponential moving average of the parameters on the device (MI355X, gfx950): one launch behind every applied
// update folds the parameter arena into the averaged arena by the rule of ema.h.  It takes its form from optim.hip and
// best.hip, which solve the same two problems: a device-held record under graph replay, and a streaming pass over the
// flat arena.
//
// ema_kernel<T> (mlp_ema_step): grid ema_grid(count) <= 2048 workgroups of 256 threads, fixed by `count` alone.
//   skip     every thread loads the status element and the hand-off error word where given (one address each: a
//            broadcast); either non-zero -> return before anything is read or written, the record included.
//   record   thread 0 reads its workgroup's record {t, d, 0, 0}, leaves t in LDS and stores {t + 1, d_t, 0, 0}.  No
//            other workgroup reads or writes that record, and launches on one stream are ordered: race-free by
//            construction.  Every thread forms d_t and omd = T(1 - d_t) from the same t (ema.h): the same bits.
//   body     grid-stride over 16-byte groups (4 floats / 2 doubles: one global_load_dwordx4 per array and lane, the
//            widest access there is) when both pointers are 16-byte aligned (nvec groups, else 0), then a scalar
//            grid-stride tail over [nvec * VEC, count).  An element's workgroup depends on its index alone; every
//            element is read and written by exactly one thread.  12 B per f32 element: p and e in, e out.
// At most 8 workgroups of 4 waves per CU and a handful of registers: occupancy is bounded by the grid cap, not by
// resources, and one 16-byte group per lane and iteration keeps 1 KiB per wave instruction in flight.  At 79,510
// parameters (78 workgroups) the launch is latency-bound: 2.56 us against 2.33 us for a copy of the arena; at 3.3 M it
// streams the two arrays once, 5.33 us against 4.03 us for the copy's two thirds of the bytes.
// Every index is checked against count / nrec by the launcher or the loop bounds; plain vector stores only; no workgroup
// waits for another; no atomics.  Measured: bench/ema_cost.py, docs/PERFORMANCE.md "Weight averaging".
#include "ema.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kEmaThreads = 256;
constexpr int kEmaMaxGrid = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md: memory-bound grid cap)

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

template <typename T>
__global__ __launch_bounds__(kEmaThreads) void ema_kernel(EmaArgs a, int64_t nvec) {
  const T* status = static_cast<const T*>(a.status);
  if (status && *status != T(0)) return;
  if (a.err && *a.err != 0) return;
  __shared__ double s_t;
  if (threadIdx.x == 0) s_t = a.rec[static_cast<int64_t>(blockIdx.x) * kEmaRecWords];
  __syncthreads();
  const double t = s_t;
  const double d = ema_decay(a.rule, t);
  const T omd = ema_omd<T>(d);
  if (threadIdx.x == 0) {
    double* r = a.rec + static_cast<int64_t>(blockIdx.x) * kEmaRecWords;
    r[0] = t + 1.0;
    r[1] = d;
    r[2] = 0.0;
    r[3] = 0.0;
  }

  using V = typename Vec<T>::type;
  constexpr int VN = Vec<T>::N;
  const T* P = static_cast<const T*>(a.params);
  T* E = static_cast<T*>(a.ema);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEmaThreads;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kEmaThreads + threadIdx.x;
  for (int64_t i = tid; i < nvec; i += stride) {
    const V p = reinterpret_cast<const V*>(P)[i];
    V e = reinterpret_cast<V*>(E)[i];
#pragma unroll
    for (int k = 0; k < VN; ++k) e[k] = ema_update<T>(e[k], p[k], omd);
    reinterpret_cast<V*>(E)[i] = e;
  }
  for (int64_t i = nvec * VN + tid; i < a.count; i += stride) E[i] = ema_update<T>(E[i], P[i], omd);
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <typename T>
void launch(const EmaArgs& a, hipStream_t st) {
  const bool vec = al(a.params, 16) && al(a.ema, 16);
  const int64_t nvec = vec ? a.count / Vec<T>::N : 0;
  hipLaunchKernelGGL((ema_kernel<T>), dim3(static_cast<unsigned>(a.nrec)), dim3(kEmaThreads), 0, st, a, nvec);
  CME_LAUNCH_CHECK(st);
}

}  // namespace

int ema_grid(int64_t count) {
  const int64_t per = static_cast<int64_t>(kEmaThreads) * 4;
  const int64_t g = (count + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : (g > kEmaMaxGrid ? kEmaMaxGrid : g));
}

void mlp_ema_step(const EmaArgs& a, void* stream) {
  CME_REQUIRE(a.dtype == 0 || a.dtype == 1, "mlp_ema_step: dtype must be 0 (f32) or 1 (f64)");
  CME_REQUIRE(a.count >= 1, "mlp_ema_step: count must be >= 1");
  CME_REQUIRE(a.params && a.ema && a.rec, "mlp_ema_step: params, ema and records are required");
  CME_REQUIRE(a.params != a.ema, "mlp_ema_step: the average needs an arena of its own");
  const uintptr_t esz = a.dtype ? 8 : 4;
  CME_REQUIRE(al(a.params, esz) && al(a.ema, esz) && al(a.rec, 8) && al(a.status, esz) && al(a.err, 4),
              "mlp_ema_step: pointers must be aligned to their element size");
  CME_REQUIRE(a.nrec == ema_grid(a.count), "mlp_ema_step: one record per workgroup (ema_grid(count))");
  CME_REQUIRE(ema_rule_ok(a.rule), "mlp_ema_step: decay must be in [0, 1)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.dtype == 0) launch<float>(a, st);
  else launch<double>(a, st);
}

}  // namespace cme
