// The stateful optimizer step for MI355X (gfx950): one launch applies momentum / Nesterov or Adam (optim.h) to the flat
// arena from the gradient bucket, updates the state buffers in place, refreshes the bf16 planes (or shadow) of W1 and
// honours the bucket's status element -- the stateful counterpart of sgd_planes_kernel / sgd_flat.
//
// optim_kernel<T, KIND, NP>: grid optim_grid(count) <= 2048 workgroups of 256 threads, fixed by `count` alone.
//   status   every thread loads the status element (one address: a broadcast); non-zero -> return before anything is
//            read or written, the counter record included.
//   counter  thread 0 reads its workgroup's record {t, b1^t, b2^t}, advances it (optim_advance), forms the update's
//            scalars in fp64 (adam_coef), leaves them in LDS and stores the advanced record back.  No other workgroup
//            reads or writes that record, and launches on one stream are ordered: race-free by construction.
//   body     grid-stride over 16-byte groups (4 floats / 2 doubles) when every pointer is 16-byte aligned (nvec
//            groups, else 0), then a scalar grid-stride tail over [nvec * VEC, count).  An element's workgroup
//            depends on its index alone; every element is read and written by exactly one thread.
//   planes   (f32) elements < w1n: the NP-way bf16 split of the new value, 8-byte stores of 4 bf16 per plane when
//            w1n % 4 == 0 and the planes are 8-byte aligned (pvec), else element by element.
// Every index is checked against count / w1n / nrec by the launcher or the loop bounds; plain vector stores only.
// At 79,510 parameters the launch is latency-bound; at 3.2 M it streams the arrays once: momentum reads p, g, v and
// writes p, v; Adam reads p, g, m, s and writes p, m, s.  Measured: bench/optim_cost.py, docs/PERFORMANCE.md
// "Stateful optimizers".
#include "optim.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kOptThreads = 256;
constexpr int kOptMaxGrid = 2048;  // 256 CUs x 8 workgroups (cdna_hip_programming.md: memory-bound grid cap)

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

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
union Coef {
  MomentumCoef<T> mom;
  AdamCoef<T> adam;
};

__device__ __forceinline__ uint16_t bf16_bits(float v, float& rest) {
  const __hip_bfloat16 h = __float2bfloat16(v);
  rest = v - __bfloat162float(h);
  return __builtin_bit_cast(uint16_t, h);
}

template <typename T, int KIND>
__device__ __forceinline__ void update(T& p, T& a, T& b, T g, const Coef<T>& c) {
  if constexpr (KIND == kMomentum) momentum_update(p, a, g, c.mom);
  else adam_update(p, a, b, g, c.adam);
}

template <typename T, int KIND, int NP>
__global__ __launch_bounds__(kOptThreads) void optim_kernel(OptimArgs a, int64_t nvec, int pvec) {
  const T* status = static_cast<const T*>(a.status);
  if (status && *status != T(0)) return;
  __shared__ Coef<T> s_c;
  if (threadIdx.x == 0) {
    double* r = a.rec + static_cast<int64_t>(blockIdx.x) * kOptimRecWords;
    OptimCounter c{r[0], r[1], r[2]};
    optim_advance(c, a.h);
    if constexpr (KIND == kMomentum) s_c.mom = momentum_coef<T>(a.h);
    else s_c.adam = adam_coef<T>(a.h, c);
    r[0] = c.t;
    r[1] = c.b1p;
    r[2] = c.b2p;
  }
  __syncthreads();
  const Coef<T> c = s_c;

  using V = typename Vec<T>::type;
  constexpr int VN = Vec<T>::N;
  T* P = static_cast<T*>(a.params);
  const T* G = static_cast<const T*>(a.grads);
  T* S1 = static_cast<T*>(a.s1);
  T* S2 = static_cast<T*>(a.s2);
  uint16_t* planes = static_cast<uint16_t*>(a.planes);
  const int64_t w1n = a.w1n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kOptThreads;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kOptThreads + threadIdx.x;

  for (int64_t i = tid; i < nvec; i += stride) {
    V p = reinterpret_cast<V*>(P)[i];
    const V g = reinterpret_cast<const V*>(G)[i];
    V s1 = reinterpret_cast<V*>(S1)[i];
    V s2 = {};
    if constexpr (KIND == kAdam) s2 = reinterpret_cast<V*>(S2)[i];
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      T pe = p[e], ae = s1[e], be = s2[e];
      update<T, KIND>(pe, ae, be, g[e], c);
      p[e] = pe; s1[e] = ae; s2[e] = be;
    }
    reinterpret_cast<V*>(P)[i] = p;
    reinterpret_cast<V*>(S1)[i] = s1;
    if constexpr (KIND == kAdam) reinterpret_cast<V*>(S2)[i] = s2;
    if constexpr (NP > 0) {
      const int64_t b = i * VN;
      if (b < w1n) {
        float rest[VN];
#pragma unroll
        for (int e = 0; e < VN; ++e) rest[e] = static_cast<float>(p[e]);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          uint16_t h[VN];
#pragma unroll
          for (int e = 0; e < VN; ++e) h[e] = bf16_bits(rest[e], rest[e]);
          uint16_t* pl = planes + q * w1n + b;
          if (pvec) {  // (w1n % 4 == 0: the whole group is inside the plane)
            if constexpr (VN == 4) *reinterpret_cast<u16x4*>(pl) = u16x4{h[0], h[1], h[2], h[3]};
          } else {
#pragma unroll
            for (int e = 0; e < VN; ++e)
              if (b + e < w1n) pl[e] = h[e];
          }
        }
      }
    }
  }
  for (int64_t i = nvec * VN + tid; i < a.count; i += stride) {
    T pe = P[i], ae = S1[i], be = T(0);
    if constexpr (KIND == kAdam) be = S2[i];
    update<T, KIND>(pe, ae, be, G[i], c);
    P[i] = pe;
    S1[i] = ae;
    if constexpr (KIND == kAdam) S2[i] = be;
    if constexpr (NP > 0) {
      if (i < w1n) {
        float rest = static_cast<float>(pe);
#pragma unroll
        for (int q = 0; q < NP; ++q) planes[q * w1n + i] = bf16_bits(rest, rest);
      }
    }
  }
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <typename T, int KIND, int NP>
void launch(const OptimArgs& a, hipStream_t st) {
  const bool vec = al(a.params, 16) && al(a.grads, 16) && al(a.s1, 16) && al(a.s2, 16);
  const int64_t nvec = vec ? a.count / Vec<T>::N : 0;
  const int pvec = (NP > 0 && Vec<T>::N == 4 && a.w1n % 4 == 0 && al(a.planes, 8)) ? 1 : 0;
  hipLaunchKernelGGL((optim_kernel<T, KIND, NP>), dim3(static_cast<unsigned>(a.nrec)), dim3(kOptThreads), 0, st, a,
                     nvec, pvec);
  CME_LAUNCH_CHECK(st);
}

template <typename T, int KIND>
void launch_np(const OptimArgs& a, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (a.np == 3) return launch<T, KIND, 3>(a, st);
    if (a.np == 1) return launch<T, KIND, 1>(a, st);
  }
  launch<T, KIND, 0>(a, st);
}

}  // namespace

int optim_grid(int64_t count) {
  const int64_t per = static_cast<int64_t>(kOptThreads) * 4;
  const int64_t g = (count + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : (g > kOptMaxGrid ? kOptMaxGrid : g));
}

void mlp_optim_step(const OptimArgs& a, void* stream) {
  CME_REQUIRE(a.dtype == 0 || a.dtype == 1, "mlp_optim_step: dtype must be 0 (f32) or 1 (f64)");
  CME_REQUIRE(a.kind == kMomentum || a.kind == kAdam, "mlp_optim_step: kind must be momentum (0) or adam (1)");
  CME_REQUIRE(a.count >= 1, "mlp_optim_step: count must be >= 1");
  CME_REQUIRE(a.params && a.grads && a.s1 && a.rec, "mlp_optim_step: params, grads, state and records are required");
  CME_REQUIRE(a.kind != kAdam || a.s2, "mlp_optim_step: adam needs the second state buffer");
  CME_REQUIRE(a.nrec == optim_grid(a.count), "mlp_optim_step: one counter record per workgroup (optim_grid(count))");
  CME_REQUIRE(a.np == 0 || a.np == 1 || a.np == 3, "mlp_optim_step: np must be 0, 1 or 3");
  CME_REQUIRE(a.np == 0 || (a.dtype == 0 && a.planes && a.w1n >= 0 && a.w1n <= a.count),
              "mlp_optim_step: bf16 planes need f32 parameters, a plane buffer and 0 <= w1n <= count");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.dtype == 0) {
    if (a.kind == kMomentum) launch_np<float, kMomentum>(a, st);
    else launch_np<float, kAdam>(a, st);
  } else {
    if (a.kind == kMomentum) launch_np<double, kMomentum>(a, st);
    else launch_np<double, kAdam>(a, st);
  }
}

}  // namespace cme
