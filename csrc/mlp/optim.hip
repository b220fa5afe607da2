// The stateful optimizer step for MI355X (gfx950): one launch applies momentum / Nesterov or Adam (optim.h) to the flat
// arena from the gradient bucket, updates the state buffers in place, refreshes the bf16 planes (or shadow) of W1 and
// honours the bucket's status element -- the stateful counterpart of sgd_planes_kernel / sgd_flat.
//
// optim_kernel<T, KIND, NP> (mlp_optim_step): grid optim_grid(count) <= 2048 workgroups of 256 threads, fixed by `count` alone.
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
//
// optim_ext_kernel<T, KIND, NP> (mlp_optim_apply: a schedule window, clipping, the last-update record, or the stateless
// kSgd rule) is the same body (optim_body, EXT = 1) with a second argument struct (OptimExt), and
//   clip     wave 0 loads the sum-of-squares partials the launch before left (lane i < npart: partial i, else 0; npart
//            <= 64 checked by the launcher) and runs clip.h's lane tree; thread 0 forms norm, coef and T(coef);
//   window   thread 0 reads t BEFORE advancing it and the factor at the clamped index (optim.h window_index: no index
//            leaves the buffer of wcap factors whatever it holds), lr_t = h.lr * f[i], and derives the scalars from it;
//   plateau  thread 0 multiplies lr_t by the scale word of the plateau record (plateau.h plateau_rate) when one is set:
//            one 8-byte load; the decision launch (plateau.hip) is the word's only writer, ordered on the stream;
//   last     thread 0 of workgroup 0 stores {t, lr_t, norm, coef}.
//   Every thread multiplies the gradient elements it reads by T(coef) when the update is clipped (coef < 1).
// optim_kernel keeps its signature and, with EXT = 0, its code as it stood.  Measured: bench/clip_cost.py, docs/PERFORMANCE.md "Schedules and clipping".
#include "optim.h"

#include "clip.h"
#include "plateau.h"

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
  SgdCoef<T> sgd;
};

__device__ __forceinline__ uint16_t bf16_bits(float v, float& rest) {
  const __hip_bfloat16 h = __float2bfloat16(v);
  rest = v - __bfloat162float(h);
  return __builtin_bit_cast(uint16_t, h);
}

template <typename T, int KIND>
__device__ __forceinline__ void update(T& p, T& a, T& b, T g, const Coef<T>& c) {
  if constexpr (KIND == kMomentum) momentum_update(p, a, g, c.mom);
  else if constexpr (KIND == kAdam) adam_update(p, a, b, g, c.adam);
  else sgd_update(p, g, c.sgd);
}

template <typename T, int KIND, int NP, int EXT>
__device__ __forceinline__ void optim_body(const OptimArgs& a, const OptimExt& x, int64_t nvec, int pvec) {
  const T* status = static_cast<const T*>(a.status);
  if (status && *status != T(0)) return;
  __shared__ Coef<T> s_c;
  __shared__ T s_scale;
  __shared__ int s_clipped;
  double sumsq = 0.0;
  if constexpr (EXT) {
    if (x.clip_norm > 0.0 && threadIdx.x < 64) {
      const int lane = static_cast<int>(threadIdx.x);
      sumsq = clip_wave_tree(lane < x.npart ? x.partials[lane] : 0.0);
    }
  }
  if (threadIdx.x == 0) {
    double* r = a.rec + static_cast<int64_t>(blockIdx.x) * kOptimRecWords;
    double pscale = 1.0;
    if constexpr (EXT) {
      if (x.plateau) pscale = *x.plateau;  // (issued with the record's loads, not behind the window lookup)
    }
    OptimCounter c{r[0], r[1], r[2]};
    OptimHyper h = a.h;
    if constexpr (EXT) {
      if (x.window) h.lr = window_rate(a.h.lr, x.window, x.wcap, c.t);
      if (x.plateau) h.lr = plateau_rate(h.lr, pscale);
      ClipCoef cc{__builtin_nan(""), 1.0, 0};
      if (x.clip_norm > 0.0) cc = clip_coef(sumsq, x.clip_norm);
      s_scale = static_cast<T>(cc.coef);
      s_clipped = cc.clipped;
      if (x.last && blockIdx.x == 0) {
        x.last[0] = c.t;
        x.last[1] = h.lr;
        x.last[2] = cc.norm;
        x.last[3] = cc.coef;
      }
    }
    optim_advance(c, h);
    if constexpr (KIND == kMomentum) s_c.mom = momentum_coef<T>(h);
    else if constexpr (KIND == kAdam) s_c.adam = adam_coef<T>(h, c);
    else s_c.sgd = sgd_coef<T>(h);
    r[0] = c.t;
    r[1] = c.b1p;
    r[2] = c.b2p;
  }
  __syncthreads();
  const Coef<T> c = s_c;
  T gscale = T(1);
  bool clipped = false;
  if constexpr (EXT) {
    gscale = s_scale;
    clipped = s_clipped != 0;
  }

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
    V s1 = {};
    if constexpr (KIND != kSgd) s1 = reinterpret_cast<V*>(S1)[i];
    V s2 = {};
    if constexpr (KIND == kAdam) s2 = reinterpret_cast<V*>(S2)[i];
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      T pe = p[e], ae = s1[e], be = s2[e], ge = g[e];
      if constexpr (EXT) {
        if (clipped) ge = clip_scale(ge, gscale);
      }
      update<T, KIND>(pe, ae, be, ge, c);
      p[e] = pe; s1[e] = ae; s2[e] = be;
    }
    reinterpret_cast<V*>(P)[i] = p;
    if constexpr (KIND != kSgd) reinterpret_cast<V*>(S1)[i] = s1;
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
    T pe = P[i], ae = T(0), be = T(0), ge = G[i];
    if constexpr (KIND != kSgd) ae = S1[i];
    if constexpr (KIND == kAdam) be = S2[i];
    if constexpr (EXT) {
      if (clipped) ge = clip_scale(ge, gscale);
    }
    update<T, KIND>(pe, ae, be, ge, c);
    P[i] = pe;
    if constexpr (KIND != kSgd) S1[i] = ae;
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

// the launch as it stood: OptimArgs alone
template <typename T, int KIND, int NP>
__global__ __launch_bounds__(kOptThreads) void optim_kernel(OptimArgs a, int64_t nvec, int pvec) {
  optim_body<T, KIND, NP, 0>(a, OptimExt{}, nvec, pvec);
}

// ... and the extended one
template <typename T, int KIND, int NP>
__global__ __launch_bounds__(kOptThreads) void optim_ext_kernel(OptimArgs a, OptimExt x, int64_t nvec, int pvec) {
  optim_body<T, KIND, NP, 1>(a, x, nvec, pvec);
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

template <typename T, int KIND, int NP, int EXT>
void launch(const OptimArgs& a, const OptimExt& x, hipStream_t st) {
  const bool vec = al(a.params, 16) && al(a.grads, 16) && al(a.s1, 16) && al(a.s2, 16);
  const int64_t nvec = vec ? a.count / Vec<T>::N : 0;
  const int pvec = (NP > 0 && Vec<T>::N == 4 && a.w1n % 4 == 0 && al(a.planes, 8)) ? 1 : 0;
  if constexpr (EXT)
    hipLaunchKernelGGL((optim_ext_kernel<T, KIND, NP>), dim3(static_cast<unsigned>(a.nrec)), dim3(kOptThreads), 0, st,
                       a, x, nvec, pvec);
  else
    hipLaunchKernelGGL((optim_kernel<T, KIND, NP>), dim3(static_cast<unsigned>(a.nrec)), dim3(kOptThreads), 0, st, a,
                       nvec, pvec);
  CME_LAUNCH_CHECK(st);
}

template <typename T, int KIND, int EXT>
void launch_np(const OptimArgs& a, const OptimExt& x, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (a.np == 3) return launch<T, KIND, 3, EXT>(a, x, st);
    if (a.np == 1) return launch<T, KIND, 1, EXT>(a, x, st);
  }
  launch<T, KIND, 0, EXT>(a, x, st);
}

template <typename T, int EXT>
void launch_kind(const OptimArgs& a, const OptimExt& x, hipStream_t st) {
  if constexpr (EXT) {
    if (a.kind == kSgd) return launch_np<T, kSgd, 1>(a, x, st);
  }
  if (a.kind == kMomentum) return launch_np<T, kMomentum, EXT>(a, x, st);
  launch_np<T, kAdam, EXT>(a, x, st);
}

void check(const OptimArgs& a, bool ext) {
  CME_REQUIRE(a.dtype == 0 || a.dtype == 1, "mlp_optim_step: dtype must be 0 (f32) or 1 (f64)");
  CME_REQUIRE(a.kind == kMomentum || a.kind == kAdam || (ext && a.kind == kSgd),
              ext ? "mlp_optim_apply: kind must be momentum (0), adam (1) or sgd (2)"
                  : "mlp_optim_step: kind must be momentum (0) or adam (1)");
  CME_REQUIRE(a.count >= 1, "mlp_optim_step: count must be >= 1");
  CME_REQUIRE(a.params && a.grads && (a.s1 || a.kind == kSgd) && a.rec,
              "mlp_optim_step: params, grads, state and records are required");
  CME_REQUIRE(a.kind != kAdam || a.s2, "mlp_optim_step: adam needs the second state buffer");
  CME_REQUIRE(a.nrec == optim_grid(a.count), "mlp_optim_step: one counter record per workgroup (optim_grid(count))");
  CME_REQUIRE(a.np == 0 || a.np == 1 || a.np == 3, "mlp_optim_step: np must be 0, 1 or 3");
  CME_REQUIRE(a.np == 0 || (a.dtype == 0 && a.planes && a.w1n >= 0 && a.w1n <= a.count),
              "mlp_optim_step: bf16 planes need f32 parameters, a plane buffer and 0 <= w1n <= count");
}

}  // namespace

int optim_grid(int64_t count) {
  const int64_t per = static_cast<int64_t>(kOptThreads) * 4;
  const int64_t g = (count + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : (g > kOptMaxGrid ? kOptMaxGrid : g));
}

void mlp_optim_step(const OptimArgs& a, void* stream) {
  check(a, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.dtype == 0) launch_kind<float, 0>(a, OptimExt{}, st);
  else launch_kind<double, 0>(a, OptimExt{}, st);
}

void mlp_optim_apply(const OptimArgs& a, const OptimExt& x, void* stream) {
  check(a, true);
  CME_REQUIRE(!x.window || x.wcap >= 1, "mlp_optim_apply: a schedule window needs a capacity of at least one factor");
  CME_REQUIRE(x.clip_norm >= 0.0, "mlp_optim_apply: clip_norm must be >= 0 (0: no clipping)");
  CME_REQUIRE(!(x.clip_norm > 0.0) || (x.partials && x.npart >= 1 && x.npart <= kClipMaxGrid),
              "mlp_optim_apply: clipping needs 1 .. 64 sum-of-squares partials");
  CME_REQUIRE(al(x.plateau, 8), "mlp_optim_apply: the plateau scale word must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.dtype == 0) launch_kind<float, 1>(a, x, st);
  else launch_kind<double, 1>(a, x, st);
}

}  // namespace cme
