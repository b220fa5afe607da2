// Gradient-norm clipping of the flat arena, one header for host and device: the sum-of-squares kernel (clip.hip), the
// apply launch that consumes its partials (optim.hip), the CPU bindings `_cpu.grad_sumsq` / `_cpu.grad_clip` (the
// kernels' bitwise oracle and the torch backend's implementation) and the fp64 oracle trainer (cpu/mlp_cpu.cpp) all
// evaluate the functions below, so the whole summation order -- element to workgroup, to thread, the lane tree, the
// wave order, the order of the partials -- is written once.
//
//   norm = sqrt(sum g^2) over the parameter segments [W1|b1|W2|b2] alone (never the padding of a segment, never the
//          status element);  coef = c / (norm + 1e-6);  coef < 1: every gradient element is multiplied by T(coef), one
//          rounding in T, before the update rule sees it;  coef >= 1: the gradient is untouched.
//   This is torch.nn.utils.clip_grad_norm_(max_norm=c, norm_type=2) with the L2 term in the loss: g is the gradient as
//   the step leaves it, scaled and with the regulariser included.  A non-finite norm propagates as in torch's default
//   (error_if_nonfinite=False): a NaN norm makes coef NaN and every element NaN, an infinite one makes coef 0.
//
// The order.  A segment is cut into groups of 16 bytes (4 floats / 2 doubles; the last group of a segment may be
// short).  The launch has clip_grid(count) workgroups of kClipThreads threads, count = the elements of all segments;
// thread `gtid` = workgroup * kClipThreads + thread takes groups gtid, gtid + stride, ... of segment 0, then of segment
// 1, ... (stride = all threads) and accumulates acc = fma(g, g, acc) in fp64 in that order (ascending index).  The 64
// lanes of a wave are combined by the tree v[i] += v[i + off], off = 32, 16, ..., 1; the waves of a workgroup are added
// in wave order, left to right; the workgroup stores one partial.  The consumer loads partial i into lane i of one wave
// (0 beyond the grid) and runs the same tree.  Only + and fma: host and device produce the same bits.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cme {

constexpr int kClipThreads = 1024;  // 16 waves: 64 workgroups keep 64 K threads' loads in flight
constexpr int kClipWaves = kClipThreads / 64;
constexpr int kClipMaxGrid = 64;  // one wave combines the partials
constexpr int kClipMaxSegs = 4;   // [W1|b1|W2|b2]
constexpr double kClipEps = 1e-6;

struct ClipSegs {
  int n = 0;
  int64_t off[kClipMaxSegs] = {0, 0, 0, 0};
  int64_t size[kClipMaxSegs] = {0, 0, 0, 0};
  __host__ __device__ int64_t count() const {
    int64_t c = 0;
    for (int i = 0; i < n; ++i) c += size[i];
    return c;
  }
};

// workgroups of the sum-of-squares launch (= partials): a function of the segments' element count alone
__host__ __device__ inline int clip_grid(int64_t count) {
  const int64_t per = static_cast<int64_t>(kClipThreads) * 4;
  const int64_t g = (count + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : (g > kClipMaxGrid ? kClipMaxGrid : g));
}

template <typename T>
struct ClipGroup {
  static constexpr int N = 16 / sizeof(T);
};

// one thread's share: vec[s] says segment s starts on a 16-byte boundary (full groups are then loaded with one
// 16-byte load on the device; the order is the same either way)
template <typename T>
__host__ __device__ inline double clip_thread_sumsq(const T* g, const ClipSegs& s, const bool* vec, int64_t gtid,
                                                    int64_t stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr int VN = ClipGroup<T>::N;
  double acc = 0.0;
  for (int q = 0; q < s.n; ++q) {
    const T* base = g + s.off[q];
    const int64_t size = s.size[q];
    const int64_t full = size / VN, groups = (size + VN - 1) / VN;
    int64_t k = gtid;
#if defined(__HIP_DEVICE_COMPILE__)
    if (vec[q]) {
      typedef T VT __attribute__((ext_vector_type(VN)));
#pragma unroll 4
      for (; k < full; k += stride) {
        const VT v = reinterpret_cast<const VT*>(base)[k];
#pragma unroll
        for (int e = 0; e < VN; ++e) {
          const double x = static_cast<double>(v[e]);
          acc = fma(x, x, acc);
        }
      }
    }
#else
    (void)vec;
    (void)full;
#endif
    for (; k < groups; k += stride) {
      const int64_t b = k * VN;
      for (int e = 0; e < VN && b + e < size; ++e) {
        const double x = static_cast<double>(base[b + e]);
        acc = fma(x, x, acc);
      }
    }
  }
  return acc;
}

// the lane tree on the host: v[0 .. 64) -> the sum lane 0 holds
inline double clip_tree64(double* v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
  return v[0];
}

#if defined(__HIPCC__)
// ... and on the device (every lane of the wave calls it; lane 0's result is the sum)
__device__ inline double clip_wave_tree(double v) {
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
  return v;
}
#endif

// the waves of a workgroup, in wave order
__host__ __device__ inline double clip_waves_sum(const double* w) {
  double s = w[0];
  for (int i = 1; i < kClipWaves; ++i) s = s + w[i];
  return s;
}

struct ClipCoef {
  double norm, coef;
  int clipped;  // !(coef >= 1): a NaN coefficient clips (and poisons), as torch's clamp(max=1) does
};

__host__ __device__ inline ClipCoef clip_coef(double sumsq, double clip_norm) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ClipCoef c;
  c.norm = sqrt(sumsq);
  c.coef = clip_norm / (c.norm + kClipEps);
  c.clipped = !(c.coef >= 1.0);
  return c;
}

template <typename T>
__host__ __device__ inline T clip_scale(T g, T s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return g * s;
}

// ---- the host evaluation of the whole order (no device code) ------------------------------------------------------
// partials: clip_grid(s.count()) doubles; returns the sum of squares the apply launch forms from them
template <typename T>
inline double clip_host_sumsq(const T* g, const ClipSegs& s, double* partials) {
  const int grid = clip_grid(s.count());
  const int64_t stride = static_cast<int64_t>(grid) * kClipThreads;
  const bool vec[kClipMaxSegs] = {false, false, false, false};
  double lanes[64], waves[kClipWaves], fin[64];
  for (int b = 0; b < grid; ++b) {
    for (int w = 0; w < kClipWaves; ++w) {
      for (int l = 0; l < 64; ++l)
        lanes[l] = clip_thread_sumsq<T>(g, s, vec, static_cast<int64_t>(b) * kClipThreads + w * 64 + l, stride);
      waves[w] = clip_tree64(lanes);
    }
    partials[b] = clip_waves_sum(waves);
  }
  for (int l = 0; l < 64; ++l) fin[l] = l < grid ? partials[l] : 0.0;
  return clip_tree64(fin);
}

// ---- the launch (clip.hip) ----------------------------------------------------------------------------------------
// grads: the gradient bucket, `arena` elements of dtype (0: f32, 1: f64); every segment lies inside it (checked);
// partials: npart = clip_grid(segs.count()) doubles, one plain store per workgroup.  No atomics, no workgroup waits for
// another; the apply launch behind it on the same stream reads the partials.
void mlp_grad_sumsq(int dtype, const void* grads, int64_t arena, const ClipSegs& segs, double* partials, int npart,
                    void* stream);

}  // namespace cme
