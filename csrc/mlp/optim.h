// The update rules of the apply launch (momentum / Nesterov, Adam, and the stateless kSgd that plain SGD runs when a
// learning-rate schedule or gradient clipping is set) of the flat parameter arena, one header for host and device:
// the kernel (optim.hip), the CPU binding `_cpu.optim_step` (the kernel tests' bitwise oracle and the torch backend's
// implementation) and the fp64 oracle trainer (cpu/mlp_cpu.cpp) all evaluate these functions.
//
// g is the gradient as the step leaves it in the arena: already scaled, regulariser included.
//   momentum  v = mu v + g;  d = nesterov ? g + mu v : v;  p -= lr d
//             (torch.optim.SGD(momentum=mu, dampening=0, nesterov=...) with v0 = 0)
//   adam      m = b1 m + (1 - b1) g;  s = b2 s + (1 - b2) g g;
//             p -= (lr / (1 - b1^t)) m / (sqrt(s) / sqrt(1 - b2^t) + eps)
//             (torch.optim.Adam without weight decay or amsgrad; t counts the applied updates from 1)
//   sgd       p = fma(-lr, g, p)   (torch.optim.SGD; no state buffer)
// lr is the rate of THIS update: h.lr times the schedule's factor when the launch has a schedule window (below).
//
// Host (g++) and device (hipcc) produce the same bits: only + - * / sqrt fma, every fused multiply-add written as an
// explicit fma, contraction switched off under clang (g++ builds here target no FMA instruction set, so it cannot
// contract), no pow -- b1^t and b2^t are running products advanced once per applied update (OptimCounter), in fp64
// whatever T is, and the per-update scalars derived from them (adam_coef) are formed in fp64 and rounded to T once.
// The build has no fast-math flag: fp32 and fp64 divide and sqrt are correctly rounded on both sides.
#pragma once

#include <cmath>
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cme {

enum OptimKind { kMomentum = 0, kAdam = 1, kSgd = 2 };

struct OptimHyper {
  double lr = 0.0;
  double mu = 0.9;
  int nesterov = 0;
  double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
};

// the count of applied updates and the running products b1^t, b2^t (t = 0: 1, 1).  t is kept as a double (exact to
// 2^53) so that a device record is four 8-byte words of one type.
struct OptimCounter {
  double t = 0.0, b1p = 1.0, b2p = 1.0;
};

__host__ __device__ inline void optim_advance(OptimCounter& c, const OptimHyper& h) {
  c.t += 1.0;
  c.b1p *= h.beta1;
  c.b2p *= h.beta2;
}

__host__ __device__ inline float optim_fma(float a, float b, float c) { return fmaf(a, b, c); }
__host__ __device__ inline double optim_fma(double a, double b, double c) { return fma(a, b, c); }
__host__ __device__ inline float optim_sqrt(float a) { return sqrtf(a); }
__host__ __device__ inline double optim_sqrt(double a) { return sqrt(a); }

template <typename T>
struct MomentumCoef {
  T nlr, mu;  // -lr, mu
  int nesterov;
};

template <typename T>
__host__ __device__ inline MomentumCoef<T> momentum_coef(const OptimHyper& h) {
  return {static_cast<T>(-h.lr), static_cast<T>(h.mu), h.nesterov};
}

template <typename T>
__host__ __device__ inline void momentum_update(T& p, T& v, T g, const MomentumCoef<T>& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T nv = optim_fma(c.mu, v, g);
  const T d = c.nesterov ? optim_fma(c.mu, nv, g) : nv;
  v = nv;
  p = optim_fma(c.nlr, d, p);
}

template <typename T>
struct SgdCoef {
  T nlr;  // -lr
};

template <typename T>
__host__ __device__ inline SgdCoef<T> sgd_coef(const OptimHyper& h) {
  return {static_cast<T>(-h.lr)};
}

template <typename T>
__host__ __device__ inline void sgd_update(T& p, T g, const SgdCoef<T>& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  p = optim_fma(c.nlr, g, p);
}

// ---- the schedule window ----------------------------------------------------------------------------------------
// The factor of update t (0-based: the count of applied updates BEFORE this one) comes from a device buffer of fp64
// doubles {t0, n, f[0 .. n)} with room for `cap` factors: i = t - t0 clamped into [0, n - 1] (n itself clamped into
// [1, cap], so no index leaves the buffer whatever the buffer holds), lr_t = h.lr * f[i] in fp64.  The host refills the
// buffer in place between launches (never during a capture), so a captured graph follows the schedule.
constexpr int kWindowHeader = 2;  // doubles before f[0]

__host__ __device__ inline int window_index(double t, double t0, double n, int cap) {
  int m = 1;
  if (n >= 2.0) m = n >= static_cast<double>(cap) ? cap : static_cast<int>(n);
  const double d = t - t0;
  int i = 0;
  if (d >= 1.0) i = d >= static_cast<double>(m - 1) ? m - 1 : static_cast<int>(d);
  return i;
}

__host__ __device__ inline double window_rate(double lr, const double* w, int cap, double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return lr * w[kWindowHeader + window_index(t, w[0], w[1], cap)];
}

template <typename T>
struct AdamCoef {
  T b1, b2, omb1, omb2;  // beta1, beta2, 1 - beta1, 1 - beta2
  T nstep;               // -lr / (1 - b1^t)
  T bc2s;                // sqrt(1 - b2^t)
  T eps;
};

// c: the counter AFTER optim_advance (t >= 1, so 1 - b^t > 0 for betas in [0, 1))
template <typename T>
__host__ __device__ inline AdamCoef<T> adam_coef(const OptimHyper& h, const OptimCounter& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  AdamCoef<T> k;
  k.b1 = static_cast<T>(h.beta1);
  k.b2 = static_cast<T>(h.beta2);
  k.omb1 = static_cast<T>(1.0 - h.beta1);
  k.omb2 = static_cast<T>(1.0 - h.beta2);
  k.nstep = static_cast<T>(-(h.lr / (1.0 - c.b1p)));
  k.bc2s = static_cast<T>(sqrt(1.0 - c.b2p));
  k.eps = static_cast<T>(h.eps);
  return k;
}

// rounding sequence per element (u = 2^-24 / 2^-53 each): omb1 g, fma -> m; omb2 g, (.) g, fma -> s; sqrt, divide,
// add -> denominator; divide; fma -> p
template <typename T>
__host__ __device__ inline void adam_update(T& p, T& m, T& s, T g, const AdamCoef<T>& k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const T nm = optim_fma(k.b1, m, k.omb1 * g);
  const T ns = optim_fma(k.b2, s, (k.omb2 * g) * g);
  const T den = optim_sqrt(ns) / k.bc2s + k.eps;
  m = nm;
  s = ns;
  p = optim_fma(k.nstep, nm / den, p);
}

// ---- the launch (optim.hip) ----------------------------------------------------------------------------------
// One launch over the flat arena [W1|b1|W2|b2|status] of `count` elements of type dtype (0: f32, 1: f64):
//   params, grads, s1 (momentum: v; adam: m; sgd: null), s2 (adam: s; else null) -- `count` elements each;
//   planes: np (0 / 1 / 3) bf16 planes [np][w1n] of the first w1n parameters (f32 only): 3 = the exact split3
//     planes, 1 = split1 or the bf16 path's shadow -- as sgd_planes_kernel / sgd_flat treat them;
//   status: the gradient bucket's status element (dtype), or null: non-zero -> the launch changes nothing, neither
//     parameters nor state nor the counter records;
//   rec: nrec = optim_grid(count) records {t, b1^t, b2^t, 0} (doubles), one per workgroup: a captured graph replays
//     the same kernel arguments, so the launch reads and advances the count itself; a single shared record would
//     race with a workgroup scheduled late, so every workgroup owns a copy (thread 0 reads it, broadcasts through
//     LDS, writes the advanced one back) and elements are assigned to workgroups by index alone.
// The extended form (mlp_optim_apply: OptimArgs plus OptimExt; kind kSgd always takes it):
//   window: the schedule window above (wcap = its capacity in factors), or null: lr_t = h.lr;
//   clip_norm > 0: partials = the npart = clip_grid(...) partial sums of squares the launch before this one left
//     (clip.h); every workgroup combines them in the header's order and scales the gradient it reads by T(coef) when
//     coef < 1;
//   last: 4 doubles {t, lr_t, grad_norm, clip_coef} written by workgroup 0 (NaN, 1 without clipping), or null;
//   plateau: the `scale` word of a plateau record (plateau.h), or null: lr_t = plateau_rate(lr_t, *plateau) after the
//     window lookup, so `last` reports the rate that was used.
// mlp_optim_step is the launch as it stood: the same kernel signature, the same code, the same bits.
// Plain vector stores only; no workgroup waits for another.
struct OptimArgs {
  int dtype = 0;
  int kind = kMomentum;
  OptimHyper h{};
  void* params = nullptr;
  const void* grads = nullptr;
  void* s1 = nullptr;
  void* s2 = nullptr;
  void* planes = nullptr;
  int np = 0;
  int64_t count = 0, w1n = 0;
  const void* status = nullptr;
  double* rec = nullptr;
  int nrec = 0;
};
struct OptimExt {
  const double* window = nullptr;
  int wcap = 0;
  const double* partials = nullptr;
  int npart = 0;
  double clip_norm = 0.0;
  double* last = nullptr;
  const double* plateau = nullptr;
};
constexpr int kOptimLastWords = 4;
constexpr int kOptimRecWords = 4;  // doubles per record (32 bytes)
int optim_grid(int64_t count);     // workgroups (= records) of the launch over `count` elements, any dtype
void mlp_optim_step(const OptimArgs& a, void* stream);  // stream: a hipStream_t
void mlp_optim_apply(const OptimArgs& a, const OptimExt& x, void* stream);

}  // namespace cme
