// An exponential moving average of the parameters, one header for host and device: the launch behind every applied
// update (ema.hip), the CPU binding `_cpu.ema_step` (the kernel tests' bitwise oracle and the torch backend's
// implementation) and the fp64 oracle trainer all evaluate the functions below, so the rule is written once.
//
// One update.  t is 0-based: the count of averaged updates BEFORE this one (a double, exact to 2^53, as OptimCounter).
//   d_t = decay                                  without warmup
//   d_t = min(decay, (1 + t) / (10 + t))         with warmup (0.1 at t = 0, 0.5 at t = 8, -> 1: the early average follows
//                                                the parameters instead of the starting point)
//   omd = T(1.0 - d_t)                           formed in fp64, rounded to T once
//   e   = fma(omd, p - e, e)   per element       (torch.lerp(e, p, 1 - d); torch.optim.swa_utils.get_ema_multi_avg_fn)
// Where p == e the element is returned as it is, bit for bit (p - e is then +0 and the fma would turn a -0 into +0).
// The average starts as a copy of the parameters (the caller's business: MlpEngine.set_ema / set_params).
//
// The record (4 doubles): {t, d of the last update (0 before any), 0, 0}; it starts as zeros.
//
// Host (g++) and device (hipcc) produce the same bits: only + - * / comparisons and an explicit fma, contraction off
// under clang (g++ builds here target no FMA instruction set, so it cannot contract).
#pragma once

#include <cmath>
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cme {

struct EmaRule {
  double decay = 0.999;  // 0 <= decay < 1
  int warmup = 0;
};

constexpr int kEmaRecWords = 4;  // doubles per record (32 bytes)

__host__ __device__ inline float ema_fma(float a, float b, float c) { return fmaf(a, b, c); }
__host__ __device__ inline double ema_fma(double a, double b, double c) { return fma(a, b, c); }

__host__ __device__ inline bool ema_rule_ok(const EmaRule& r) { return r.decay >= 0.0 && r.decay < 1.0; }

// the decay of update t
__host__ __device__ inline double ema_decay(const EmaRule& r, double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!r.warmup) return r.decay;
  const double w = (1.0 + t) / (10.0 + t);
  return w < r.decay ? w : r.decay;
}

// 1 - d_t in the element type
template <typename T>
__host__ __device__ inline T ema_omd(double d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return static_cast<T>(1.0 - d);
}

template <typename T>
__host__ __device__ inline T ema_update(T e, T p, T omd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (p == e) return e;
  const T diff = p - e;
  return ema_fma(omd, diff, e);
}

// ---- the launch (ema.hip) -------------------------------------------------------------------------------------------
// mlp_ema_step: ONE launch behind every applied update.  ema_grid(count) workgroups of 256 threads, at most 2048, fixed
// by `count` alone; rec = nrec = ema_grid(count) records, one per workgroup: a captured graph replays the same kernel
// arguments, so the launch reads and advances the count itself, and a single shared record would race with a workgroup
// scheduled late (optim.h).  Thread 0 of every workgroup reads its record, broadcasts t through LDS and stores the
// advanced record; every thread forms the same omd.  `count` elements of dtype 0: f32 / 1: f64 (the arena [W1|b1|W2|b2]
// without the status element), assigned to workgroups by index alone; 16-byte loads and stores when params and ema are
// both 16-byte aligned, then a scalar tail, else all scalar.  params and ema are read once, ema is written once.  Plain
// vector stores only; no workgroup waits for another; no atomics.
//   status  the gradient bucket's status element (dtype), or null
//   err     the engine's sticky hand-off word, or null
// Either non-zero: the update before this launch was not applied, and the launch changes nothing -- neither the average
// nor any record.
struct EmaArgs {
  int dtype = 0;
  EmaRule rule{};
  const void* params = nullptr;
  void* ema = nullptr;
  int64_t count = 0;
  double* rec = nullptr;
  int nrec = 0;
  const void* status = nullptr;
  const int32_t* err = nullptr;
};
int ema_grid(int64_t count);  // workgroups (= records) of the launch over `count` elements, any dtype
void mlp_ema_step(const EmaArgs& a, void* stream);  // stream: a hipStream_t

}  // namespace cme
