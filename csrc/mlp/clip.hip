// The global gradient norm's sum of squares for MI355X (gfx950): the first of the two launches of gradient-norm
// clipping (clip.h).  The apply launch (optim.hip) behind it on the same stream combines the partials, forms the norm
// and the coefficient and scales the gradient it reads -- no atomics, no workgroup waits for another, graph-safe.
//
// grad_sumsq_kernel<T>: clip_grid(count) <= 64 workgroups of 1024 threads, fixed by the segments' element count alone.
//   thread   clip_thread_sumsq (clip.h): groups gtid, gtid + stride, ... of each segment in turn, one 16-byte load per
//            full group when the segment starts on a 16-byte boundary (else element by element), fp64 fma(g, g, acc);
//   wave     the fixed shuffle tree clip_wave_tree; lane 0 leaves the wave's sum in LDS;
//   group    thread 0 adds the 16 wave sums in wave order and stores the workgroup's partial (one plain vector store).
// Every segment is checked against the bucket's length by the launcher, and a group's elements against its segment's
// size by the loop bounds: padding and the status element are never read.  The launch reads the bucket once: 318 KB at
// 79,510 parameters (latency-bound), 12.8 MB at 3.2 M.  Measured: bench/clip_cost.py, docs/PERFORMANCE.md "Schedules
// and clipping".
#include "clip.h"

#include "common/hip_common.h"

namespace cme {

namespace {

struct SumsqArgs {
  const void* grads;
  ClipSegs segs;
  bool vec[kClipMaxSegs];
  double* partials;
};

template <typename T>
__global__ __launch_bounds__(kClipThreads) void grad_sumsq_kernel(SumsqArgs a) {
  __shared__ double s_w[kClipWaves];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kClipThreads;
  const int64_t gtid = static_cast<int64_t>(blockIdx.x) * kClipThreads + threadIdx.x;
  const double acc = clip_thread_sumsq<T>(static_cast<const T*>(a.grads), a.segs, a.vec, gtid, stride);
  const double w = clip_wave_tree(acc);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) a.partials[blockIdx.x] = clip_waves_sum(s_w);
}

}  // namespace

void mlp_grad_sumsq(int dtype, const void* grads, int64_t arena, const ClipSegs& segs, double* partials, int npart,
                    void* stream) {
  CME_REQUIRE(dtype == 0 || dtype == 1, "mlp_grad_sumsq: dtype must be 0 (f32) or 1 (f64)");
  CME_REQUIRE(grads && partials, "mlp_grad_sumsq: the gradient bucket and the partials are required");
  CME_REQUIRE(segs.n >= 1 && segs.n <= kClipMaxSegs, "mlp_grad_sumsq: 1 .. 4 segments");
  const int64_t es = dtype == 0 ? 4 : 8;
  SumsqArgs a{grads, segs, {false, false, false, false}, partials};
  for (int i = 0; i < segs.n; ++i) {
    CME_REQUIRE(segs.off[i] >= 0 && segs.size[i] >= 0 && segs.off[i] <= arena && segs.size[i] <= arena - segs.off[i],
                "mlp_grad_sumsq: a segment lies outside the gradient bucket");
    a.vec[i] = ((reinterpret_cast<uintptr_t>(grads) + static_cast<uintptr_t>(segs.off[i] * es)) & 15) == 0;
  }
  CME_REQUIRE(npart == clip_grid(segs.count()), "mlp_grad_sumsq: one partial per workgroup (clip_grid(count))");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == 0)
    hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3(static_cast<unsigned>(npart)), dim3(kClipThreads), 0, st, a);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<double>, dim3(static_cast<unsigned>(npart)), dim3(kClipThreads), 0, st, a);
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
