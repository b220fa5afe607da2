// The per-epoch shuffle of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0 in
// the order of the keyed permutation (shuffle.h shuffle_index) and rewrites every layout the step kernels read -- X,
// labels, XT, Xs, Xw, XTw -- in place, so every pointer an MlpStep has bound and every captured graph stays valid.
//
// shuffle_kernel<T, VEC, VEC_T>: the grid, the LDS tile and the layouts written from it are resident_layouts.h's.
//   perm    thread d < 64 computes its destination sample's source row (or d itself: identity) into LDS; the
//           chunk-0 workgroup also stores perm[] and the gathered label.
//   gather  the 64 source-row chunks -> the tile.  VEC: 16 lanes read one row chunk with 16-byte loads (so X0 is
//           16-byte aligned too), 16 rows per pass; else one element per lane.  The same registers go straight to X
//           (and, converted, to Xw) before the barrier: full rows, coalesced.
//   XT, Xs  from the tile.
//           With a sampler's alias table (sample.h) the source row is a keyed draw with replacement instead: one hash
//           and one dependent 8-byte load per destination sample, in the same 64 threads.
// LDS 17.3 KB per workgroup, 14-26 VGPRs, no scratch, 8 waves per SIMD.  With the sampler's branch compiled in the
// compiler's resource report is unchanged in every form: LDS 17 664 B, 14-26 VGPRs, 52-58 SGPRs, no scratch, 8 waves.
// Measured (bench/shuffle_cost.py, docs/PERFORMANCE.md "Per-epoch shuffle"): 60 000 x 784 pixels in 38-43 us with X, XT
// and Xs (1.8 x a copy of the same bytes), 117-122 us with the bf16 copies.  A variant of the XT step that read the
// tile as four-byte words and transposed 4 x 4 byte blocks in registers (a quarter of the LDS reads) measured the
// same, so the one-byte LDS reads do not bound the kernel; the simpler form stays.  128 samples per workgroup (128-byte
// XT runs, 34 KB of LDS) measured 45-50 us and 106-109 us: slower where it counts, so 64 stays.
#include "shuffle.h"

#include "resident_layouts.h"

namespace cme {

namespace {

using namespace gather;

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kThreads) void shuffle_kernel(ShuffleArgs a) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kChunk / ES;  // features per chunk
  __shared__ __attribute__((aligned(16))) unsigned char tile[kRows * kPitch];
  __shared__ int src[kRows];
  const int t = threadIdx.x;
  const int64_t d0 = static_cast<int64_t>(blockIdx.x) * kRows;
  const int chunk = blockIdx.y;
  const int f0 = chunk * FC;  // first feature of the chunk
  const int N = a.N, P = a.P;
  const int nf = min(FC, P - f0);  // valid features of the chunk (>= 1 by the grid)

  if (t < kRows) {
    const int64_t d = d0 + t;
    int s = -1;
    if (d < N) {
      s = source_of(a, d);
      if (chunk == 0) store_order(a, d, s);
    }
    src[t] = s;
  }
  __syncthreads();

  const T* X0 = static_cast<const T*>(a.X0);
  T* X = static_cast<T*>(a.X);
  uint16_t* Xw = static_cast<uint16_t*>(a.Xw);
  // ---- gather: source rows -> LDS (+ X, Xw straight from the registers)
  if constexpr (VEC) {
    constexpr int EV = 16 / ES;  // elements per 16-byte load
    const int g = t & 15;        // 16-byte granule of the chunk
    const int fg = f0 + g * EV;  // its first feature; P % EV == 0, so a granule is wholly inside the row or outside
#pragma unroll
    for (int pass = 0; pass < kRows / 16; ++pass) {
      const int r = pass * 16 + (t >> 4);
      const int s = src[r];
      u32x4 v = {0u, 0u, 0u, 0u};
      if (s >= 0 && fg < P) {
        v = *reinterpret_cast<const u32x4*>(X0 + static_cast<int64_t>(s) * P + fg);
        store16(X, Xw, (d0 + r) * P + fg, v);
      }
      *reinterpret_cast<u32x4*>(tile + r * kPitch + g * 16) = v;
    }
  } else {
    for (int idx = t; idx < kRows * FC; idx += kThreads) {
      const int r = idx / FC, c = idx - r * FC;
      const int s = src[r];
      T v = 0;
      if (s >= 0 && c < nf) {
        v = X0[static_cast<int64_t>(s) * P + f0 + c];
        store1(X, Xw, (d0 + r) * P + f0 + c, v);
      }
      *reinterpret_cast<T*>(tile + r * kPitch + c * ES) = v;
    }
  }
  __syncthreads();

  write_xt<T, VEC_T>(tile, static_cast<T*>(a.XT), static_cast<uint16_t*>(a.XTw), t, d0, f0, nf, N);
  if constexpr (ES == 1) write_xs(tile, a.Xs, t, d0, chunk, N, P);
}

}  // namespace

void mlp_shuffle(const ShuffleArgs& a, void* stream) {
  check_gather_args(a, "mlp_shuffle");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool launched = with_form(a.es, vec_rows(a) && al16(a.X0), vec_runs(a), [&](auto t, auto vec, auto vec_t) {
    hipLaunchKernelGGL((shuffle_kernel<decltype(t), decltype(vec)::value, decltype(vec_t)::value>), grid_of(a),
                       dim3(kThreads), 0, st, a);
  });
  if (!launched) throw std::invalid_argument("mlp_shuffle: element size must be 1, 2, 4 or 8");
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
