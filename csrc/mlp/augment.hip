// Random-shift augmentation of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0
// in the order of the keyed permutation (shuffle.h shuffle_index, or the loaded order), moves every image by its own
// (dx, dy) (augment.h augment_shift / augment_src_yx) and rewrites every layout the step kernels read -- X, labels,
// XT, Xs, Xw, XTw -- in place, so every pointer an MlpStep has bound and every captured graph stays valid.
//
// augment_kernel<T, VEC, VEC_T>: the grid, the LDS tile and the layouts written from it are resident_layouts.h's.
//   rows    thread d < 64 computes its destination sample's source row (or d itself: identity; -1 past N) and that
//           row's shift into LDS as {source, dx, dy, dy * w + dx}; the chunk-0 workgroup also stores perm[], the
//           gathered label and shifts[].
//   gather  the tile of the SHIFTED bytes, one element per lane: a thread keeps one destination feature (its (y, x)
//           is divided out once) and walks the rows, so a wave reads 64 adjacent elements of one source row,
//           displaced by dy * w + dx; every lane is masked by the index rule for itself, so no address outside row s
//           of X0 is ever formed and every load is an aligned element load.  Pixels without a source are zeros.
//   X, XT, Xs  from the tile (X with 16-byte LDS reads where VEC).
// No atomics.  LDS 18 432 B per workgroup, 14-23 VGPRs, no scratch, 8 waves per SIMD (the compiler's resource report
// of the gfx950 build).  With a sampler's alias table (sample.h) the source row is a keyed draw and the shift is keyed
// by the destination (resident_layouts.h augment_id); with that branch compiled in the report is the same but for the
// SGPRs: 62-66 before, 64-68 now.
// Measured (bench/augment_cost.py, docs/PERFORMANCE.md "Augmentation"): 60 000 x 784 pixels in 73 us with X, XT and Xs
// against 44 us for the shuffle launch in the same run (1.66 x), 156 us against 122 us with the bf16 copies (1.28 x).
// The staged form of the gather (aligned 16-byte loads of the covering span into a second LDS buffer) was not built.
#include "augment.h"

#include "resident_layouts.h"

namespace cme {

namespace {

using namespace gather;

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kThreads) void augment_kernel(AugmentArgs aa) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kChunk / ES;  // features per chunk
  static_assert(kThreads % FC == 0, "a thread keeps one feature of the chunk");
  constexpr int RP = kThreads / FC;  // rows per pass of the gather
  __shared__ __attribute__((aligned(16))) unsigned char tile[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) int rows[kRows * 4];  // {source row or -1, dx, dy, dy * w + dx}
  const ShuffleArgs& a = aa.base;
  const int t = threadIdx.x;
  const int64_t d0 = static_cast<int64_t>(blockIdx.x) * kRows;
  const int chunk = blockIdx.y;
  const int f0 = chunk * FC;  // first feature of the chunk
  const int N = a.N, P = a.P;
  const int nf = min(FC, P - f0);  // valid features of the chunk (>= 1 by the grid)
  const int ih = aa.h, iw = aa.w;

  if (t < kRows) {
    const int64_t d = d0 + t;
    int s = -1;
    AugmentShift sh{0, 0};
    if (d < N) {
      s = source_of(a, d);
      sh = augment_shift(augment_id(a, d, s), aa.akey, aa.max_dx, aa.max_dy);
      if (chunk == 0) {
        store_order(a, d, s);
        if (aa.shifts) {
          aa.shifts[2 * d] = sh.dx;
          aa.shifts[2 * d + 1] = sh.dy;
        }
      }
    }
    *reinterpret_cast<i32x4*>(rows + 4 * t) = i32x4{s, sh.dx, sh.dy, sh.dy * iw + sh.dx};
  }
  __syncthreads();

  // ---- gather: the shifted source rows -> LDS, one element per lane; the thread's feature is fixed
  const T* X0 = static_cast<const T*>(a.X0);
  {
    const int c = t & (FC - 1);
    const int f = f0 + c;
    const bool inrow = c < nf;  // f < P
    const int y = inrow ? f / iw : 0, x = inrow ? f - y * iw : 0;
#pragma unroll 8
    for (int r = t / FC; r < kRows; r += RP) {
      const i32x4 rw = *reinterpret_cast<const i32x4*>(rows + 4 * r);
      T v = 0;
      if (rw[0] >= 0 && inrow) {
        const int sf = augment_src_yx(y, x, rw[1], rw[2], ih, iw);  // in [0, P), or -1
        if (sf >= 0) v = X0[static_cast<int64_t>(rw[0]) * P + sf];
      }
      *reinterpret_cast<T*>(tile + r * kPitch + c * ES) = v;
    }
  }
  __syncthreads();

  // ---- X (and Xw): full rows from the tile
  T* X = static_cast<T*>(a.X);
  uint16_t* Xw = static_cast<uint16_t*>(a.Xw);
  if (X || Xw) {
    if constexpr (VEC) {
      constexpr int EV = 16 / ES;  // elements per 16-byte store
      const int g = t & 15;        // 16-byte granule of the chunk
      const int fg = f0 + g * EV;  // its first feature; P % EV == 0, so a granule is wholly inside the row or outside
#pragma unroll
      for (int pass = 0; pass < kRows / 16; ++pass) {
        const int r = pass * 16 + (t >> 4);
        if (d0 + r < N && fg < P) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(tile + r * kPitch + g * 16);
          store16(X, Xw, (d0 + r) * P + fg, v);
        }
      }
    } else {
      for (int idx = t; idx < kRows * FC; idx += kThreads) {
        const int r = idx / FC, c = idx - r * FC;
        if (d0 + r < N && c < nf) {
          const T v = *reinterpret_cast<const T*>(tile + r * kPitch + c * ES);
          const int64_t o = (d0 + r) * P + f0 + c;  // (store1's text: through the call three forms keep 2 more VGPRs)
          if (X) X[o] = v;
          if constexpr (ES == 1) {
            if (Xw) Xw[o] = bf16_of_u8(v);
          }
        }
      }
    }
  }

  write_xt<T, VEC_T>(tile, static_cast<T*>(a.XT), static_cast<uint16_t*>(a.XTw), t, d0, f0, nf, N);
  if constexpr (ES == 1) write_xs(tile, a.Xs, t, d0, chunk, N, P);
}

}  // namespace

void mlp_augment(const AugmentArgs& aa, void* stream) {
  const ShuffleArgs& a = aa.base;
  check_gather_args(a, "mlp_augment");
  CME_REQUIRE(a.es == 1 || a.es == 2 || a.es == 4 || a.es == 8, "mlp_augment: element size must be 1, 2, 4 or 8");
  CME_REQUIRE(aa.h >= 1 && aa.w >= 1 && static_cast<int64_t>(aa.h) * aa.w == a.P,
              "mlp_augment: the image shape h x w must have h * w == P");
  CME_REQUIRE(aa.max_dx >= 0 && aa.max_dx < aa.w && aa.max_dy >= 0 && aa.max_dy < aa.h,
              "mlp_augment: the shift bounds must satisfy 0 <= max_dx < w and 0 <= max_dy < h");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(aa.shifts) & 3) == 0, "mlp_augment: shifts must be 4-byte aligned");
  const uintptr_t ea = static_cast<uintptr_t>(a.es) - 1;  // elements are loaded and stored at their natural alignment
  CME_REQUIRE(((reinterpret_cast<uintptr_t>(a.X0) | reinterpret_cast<uintptr_t>(a.X) |
                reinterpret_cast<uintptr_t>(a.XT)) & ea) == 0,
              "mlp_augment: X0, X and XT must be aligned to the element size");
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_form(a.es, vec_rows(a), vec_runs(a), [&](auto t, auto vec, auto vec_t) {
    hipLaunchKernelGGL((augment_kernel<decltype(t), decltype(vec)::value, decltype(vec_t)::value>), grid_of(a),
                       dim3(kThreads), 0, st, aa);
  });
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
