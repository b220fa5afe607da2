// Affine augmentation of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0 in the
// order of the keyed permutation (shuffle.h shuffle_index, or the loaded order), resamples every image through its own
// inverse affine map (affine.h: a table entry per sample, four taps, a bilinear blend) moved by its own (dx, dy)
// (augment.h augment_shift) and rewrites every layout the step kernels read -- X, labels, XT, Xs, Xw, XTw -- in place,
// so every pointer an MlpStep has bound and every captured graph stays valid.
//
// affine_kernel<T, VEC, VEC_T>: the grid, the LDS tile and the layouts written from it are resident_layouts.h's.
//   rows    thread d < 64 computes its destination sample's source row (or d itself: identity; -1 past N), that row's
//           shift and its table entry into LDS as {source, dx, dy, 0, q00, q01, q10, q11}; the chunk-0 workgroup also
//           stores perm[], the gathered label, shifts[] and transforms[].
//   gather  the tile of the BLENDED elements, one per lane: a thread keeps one destination feature (its (y, x) is
//           divided out once) and walks the rows; per row affine.h's affine_pixel forms the four taps, tests each
//           against the image and its weight, and only then forms its address, so no address outside row s of X0 is
//           ever formed and every load is an aligned element load from global memory (a workgroup's 64 source rows
//           are read again by its sibling chunk workgroups out of L2).  Pixels without a tap are zeros.  uint8 blends
//           in integers; bf16 / f32 / f64 through affine.h's fixed fp64 chain.
//   X, XT, Xs  from the tile (X with 16-byte LDS reads where VEC).
// No atomics.  LDS 19 456 B per workgroup (the 17 408 B tile + 2 048 B of row records), 30 VGPRs (1-byte elements) and
// 32-35 (2 / 4 / 8-byte), 66-68 SGPRs, no scratch, 8 waves per SIMD (the compiler's resource report of the gfx950
// build).  With a sampler's alias table (sample.h) the source row is a keyed draw and the shift and the table entry
// are keyed by the destination (resident_layouts.h augment_id); with that branch compiled in the report is the same but
// for the SGPRs: 66-68 before, 70-72 now.
// Measured (bench/affine_cost.py, docs/PERFORMANCE.md "Affine augmentation"): 60 000 x 784 pixels in 185 us with X, XT
// and Xs against 73 us for the Shift launch and 44 us for the shuffle launch in the same run (2.55 x the Shift launch),
// 245 us against 147 us and 112 us with the bf16 copies (1.66 x).  Inside three times the Shift launch, so the staged
// form of the gather (the workgroup's 64 whole source rows in LDS, 50 KB at 784 uint8 pixels) was not built.
#include "affine.h"

#include "resident_layouts.h"

namespace cme {

namespace {

using namespace gather;

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kThreads) void affine_kernel(AffineArgs fa) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kChunk / ES;  // features per chunk
  static_assert(kThreads % FC == 0, "a thread keeps one feature of the chunk");
  constexpr int RP = kThreads / FC;  // rows per pass of the gather
  __shared__ __attribute__((aligned(16))) unsigned char tile[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) int rows[kRows * 8];  // {source row or -1, dx, dy, 0, q00, q01, q10, q11}
  const AugmentArgs& aa = fa.aug;
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
    i32x4 q{65536, 0, 0, 65536};
    if (d < N) {
      s = source_of(a, d);
      const uint32_t id = augment_id(a, d, s);
      sh = augment_shift(id, aa.akey, aa.max_dx, aa.max_dy);
      const int k = static_cast<int>(affine_index(id, aa.akey, static_cast<uint32_t>(fa.T)));
      q = *reinterpret_cast<const i32x4*>(fa.table + 4 * k);  // k < T by the reduction
      if (chunk == 0) {
        store_order(a, d, s);
        if (aa.shifts) {
          aa.shifts[2 * d] = sh.dx;
          aa.shifts[2 * d + 1] = sh.dy;
        }
        if (fa.transforms) fa.transforms[d] = k;
      }
    }
    *reinterpret_cast<i32x4*>(rows + 8 * t) = i32x4{s, sh.dx, sh.dy, 0};
    *reinterpret_cast<i32x4*>(rows + 8 * t + 4) = q;
  }
  __syncthreads();

  // ---- gather: the blended pixels -> LDS, one element per lane; the thread's feature is fixed
  const T* X0 = static_cast<const T*>(a.X0);
  {
    const int c = t & (FC - 1);
    const int f = f0 + c;
    const bool inrow = c < nf;  // f < P
    const int y = inrow ? f / iw : 0, x = inrow ? f - y * iw : 0;
#pragma unroll 4
    for (int r = t / FC; r < kRows; r += RP) {
      const i32x4 rw = *reinterpret_cast<const i32x4*>(rows + 8 * r);
      T v = 0;
      if (rw[0] >= 0 && inrow) {
        const i32x4 q = *reinterpret_cast<const i32x4*>(rows + 8 * r + 4);
        v = affine_pixel<T>(X0 + static_cast<int64_t>(rw[0]) * P, y, x, rw[1], rw[2],
                            AffineEntry{q[0], q[1], q[2], q[3]}, ih, iw);
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
          store1(X, Xw, (d0 + r) * P + f0 + c, v);
        }
      }
    }
  }

  write_xt<T, VEC_T>(tile, static_cast<T*>(a.XT), static_cast<uint16_t*>(a.XTw), t, d0, f0, nf, N);
  if constexpr (ES == 1) write_xs(tile, a.Xs, t, d0, chunk, N, P);
}

}  // namespace

void mlp_affine(const AffineArgs& fa, void* stream) {
  const AugmentArgs& aa = fa.aug;
  const ShuffleArgs& a = aa.base;
  check_gather_args(a, "mlp_affine");
  CME_REQUIRE(a.es == 1 || a.es == 2 || a.es == 4 || a.es == 8, "mlp_affine: element size must be 1, 2, 4 or 8");
  CME_REQUIRE(affine_kind_size(fa.kind) == a.es,
              "mlp_affine: the element kind (0 uint8, 1 bf16, 2 f32, 3 f64) must be one of the element size");
  CME_REQUIRE(aa.h >= 1 && aa.w >= 1 && static_cast<int64_t>(aa.h) * aa.w == a.P,
              "mlp_affine: the image shape h x w must have h * w == P");
  CME_REQUIRE(aa.h <= kAffineMaxSide && aa.w <= kAffineMaxSide, "mlp_affine: h and w must be <= 2^24");
  CME_REQUIRE(aa.max_dx >= 0 && aa.max_dx < aa.w && aa.max_dy >= 0 && aa.max_dy < aa.h,
              "mlp_affine: the shift bounds must satisfy 0 <= max_dx < w and 0 <= max_dy < h");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(aa.shifts) & 3) == 0, "mlp_affine: shifts must be 4-byte aligned");
  CME_REQUIRE(fa.table != nullptr && al16(fa.table), "mlp_affine: the table is required, 16-byte aligned");
  CME_REQUIRE(fa.T >= 1 && fa.T <= kAffineMaxTable, "mlp_affine: the table must have 1 <= T <= 65536 entries");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(fa.transforms) & 3) == 0, "mlp_affine: transforms must be 4-byte aligned");
  const uintptr_t ea = static_cast<uintptr_t>(a.es) - 1;  // elements are loaded and stored at their natural alignment
  CME_REQUIRE(((reinterpret_cast<uintptr_t>(a.X0) | reinterpret_cast<uintptr_t>(a.X) |
                reinterpret_cast<uintptr_t>(a.XT)) & ea) == 0,
              "mlp_affine: X0, X and XT must be aligned to the element size");
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_form(a.es, vec_rows(a), vec_runs(a), [&](auto t, auto vec, auto vec_t) {
    hipLaunchKernelGGL((affine_kernel<decltype(t), decltype(vec)::value, decltype(vec_t)::value>), grid_of(a),
                       dim3(kThreads), 0, st, fa);
  });
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
