// Elastic distortion of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0 in the
// order of the keyed permutation (shuffle.h shuffle_index, or the loaded order), resamples every image through its own
// inverse affine map and shift (affine.h) with every source position moved by the image's own smooth displacement
// field (warp.h: a lattice of keyed random nodes per sample, a cubic B-spline through integer axis tables) and
// rewrites every layout the step kernels read -- X, labels, XT, Xs, Xw, XTw -- in place, so every pointer an MlpStep
// has bound and every captured graph stays valid.
//
// warp_kernel<T, VEC, VEC_T>: the grid, the LDS tile and the layouts written from it are resident_layouts.h's.
//   rows    as affine_kernel: thread d < 64 computes its destination sample's source row (-1 past N), shift and table
//           entry into LDS, and warp_node_key of the row; the chunk-0 workgroup also stores perm[], the gathered label,
//           shifts[] and transforms[].
//   nodes   after a barrier all 256 threads hash the 64 samples' L lattice nodes into LDS, one packed {ddx, ddy} word
//           per node at [sample][64]: 16 KB, of which a default 6 x 6 lattice fills 9 KB.  Every chunk forms the whole
//           lattice (9 hashes per thread at L = 36): restricting it to the lattice rows the chunk's image rows touch
//           was not measured.
//   gather  a thread keeps one destination feature: its (y, x) and its two axis entries (ten integers) are formed once,
//           before the row loop.  Per row it reads its 16 nodes from LDS, forms the displacement (warp_displace) and
//           the four taps (warp_taps), tests each tap against the image and its weight and only then forms its
//           address: no address outside row s of X0 is ever formed.  Pixels without a tap are zeros.
//   LDS     ds_read_b32 banks per 32-lane half, and a half never spans two samples: a wave covers one row of the tile
//           for 1 / 2 / 4-byte elements and two rows, one per half, for 8-byte elements.  Inside a half neighbouring
//           features share a cell, so a read touches a handful of distinct nodes of one sample (broadcasts otherwise),
//           all within 64 consecutive words; two of them share a bank only 32 words apart, four lattice rows of an
//           8-wide lattice, which 32 consecutive features reach on images under 8 pixels wide only.  The pitch of 64
//           words therefore needs no padding or rotation.
//   X, XT, Xs  from the tile (X with 16-byte LDS reads where VEC).
// No atomics.  The compiler's resource report of the gfx950 build: LDS 36 352 B per workgroup (the 17 408 B tile,
// 2 048 B of row records, 512 B of node keys, 16 384 B of nodes): four workgroups per CU of 160 KiB, so LDS and not
// the registers bounds the residency at 4 waves per SIMD; 62-64 VGPRs in every form (8 waves per SIMD by registers),
// 72-76 SGPRs, no scratch.  With a sampler's alias table (sample.h) the source row is a keyed draw and the shift, the
// table entry and the lattice are keyed by the destination (resident_layouts.h augment_id); with that branch compiled
// in the report is the same but for the SGPRs: 74-78.
// Measured: bench/warp_cost.py, docs/PERFORMANCE.md "Elastic distortion".
#include "warp.h"

#include "resident_layouts.h"

namespace cme {

namespace {

using namespace gather;

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kNodePitch = kWarpMaxNodes;  // words per sample

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kThreads) void warp_kernel(WarpArgs wa) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kChunk / ES;  // features per chunk
  static_assert(kThreads % FC == 0, "a thread keeps one feature of the chunk");
  constexpr int RP = kThreads / FC;  // rows per pass of the gather
  __shared__ __attribute__((aligned(16))) unsigned char tile[kRows * kPitch];
  __shared__ __attribute__((aligned(16))) int rows[kRows * 8];  // {source row or -1, dx, dy, 0, q00, q01, q10, q11}
  __shared__ uint64_t nkeys[kRows];
  __shared__ uint32_t nodes[kRows * kNodePitch];  // {ddx, ddy} as two int16
  const AffineArgs& fa = wa.aff;
  const AugmentArgs& aa = fa.aug;
  const ShuffleArgs& a = aa.base;
  const int t = threadIdx.x;
  const int64_t d0 = static_cast<int64_t>(blockIdx.x) * kRows;
  const int chunk = blockIdx.y;
  const int f0 = chunk * FC;  // first feature of the chunk
  const int N = a.N, P = a.P;
  const int nf = min(FC, P - f0);  // valid features of the chunk (>= 1 by the grid)
  const int ih = aa.h, iw = aa.w;
  const int L = (wa.gy + 3) * (wa.gx + 3);  // <= kWarpMaxNodes by the launcher

  if (t < kRows) {
    const int64_t d = d0 + t;
    int s = -1;
    AugmentShift sh{0, 0};
    i32x4 q{65536, 0, 0, 65536};
    uint64_t nk = 0;
    if (d < N) {
      s = source_of(a, d);
      const uint32_t id = augment_id(a, d, s);
      sh = augment_shift(id, aa.akey, aa.max_dx, aa.max_dy);
      const int k = static_cast<int>(affine_index(id, aa.akey, static_cast<uint32_t>(fa.T)));
      q = *reinterpret_cast<const i32x4*>(fa.table + 4 * k);  // k < T by the reduction
      nk = warp_node_key(id, aa.akey);
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
    nkeys[t] = nk;
  }
  __syncthreads();

  // ---- nodes: the 64 samples' lattices -> LDS (rows past N hold zeros and are never read)
  for (int idx = t; idx < kRows * L; idx += kThreads) {
    const int r = idx / L, j = idx - r * L;
    nodes[r * kNodePitch + j] = warp_pack(warp_node(nkeys[r], static_cast<uint32_t>(j), wa.A));
  }
  __syncthreads();

  // ---- gather: the blended pixels -> LDS, one element per lane; the thread's feature is fixed
  const T* X0 = static_cast<const T*>(a.X0);
  {
    const int c = t & (FC - 1);
    const int f = f0 + c;
    const bool inrow = c < nf;  // f < P
    const int y = inrow ? f / iw : 0, x = inrow ? f - y * iw : 0;
    WarpAxis ay, ax;  // (y < ih and x < iw: inside the [ih + iw][5] table)
    {
      const int32_t* ey = wa.axes + 5 * y;
      const int32_t* ex = wa.axes + 5 * (ih + x);
      // (the clamps change nothing for a table of warp_axis_entry; they keep every node read inside the lattice)
      ay = WarpAxis{min(max(ey[0], 0), wa.gy - 1), {ey[1], ey[2], ey[3], ey[4]}};
      ax = WarpAxis{min(max(ex[0], 0), wa.gx - 1), {ex[1], ex[2], ex[3], ex[4]}};
    }
#pragma unroll 2
    for (int r = t / FC; r < kRows; r += RP) {
      const i32x4 rw = *reinterpret_cast<const i32x4*>(rows + 8 * r);
      T v = 0;
      if (rw[0] >= 0 && inrow) {
        const i32x4 q = *reinterpret_cast<const i32x4*>(rows + 8 * r + 4);
        const uint32_t* nr = nodes + r * kNodePitch;
        // ay.i + 3 <= gy + 2 and ax.i + 3 <= gx + 2: every node index is < L
        const WarpDisp dd = warp_displace(ay, ax, wa.gx, [&](int j) { return warp_unpack(nr[j]); });
        const AffineTaps tp = warp_taps(y, x, rw[1], rw[2], AffineEntry{q[0], q[1], q[2], q[3]}, ih, iw, dd);
        v = warp_blend<T>(X0 + static_cast<int64_t>(rw[0]) * P, tp, ih, iw);
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

void mlp_warp(const WarpArgs& wa, void* stream) {
  const AffineArgs& fa = wa.aff;
  const AugmentArgs& aa = fa.aug;
  const ShuffleArgs& a = aa.base;
  check_gather_args(a, "mlp_warp");
  CME_REQUIRE(a.es == 1 || a.es == 2 || a.es == 4 || a.es == 8, "mlp_warp: element size must be 1, 2, 4 or 8");
  CME_REQUIRE(affine_kind_size(fa.kind) == a.es,
              "mlp_warp: the element kind (0 uint8, 1 bf16, 2 f32, 3 f64) must be one of the element size");
  CME_REQUIRE(aa.h >= 1 && aa.w >= 1 && static_cast<int64_t>(aa.h) * aa.w == a.P,
              "mlp_warp: the image shape h x w must have h * w == P");
  CME_REQUIRE(aa.h <= kAffineMaxSide && aa.w <= kAffineMaxSide, "mlp_warp: h and w must be <= 2^24");
  CME_REQUIRE(aa.max_dx >= 0 && aa.max_dx < aa.w && aa.max_dy >= 0 && aa.max_dy < aa.h,
              "mlp_warp: the shift bounds must satisfy 0 <= max_dx < w and 0 <= max_dy < h");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(aa.shifts) & 3) == 0, "mlp_warp: shifts must be 4-byte aligned");
  CME_REQUIRE(fa.table != nullptr && al16(fa.table), "mlp_warp: the table is required, 16-byte aligned");
  CME_REQUIRE(fa.T >= 1 && fa.T <= kAffineMaxTable, "mlp_warp: the table must have 1 <= T <= 65536 entries");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(fa.transforms) & 3) == 0, "mlp_warp: transforms must be 4-byte aligned");
  CME_REQUIRE(wa.axes != nullptr && (reinterpret_cast<uintptr_t>(wa.axes) & 3) == 0,
              "mlp_warp: the axis tables are required, 4-byte aligned");
  CME_REQUIRE(wa.gy >= 1 && wa.gy <= kWarpMaxGrid && wa.gx >= 1 && wa.gx <= kWarpMaxGrid,
              "mlp_warp: the grid must satisfy 1 <= gy, gx <= 5");
  CME_REQUIRE(wa.A >= 0 && wa.A <= kWarpMaxA, "mlp_warp: the nodes' bound must satisfy 0 <= A <= 2048");
  const uintptr_t ea = static_cast<uintptr_t>(a.es) - 1;  // elements are loaded and stored at their natural alignment
  CME_REQUIRE(((reinterpret_cast<uintptr_t>(a.X0) | reinterpret_cast<uintptr_t>(a.X) |
                reinterpret_cast<uintptr_t>(a.XT)) & ea) == 0,
              "mlp_warp: X0, X and XT must be aligned to the element size");
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_form(a.es, vec_rows(a), vec_runs(a), [&](auto t, auto vec, auto vec_t) {
    hipLaunchKernelGGL((warp_kernel<decltype(t), decltype(vec)::value, decltype(vec_t)::value>), grid_of(a),
                       dim3(kThreads), 0, st, wa);
  });
  CME_LAUNCH_CHECK(st);
}

}  // namespace cme
