// Elastic distortion of the resident training set (warp.hip): a smooth random displacement field per image and epoch,
// on top of the affine map and the shift of affine.h.
//
// Once per epoch the warping gather rewrites every resident layout from the pristine rows, like the affine gather
// (affine.h), and on the way moves every destination pixel's source position by its own small displacement, read off a
// coarse lattice of random control nodes through a uniform cubic B-spline (Simard, Steinkraus and Platt 2003 smooth a
// random field with a Gaussian; the cubic B-spline is its compact, integer-friendly stand-in).  The rule is stateless;
// the device does integer work only, plus affine.h's fp64 chain for non-byte elements, and the host (g++,
// bindings_cpu.cpp `warp_axes` / `epoch_nodes` / `warp_field` / `warp_rows`, the native test) computes the same values
// from this same header.  Only the host evaluates real-valued formulas.
//
//   * policy: alpha, the bound of a node's displacement in pixels (0 <= alpha <= 8), as A = llrint(alpha * 256), the
//     bound in Q8 (0 <= A <= kWarpMaxA = 2048); the grid (gy, gx), cells per axis, each in 1 .. kWarpMaxGrid = 5.  The
//     lattice has (gy + 3) rows of (gx + 3) nodes, node = row * (gx + 3) + column, L = (gy + 3)(gx + 3) <= 64 nodes.
//   * nodes, per source sample, epoch and node: key = augment_key(seed, iter) is augment.h's.  One 64-bit hash
//       warp_node_key(src, key) = shuffle_mix64(shuffle_mix64(key ^ kWarpNodeStream) + (src + 1) * golden)
//       hash = shuffle_mix64(warp_node_key + (node + 1) * golden)
//     whose low half gives ddx and whose high half gives ddy, each augment_reduce(half, A): [-A, A] in Q8 pixel, both
//     ends reached.  A node depends on (seed, iter, source index, node) alone.
//   * axis tables, built once per (grid, h, w) by the host in fp64 (warp_axis_entry), int32 [h + w][5], the h entries
//     of the y axis first: coordinate x of an axis of n pixels and g cells has
//       u = (2 x + 1) g / (2 n), i = floor(u) in [0, g - 1], t = u - i  (i and the numerator of t in integers),
//       b0 = (1 - t)^3 / 6, b1 = (3 t^3 - 6 t^2 + 4) / 6, b2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6, b3 = t^3 / 6,
//     each stored as Q12 w_k = llrint(b_k * 4096); then the largest (the first of equals) takes 4096 - sum more, so
//     the four sum to exactly kWarpOne = 4096.  The entry is {i, w0, w1, w2, w3} over nodes i .. i + 3 of the axis.
//     No weight is negative (the largest is >= 1024 and moves by at most 2).  A pure function of (g, n); no libm
//     beyond the rounding.
//   * per destination pixel (y, x), with the entries ay = axes[y], ax = axes[h + x]: for a = 0 .. 3
//       r_a = sum_b ax.w[b] * node[ay.i + a][ax.i + b]                 (int32: |r_a| <= 2048 * 4096 = 2^23)
//       d   = sum_a ay.w[a] * r_a                                      (int64, Q32 pixel: |d| <= 2^35)
//       d17 = (d + 2^14) >> 15                                         (affine_taps' unit, 2^-17 pixel: |d17| <= 2^20)
//     once for ddx (d17x) and once for ddy (d17y).  The source position is affine.h's sx, sy -- the same two
//     expressions of the sample's table entry and shift -- plus d17x, d17y (warp_taps); from there ix, fx, iy, fy, the
//     tap order, the skip rule (a tap's address is formed only after its range test) and the blends are affine.h's own
//     functions.  Zeros move in where no tap is present.
//
// Consequences: A == 0 makes every d17 zero, so the rule is bitwise affine.h's (and with an identity entry bitwise
// augment.h's) for every element type.  A lattice whose nodes all hold (c, c) displaces every pixel by exactly c / 256
// pixel: r_a = 4096 c, d = 2^24 c, d17 = 512 c.
//
// Field accuracy.  Against the real-valued field D = sum_a sum_b b_a(ty) b_b(tx) node / 256 of the same Q8 nodes the
// integer field differs only through the weights and the last shift.  Per axis, three weights are rounded (each off by
// at most 1/2 unit of 2^-12) and the adjusted one is off by minus the sum of the other three's errors (the real weights
// sum to 1, the stored ones to 4096), at most 3/2 units: E = sum_k |w_k / 4096 - b_k| <= 3 / 4096.  With stored weights
// that are non-negative and sum to one on each axis,
//   |sum_ab (w_a w_b / 2^24 - b_a b_b) node_ab / 256| <= (E_y sum_b w_b / 4096 + E_x sum_a b_a) alpha = 6 alpha / 4096,
// and the shift adds at most half a unit of 2^-17 pixel: |d17 / 2^17 - D| <= 6 alpha / 4096 + 2^-18 pixel
// (warp_field_bound: 0.0117 pixel at alpha = 8; the worst case measured over six shapes and grids is 0.0047).
#pragma once

#include "affine.h"

namespace cme {

constexpr uint64_t kWarpNodeStream = 0x8f1bbcdc6ed9eba1ull;  // (a fixed non-zero constant; part of the format)
constexpr int kWarpMaxGrid = 5;
constexpr int kWarpMaxNodes = (kWarpMaxGrid + 3) * (kWarpMaxGrid + 3);  // 64
constexpr int kWarpMaxA = 2048;  // alpha <= 8 pixels in Q8
constexpr int kWarpOne = 4096;   // the Q12 weights of an axis entry sum to this

struct WarpNode {
  int ddx, ddy;  // Q8 pixel, each in [-A, A]
};

// ---- per sample and node
__host__ __device__ inline uint64_t warp_node_key(uint32_t src, uint64_t key) {
  return shuffle_mix64(shuffle_mix64(key ^ kWarpNodeStream) + (static_cast<uint64_t>(src) + 1u) * 0x9e3779b97f4a7c15ull);
}
__host__ __device__ inline WarpNode warp_node(uint64_t node_key, uint32_t node, int A) {
  const uint64_t h = shuffle_mix64(node_key + (static_cast<uint64_t>(node) + 1u) * 0x9e3779b97f4a7c15ull);
  return WarpNode{augment_reduce(static_cast<uint32_t>(h), A), augment_reduce(static_cast<uint32_t>(h >> 32), A)};
}
// a node as the kernel keeps it: two int16 in one word, ddx low (|dd| <= 2048 fits)
__host__ __device__ inline uint32_t warp_pack(const WarpNode& n) {
  return (static_cast<uint32_t>(n.ddx) & 0xffffu) | (static_cast<uint32_t>(n.ddy) << 16);
}
__host__ __device__ inline WarpNode warp_unpack(uint32_t v) {
  return WarpNode{static_cast<int16_t>(v & 0xffffu), static_cast<int16_t>(v >> 16)};
}

// ---- the axis tables (host only: fp64)
struct WarpAxis {
  int32_t i, w[4];
};

inline WarpAxis warp_axis_entry(int x, int n, int g) {
  const int64_t num = (2 * static_cast<int64_t>(x) + 1) * g, den = 2 * static_cast<int64_t>(n);
  const int64_t i = num / den;  // < g: 2 x + 1 < 2 n
  const double t = static_cast<double>(num - i * den) / static_cast<double>(den), s = 1.0 - t;
  const double b[4] = {s * s * s / 6.0, (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0,
                       (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0, t * t * t / 6.0};
  WarpAxis e{static_cast<int32_t>(i), {0, 0, 0, 0}};
  int sum = 0, big = 0;
  for (int k = 0; k < 4; ++k) {
    e.w[k] = static_cast<int32_t>(std::llrint(b[k] * kWarpOne));
    sum += e.w[k];
    if (e.w[k] > e.w[big]) big = k;
  }
  e.w[big] += kWarpOne - sum;
  return e;
}

// the derived bound of the header comment, in pixels
inline double warp_field_bound(double alpha) { return 6.0 * alpha / kWarpOne + 0x1p-18; }

// ---- per pixel
struct WarpDisp {
  int x, y;  // 2^-17 pixel
};

// node(j) -> the WarpNode of lattice node j = row * (gx + 3) + column of the pixel's sample
template <typename Node>
__host__ __device__ inline WarpDisp warp_displace(const WarpAxis& ay, const WarpAxis& ax, int gx, Node&& node) {
  int64_t dx = 0, dy = 0;
  for (int a = 0; a < 4; ++a) {
    const int j0 = (ay.i + a) * (gx + 3) + ax.i;
    int rx = 0, ry = 0;
    for (int b = 0; b < 4; ++b) {
      const WarpNode n = node(j0 + b);
      rx += ax.w[b] * n.ddx;
      ry += ax.w[b] * n.ddy;
    }
    dx += static_cast<int64_t>(ay.w[a]) * rx;
    dy += static_cast<int64_t>(ay.w[a]) * ry;
  }
  return WarpDisp{static_cast<int>((dx + (1 << 14)) >> 15), static_cast<int>((dy + (1 << 14)) >> 15)};
}

// affine_taps with the source position moved by d: sx and sy are affine.h's two expressions, term for term
__host__ __device__ inline AffineTaps warp_taps(int y, int x, int dx, int dy, const AffineEntry& q, int h, int w,
                                                const WarpDisp& d) {
  const int u = 2 * x - (w - 1) - 2 * dx, v = 2 * y - (h - 1) - 2 * dy;
  const int64_t sx =
      static_cast<int64_t>(q.q00) * u + static_cast<int64_t>(q.q01) * v + static_cast<int64_t>(w - 1) * 65536 + d.x;
  const int64_t sy =
      static_cast<int64_t>(q.q10) * u + static_cast<int64_t>(q.q11) * v + static_cast<int64_t>(h - 1) * 65536 + d.y;
  return AffineTaps{sx >> 17, sy >> 17, static_cast<int>((sx >> 9) & 255), static_cast<int>((sy >> 9) & 255)};
}

// One destination pixel from its taps, as affine_pixel blends it: `row` points at the h * w elements of the source
// image and is indexed by present taps only.
template <typename U>
__host__ __device__ inline U warp_blend(const U* row, const AffineTaps& t, int h, int w) {
  if constexpr (sizeof(U) == 1) {
    return static_cast<U>(affine_blend_u8(t, h, w, [&](int sf) { return row[sf]; }));
  } else {
    double r = 0.0;
    bool any;
    if constexpr (sizeof(U) == 2) {
      any = affine_blend_f64(
          t, h, w, [&](int sf) { return static_cast<double>(affine_f32_of_bits(static_cast<uint32_t>(row[sf]) << 16)); },
          r);
      return any ? affine_bf16_of_f32(affine_f32_of_f64(r)) : U{0};
    } else if constexpr (sizeof(U) == 4) {
      any = affine_blend_f64(t, h, w, [&](int sf) { return static_cast<double>(affine_f32_of_bits(row[sf])); }, r);
      return any ? affine_bits_of_f32(affine_f32_of_f64(r)) : U{0};
    } else {
      any = affine_blend_f64(t, h, w, [&](int sf) { return affine_f64_of_bits(row[sf]); }, r);
      return any ? affine_bits_of_f64(r) : U{0};
    }
  }
}

// One launch rewrites every resident layout as mlp_affine does (`aff`: the same fields with the same meaning), each
// image's source positions moved by the field of its own lattice.  axes: int32 [h + w][5] on the device (warp_axis_entry
// of (y, h, gy) for y < h, then of (x, w, gx)), 4-byte aligned; gy, gx: cells per axis; A: the nodes' bound in Q8.
// `stream` is a hipStream_t.  No sync, no read-back.
struct WarpArgs {
  AffineArgs aff;
  const int32_t* axes = nullptr;
  int gy = 0, gx = 0, A = 0;
};
void mlp_warp(const WarpArgs& a, void* stream);

}  // namespace cme
