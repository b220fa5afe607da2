// Host-side tests of the elastic distortion rule (csrc/mlp/warp.h), exhaustively on small images: the node reduction's
// range and determinism, the axis tables' fix-up (the weights sum to exactly 4096, none is negative, the cell lies in
// the grid), the integer ranges at the extreme parameters (r_a inside int32, d17 inside 2^20), the constant lattice, the
// derived field bound against the fp64 B-spline, and A == 0 against affine_pixel for every element kind.  Built with
// ASan + UBSan under CME_SANITIZE=ON: the images and the lattices are allocations of exactly their size, so a tap or a
// node outside them is reported, and a signed overflow in the int32 sums aborts.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mlp/warp.h"
#include "tests/test_macros.h"

using namespace cme;

namespace {

const int kShapes[5][2] = {{1, 1}, {1, 7}, {5, 6}, {8, 9}, {28, 28}};
const AffineEntry kEntries[] = {{65536, 0, 0, 65536},   {-65536, 0, 0, -65536}, {0, 65536, -65536, 0},
                                {46341, 46341, -46341, 46341}, {4096, 0, 0, 4096},     {1048576, 0, 0, 1048576},
                                {(1 << 23) - 1, (1 << 23) - 1, (1 << 23) - 1, (1 << 23) - 1}, {65535, 1, -1, 65537}};

std::vector<WarpAxis> axes_of(int h, int w, int gy, int gx) {
  std::vector<WarpAxis> ax;
  for (int y = 0; y < h; ++y) ax.push_back(warp_axis_entry(y, h, gy));
  for (int x = 0; x < w; ++x) ax.push_back(warp_axis_entry(x, w, gx));
  return ax;
}

WarpDisp displace(const std::vector<WarpAxis>& ax, const std::vector<WarpNode>& nodes, int h, int y, int x, int gx) {
  return warp_displace(ax[y], ax[h + x], gx, [&](int j) { return nodes.at(static_cast<size_t>(j)); });
}

void bspline(double t, double* b) {
  const double s = 1.0 - t;
  b[0] = s * s * s / 6.0;
  b[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
  b[2] = (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0;
  b[3] = t * t * t / 6.0;
}

template <typename U>
void check_still(bool* success, const std::vector<U>& img, int h, int w) {
  const std::vector<WarpAxis> ax = axes_of(h, w, 3, 2);
  const std::vector<WarpNode> nodes(6 * 5, WarpNode{0, 0});
  for (const AffineEntry& q : kEntries)
    for (int dy = -(h - 1); dy <= h - 1; ++dy)
      for (int dx = -(w - 1); dx <= w - 1; ++dx)
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            const WarpDisp d = displace(ax, nodes, h, y, x, 2);
            EXPECT_TRUE(d.x == 0 && d.y == 0);
            const U got = warp_blend<U>(img.data(), warp_taps(y, x, dx, dy, q, h, w, d), h, w);
            const U want = affine_pixel<U>(img.data(), y, x, dx, dy, q, h, w);
            EXPECT_TRUE(std::memcmp(&got, &want, sizeof(U)) == 0);
          }
}

}  // namespace

CME_TEST(node_reduction_stays_in_range_reaches_both_ends_and_is_deterministic) {
  for (int A : {0, 1, 5, 256, 2047, kWarpMaxA}) {
    EXPECT_EQ(augment_reduce(0u, A), -A);
    EXPECT_EQ(augment_reduce(0xffffffffu, A), A);
    EXPECT_EQ(augment_reduce(0x80000000u, A), 0);
  }
  const uint64_t key = augment_key(3u, 9u);
  int lo = 0, hi = 0, same_sample = 0, same_epoch = 0;
  for (uint32_t src = 0; src < 2000; ++src) {
    const uint64_t nk = warp_node_key(src, key);
    EXPECT_TRUE(nk == warp_node_key(src, key));
    for (uint32_t j = 0; j < 64; ++j) {
      const WarpNode n = warp_node(nk, j, 5);
      EXPECT_TRUE(n.ddx >= -5 && n.ddx <= 5 && n.ddy >= -5 && n.ddy <= 5);
      lo += (n.ddx == -5) + (n.ddy == -5);
      hi += (n.ddx == 5) + (n.ddy == 5);
      const WarpNode big = warp_node(nk, j, kWarpMaxA);
      EXPECT_TRUE(big.ddx >= -kWarpMaxA && big.ddx <= kWarpMaxA && big.ddy >= -kWarpMaxA && big.ddy <= kWarpMaxA);
      const WarpNode back = warp_unpack(warp_pack(big));
      EXPECT_TRUE(back.ddx == big.ddx && back.ddy == big.ddy);
      const WarpNode other = warp_node(warp_node_key(src + 1, key), j, kWarpMaxA);
      same_sample += other.ddx == big.ddx && other.ddy == big.ddy;
      const WarpNode next = warp_node(warp_node_key(src, augment_key(3u, 10u)), j, kWarpMaxA);
      same_epoch += next.ddx == big.ddx && next.ddy == big.ddy;
      EXPECT_TRUE(warp_node(nk, j, 0).ddx == 0 && warp_node(nk, j, 0).ddy == 0);
    }
  }
  EXPECT_TRUE(lo > 20000 && hi > 20000);  // 256 000 draws of 11 values: 23 273 expected
  EXPECT_TRUE(same_sample < 5 && same_epoch < 5);
  for (int v : {-2048, -1, 0, 1, 2048}) {
    const WarpNode n = warp_unpack(warp_pack(WarpNode{v, -v}));
    EXPECT_TRUE(n.ddx == v && n.ddy == -v);
  }
}

CME_TEST(axis_entries_sum_to_4096_have_no_negative_weight_and_stay_in_the_grid) {
  for (int g = 1; g <= kWarpMaxGrid; ++g)
    for (int n : {1, 2, 3, 5, 6, 7, 9, 21, 28, 37, 64, 255, 1000, 4097}) {
      int last = 0;
      for (int x = 0; x < n; ++x) {
        const WarpAxis e = warp_axis_entry(x, n, g);
        EXPECT_TRUE(e.i >= 0 && e.i < g && e.i >= last);
        last = e.i;
        int sum = 0;
        for (int k = 0; k < 4; ++k) {
          EXPECT_TRUE(e.w[k] >= 0 && e.w[k] <= 2731);  // b1(0) = 2 / 3 is the largest weight
          sum += e.w[k];
        }
        EXPECT_EQ(sum, kWarpOne);
        const WarpAxis m = warp_axis_entry(n - 1 - x, n, g);  // the mirror pixel: t -> 1 - t, the weights reversed ...
        if (m.i == g - 1 - e.i)                               // (... away from a cell border, where floor breaks the tie)
          for (int k = 0; k < 4; ++k) EXPECT_TRUE(std::abs(m.w[3 - k] - e.w[k]) <= 2);
        // each weight is within 3/2 units of the real one (the header's bound on the adjusted weight)
        const double u = (2.0 * x + 1.0) * g / (2.0 * n);
        double b[4];
        bspline(u - e.i, b);
        double E = 0.0;
        for (int k = 0; k < 4; ++k) E += std::fabs(e.w[k] / 4096.0 - b[k]);
        EXPECT_TRUE(E <= 3.0 / 4096 + 1e-12);
      }
    }
}

CME_TEST(extreme_lattices_stay_inside_int32_and_the_field_inside_2_pow_20) {
  for (const auto& s : kShapes)
    for (int gy : {1, 3, 5})
      for (int gx : {1, 2, 5}) {
        const int h = s[0], w = s[1], L = (gy + 3) * (gx + 3);
        const std::vector<WarpAxis> ax = axes_of(h, w, gy, gx);
        for (int pattern = 0; pattern < 4; ++pattern) {
          std::vector<WarpNode> nodes(L);
          for (int j = 0; j < L; ++j) {
            const int sx = pattern == 0 ? 1 : pattern == 1 ? -1 : (j % 2 ? 1 : -1), sy = pattern == 3 ? -sx : sx;
            nodes[j] = WarpNode{sx * kWarpMaxA, sy * kWarpMaxA};
          }
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
              // the rows' sums, as warp_displace forms them (int32 under UBSan), restated in int64
              for (int a = 0; a < 4; ++a) {
                int64_t r = 0;
                for (int b = 0; b < 4; ++b)
                  r += static_cast<int64_t>(ax[h + x].w[b]) * nodes[(ax[y].i + a) * (gx + 3) + ax[h + x].i + b].ddx;
                EXPECT_TRUE(r >= -(int64_t{1} << 23) && r <= (int64_t{1} << 23));
              }
              const WarpDisp d = displace(ax, nodes, h, y, x, gx);
              EXPECT_TRUE(d.x >= -(1 << 20) && d.x <= (1 << 20) && d.y >= -(1 << 20) && d.y <= (1 << 20));
              if (pattern == 0) EXPECT_TRUE(d.x == (1 << 20) && d.y == (1 << 20));
              if (pattern == 1) EXPECT_TRUE(d.x == -(1 << 20) && d.y == -(1 << 20));
            }
        }
      }
}

CME_TEST(a_constant_lattice_displaces_every_pixel_by_exactly_c_over_256) {
  const int h = 8, w = 9;
  for (int gy : {1, 4})
    for (int gx : {2, 5}) {
      const std::vector<WarpAxis> ax = axes_of(h, w, gy, gx);
      for (int c : {-2048, -257, -1, 0, 1, 3, 256, 2048}) {
        const std::vector<WarpNode> nodes((gy + 3) * (gx + 3), WarpNode{c, -c});
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x) {
            const WarpDisp d = displace(ax, nodes, h, y, x, gx);
            EXPECT_TRUE(d.x == 512 * c && d.y == -512 * c);
          }
      }
    }
}

CME_TEST(the_integer_field_is_within_the_derived_bound_of_the_fp64_bspline) {
  const uint64_t key = augment_key(1u, 2u);
  double worst = 0.0;
  for (const auto& s : kShapes)
    for (int gy : {1, 3, 5})
      for (int gx : {1, 3, 5}) {
        const int h = s[0], w = s[1], L = (gy + 3) * (gx + 3);
        const std::vector<WarpAxis> ax = axes_of(h, w, gy, gx);
        for (uint32_t src = 0; src < 4; ++src) {
          std::vector<WarpNode> nodes(L);
          for (int j = 0; j < L; ++j) nodes[j] = warp_node(warp_node_key(src, key), static_cast<uint32_t>(j), kWarpMaxA);
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
              double by[4], bx[4], fx = 0.0, fy = 0.0;
              bspline((2.0 * y + 1.0) * gy / (2.0 * h) - ax[y].i, by);
              bspline((2.0 * x + 1.0) * gx / (2.0 * w) - ax[h + x].i, bx);
              for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) {
                  const WarpNode& n = nodes[(ax[y].i + a) * (gx + 3) + ax[h + x].i + b];
                  fx += by[a] * bx[b] * n.ddx / 256.0;
                  fy += by[a] * bx[b] * n.ddy / 256.0;
                }
              const WarpDisp d = displace(ax, nodes, h, y, x, gx);
              worst = std::fmax(worst, std::fmax(std::fabs(d.x * 0x1p-17 - fx), std::fabs(d.y * 0x1p-17 - fy)));
            }
        }
      }
  std::printf("  worst distance of the integer field from the fp64 field: %.5f pixel (bound %.5f)\n", worst,
              warp_field_bound(8.0));
  EXPECT_TRUE(worst <= warp_field_bound(8.0));
  EXPECT_NEAR(warp_field_bound(8.0), 0.01172256, 1e-7);
  EXPECT_NEAR(warp_field_bound(0.0), 0x1p-18, 0.0);
}

CME_TEST(a_zero_bound_is_bitwise_the_affine_rule_for_every_element_kind) {
  for (const auto& s : {kShapes[0], kShapes[1], kShapes[2]}) {
    const int h = s[0], w = s[1], p = h * w;
    std::vector<uint8_t> b(p);
    std::vector<uint16_t> h16(p);
    std::vector<uint32_t> f32(p);
    std::vector<uint64_t> f64(p);
    for (int f = 0; f < p; ++f) {
      b[f] = static_cast<uint8_t>(1 + (f * 37) % 255);
      const float v = (f % 2 ? -1.0f : 1.0f) * (0.37f + 1.625f * f);
      f32[f] = affine_bits_of_f32(v);
      h16[f] = affine_bf16_of_f32(v);
      f64[f] = affine_bits_of_f64(static_cast<double>(v) / 3.0);
    }
    check_still(success, b, h, w);
    check_still(success, h16, h, w);
    check_still(success, f32, h, w);
    check_still(success, f64, h, w);
  }
}

CME_TEST(a_moving_field_forms_no_tap_outside_the_image) {
  // images of exactly h * w elements under the extreme entries, full-range shifts and lattices at the bound: ASan
  // reports a tap outside them; some pixels keep a tap and some keep none
  for (const auto& s : {kShapes[1], kShapes[2], kShapes[3]}) {
    const int h = s[0], w = s[1];
    const std::vector<uint8_t> img(static_cast<size_t>(h) * w, 255);
    const std::vector<WarpAxis> ax = axes_of(h, w, 5, 1);
    std::vector<WarpNode> nodes(8 * 4);
    for (size_t j = 0; j < nodes.size(); ++j)
      nodes[j] = warp_node(warp_node_key(static_cast<uint32_t>(j), 77u), 3u, kWarpMaxA);
    int empty = 0, lit = 0;
    for (const AffineEntry& q : kEntries)
      for (int dy : {-(h - 1), 0, h - 1})
        for (int dx : {-(w - 1), 0, w - 1})
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
              const WarpDisp d = displace(ax, nodes, h, y, x, 1);
              const uint8_t v = warp_blend<uint8_t>(img.data(), warp_taps(y, x, dx, dy, q, h, w, d), h, w);
              empty += v == 0;
              lit += v != 0;
            }
    EXPECT_TRUE(empty > 0 && lit > 0);
  }
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
