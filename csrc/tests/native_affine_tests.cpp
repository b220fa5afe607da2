// Host-side tests of the affine augmentation rule (csrc/mlp/affine.h), exhaustively on small images: identity entries
// against augment_src_yx for every shift in range, the uint8 blend's ceiling on all-255 images under extreme entries,
// skipped taps and pixels without a tap, the range of the index reduction and its determinism.  Built with ASan + UBSan
// under CME_SANITIZE=ON: the images are allocations of exactly h * w elements, so a tap outside them is reported.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mlp/affine.h"
#include "tests/test_macros.h"

using namespace cme;

namespace {

const AffineEntry kIdentity{65536, 0, 0, 65536};
const int kShapes[4][2] = {{1, 1}, {1, 7}, {5, 6}, {8, 9}};

// entries that leave the image on every side: the largest magnitudes the table admits, pure flips, a quarter turn,
// sixteen-fold shrinking and enlarging, and sub-pixel maps
const AffineEntry kExtreme[] = {
    {(1 << 23) - 1, (1 << 23) - 1, (1 << 23) - 1, (1 << 23) - 1}, {-(1 << 23) + 1, (1 << 23) - 1, -(1 << 23) + 1, 1},
    {-65536, 0, 0, -65536}, {0, 65536, -65536, 0}, {4096, 0, 0, 4096}, {1048576, 0, 0, 1048576},
    {65536, 113512, 0, 65536}, {46341, 46341, -46341, 46341}, {1, 0, 0, 1}, {0, 0, 0, 0}, {65535, 1, -1, 65537},
    {32768, 32768, 32768, -32768}, {65536 + 255, 0, 0, 65536 - 255}};

template <typename U>
std::vector<U> transformed(const std::vector<U>& img, int dx, int dy, const AffineEntry& q, int h, int w) {
  std::vector<U> out(img.size());
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[y * w + x] = affine_pixel<U>(img.data(), y, x, dx, dy, q, h, w);
  return out;
}

template <typename U>
void check_identity(bool* success, const std::vector<U>& img, int h, int w) {
  for (int dy = -(h - 1); dy <= h - 1; ++dy)
    for (int dx = -(w - 1); dx <= w - 1; ++dx) {
      const std::vector<U> got = transformed(img, dx, dy, kIdentity, h, w);
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          const int sf = augment_src_yx(y, x, dx, dy, h, w);
          const U want = sf >= 0 ? img[sf] : U{0};
          EXPECT_TRUE(std::memcmp(&got[y * w + x], &want, sizeof(U)) == 0);
        }
    }
}

}  // namespace

CME_TEST(identity_entries_equal_the_shift_gather_for_every_element_kind) {
  for (const auto& s : kShapes) {
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
      f64[f] = affine_bits_of_f64(-0.1 - 1e-3 * f);
    }
    f32[0] = 0x80000000u;            // -0.0f
    f64[p - 1] = 0x8000000000000000ull;  // -0.0
    check_identity(success, b, h, w);
    check_identity(success, h16, h, w);
    check_identity(success, f32, h, w);
    check_identity(success, f64, h, w);
  }
}

CME_TEST(uint8_output_stays_at_or_below_255_under_extreme_entries) {
  for (const auto& s : kShapes) {
    const int h = s[0], w = s[1];
    const std::vector<uint8_t> img(static_cast<size_t>(h) * w, 255);
    for (const AffineEntry& q : kExtreme)
      for (int dy = -(h - 1); dy <= h - 1; ++dy)
        for (int dx = -(w - 1); dx <= w - 1; ++dx)
          for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
              const AffineTaps t = affine_taps(y, x, dx, dy, q, h, w);
              uint32_t wsum = 0, present = 0;
              for (int k = 0; k < 4; ++k) {
                wsum += affine_tap_weight(t, k);
                const int sf = affine_tap_feature(t, k, h, w);
                EXPECT_TRUE(sf >= -1 && sf < h * w);
                if (sf >= 0) present += affine_tap_weight(t, k);
              }
              EXPECT_EQ(wsum, 65536u);  // the four weights always sum to 2^16
              const uint32_t got = affine_blend_u8(t, h, w, [&](int sf) { return img[sf]; });
              EXPECT_TRUE(got <= 255u);
              EXPECT_EQ(got, (present * 255u + 32768u) >> 16);
              EXPECT_EQ(static_cast<uint32_t>(affine_pixel<uint8_t>(img.data(), y, x, dx, dy, q, h, w)), got);
            }
  }
}

CME_TEST(skipped_taps_and_pixels_without_a_tap) {
  const int h = 5, w = 6;
  std::vector<uint8_t> img(h * w);
  std::vector<uint64_t> f64(h * w);
  for (int f = 0; f < h * w; ++f) img[f] = static_cast<uint8_t>(10 + f), f64[f] = affine_bits_of_f64(10.0 + f);
  // the identity's taps with the x fraction set to one half: taps (y, x) and (y, x + 1) with weights 1/2 each; the
  // lower two have weight 0 and are skipped although they lie inside the image
  const AffineEntry q{65536, 0, 0, 65536};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      AffineTaps t = affine_taps(y, x, 0, 0, q, h, w);
      EXPECT_TRUE(t.ix == x && t.iy == y && t.fx == 0 && t.fy == 0);
      t.fx = 128;
      EXPECT_EQ(affine_tap_feature(t, 0, h, w), y * w + x);
      EXPECT_EQ(affine_tap_feature(t, 1, h, w), x + 1 < w ? y * w + x + 1 : -1);  // the right neighbour, or outside
      EXPECT_EQ(affine_tap_feature(t, 2, h, w), -1);                              // weight 0: skipped
      EXPECT_EQ(affine_tap_feature(t, 3, h, w), -1);
      const uint32_t right = x + 1 < w ? img[y * w + x + 1] : 0u;
      EXPECT_EQ(affine_blend_u8(t, h, w, [&](int sf) { return img[sf]; }),
                (32768u * img[y * w + x] + 32768u * right + 32768u) >> 16);
      double r = -1.0;
      EXPECT_TRUE(affine_blend_f64(t, h, w, [&](int sf) { return affine_f64_of_bits(f64[sf]); }, r));
      EXPECT_EQ(r, 0.5 * (10.0 + y * w + x) + (x + 1 < w ? 0.5 * (10.0 + y * w + x + 1) : 0.0));
    }
  // a 16-fold shrinking about the centre leaves (nearly) every destination pixel of so small an image without a tap:
  // zeros of every kind, and `out` untouched
  const AffineEntry shrink{1048576, 0, 0, 1048576};
  int none = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const AffineTaps t = affine_taps(y, x, 0, 0, shrink, h, w);
      bool any = false;
      for (int k = 0; k < 4; ++k) any = any || affine_tap_feature(t, k, h, w) >= 0;
      double r = -7.0;
      EXPECT_EQ(affine_blend_f64(t, h, w, [&](int sf) { return affine_f64_of_bits(f64[sf]); }, r), any);
      if (!any) {
        ++none;
        EXPECT_EQ(r, -7.0);
        EXPECT_EQ(affine_pixel<uint8_t>(img.data(), y, x, 0, 0, shrink, h, w), 0);
        EXPECT_EQ(affine_pixel<uint64_t>(f64.data(), y, x, 0, 0, shrink, h, w), uint64_t{0});
      }
    }
  EXPECT_TRUE(none >= h * w - 4);
  // negative source coordinates floor: sx = -1/4 pixel -> ix = -1, fx = 192
  const AffineTaps t = affine_taps(0, 0, 0, 0, AffineEntry{65536, 0, 0, 65536}, 1, 1);
  EXPECT_TRUE(t.ix == 0 && t.iy == 0);
  const AffineTaps left = affine_taps(0, 0, 1, 0, AffineEntry{32768, 0, 0, 65536}, 1, 2);  // u = -3: sx = -1/4 pixel
  EXPECT_TRUE(left.ix == -1 && left.fx == 192);
}

CME_TEST(bf16_rounding_is_to_nearest_even) {
  EXPECT_EQ(affine_bf16_of_f32(1.0f), 0x3f80);
  EXPECT_EQ(affine_bf16_of_f32(affine_f32_of_bits(0x3f808000u)), 0x3f80);  // a tie: to the even 0x3f80
  EXPECT_EQ(affine_bf16_of_f32(affine_f32_of_bits(0x3f818000u)), 0x3f82);  // a tie: to the even 0x3f82
  EXPECT_EQ(affine_bf16_of_f32(affine_f32_of_bits(0x3f808001u)), 0x3f81);
  EXPECT_EQ(affine_bf16_of_f32(affine_f32_of_bits(0x7f7fffffu)), 0x7f80);  // the largest f32 rounds to infinity
  EXPECT_EQ(affine_bf16_of_f32(affine_f32_of_bits(0x7fc00001u)) & 0x7fc0, 0x7fc0);  // a NaN stays a NaN
}

CME_TEST(index_reduction_covers_the_table_ends_included) {
  const uint64_t key = augment_key(7u, 1234u);
  for (uint32_t T : {1u, 2u, 1024u}) {
    std::vector<int> seen(T, 0);
    for (uint32_t src = 0; src < 200000u; ++src) {
      const uint32_t k = affine_index(src, key, T);
      EXPECT_TRUE(k < T);
      if (k < T) seen[k] = 1;
    }
    int n = 0;
    for (int s : seen) n += s;
    EXPECT_EQ(n, static_cast<int>(T));  // every entry, the first and the last included
  }
  EXPECT_TRUE(affine_index(0u, key, 65536u) < 65536u);
}

CME_TEST(index_depends_on_seed_iter_and_source_alone) {
  for (uint32_t seed : {0u, 5u, 0xffffffffu})
    for (uint32_t iter : {0u, 75u, 0xffffffffu}) {
      const uint64_t key = augment_key(seed, iter);
      for (uint32_t src : {0u, 1u, 999u, 59999u, 0xfffffffeu})
        EXPECT_EQ(affine_index(src, key, 1024u), affine_index(src, augment_key(seed, iter), 1024u));
    }
  // a stream of its own: not the shift's hash reduced again, and another epoch or seed gives other entries
  int same_as_shift = 0, same_next_epoch = 0, same_next_seed = 0;
  const uint64_t key = augment_key(3u, 9u);
  for (uint32_t src = 0; src < 1000u; ++src) {
    const uint32_t k = affine_index(src, key, 5u);
    same_as_shift += static_cast<int>(k) == augment_shift(src, key, 2, 0).dx + 2;
    same_next_epoch += k == affine_index(src, augment_key(3u, 10u), 5u);
    same_next_seed += k == affine_index(src, augment_key(4u, 9u), 5u);
  }
  EXPECT_TRUE(same_as_shift < 300 && same_next_epoch < 300 && same_next_seed < 300);  // 200 expected by chance
}

CME_TEST(table_entries_are_identity_for_identity_parameters_and_deterministic) {
  for (uint32_t seed : {0u, 9u})
    for (uint32_t k : {0u, 1u, 1023u, 65535u}) {
      const AffineEntry e = affine_table_entry(seed, k, 0.0, 1.0, 1.0, 0.0);
      EXPECT_TRUE(e.q00 == 65536 && e.q01 == 0 && e.q10 == 0 && e.q11 == 65536);
      const AffineEntry a = affine_table_entry(seed, k, 180.0, 1.0 / 16, 16.0, 60.0);
      const AffineEntry b = affine_table_entry(seed, k, 180.0, 1.0 / 16, 16.0, 60.0);
      EXPECT_TRUE(a.q00 == b.q00 && a.q01 == b.q01 && a.q10 == b.q10 && a.q11 == b.q11);
      for (int32_t q : {a.q00, a.q01, a.q10, a.q11}) EXPECT_TRUE(q > -(1 << 23) && q < (1 << 23));
    }
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
