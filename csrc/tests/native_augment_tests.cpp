// Host-side tests of the augmentation rule (csrc/mlp/augment.h): the range and determinism of augment_shift, the
// key's separation from the shuffle's, and augment_src_feature checked exhaustively on small images against a two-loop
// restatement.  Built with ASan + UBSan under CME_SANITIZE=ON: the images are allocations of exactly h * w elements,
// so a source index outside them is reported.
#include <cstdint>
#include <vector>

#include "mlp/augment.h"
#include "tests/test_macros.h"

using namespace cme;

CME_TEST(shift_stays_in_range_and_zero_bound_gives_zero) {
  for (int m : {0, 1, 2, 27}) {
    const uint64_t key = augment_key(7u, 1234u);
    int lo_x = m, hi_x = -m, lo_y = m, hi_y = -m;
    for (uint32_t src = 0; src < 20000u; ++src) {
      const AugmentShift s = augment_shift(src, key, m, m);
      EXPECT_TRUE(s.dx >= -m && s.dx <= m && s.dy >= -m && s.dy <= m);
      lo_x = s.dx < lo_x ? s.dx : lo_x, hi_x = s.dx > hi_x ? s.dx : hi_x;
      lo_y = s.dy < lo_y ? s.dy : lo_y, hi_y = s.dy > hi_y ? s.dy : hi_y;
      const AugmentShift only_x = augment_shift(src, key, m, 0), only_y = augment_shift(src, key, 0, m);
      EXPECT_TRUE(only_x.dy == 0 && only_x.dx == s.dx && only_y.dx == 0 && only_y.dy == s.dy);
    }
    EXPECT_TRUE(lo_x == -m && hi_x == m && lo_y == -m && hi_y == m);  // both ends are reached
  }
  // the ends of the 32-bit range map to the ends of [-m, m]
  EXPECT_EQ(augment_reduce(0u, 2), -2);
  EXPECT_EQ(augment_reduce(0xffffffffu, 2), 2);
  EXPECT_EQ(augment_reduce(0x80000000u, 2), 0);
  EXPECT_EQ(augment_reduce(0xffffffffu, 0), 0);
}

CME_TEST(shift_depends_on_seed_iter_and_source_alone) {
  // nothing but (seed, iter, src) enters: the same sample of a set of any size gets the same shift
  for (uint32_t seed : {0u, 5u, 0xffffffffu})
    for (uint32_t iter : {0u, 75u, 0xffffffffu}) {
      const uint64_t key = augment_key(seed, iter);
      EXPECT_TRUE(key == augment_key(seed, iter));
      EXPECT_TRUE(key != shuffle_key(seed, iter));  // a stream of its own
      EXPECT_TRUE(key != augment_key(seed, iter + 1u) && key != augment_key(seed + 1u, iter));
      for (uint32_t src : {0u, 1u, 999u, 59999u, 0xfffffffeu}) {
        const AugmentShift a = augment_shift(src, key, 2, 3), b = augment_shift(src, key, 2, 3);
        EXPECT_TRUE(a.dx == b.dx && a.dy == b.dy);
      }
    }
  // ... and the shuffle's key, used as an augmentation key, gives other shifts
  int differ = 0;
  for (uint32_t src = 0; src < 1000u; ++src) {
    const AugmentShift a = augment_shift(src, augment_key(3u, 9u), 2, 2);
    const AugmentShift b = augment_shift(src, shuffle_key(3u, 9u), 2, 2);
    differ += a.dx != b.dx || a.dy != b.dy;
  }
  EXPECT_TRUE(differ > 900);
}

static void check_shape(bool* success, int h, int w) {
  std::vector<int> img(static_cast<size_t>(h) * w);  // exactly h * w elements: the image holds its own indices
  for (int f = 0; f < h * w; ++f) img[f] = f;
  for (int dy = -(h - 1); dy <= h - 1; ++dy)
    for (int dx = -(w - 1); dx <= w - 1; ++dx) {
      std::vector<int> want(static_cast<size_t>(h) * w, -1);  // the two-loop restatement: out[y][x] = in[y - dy][x - dx]
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          const int sy = y - dy, sx = x - dx;
          if (sy >= 0 && sy < h && sx >= 0 && sx < w) want[y * w + x] = img[sy * w + sx];
        }
      for (int f = 0; f < h * w; ++f) {
        const int sf = augment_src_feature(f, dx, dy, h, w);
        EXPECT_TRUE(sf >= -1 && sf < h * w);
        const int got = sf >= 0 ? img[sf] : -1;
        EXPECT_EQ(got, want[f]);
        EXPECT_EQ(sf, augment_src_yx(f / w, f % w, dx, dy, h, w));
      }
    }
  // positive dx moves content right, positive dy moves it down
  if (w > 1) EXPECT_EQ(augment_src_feature(1, 1, 0, h, w), 0);
  if (h > 1) EXPECT_EQ(augment_src_feature(w, 0, 1, h, w), 0);
  EXPECT_EQ(augment_src_feature(0, w > 1 ? 1 : 0, h > 1 ? 1 : 0, h, w), (h > 1 || w > 1) ? -1 : 0);
}

CME_TEST(source_feature_exhaustive_5x6) { check_shape(success, 5, 6); }

CME_TEST(source_feature_exhaustive_1x7) { check_shape(success, 1, 7); }

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
