// Host-side tests of the weight-averaging rule (csrc/mlp/ema.h): the decay sequence with and without warmup (monotone,
// bounded by `decay`, exact values at t = 0, 1, 90, 10^6), the fixed point p == e (signed zeros included) and one
// update against long-double arithmetic rounded once: exact for float, where the fused product-sum fits the 64-bit
// mantissa; for double it does not fit, the long-double result is itself rounded, and the check is a +-1 ulp bracket
// (the bitwise oracle for both types is the exact rational arithmetic of tests/test_ema.py).  Built with ASan + UBSan
// under CME_SANITIZE=ON: the arrays are allocations of exactly n elements, so a read past them is reported.
#include <cmath>
#include <cstring>
#include <random>
#include <vector>

#include "mlp/ema.h"
#include "tests/test_macros.h"

using namespace cme;

template <typename T>
static bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof a) == 0;
}

CME_TEST(decay_sequence_with_and_without_warmup) {
  const EmaRule plain{0.999, 0};
  const EmaRule warm{0.999, 1};
  for (double t : {0.0, 1.0, 90.0, 1e6}) EXPECT_TRUE(same_bits(ema_decay(plain, t), 0.999));
  EXPECT_TRUE(same_bits(ema_decay(warm, 0.0), 1.0 / 10.0));
  EXPECT_TRUE(same_bits(ema_decay(warm, 1.0), 2.0 / 11.0));
  EXPECT_TRUE(same_bits(ema_decay(warm, 90.0), 91.0 / 100.0));
  EXPECT_TRUE(same_bits(ema_decay(warm, 1e6), 0.999));  // (1 + 1e6) / (10 + 1e6) > 0.999: capped
  double last = 0.0;
  for (int t = 0; t < 20000; ++t) {
    const double d = ema_decay(warm, static_cast<double>(t));
    EXPECT_TRUE(d >= last && d <= 0.999 && d >= 0.1);
    last = d;
  }
  EXPECT_TRUE(same_bits(last, 0.999));
  // the cap takes over where (1 + t) / (10 + t) first reaches 0.999: t = 8990
  EXPECT_TRUE(ema_decay(warm, 8989.0) < 0.999 && same_bits(ema_decay(warm, 8991.0), 0.999));
  EXPECT_TRUE(same_bits(ema_decay(EmaRule{0.0, 1}, 5.0), 0.0) && same_bits(ema_decay(EmaRule{0.0, 0}, 5.0), 0.0));
  EXPECT_TRUE(ema_rule_ok(EmaRule{0.0, 0}) && !ema_rule_ok(EmaRule{1.0, 0}) && !ema_rule_ok(EmaRule{-0.5, 1}) &&
              !ema_rule_ok(EmaRule{std::nan(""), 0}));
}

template <typename T>
static void fixed_point(bool* success) {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::vector<T> v(257);
  for (T& x : v) x = static_cast<T>(nd(rng));
  v[0] = T(0);
  v[1] = -T(0);
  for (double d : {0.0, 0.5, 0.999}) {
    const T omd = ema_omd<T>(d);
    for (T x : v) EXPECT_TRUE(same_bits(ema_update<T>(x, x, omd), x));
  }
  // decay 0: the average becomes the parameters (omd = 1: e + (p - e) where that is exact)
  EXPECT_TRUE(same_bits(ema_update<T>(T(1), T(3), ema_omd<T>(0.0)), T(3)));
}

CME_TEST(fixed_point_f32) { fixed_point<float>(success); }
CME_TEST(fixed_point_f64) { fixed_point<double>(success); }

// one update in long double (64-bit mantissa: the difference and the fused product-sum of two T values with |exponent
// gap| small are exact there for float; for double the check uses operands whose difference is exact)
template <typename T>
static void one_update(bool* success) {
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> ud(0.5, 1.0);
  for (int warm = 0; warm < 2; ++warm) {
    const EmaRule r{0.999, warm};
    for (int t = 0; t < 5; ++t) {
      const double d = ema_decay(r, static_cast<double>(t));
      const T omd = ema_omd<T>(d);
      EXPECT_TRUE(same_bits(omd, static_cast<T>(1.0 - d)));
      for (int i = 0; i < 512; ++i) {
        // e and p in [0.5, 1): one binade, so p - e is exact in T and the only rounding is the fma's
        const T e = static_cast<T>(ud(rng)), p = static_cast<T>(ud(rng));
        const long double diff = static_cast<long double>(p) - static_cast<long double>(e);
        EXPECT_TRUE(static_cast<long double>(static_cast<T>(diff)) == diff);
        const T want = static_cast<T>(fmal(static_cast<long double>(omd), diff, static_cast<long double>(e)));
        const T got = ema_update<T>(e, p, omd);
        if (sizeof(T) == 4) {
          // float: omd * diff has <= 48 significant bits and the sum fits the 64-bit mantissa: want is rounded once
          EXPECT_TRUE(same_bits(got, want));
        } else {
          // double: the long-double fma rounds to 64 bits first; a second rounding can move the last bit
          const T lo = std::nextafter(want, -T(2)), hi = std::nextafter(want, T(2));
          EXPECT_TRUE(got >= lo && got <= hi);
        }
      }
    }
  }
}

CME_TEST(one_update_against_long_double_f32) { one_update<float>(success); }
CME_TEST(one_update_against_long_double_f64) { one_update<double>(success); }

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
