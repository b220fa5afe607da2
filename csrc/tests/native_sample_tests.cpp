// Host-side tests of the sampling rule (csrc/mlp/sample.h): the alias table's structure and the exact sum of the
// probabilities it implies, the rows it must never draw, its refusals, and the draw's range, determinism and separation
// from the shuffle's and the augmentation's streams.  Built with ASan + UBSan under CME_SANITIZE=ON: the tables are
// allocations of exactly 2 n words, so a column or an alias outside them is reported.
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <vector>

#include "mlp/augment.h"
#include "mlp/sample.h"
#include "tests/test_macros.h"

using namespace cme;

namespace {

std::vector<uint32_t> table_of(const std::vector<double>& w) {
  std::vector<uint32_t> t(2 * w.size());
  sample_alias_table(w.data(), static_cast<int64_t>(w.size()), t.data());
  return t;
}

// p[i] in units of 2^-32 / n, from the integer table alone
std::vector<uint64_t> implied(const std::vector<uint32_t>& t) {
  const size_t n = t.size() / 2;
  std::vector<uint64_t> p(n, 0);
  for (size_t j = 0; j < n; ++j) {
    const uint64_t thr = t[2 * j], al = t[2 * j + 1];
    if (al == j) {
      p[j] += uint64_t{1} << 32;
    } else {
      p[j] += thr;
      p[al] += (uint64_t{1} << 32) - thr;
    }
  }
  return p;
}

bool refuses(const std::vector<double>& w) {
  std::vector<uint32_t> t(2 * w.size() + 2);
  try {
    sample_alias_table(w.data(), static_cast<int64_t>(w.size()), t.data());
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

std::vector<double> skewed(size_t n) {  // every 7th weight zero, the rest u^8 of a keyed u
  std::vector<double> w(n);
  for (size_t i = 0; i < n; ++i) {
    const double u = static_cast<double>(shuffle_mix64(i + 1) >> 11) / 9007199254740992.0;
    const double u2 = u * u, u4 = u2 * u2;
    w[i] = i % 7 == 0 ? 0.0 : u4 * u4;
  }
  return w;
}

}  // namespace

CME_TEST(table_sums_exactly_and_never_draws_a_zero_weight_row) {
  for (size_t n : {size_t{2}, size_t{63}, size_t{1000}, size_t{60000}}) {
    const std::vector<double> w = skewed(n);
    const std::vector<uint32_t> t = table_of(w);
    const std::vector<uint64_t> p = implied(t);
    uint64_t sum = 0;
    std::vector<char> is_alias(n, 0);
    for (size_t j = 0; j < n; ++j) {
      EXPECT_TRUE(t[2 * j + 1] < n);
      if (t[2 * j + 1] != j) is_alias[t[2 * j + 1]] = 1;
      sum += p[j];
    }
    EXPECT_TRUE(sum == static_cast<uint64_t>(n) << 32);
    for (size_t j = 0; j < n; ++j)
      if (w[j] == 0.0) EXPECT_TRUE(p[j] == 0 && t[2 * j] == 0 && !is_alias[j] && t[2 * j + 1] != j);
    // ... and the draws stay in range and never land on such a row
    const uint64_t key = sample_key(3u, 17u);
    for (uint32_t d = 0; d < n; ++d) {
      const uint32_t s = sample_draw(d, static_cast<uint32_t>(n), key, t.data());
      EXPECT_TRUE(s < n && w[s] > 0.0);
      EXPECT_EQ(s, sample_draw(d, static_cast<uint32_t>(n), key, t.data()));
    }
  }
}

CME_TEST(uniform_and_single_weight_tables) {
  const std::vector<uint32_t> u = table_of(std::vector<double>(5, 0.25));
  for (uint32_t j = 0; j < 5; ++j) EXPECT_EQ(u[2 * j + 1], j);  // every column always yields itself
  std::vector<double> one(9, 0.0);
  one[4] = 3.0;
  const std::vector<uint32_t> t = table_of(one);
  for (uint32_t j = 0; j < 9; ++j) {
    EXPECT_EQ(t[2 * j + 1], 4u);
    if (j != 4) EXPECT_EQ(t[2 * j], 0u);
  }
  for (uint32_t d = 0; d < 9; ++d) EXPECT_EQ(sample_draw(d, 9u, sample_key(0u, 0u), t.data()), 4u);
  const std::vector<uint32_t> single = table_of({2.0});
  EXPECT_EQ(single[1], 0u);
  EXPECT_EQ(sample_draw(0u, 1u, sample_key(1u, 2u), single.data()), 0u);
  // the same weights give the same table: a pure function
  EXPECT_TRUE(table_of(skewed(1000)) == table_of(skewed(1000)));
}

CME_TEST(table_refuses_bad_weights) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT_TRUE(refuses({1.0, -1.0}));
  EXPECT_TRUE(refuses({1.0, nan}));
  EXPECT_TRUE(refuses({inf, 1.0}));
  EXPECT_TRUE(refuses({0.0, 0.0, 0.0}));
  EXPECT_TRUE(refuses({}));
  EXPECT_TRUE(refuses({1e308, 1e308}));  // the sum overflows
  EXPECT_TRUE(!refuses({0.0, 1e-300}));
  double w = 1.0;
  uint32_t out[2];
  bool threw = false;
  try {
    sample_alias_table(&w, int64_t{1} << 31, out);  // refused before anything is read
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

CME_TEST(key_is_a_stream_of_its_own) {
  for (uint32_t seed : {0u, 5u, 0xffffffffu})
    for (uint32_t iter : {0u, 75u, 0xffffffffu}) {
      const uint64_t key = sample_key(seed, iter);
      EXPECT_TRUE(key == sample_key(seed, iter));
      EXPECT_TRUE(key != shuffle_key(seed, iter) && key != augment_key(seed, iter));
      EXPECT_TRUE(key != sample_key(seed, iter + 1u) && key != sample_key(seed + 1u, iter));
    }
  const uint32_t n = 1000;
  const std::vector<uint32_t> t = table_of(std::vector<double>(n, 1.0));
  int vs_iter = 0, vs_aug = 0, vs_perm = 0;
  for (uint32_t d = 0; d < n; ++d) {
    const uint32_t s = sample_draw(d, n, sample_key(3u, 9u), t.data());
    vs_iter += s != sample_draw(d, n, sample_key(3u, 10u), t.data());
    vs_aug += s != sample_draw(d, n, augment_key(3u, 9u), t.data());
    vs_perm += s != shuffle_index(d, n, shuffle_key(3u, 9u));
  }
  EXPECT_TRUE(vs_iter > 900 && vs_aug > 900 && vs_perm > 900);
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
