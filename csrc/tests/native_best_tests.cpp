// Host-side tests of the keep-best rule (csrc/mlp/best.h): scripted metric sequences through best_decide for both
// monitors -- the first evaluation, exact ties, improvements below / at / above min_delta, NaN first and later, n = 0,
// patience 0 / 2 / none, an improvement after the stop -- and the rank-order sum of the triples.  Built with ASan +
// UBSan under CME_SANITIZE=ON: the rows are allocations of exactly R triples, so a read past them is reported.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "mlp/best.h"
#include "tests/test_macros.h"

using namespace cme;

static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Step {
  double metric;
  bool improved;
  double best_index, bad, stopped;
};

static void run_script(bool* success, const BestRule& rule, const std::vector<Step>& script) {
  BestRecord rec = best_start();
  EXPECT_TRUE(rec.evals == 0.0 && rec.best_index == -1.0 && std::isnan(rec.best_metric) && rec.bad == 0.0 &&
              rec.stopped == 0.0 && rec.stop_index == -1.0 && std::isnan(rec.last_metric) && rec.spare == 0.0);
  double n = 0.0;
  for (const Step& s : script) {
    const bool got = best_decide(rec, rule, s.metric);
    n += 1.0;
    EXPECT_TRUE(got == s.improved);
    EXPECT_TRUE(rec.evals == n);
    EXPECT_TRUE(rec.best_index == s.best_index);
    EXPECT_TRUE(rec.bad == s.bad);
    EXPECT_TRUE(rec.stopped == s.stopped);
    EXPECT_TRUE(same_bits(rec.last_metric, s.metric) || (std::isnan(rec.last_metric) && std::isnan(s.metric)));
  }
}

CME_TEST(loss_sequence_ties_nan_and_patience_two) {
  // improve, worse, tie, improve, NaN, worse, worse (stop: three bad in a row with patience 2), improve (ignored)
  run_script(success, BestRule{kBestLoss, 0.0, 2},
             {{2.0, true, 0, 0, 0},
              {2.5, false, 0, 1, 0},
              {2.0, false, 0, 2, 0},
              {1.5, true, 3, 0, 0},
              {kNaN, false, 3, 1, 0},
              {1.75, false, 3, 2, 0},
              {1.5, false, 3, 3, 1},
              {0.5, false, 3, 3, 1}});
  BestRecord rec = best_start();
  const BestRule rule{kBestLoss, 0.0, 2};
  const double seq[] = {2.0, 2.5, 2.0, 1.5, kNaN, 1.75, 1.5, 0.5};
  for (double m : seq) best_decide(rec, rule, m);
  EXPECT_TRUE(rec.stop_index == 6.0 && rec.best_metric == 1.5 && rec.evals == 8.0 && rec.last_metric == 0.5);
}

CME_TEST(accuracy_sequence_and_min_delta) {
  // min_delta = 0.25 (exact in binary): +0.125 is too small, +0.25 exactly is not MORE than min_delta, +0.5 is
  run_script(success, BestRule{kBestAccuracy, 0.25, -1},
             {{0.25, true, 0, 0, 0},
              {0.375, false, 0, 1, 0},
              {0.5, false, 0, 2, 0},
              {0.75, true, 3, 0, 0},
              {0.75, false, 3, 1, 0},
              {0.125, false, 3, 2, 0}});
  run_script(success, BestRule{kBestLoss, 0.25, -1},
             {{1.0, true, 0, 0, 0}, {0.875, false, 0, 1, 0}, {0.75, false, 0, 2, 0}, {0.5, true, 3, 0, 0}});
}

CME_TEST(nan_first_then_a_number_and_patience_zero) {
  run_script(success, BestRule{kBestLoss, 0.0, -1},
             {{kNaN, false, -1, 1, 0}, {kNaN, false, -1, 2, 0}, {3.0, true, 2, 0, 0}});
  // patience 0: the first non-improving evaluation stops
  run_script(success, BestRule{kBestAccuracy, 0.0, 0},
             {{0.5, true, 0, 0, 0}, {0.75, true, 1, 0, 0}, {0.75, false, 1, 1, 1}, {1.0, false, 1, 1, 1}});
  // ... a NaN before any best counts as a bad evaluation too
  run_script(success, BestRule{kBestLoss, 0.0, 0}, {{kNaN, false, -1, 1, 1}, {1.0, false, -1, 1, 1}});
  // no patience: never stops
  std::vector<Step> many = {{1.0, true, 0, 0, 0}};
  for (int i = 1; i <= 40; ++i) many.push_back({2.0, false, 0, double(i), 0});
  run_script(success, BestRule{kBestLoss, 0.0, -1}, many);
}

CME_TEST(metric_sums_the_triples_in_rank_order) {
  // three ranks whose loss sums do not add associatively: (a + b) + c != a + (b + c)
  std::vector<double> rows = {3.0, 1.0, 1e16, 2.0, 2.0, 1.0, 1.0, 0.0, 1.0};  // exactly R = 3 triples
  const double loss = best_metric_of(rows.data(), 3, kBestLoss);
  const double want = ((0.0 + 1e16) + 1.0 + 1.0) / 6.0;
  EXPECT_TRUE(same_bits(loss, want));
  EXPECT_TRUE(!same_bits(loss, (1e16 + (1.0 + 1.0)) / 6.0));
  EXPECT_TRUE(same_bits(best_metric_of(rows.data(), 3, kBestAccuracy), 3.0 / 6.0));
  EXPECT_TRUE(same_bits(best_metric_of(rows.data(), 1, kBestAccuracy), 1.0 / 3.0));
  // n = 0: a NaN metric, the one quiet NaN of best_start, which never improves
  std::vector<double> empty = {0.0, 0.0, 0.0};
  const double m = best_metric_of(empty.data(), 1, kBestLoss);
  EXPECT_TRUE(std::isnan(m) && same_bits(m, best_start().best_metric));
  BestRecord rec = best_start();
  EXPECT_TRUE(!best_decide(rec, BestRule{kBestLoss, 0.0, -1}, m) && rec.best_index == -1.0 && rec.bad == 1.0);
  double raw[kBestRecWords];
  best_store(raw, rec);
  const BestRecord back = best_load(raw);
  EXPECT_TRUE(back.evals == 1.0 && back.bad == 1.0 && std::isnan(back.last_metric));
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
