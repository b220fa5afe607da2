// Host-side tests of the reduce-on-plateau rule (csrc/mlp/plateau.h): scripted metric sequences through plateau_decide,
// each hitting a named branch -- the first evaluation NaN, a tie, the reduction at bad = patience + 1 and not at
// patience, a cooldown swallowing bad evaluations, the clamp at min_factor, a reduction ignored under eps (reductions
// unchanged, cooldown restarted) -- the record's start values and plateau_rate(x, 1.0) == x.  Built with ASan + UBSan
// under CME_SANITIZE=ON.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "mlp/plateau.h"
#include "tests/test_macros.h"

using namespace cme;

static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static PlateauRule rule_of(int monitor, double factor, int patience, double threshold, int mode, int cooldown,
                           double min_factor, double eps) {
  PlateauRule r;
  r.monitor = monitor; r.factor = factor; r.patience = patience; r.threshold = threshold; r.threshold_mode = mode;
  r.cooldown = cooldown; r.min_factor = min_factor; r.eps = eps;
  return r;
}

struct Step {
  double metric;
  bool reduced;
  double best, bad, cooldown_left, scale, reductions;
};

static void run_script(bool* success, const PlateauRule& rule, const std::vector<Step>& script) {
  EXPECT_TRUE(plateau_rule_ok(rule));
  PlateauRecord rec = plateau_start(rule.monitor);
  double n = 0.0, last_reduced = -1.0;
  for (const Step& s : script) {
    const bool got = plateau_decide(rec, rule, s.metric);
    if (got) last_reduced = n;
    n += 1.0;
    EXPECT_TRUE(got == s.reduced);
    EXPECT_TRUE(rec.evals == n);
    EXPECT_TRUE(same_bits(rec.best, s.best));
    EXPECT_TRUE(rec.bad == s.bad);
    EXPECT_TRUE(rec.cooldown_left == s.cooldown_left);
    EXPECT_TRUE(same_bits(rec.scale, s.scale));
    EXPECT_TRUE(rec.reductions == s.reductions);
    EXPECT_TRUE(rec.last_reduced_index == last_reduced);
    EXPECT_TRUE(same_bits(rec.last_metric, s.metric) || (std::isnan(rec.last_metric) && std::isnan(s.metric)));
  }
}

CME_TEST(start_values_and_the_rate) {
  const PlateauRecord lo = plateau_start(kBestLoss), hi = plateau_start(kBestAccuracy);
  EXPECT_TRUE(lo.evals == 0.0 && lo.best == kInf && lo.bad == 0.0 && lo.cooldown_left == 0.0 && lo.scale == 1.0 &&
              lo.reductions == 0.0 && std::isnan(lo.last_metric) && lo.last_reduced_index == -1.0);
  EXPECT_TRUE(hi.best == -kInf && hi.scale == 1.0 && hi.last_reduced_index == -1.0);
  EXPECT_TRUE(same_bits(lo.last_metric, __builtin_nan("")));
  double raw[kPlateauRecWords];
  plateau_store(raw, lo);
  EXPECT_TRUE(raw[kPlateauScaleWord] == 1.0);
  const PlateauRecord back = plateau_load(raw);
  EXPECT_TRUE(back.best == kInf && back.scale == 1.0 && std::isnan(back.last_metric));
  const double xs[] = {0.0, 1.0, 0.1, 1e-300, 4.9e-324, 3.0e38, 1.7976931348623157e308, -0.0, 0.001 * 0.37};
  for (double x : xs) EXPECT_TRUE(same_bits(plateau_rate(x, 1.0), x));
  EXPECT_TRUE(same_bits(plateau_rate(0.1 * 0.3, 0.1), (0.1 * 0.3) * 0.1));
  // the ranges the launcher checks
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 1.0, 0, 0.0, kPlateauRel, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.0, 0, 0.0, kPlateauRel, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, -1, 0.0, kPlateauRel, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, 0, -1.0, kPlateauRel, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, 0, 0.0, 2, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauRel, -1, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauRel, 0, 1.5, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauRel, 0, 0.0, -1.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(2, 0.5, 0, 0.0, kPlateauRel, 0, 0.0, 0.0)));
  EXPECT_TRUE(!plateau_rule_ok(rule_of(kBestLoss, kNaN, 0, 0.0, kPlateauRel, 0, 0.0, 0.0)));
}

CME_TEST(first_evaluation_nan_and_a_tie) {
  // patience 1, abs threshold 0: NaN first is a bad evaluation with best still +inf; the second bad one reduces
  run_script(success, rule_of(kBestLoss, 0.5, 1, 0.0, kPlateauAbs, 0, 0.0, 0.0),
             {{kNaN, false, kInf, 1, 0, 1.0, 0},
              {kNaN, true, kInf, 0, 0, 0.5, 1},
              {2.0, false, 2.0, 0, 0, 0.5, 1},
              {2.0, false, 2.0, 1, 0, 0.5, 1},   // a tie is not better (strict)
              {2.0, true, 2.0, 0, 0, 0.25, 2},   // ... and neither is the next one: reduced
              {1.0, false, 1.0, 0, 0, 0.25, 2}});
  // mode max: a tie and a NaN are bad, rel threshold 0.25: 0.5 -> needs > 0.625
  run_script(success, rule_of(kBestAccuracy, 0.5, 1, 0.25, kPlateauRel, 0, 0.0, 0.0),
             {{0.5, false, 0.5, 0, 0, 1.0, 0},
              {0.625, false, 0.5, 1, 0, 1.0, 0},  // exactly best * 1.25: not MORE
              {kNaN, true, 0.5, 0, 0, 0.5, 1},
              {0.75, false, 0.75, 0, 0, 0.5, 1}});
}

CME_TEST(reduction_at_patience_plus_one_and_not_at_patience) {
  // patience 2: bad evaluations 1 and 2 are tolerated, number 3 reduces
  run_script(success, rule_of(kBestLoss, 0.1, 2, 0.0, kPlateauAbs, 0, 0.0, 1e-8),
             {{2.0, false, 2.0, 0, 0, 1.0, 0},
              {2.5, false, 2.0, 1, 0, 1.0, 0},
              {2.5, false, 2.0, 2, 0, 1.0, 0},
              {2.5, true, 2.0, 0, 0, 0.1, 1},
              {2.5, false, 2.0, 1, 0, 0.1, 1},
              {2.5, false, 2.0, 2, 0, 0.1, 1},
              {2.5, true, 2.0, 0, 0, 0.1 * 0.1, 2}});
  // patience 0: the first bad evaluation reduces; min, rel threshold 0.5: "not halved" is bad
  run_script(success, rule_of(kBestLoss, 0.5, 0, 0.5, kPlateauRel, 0, 0.0, 0.0),
             {{4.0, false, 4.0, 0, 0, 1.0, 0},
              {2.0, true, 4.0, 0, 0, 0.5, 1},    // exactly half: not LESS than best * 0.5
              {1.5, false, 1.5, 0, 0, 0.5, 1},
              {1.0, true, 1.5, 0, 0, 0.25, 2}});
}

CME_TEST(cooldown_swallows_bad_evaluations) {
  // patience 0, cooldown 2: after a reduction the next two bad evaluations are not counted
  run_script(success, rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauAbs, 2, 0.0, 0.0),
             {{2.0, false, 2.0, 0, 0, 1.0, 0},
              {3.0, true, 2.0, 0, 2, 0.5, 1},
              {3.0, false, 2.0, 0, 1, 0.5, 1},
              {3.0, false, 2.0, 0, 0, 0.5, 1},
              {3.0, true, 2.0, 0, 2, 0.25, 2},
              {1.0, false, 1.0, 0, 1, 0.25, 2},  // an improvement inside the cooldown still becomes the best
              {3.0, false, 1.0, 0, 0, 0.25, 2},
              {3.0, true, 1.0, 0, 2, 0.125, 3}});
}

CME_TEST(clamp_at_min_factor_and_a_reduction_ignored_under_eps) {
  // factor 0.5, min_factor 0.2: 1 -> 0.5 -> 0.25 -> 0.2 (clamped) -> 0.2 (scale - new = 0: not > eps)
  run_script(success, rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauAbs, 1, 0.2, 1e-8),
             {{2.0, false, 2.0, 0, 0, 1.0, 0},
              {3.0, true, 2.0, 0, 1, 0.5, 1},
              {3.0, false, 2.0, 0, 0, 0.5, 1},
              {3.0, true, 2.0, 0, 1, 0.25, 2},
              {3.0, false, 2.0, 0, 0, 0.25, 2},
              {3.0, true, 2.0, 0, 1, 0.2, 3},    // max(0.125, 0.2)
              {3.0, false, 2.0, 0, 0, 0.2, 3},
              {3.0, false, 2.0, 0, 1, 0.2, 3},   // ignored: reductions unchanged, but the cooldown restarted
              {3.0, false, 2.0, 0, 0, 0.2, 3}});
  // eps larger than the step: 1 -> 0.5 is a change of 0.5 <= eps 0.5 (not MORE): ignored from the start
  run_script(success, rule_of(kBestLoss, 0.5, 0, 0.0, kPlateauAbs, 3, 0.0, 0.5),
             {{2.0, false, 2.0, 0, 0, 1.0, 0},
              {3.0, false, 2.0, 0, 3, 1.0, 0},
              {3.0, false, 2.0, 0, 2, 1.0, 0}});
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
