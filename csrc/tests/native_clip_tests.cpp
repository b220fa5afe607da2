// Host-side tests of gradient-norm clipping (csrc/mlp/clip.h), the schedule window (csrc/mlp/optim.h) and the fp64
// oracle trainer's rate table and clip threshold: the header's summation order against a plain sum at sizes around the
// group, wave, workgroup and grid boundaries, segments with padding the sum must never read, the clamped window lookup,
// and one-epoch-at-a-time training continuing the rates.  Built with ASan + UBSan under CME_SANITIZE=ON: every segment is
// an allocation of its own size, so a read past a segment's end is reported.
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "cpu/mlp_cpu.h"
#include "mlp/clip.h"
#include "mlp/optim.h"
#include "tests/test_macros.h"

using namespace cme;

template <typename T>
static void sumsq_cases(bool* success) {
  const int64_t counts[] = {1, 3, 63, 64, 255, 257, 1025, 4096, 4097, int64_t(kClipThreads) * 4 * kClipMaxGrid + 5};
  for (int64_t n : counts) {
    std::vector<T> g(n);  // exactly n elements: ASan sees any read past the segment
    double ref = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      g[i] = static_cast<T>(((i * 37) % 19 - 9) / 8.0);
      ref += static_cast<double>(g[i]) * static_cast<double>(g[i]);
    }
    ClipSegs s;
    s.n = 1;
    s.size[0] = n;
    std::vector<double> part(clip_grid(n));
    const double total = clip_host_sumsq(g.data(), s, part.data());
    EXPECT_TRUE(clip_grid(n) >= 1 && clip_grid(n) <= kClipMaxGrid);
    EXPECT_NEAR(total, ref, (n + 2) * std::ldexp(1.0, -53) * ref);
    double again = 0.0;
    for (double p : part) again += p;
    EXPECT_NEAR(again, total, 64 * std::ldexp(1.0, -53) * total);
  }
}

CME_TEST(sumsq_order_matches_a_plain_sum) {
  sumsq_cases<float>(success);
  sumsq_cases<double>(success);
  EXPECT_TRUE(clip_grid(0) == 1 && clip_grid(1) == 1 && clip_grid(int64_t(1) << 40) == kClipMaxGrid);
}

// padding between the segments and the status element behind them hold NaN: none of it may enter the norm
CME_TEST(sumsq_reads_the_segments_only) {
  const int64_t sizes[4] = {179, 7, 67, 3};
  std::vector<double> g;
  ClipSegs s;
  s.n = 4;
  double ref = 0.0;
  for (int q = 0; q < 4; ++q) {
    s.off[q] = static_cast<int64_t>(g.size());
    s.size[q] = sizes[q];
    for (int64_t i = 0; i < sizes[q]; ++i) {
      g.push_back(0.25 * ((i + q) % 7) - 0.5);
      ref += g.back() * g.back();
    }
    while (g.size() % 64) g.push_back(std::numeric_limits<double>::quiet_NaN());
  }
  g.push_back(std::numeric_limits<double>::quiet_NaN());  // the status element
  EXPECT_TRUE(s.count() == 256);
  double part[kClipMaxGrid];
  const double total = clip_host_sumsq(g.data(), s, part);
  EXPECT_NEAR(total, ref, 258 * std::ldexp(1.0, -53) * ref);
  // empty segments contribute nothing
  ClipSegs e = s;
  e.size[1] = e.size[3] = 0;
  EXPECT_TRUE(std::isfinite(clip_host_sumsq(g.data(), e, part)));
}

CME_TEST(clip_coefficient_follows_torch) {
  const ClipCoef below = clip_coef(4.0, 1.0);  // norm 2
  EXPECT_TRUE(below.clipped == 1);
  EXPECT_NEAR(below.coef, 1.0 / (2.0 + 1e-6), 1e-15);
  const ClipCoef above = clip_coef(4.0, 3.0);
  EXPECT_TRUE(above.clipped == 0 && above.coef > 1.0);
  const ClipCoef nan = clip_coef(std::numeric_limits<double>::quiet_NaN(), 1.0);
  EXPECT_TRUE(nan.clipped == 1 && std::isnan(nan.coef));  // a NaN norm poisons the gradient, as torch's default
  const ClipCoef inf = clip_coef(std::numeric_limits<double>::infinity(), 1.0);
  EXPECT_TRUE(inf.clipped == 1 && inf.coef == 0.0);
  EXPECT_TRUE(clip_scale(3.0f, static_cast<float>(below.coef)) == 3.0f * static_cast<float>(below.coef));
}

CME_TEST(window_lookup_clamps_at_both_ends) {
  const double w[] = {3.0, 4.0, 0.1, 0.2, 0.3, 0.4, 9.0};  // t0 = 3, n = 4; the 9 lies beyond n
  EXPECT_TRUE(window_index(0, 3, 4, 5) == 0 && window_index(3, 3, 4, 5) == 0 && window_index(5, 3, 4, 5) == 2);
  EXPECT_TRUE(window_index(6, 3, 4, 5) == 3 && window_index(1e15, 3, 4, 5) == 3);
  // whatever the buffer holds, no index leaves the capacity: n beyond it, zero, negative, NaN
  EXPECT_TRUE(window_index(100, 0, 1e9, 5) == 4 && window_index(100, 0, 0, 5) == 0 && window_index(100, 0, -3, 5) == 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT_TRUE(window_index(100, 0, nan, 5) == 0 && window_index(nan, 0, 4, 5) == 0 && window_index(7, nan, 4, 5) == 0);
  EXPECT_TRUE(window_rate(0.5, w, 5, 4.0) == 0.5 * 0.2 && window_rate(0.5, w, 5, 99.0) == 0.5 * 0.4);
}

// the fp64 oracle with a rate table and a clip threshold: 2 epochs at once == one epoch at a time with the counter
// carried and the table's halves; plain SGD runs the kSgd rule and logs every update
CME_TEST(oracle_train_takes_a_rate_table_and_a_clip_threshold) {
  const int P = 6, H = 5, C = 3, N = 10, total = H * P + H + C * H + C;
  std::vector<double> X(N * P);
  std::vector<int> y(N);
  for (int i = 0; i < N * P; ++i) X[i] = ((i * 37) % 11) / 10.0;
  for (int i = 0; i < N; ++i) y[i] = i % C;
  const std::vector<double> rates = {0.01, 0.03, 0.05, 0.05, 0.025, 0.0125};  // 2 epochs x 3 batches
  for (int kind : {-1, int(kMomentum), int(kAdam)}) {
    std::vector<std::vector<double>> prm[2];
    std::vector<double> logs[2];
    for (int split = 0; split < 2; ++split) {
      std::vector<double> W1(H * P), b1(H), W2(C * H), b2(C), s1(total, 0.0), s2(total, 0.0);
      cpu::NetView net{P, H, C, W1.data(), b1.data(), W2.data(), b2.data()};
      cpu::init_params(net);
      OptimCounter ctr;
      cpu::TrainOpts o;
      o.lr = 0.05;
      o.batch = 4;
      o.optim_kind = kind;
      if (kind >= 0) {
        o.s1 = s1.data();
        o.s2 = s2.data();
      }
      o.counter = &ctr;
      o.clip_norm = 0.02;
      o.update_log = &logs[split];
      o.epochs = split ? 1 : 2;
      for (int rep = 0; rep < (split ? 2 : 1); ++rep) {
        o.rates = rates.data() + (split ? 3 * rep : 0);
        o.nrates = split ? 3 : 6;
        cpu::train(net, X.data(), y.data(), N, o);
      }
      EXPECT_TRUE(ctr.t == 6);
      prm[split] = {W1, b1, W2, b2, s1};
    }
    for (size_t i = 0; i < prm[0].size(); ++i) EXPECT_VECTOR_EQ(prm[0][i], prm[1][i]);
    EXPECT_VECTOR_EQ(logs[0], logs[1]);
    EXPECT_TRUE(logs[0].size() == 24);
    bool clipped = false;
    for (int u = 0; u < 6; ++u) {
      EXPECT_TRUE(logs[0][4 * u] == u && logs[0][4 * u + 1] == rates[u] && logs[0][4 * u + 2] > 0.0);
      clipped = clipped || logs[0][4 * u + 3] < 1.0;
    }
    EXPECT_TRUE(clipped);
  }
  std::vector<double> W1(H * P), b1(H), W2(C * H), b2(C);
  cpu::NetView net{P, H, C, W1.data(), b1.data(), W2.data(), b2.data()};
  for (int bad_case = 0; bad_case < 2; ++bad_case) {
    cpu::TrainOpts bad;
    OptimCounter ctr;
    bad.batch = 4;
    bad.rates = rates.data();
    bad.nrates = 2;  // too short a table
    if (bad_case == 0) bad.counter = &ctr;
    else bad.nrates = 6;  // ... or no counter
    bool threw = false;
    try {
      cpu::train(net, X.data(), y.data(), N, bad);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    EXPECT_TRUE(threw);
  }
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
