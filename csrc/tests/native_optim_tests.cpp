// Host-side tests of the update rules (csrc/mlp/optim.h) and of the fp64 oracle trainer that uses them: the header's
// functions over the edge inputs of the kernel tests (zeros, a denormal gradient, Adam with s = 0 and g = 0), the
// counter's running products, and one-epoch-at-a-time training continuing the state.  Built with ASan + UBSan under
// CME_SANITIZE=ON.
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "cpu/mlp_cpu.h"
#include "mlp/optim.h"
#include "tests/test_macros.h"

using namespace cme;

template <typename T>
static bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

template <typename T>
static void momentum_cases(bool* success) {
  OptimHyper h;
  h.lr = 0.1;
  h.mu = 0.5;
  for (int nest = 0; nest < 2; ++nest) {
    h.nesterov = nest;
    const auto k = momentum_coef<T>(h);
    T p = T(1), v = T(0);
    momentum_update(p, v, T(2), k);  // v0 = 0: v = g, d = g (+ mu g)
    EXPECT_TRUE(same_bits(v, T(2)));
    EXPECT_NEAR(p, 1.0 - 0.1 * (nest ? 3.0 : 2.0), 1e-6);
    momentum_update(p, v, T(0), k);  // zero gradient: the velocity decays, the parameter still moves
    EXPECT_TRUE(same_bits(v, T(1)));
    T q = T(0), w = T(0);
    momentum_update(q, w, T(0), k);  // all zeros stay zeros
    EXPECT_TRUE(same_bits(q, T(0)) && same_bits(w, T(0)));
    const T den = std::numeric_limits<T>::denorm_min() * T(8);
    T r = T(0), u = T(0);
    momentum_update(r, u, den, k);  // a denormal gradient is kept in the state, not flushed
    EXPECT_TRUE(same_bits(u, den));
  }
}

template <typename T>
static void adam_cases(bool* success) {
  OptimHyper h;
  h.lr = 0.1;
  OptimCounter c;
  const T den = std::numeric_limits<T>::denorm_min() * T(8);
  T p[4] = {T(1.5), T(-0.0), T(0), T(3)}, m[4] = {}, s[4] = {};
  const T g[4] = {T(0), T(0), T(0), den};
  const T p0[4] = {p[0], p[1], p[2], p[3]};
  for (int t = 1; t <= 5; ++t) {
    optim_advance(c, h);
    const auto k = adam_coef<T>(h, c);
    EXPECT_TRUE(k.bc2s > T(0) && k.nstep < T(0));
    for (int i = 0; i < 4; ++i) adam_update(p[i], m[i], s[i], g[i], k);
  }
  for (int i = 0; i < 3; ++i)  // s = 0 and g = 0: the update is exactly 0, signed zeros included
    EXPECT_TRUE(same_bits(p[i], p0[i]) && same_bits(m[i], T(0)) && same_bits(s[i], T(0)));
  EXPECT_TRUE(m[3] > T(0) && std::isfinite(static_cast<double>(p[3])));
  // the first update of a fresh state moves by lr * sign(g) (up to eps): m / sqrt(s) = (1 - b1) / sqrt(1 - b2) bias-corrected
  OptimCounter c1;
  optim_advance(c1, h);
  T q = T(1), qm = T(0), qs = T(0);
  adam_update(q, qm, qs, T(-0.25), adam_coef<T>(h, c1));
  EXPECT_NEAR(q, 1.1, 1e-6);
}

CME_TEST(momentum_edge_inputs_f32) { momentum_cases<float>(success); }
CME_TEST(momentum_edge_inputs_f64) { momentum_cases<double>(success); }
CME_TEST(adam_edge_inputs_f32) { adam_cases<float>(success); }
CME_TEST(adam_edge_inputs_f64) { adam_cases<double>(success); }

CME_TEST(counter_keeps_running_products) {
  OptimHyper h;
  OptimCounter c;
  double b1 = 1.0, b2 = 1.0;
  for (int t = 1; t <= 100; ++t) {
    optim_advance(c, h);
    b1 *= h.beta1;
    b2 *= h.beta2;
    EXPECT_TRUE(c.t == t && same_bits(c.b1p, b1) && same_bits(c.b2p, b2));
  }
  EXPECT_NEAR(c.b1p, std::pow(0.9, 100), 1e-18);
}

// the fp64 oracle: 2 epochs at once == one epoch at a time with the state carried; without an optimizer nothing changes
CME_TEST(oracle_train_continues_its_state) {
  const int P = 6, H = 5, C = 3, N = 10, total = H * P + H + C * H + C;
  std::vector<double> X(N * P);
  std::vector<int> y(N);
  for (int i = 0; i < N * P; ++i) X[i] = ((i * 37) % 11) / 10.0;
  for (int i = 0; i < N; ++i) y[i] = i % C;
  for (int kind = kMomentum; kind <= kAdam; ++kind) {
    std::vector<std::vector<double>> prm[2];
    for (int split = 0; split < 2; ++split) {
      std::vector<double> W1(H * P), b1(H), W2(C * H), b2(C), s1(total, 0.0), s2(total, 0.0);
      cpu::NetView net{P, H, C, W1.data(), b1.data(), W2.data(), b2.data()};
      cpu::init_params(net);
      OptimCounter ctr;
      cpu::TrainOpts o;
      o.lr = 0.05;
      o.batch = 4;
      o.optim_kind = kind;
      o.s1 = s1.data();
      o.s2 = s2.data();
      o.counter = &ctr;
      o.epochs = split ? 1 : 2;
      for (int rep = 0; rep < (split ? 2 : 1); ++rep) cpu::train(net, X.data(), y.data(), N, o);
      EXPECT_TRUE(ctr.t == 6);
      prm[split] = {W1, b1, W2, b2, s1};
    }
    for (size_t i = 0; i < prm[0].size(); ++i) EXPECT_VECTOR_EQ(prm[0][i], prm[1][i]);
  }
  cpu::TrainOpts bad;
  bad.optim_kind = kAdam;  // no state buffers
  std::vector<double> W1(H * P), b1(H), W2(C * H), b2(C);
  cpu::NetView net{P, H, C, W1.data(), b1.data(), W2.data(), b2.data()};
  bool threw = false;
  try {
    cpu::train(net, X.data(), y.data(), N, bad);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

int main(int argc, char** argv) { return cme::test::run_all(argc > 1 ? argv[1] : nullptr); }
