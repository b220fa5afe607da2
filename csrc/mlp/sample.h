// Sampling the resident training set with replacement (balanced / weighted): the keyed draw that the four per-epoch
// gathers (shuffle.hip, augment.hip, affine.hip, warp.hip) take a destination sample's source row from instead of the
// keyed permutation (shuffle.h), and the alias table behind it.  One header for hipcc and g++: the gathers compile
// sample_draw, the host (bindings_cpu.cpp `alias_table` / `epoch_draws`) builds the table once and forms the same draws
// from this same text.  The draw path is 32- and 64-bit integer arithmetic only: no `%`, no floating point, no state.
//
//   * key: sample_key(seed, iter) = shuffle_mix64(shuffle_key(seed, iter) ^ kSampleStream), `iter` the trainer's
//     iteration counter at the start of the epoch, exactly as for the shuffle and the augmentation.  The fixed
//     constant (and the mixing) makes it a stream distinct from shuffle_key and augment_key for the same arguments.
//   * table: for weights w[0 .. N) (Walker / Vose) uint32 [N][2] = {threshold, alias}.  Column j yields row j with
//     probability threshold[j] / 2^32 and row alias[j] otherwise.  A column that always yields itself is stored as
//     alias == j (its threshold, 2^32, does not fit; 0xffffffff is written and never decides anything).  A zero-weight
//     row has threshold 0 and is nobody's alias: it is never drawn.
//   * draw: sample_draw(d, N, key, table): one 64-bit hash per destination d -- splitmix64's output at position d + 1
//     of the sequence seeded with the key, as augment_shift forms its hash -- the column j = (uint64(low32) * N) >> 32
//     and then high32 < threshold[j] ? j : alias[j].  The two halves of one splitmix64 output are the two variates.
//
// The build (sample_alias_table; host only, fp64, nothing but + - * / and floor, so no math library and no
// contraction is involved: a pure function of the weights).  Its order is part of the format:
//   1. S = the compensated (Kahan) sum of w[0], w[1], ... in index order; q[i] = (w[i] / S) * N.
//   2. Two work lists.  `small`, a FIFO queue, receives the rows with q[i] < 1: first every zero-weight row in
//      ascending index order, then the others in ascending index order.  `large`, a LIFO stack, receives the rows
//      with q[i] >= 1 in ascending index order (the highest index is on top).
//   3. While both hold a row: l = the queue's front (popped), g = the stack's top (left in place).
//      threshold[l] = min(floor(q[l] * 2^32 + 0.5), 2^32 - 1), alias[l] = g, q[g] = (q[g] + q[l]) - 1.  If now
//      q[g] < 1, g is popped and appended to the queue's back.
//   4. Every row left in either list always yields itself: alias = own index.
// A zero-weight row is paired before any other (2.), while a large row must still exist; should rounding ever leave one
// without a partner the build refuses rather than let it be drawn.
//
// Error bound.  Let U = 2^32, u = 2^-53, q*[i] = N w[i] / sum(w), and p[i] the probability the integer table implies
// for row i in units of 2^-32 / N:  p[i] = T[i] + sum over the columns j that alias to i of (U - T[j]),  T = the
// threshold, U for a column that always yields itself.  sum(p) = N U exactly, whatever the thresholds.  Write A(i) for
// the columns that alias to i and a[i] for their number.
//   * q[i] as first computed differs from q*[i] by at most q*[i] e0, e0 = 6 u: the compensated sum of non-negative
//     terms is within (2 u + O(N u^2)) of the exact one, N u^2 < 2^-75 for N < 2^31, and the division and the product
//     (N is exact in fp64) add one rounding each; 6 u covers them and the second-order terms.
//   * each of the a[i] updates of q[i] rounds twice, each time a value of magnitude at most q[i] + 1 with q[i] never
//     above its first value: the residue r[i] that row i ends with is  q[i] - sum over A(i) of (1 - r[j]) + e[i],
//     |e[i]| <= E[i] = 2 a[i] u (q*[i] (1 + e0) + 1).
//   * T[j] = U r[j] - f[j] with |f[j]| <= 1/2 (U r[j] is exact; round to nearest), except that a threshold that would
//     round to U is stored as U - 1: then f[j] < 1.  Write c[i] for the number of such columns among i and A(i).
//   * a row of step 4 is stored as T = U although its residue r is 1 only up to the rounding gathered on the way.  At
//     the end one list is empty, so these residues are all >= 1 or all < 1, and their deviations from 1 sum to
//     sum(q as first computed) - N + sum(e): each is at most D = N e0 + sum over all k of E[k] in magnitude.
//   Substituting:  p[i] - U q*[i] = U q*[i] d[i] + U e[i] + sum over A(i) of f[j] - f[i] (rows of step 3)
//                                                                                  + U (1 - r[i]) (rows of step 4), so
//     | p[i] - U q*[i] |  <=  (a[i] + 1 + c[i]) / 2  +  U (q*[i] e0 + E[i])  +  [alias[i] == i] U D       (units).
//   The first term is the integer rounding, one half per column that contributes to row i; the second the fp64
//   rounding along the row's own chain; the third, for rows that end as "always itself" only, the rounding of the whole
//   build, which lands on them.  At N = 60 000 with q* <= 4 000 and a <= 4 100 the terms are about 2 050, 15 and 25
//   units; the measured worst case (tests/test_sampling.py, profiles/sampler/table_error.jsonl) is 16 units, at a
//   row with 603 aliasing columns under log-normal weights at N = 60 000, since the f[j] cancel like a random walk.  In
//   probability a unit is 2^-32 / N.
//
// Refused with std::invalid_argument: N == 0 or N >= 2^31, a negative, NaN or infinite weight, a sum that is zero or
// overflows.
#pragma once

#include <cstdint>

#include "shuffle.h"

#ifndef __HIP_DEVICE_COMPILE__
#include <stdexcept>
#include <vector>
#endif

namespace cme {

constexpr uint64_t kSampleStream = 0x3c6ef372fe94f82bull;  // (any fixed non-zero constant; part of the format)

__host__ __device__ inline uint64_t sample_key(uint32_t seed, uint32_t iter) {
  return shuffle_mix64(shuffle_key(seed, iter) ^ kSampleStream);
}

// table: uint32 [n][2] = {threshold, alias}, 8-byte aligned; d < n; every alias < n (sample_alias_table's are)
__host__ __device__ inline uint32_t sample_draw(uint32_t d, uint32_t n, uint64_t key, const uint32_t* table) {
  const uint64_t h = shuffle_mix64(key + (static_cast<uint64_t>(d) + 1u) * 0x9e3779b97f4a7c15ull);
  const uint32_t j = static_cast<uint32_t>((static_cast<uint64_t>(static_cast<uint32_t>(h)) * n) >> 32);
  uint64_t e;  // the pair in one 8-byte load (little-endian)
  __builtin_memcpy(&e, __builtin_assume_aligned(table + 2 * static_cast<uint64_t>(j), 8), 8);
  const uint32_t threshold = static_cast<uint32_t>(e), alias = static_cast<uint32_t>(e >> 32);
  return static_cast<uint32_t>(h >> 32) < threshold ? j : alias;
}

#ifndef __HIP_DEVICE_COMPILE__
// out: uint32 [n][2].  The order of the build is the one documented above.
inline void sample_alias_table(const double* w, int64_t n, uint32_t* out) {
  if (n < 1 || n >= (int64_t{1} << 31)) throw std::invalid_argument("alias_table: N must be in [1, 2^31)");
  double sum = 0.0, comp = 0.0;  // Kahan
  for (int64_t i = 0; i < n; ++i) {
    const double x = w[i];
    if (!(x >= 0.0) || x - x != 0.0)  // (NaN fails the first test, an infinity the second)
      throw std::invalid_argument("alias_table: the weights must be finite and >= 0");
    const double y = x - comp;
    const double t = sum + y;
    comp = (t - sum) - y;
    sum = t;
  }
  if (!(sum > 0.0)) throw std::invalid_argument("alias_table: the weights must not all be zero");
  if (sum - sum != 0.0) throw std::invalid_argument("alias_table: the sum of the weights overflows");
  const double nd = static_cast<double>(n), two32 = 4294967296.0;
  std::vector<double> q(static_cast<size_t>(n));
  std::vector<uint32_t> small, large;
  small.reserve(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    q[i] = (w[i] / sum) * nd;
    if (w[i] == 0.0) small.push_back(static_cast<uint32_t>(i));
  }
  for (int64_t i = 0; i < n; ++i) {
    if (w[i] == 0.0) continue;
    (q[i] < 1.0 ? small : large).push_back(static_cast<uint32_t>(i));
  }
  size_t head = 0;
  while (head < small.size() && !large.empty()) {
    const uint32_t l = small[head++], g = large.back();
    const uint64_t t = static_cast<uint64_t>(q[l] * two32 + 0.5);  // the floor of a non-negative value below 2^33
    out[2 * static_cast<size_t>(l)] = t > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(t);
    out[2 * static_cast<size_t>(l) + 1] = g;
    q[g] = (q[g] + q[l]) - 1.0;
    if (q[g] < 1.0) {
      large.pop_back();
      small.push_back(g);
    }
  }
  for (; head < small.size(); ++head) {
    const uint32_t l = small[head];
    if (w[l] == 0.0) throw std::invalid_argument("alias_table: rounding left a zero-weight row without a partner");
    out[2 * static_cast<size_t>(l)] = 0xffffffffu;
    out[2 * static_cast<size_t>(l) + 1] = l;
  }
  for (const uint32_t g : large) {
    out[2 * static_cast<size_t>(g)] = 0xffffffffu;
    out[2 * static_cast<size_t>(g) + 1] = g;
  }
}
#endif

}  // namespace cme
