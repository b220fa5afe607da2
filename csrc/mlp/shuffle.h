// The per-epoch shuffle of the resident training set (shuffle.hip) and its keyed permutation.
//
// shuffle_index(i, n, key): for every n >= 1 and every key, i -> shuffle_index(i, n, key) is a bijection of [0, n).
// Stateless (no sort, no scratch array): a gather kernel computes a sample's source row from its destination index
// alone, and the host (g++, bindings_cpu.cpp `epoch_permutation`) computes the same value from this same header --
// 32- and 64-bit integer arithmetic only.
//
//   * a balanced Feistel network over 2 k bits, k the smallest with 4^k >= n (k >= 1), kShuffleRounds rounds; the
//     round function is murmur3's 32-bit finaliser of (right half ^ round key), truncated to k bits; the round keys
//     are successive splitmix64 outputs seeded with `key` (one 32-bit half of an output per round);
//   * cycle walking: the network permutes [0, 4^k) and 4^k < 4 n, so it is applied again until the value is < n
//     (under 4 applications expected).  The walk always ends -- the cycle through i leads back to i < n -- and the
//     loop is bounded by the domain size all the same.
//
// The key of epoch e: shuffle_key(seed, iter) = (seed << 32) ^ iter, `iter` the trainer's iteration counter at the
// start of the epoch; both are taken as unsigned 32-bit values, so the packing is injective.  An epoch's order
// depends on (seed, iter) alone: a re-run epoch or a resumed run reproduces it.
#pragma once

#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cme {

constexpr int kShuffleRounds = 6;

__host__ __device__ inline uint64_t shuffle_key(uint32_t seed, uint32_t iter) {
  return (static_cast<uint64_t>(seed) << 32) ^ static_cast<uint64_t>(iter);
}

__host__ __device__ inline uint32_t shuffle_mix32(uint32_t x) {  // murmur3 fmix32
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

__host__ __device__ inline uint64_t shuffle_mix64(uint64_t z) {  // splitmix64's output function
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__host__ __device__ inline uint32_t shuffle_index(uint32_t i, uint32_t n, uint64_t key) {
  if (n <= 1) return 0;
  int k = 1;
  while (k < 16 && (uint64_t{1} << (2 * k)) < n) ++k;
  const uint32_t mask = (1u << k) - 1u;
  uint32_t rk[kShuffleRounds];
  uint64_t s = key;
  for (int r = 0; r < kShuffleRounds; r += 2) {
    s += 0x9e3779b97f4a7c15ull;
    const uint64_t z = shuffle_mix64(s);
    rk[r] = static_cast<uint32_t>(z);
    if (r + 1 < kShuffleRounds) rk[r + 1] = static_cast<uint32_t>(z >> 32);
  }
  const uint64_t domain = uint64_t{1} << (2 * k);
  uint32_t x = i;
  for (uint64_t t = 0; t < domain; ++t) {
    uint32_t l = x >> k, r = x & mask;
    for (int q = 0; q < kShuffleRounds; ++q) {
      const uint32_t f = shuffle_mix32(r ^ rk[q]) & mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << k) | r;
    if (x < n) break;
  }
  return x;
}

// One launch rewrites every resident layout of the training set so that sample i is source sample perm[i] =
// shuffle_index(i, N, key) (identity != 0: perm[i] = i), reading the pristine copies X0 / labels0 (distinct from
// every destination).  es = bytes per element of X0 / X / XT (1: the split paths' raw pixels; 2 / 4 / 8: the mfma
// path's bf16 / f32 / f64).  Null destinations are skipped.  XT is [P (+ 1)][N] (rows >= P are not touched); Xs the
// forward's fragment order (mma_tile.h xs_off; es == 1), its zero padding rewritten as zeros; Xw [N][P] and
// XTw [P (+ 1)][N] the bf16 copies of the wide engines (es == 1; the conversion of 0..255 is exact); perm int32 [N].
// `stream` is a hipStream_t.  No sync, no read-back.
// sample_table != null (sample.h: device uint32 [N][2], 8-byte aligned): perm[i] = sample_draw(i, N, sample_key,
// sample_table) instead -- a draw with replacement, so rows may repeat; identity != 0 still gives perm[i] = i.
struct ShuffleArgs {
  const void* X0 = nullptr;
  const int* labels0 = nullptr;
  void* X = nullptr;
  int* labels = nullptr;
  void* XT = nullptr;
  void* Xs = nullptr;
  void* Xw = nullptr;
  void* XTw = nullptr;
  int* perm = nullptr;
  int N = 0, P = 0, es = 1;
  uint64_t key = 0;
  int identity = 0;
  const uint32_t* sample_table = nullptr;
  uint64_t sample_key = 0;
};
void mlp_shuffle(const ShuffleArgs& a, void* stream);

}  // namespace cme
