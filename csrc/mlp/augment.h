// Random-shift augmentation of the resident training set (augment.hip) and its keyed shifts.
//
// Once per epoch the augmenting gather rewrites every resident layout from the pristine rows, like the shuffle
// (shuffle.h), and on the way moves each image by its own (dx, dy).  The rule is stateless and integer-only, so the
// kernel computes a sample's shift from its SOURCE (loaded) index alone and the host (g++, bindings_cpu.cpp
// `epoch_shifts` / `augment_rows`) computes the same values from this same header.  (With a sampler, sample.h, one
// source row may sit at many places of an epoch: the index hashed is then the DESTINATION's, resident_layouts.h
// augment_id, here and in affine.h / warp.h.)
//
//   * key: augment_key(seed, iter) = shuffle_mix64(shuffle_key(seed, iter) ^ kAugmentStream), `iter` the trainer's
//     iteration counter at the start of the epoch, exactly as for the shuffle.  The fixed constant (and the mixing)
//     makes it a stream distinct from shuffle_key(seed, iter) for the same arguments.
//   * shift: one 64-bit hash per sample -- splitmix64's output at position src + 1 of the sequence seeded with the
//     key -- one 32-bit half per axis (low: dx, high: dy), each reduced to [0, 2 m] by multiply-shift,
//     (uint64(h32) * (2 m + 1)) >> 32, then moved to [-m, m].  No `%`.  Residual bias: 2^32 is no multiple of 2 m + 1
//     in general, so a cell's probability differs from 1 / (2 m + 1) by less than 2^-32, a relative bias below
//     2^-32 * (2 m + 1).  m == 0 gives 0.  The shift depends on (src, key) alone: the shuffle's order does not change
//     which shift a sample gets.
//   * source feature: the image is h rows of w pixels, feature f = y * w + x.  Destination pixel (y, x) takes source
//     pixel (y - dy, x - dx): positive dx moves content right, positive dy moves it down.  A pixel whose source lies
//     outside the image is filled with all-zero bits (0 for uint8, 0.0 for bf16 / f32 / f64), so the rule does not
//     depend on the element type.  Requires h * w == P, 0 <= max_dx < w, 0 <= max_dy < h.
#pragma once

#include <cstdint>

#include "shuffle.h"

namespace cme {

constexpr uint64_t kAugmentStream = 0xa5a5c3c35a5a3c3cull;  // (any fixed non-zero constant; part of the format)

__host__ __device__ inline uint64_t augment_key(uint32_t seed, uint32_t iter) {
  return shuffle_mix64(shuffle_key(seed, iter) ^ kAugmentStream);
}

struct AugmentShift {
  int dx, dy;
};

__host__ __device__ inline int augment_reduce(uint32_t h32, int m) {  // [0, 2^32) -> [-m, m]
  return static_cast<int>((static_cast<uint64_t>(h32) * static_cast<uint64_t>(2 * m + 1)) >> 32) - m;
}

__host__ __device__ inline AugmentShift augment_shift(uint32_t src, uint64_t key, int max_dx, int max_dy) {
  const uint64_t h = shuffle_mix64(key + (static_cast<uint64_t>(src) + 1u) * 0x9e3779b97f4a7c15ull);
  return AugmentShift{augment_reduce(static_cast<uint32_t>(h), max_dx),
                      augment_reduce(static_cast<uint32_t>(h >> 32), max_dy)};
}

// The one index rule, by coordinates: the source feature of destination pixel (y, x), or -1 outside the image.
__host__ __device__ inline int augment_src_yx(int y, int x, int dx, int dy, int h, int w) {
  const int sy = y - dy, sx = x - dx;
  return (sy >= 0 && sy < h && sx >= 0 && sx < w) ? sy * w + sx : -1;
}

__host__ __device__ inline int augment_src_feature(int f, int dx, int dy, int h, int w) {
  const int y = f / w;
  return augment_src_yx(y, f - y * w, dx, dy, h, w);
}

// One launch rewrites every resident layout as mlp_shuffle does (`base`: the same fields with the same meaning;
// base.identity != 0: no reordering, the shifts still apply -- they are keyed by the source index, which is then i;
// base.sample_table != null: the source index is a draw and the shifts are keyed by i),
// each image moved by augment_shift(source index, akey, max_dx, max_dy) on the way.  shifts: int32 [N][2] = (dx, dy)
// of RESIDENT sample i (indexed like perm), or null.  `stream` is a hipStream_t.  No sync, no read-back.
struct AugmentArgs {
  ShuffleArgs base;
  int h = 0, w = 0, max_dx = 0, max_dy = 0;
  uint64_t akey = 0;
  int* shifts = nullptr;
};
void mlp_augment(const AugmentArgs& a, void* stream);

}  // namespace cme
