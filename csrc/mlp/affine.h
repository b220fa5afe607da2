// Affine augmentation of the resident training set (affine.hip): rotate, scale, shear and shift per epoch.
//
// Once per epoch the affine gather rewrites every resident layout from the pristine rows, like the shuffle (shuffle.h)
// and the shifting gather (augment.h), and on the way resamples each image through its own inverse affine map with
// four taps and a bilinear blend.  The rule is stateless; the device does integer work only, plus one fixed fp64 chain
// for non-byte elements, and the host (g++, bindings_cpu.cpp `affine_table` / `epoch_transforms` / `affine_rows`, the
// native test) computes the same values from this same header.  Only the host evaluates transcendental formulas.
//
//   * table: T entries (1 <= T <= 65536), built once by the host in fp64 (affine_table_entry).  The uniforms are
//     u = (h >> 11) * 2^-53 of successive outputs of the splitmix64 sequence seeded with
//     shuffle_mix64(seed ^ kAffineTableStream); entry k takes outputs 3 k, 3 k + 1, 3 k + 2 as u1, u2, u3:
//       theta = rotate * (2 u1 - 1) degrees, s = lo + (hi - lo) u2, phi = shear * (2 u3 - 1) degrees.
//     The forward map is A = s R(theta) [[1, tan phi], [0, 1]]; the entry is its inverse
//       inv(A) = (1 / s) [[c + t sn, sn - t c], [-sn, c]]      (c = cos theta, sn = sin theta, t = tan phi)
//     as four int32 Q16 values q = llrint(inv(A) * 65536), row-major {q00, q01, q10, q11}.  |q| < 2^23 for every
//     admitted parameter (1 / s <= 16, |t| <= tan 60 deg).  rotate = 0, scale = 1, shear = 0 gives {65536, 0, 0, 65536}.
//   * per sample and epoch: key = augment_key(seed, iter) and the shift (dx, dy) = augment_shift(src, key, ...) are
//     augment.h's, unchanged.  The table index is a second hash of the same construction on the key's own stream,
//     affine_index(src, key, T) = (uint64(low half of shuffle_mix64(shuffle_mix64(key ^ kAffineIndexStream) +
//     (src + 1) * golden)) * T) >> 32: multiply-shift, no `%`, [0, T) with both ends reached.
//   * per destination pixel (y, x) of an h x w image, in doubled coordinates so that the centre is exact:
//       u = 2 x - (w - 1) - 2 dx, v = 2 y - (h - 1) - 2 dy,
//       sx = q00 u + q01 v + (w - 1) 65536, sy = q10 u + q11 v + (h - 1) 65536       (int64; units of 2^-17 pixel)
//       ix = floor(sx / 2^17), fx = floor(sx / 2^9) mod 256 (an 8-bit fraction, truncated); iy, fy likewise.
//     Taps in the order 00, 01, 10, 11: (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1) with the weights
//     (256 - fy)(256 - fx), (256 - fy) fx, fy (256 - fx), fy fx.  A tap is skipped when its weight is 0 or it lies
//     outside the image; its address is formed only after that test.
//       uint8:             out = (sum w p + 32768) >> 16: integer only, never above 255 (the weights sum to 65536).
//       bf16 / f32 / f64:  fp64: the first present tap sets acc = double(w) * double(p), each later one
//                          acc = fma(double(w), double(p), acc); no tap: all-zero bits; else T(acc * 2^-16): one
//                          round-to-nearest-even to f32, and for bf16 the RNE of that f32 (affine_bf16_of_f32).
//     With an identity entry fx = fy = 0 and ix = x - dx, iy = y - dy: the rule is bitwise augment.h's, zero fill
//     included, for every element type.  Requires h * w == P, h, w <= kAffineMaxSide (u, v and the products stay in
//     range), 0 <= max_dx < w, 0 <= max_dy < h.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // __dmul_rn, __fma_rn, __double2float_rn and the bit casts of the device side
#endif

#include "augment.h"

namespace cme {

constexpr uint64_t kAffineTableStream = 0x3c6ef372fe94f82bull;  // (fixed non-zero constants; part of the format)
constexpr uint64_t kAffineIndexStream = 0x71374491b5c0fbcfull;
constexpr int kAffineMaxTable = 65536;
constexpr int kAffineMaxSide = 1 << 24;

// the element kinds of the blend (AffineArgs::kind; `affine_rows`): the gather needs more than the element's size
enum AffineKind : int { kAffineU8 = 0, kAffineBf16 = 1, kAffineF32 = 2, kAffineF64 = 3 };

__host__ __device__ inline int affine_kind_size(int kind) {  // bytes per element, 0 for no kind
  return kind == kAffineU8 ? 1 : kind == kAffineBf16 ? 2 : kind == kAffineF32 ? 4 : kind == kAffineF64 ? 8 : 0;
}

struct AffineEntry {
  int32_t q00, q01, q10, q11;
};

// ---- the table (host only: libm)
inline double affine_uniform(uint64_t h) { return static_cast<double>(h >> 11) * 0x1p-53; }

inline AffineEntry affine_table_entry(uint32_t seed, uint32_t k, double rotate, double lo, double hi, double shear) {
  const uint64_t s0 = shuffle_mix64(static_cast<uint64_t>(seed) ^ kAffineTableStream);
  const auto draw = [&](uint64_t i) { return affine_uniform(shuffle_mix64(s0 + (i + 1u) * 0x9e3779b97f4a7c15ull)); };
  const double u1 = draw(3ull * k), u2 = draw(3ull * k + 1u), u3 = draw(3ull * k + 2u);
  const double rad = 3.14159265358979323846 / 180.0;
  const double theta = rotate * (2.0 * u1 - 1.0) * rad;
  const double s = lo + (hi - lo) * u2;
  const double phi = shear * (2.0 * u3 - 1.0) * rad;
  const double c = std::cos(theta), sn = std::sin(theta), t = std::tan(phi), inv = 1.0 / s;
  const double m00 = (c + t * sn) * inv, m01 = (sn - t * c) * inv, m10 = -sn * inv, m11 = c * inv;
  return AffineEntry{static_cast<int32_t>(std::llrint(m00 * 65536.0)), static_cast<int32_t>(std::llrint(m01 * 65536.0)),
                     static_cast<int32_t>(std::llrint(m10 * 65536.0)), static_cast<int32_t>(std::llrint(m11 * 65536.0))};
}

// ---- per sample
__host__ __device__ inline uint32_t affine_index(uint32_t src, uint64_t key, uint32_t T) {  // [0, T)
  const uint64_t h = shuffle_mix64(shuffle_mix64(key ^ kAffineIndexStream) +
                                   (static_cast<uint64_t>(src) + 1u) * 0x9e3779b97f4a7c15ull);
  return static_cast<uint32_t>((static_cast<uint64_t>(static_cast<uint32_t>(h)) * T) >> 32);
}

// ---- per pixel
struct AffineTaps {
  int64_t ix, iy;  // the 00 tap
  int fx, fy;      // 8-bit fractions
};

__host__ __device__ inline AffineTaps affine_taps(int y, int x, int dx, int dy, const AffineEntry& q, int h, int w) {
  const int u = 2 * x - (w - 1) - 2 * dx, v = 2 * y - (h - 1) - 2 * dy;
  const int64_t sx = static_cast<int64_t>(q.q00) * u + static_cast<int64_t>(q.q01) * v + static_cast<int64_t>(w - 1) * 65536;
  const int64_t sy = static_cast<int64_t>(q.q10) * u + static_cast<int64_t>(q.q11) * v + static_cast<int64_t>(h - 1) * 65536;
  // (>> of a negative int64 is the arithmetic shift on every compiler this builds with: floor)
  return AffineTaps{sx >> 17, sy >> 17, static_cast<int>((sx >> 9) & 255), static_cast<int>((sy >> 9) & 255)};
}

// tap k (0 .. 3 = 00, 01, 10, 11): its weight, and its source feature or -1 when it is skipped
__host__ __device__ inline uint32_t affine_tap_weight(const AffineTaps& t, int k) {
  const uint32_t wy = (k & 2) ? static_cast<uint32_t>(t.fy) : 256u - static_cast<uint32_t>(t.fy);
  const uint32_t wx = (k & 1) ? static_cast<uint32_t>(t.fx) : 256u - static_cast<uint32_t>(t.fx);
  return wy * wx;
}
__host__ __device__ inline int affine_tap_feature(const AffineTaps& t, int k, int h, int w) {
  const int64_t ty = t.iy + (k >> 1), tx = t.ix + (k & 1);
  if (affine_tap_weight(t, k) == 0u || ty < 0 || ty >= h || tx < 0 || tx >= w) return -1;
  return static_cast<int>(ty) * w + static_cast<int>(tx);
}

// uint8: load(sf) -> the pixel at source feature sf in [0, h * w); called for present taps only
template <typename Load>
__host__ __device__ inline uint32_t affine_blend_u8(const AffineTaps& t, int h, int w, Load&& load) {
  uint32_t sum = 32768u;
  for (int k = 0; k < 4; ++k) {
    const int sf = affine_tap_feature(t, k, h, w);
    if (sf >= 0) sum += affine_tap_weight(t, k) * static_cast<uint32_t>(load(sf));
  }
  return sum >> 16;
}

__host__ __device__ inline double affine_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
__host__ __device__ inline double affine_fma(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fma_rn(a, b, c);
#else
  return std::fma(a, b, c);
#endif
}

// bf16 / f32 / f64: load(sf) -> double(pixel); returns false (and leaves `out` alone) when no tap is present, else
// out = acc * 2^-16 before the rounding to the element type
template <typename Load>
__host__ __device__ inline bool affine_blend_f64(const AffineTaps& t, int h, int w, Load&& load, double& out) {
  bool any = false;
  double acc = 0.0;
  for (int k = 0; k < 4; ++k) {
    const int sf = affine_tap_feature(t, k, h, w);
    if (sf >= 0) {
      const double wt = static_cast<double>(affine_tap_weight(t, k)), p = load(sf);
      acc = any ? affine_fma(wt, p, acc) : affine_mul(wt, p);
      any = true;
    }
  }
  if (any) out = affine_mul(acc, 0x1p-16);
  return any;
}

// the element conversions of the non-byte kinds, on bit patterns
__host__ __device__ inline float affine_f32_of_bits(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float f;
  std::memcpy(&f, &b, 4);
  return f;
#endif
}
__host__ __device__ inline uint32_t affine_bits_of_f32(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
#endif
}
__host__ __device__ inline double affine_f64_of_bits(uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double(static_cast<long long>(b));
#else
  double d;
  std::memcpy(&d, &b, 8);
  return d;
#endif
}
__host__ __device__ inline uint64_t affine_bits_of_f64(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<uint64_t>(__double_as_longlong(d));
#else
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
#endif
}
__host__ __device__ inline float affine_f32_of_f64(double d) {  // one round-to-nearest-even
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2float_rn(d);
#else
  return static_cast<float>(d);
#endif
}
// round-to-nearest-even of an f32 to bf16 (a NaN stays a quiet NaN)
__host__ __device__ inline uint16_t affine_bf16_of_f32(float f) {
  const uint32_t b = affine_bits_of_f32(f);
  if ((b & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((b >> 16) | 0x40u);
  return static_cast<uint16_t>((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

// One destination pixel of an image whose elements are the unsigned integers U of a kind's size: `row` points at the
// h * w elements of the source image and is indexed by present taps only.
template <typename U>
__host__ __device__ inline U affine_pixel(const U* row, int y, int x, int dx, int dy, const AffineEntry& q, int h,
                                          int w) {
  const AffineTaps t = affine_taps(y, x, dx, dy, q, h, w);
  if constexpr (sizeof(U) == 1) {
    return static_cast<U>(affine_blend_u8(t, h, w, [&](int sf) { return row[sf]; }));
  } else {
    double r = 0.0;
    bool any;
    if constexpr (sizeof(U) == 2) {
      any = affine_blend_f64(
          t, h, w, [&](int sf) { return static_cast<double>(affine_f32_of_bits(static_cast<uint32_t>(row[sf]) << 16)); },
          r);
      return any ? affine_bf16_of_f32(affine_f32_of_f64(r)) : U{0};
    } else if constexpr (sizeof(U) == 4) {
      any = affine_blend_f64(t, h, w, [&](int sf) { return static_cast<double>(affine_f32_of_bits(row[sf])); }, r);
      return any ? affine_bits_of_f32(affine_f32_of_f64(r)) : U{0};
    } else {
      any = affine_blend_f64(t, h, w, [&](int sf) { return affine_f64_of_bits(row[sf]); }, r);
      return any ? affine_bits_of_f64(r) : U{0};
    }
  }
}

// One launch rewrites every resident layout as mlp_augment does (`base`, h, w, max_dx, max_dy, akey, shifts: the same
// fields with the same meaning), each image resampled through table entry affine_index(source index, akey, T) and
// moved by its shift.  table: int32 [T][4] on the device, 16-byte aligned; kind: the AffineKind of base.es;
// transforms: int32 [N], the table index of RESIDENT sample i (indexed like perm), or null.  `stream` is a
// hipStream_t.  No sync, no read-back.
struct AffineArgs {
  AugmentArgs aug;
  const int32_t* table = nullptr;
  int T = 0;
  int kind = kAffineU8;
  int* transforms = nullptr;
};
void mlp_affine(const AffineArgs& a, void* stream);

}  // namespace cme
