// The gather tile of the per-epoch shuffle and of the augmenting gather (shuffle.hip, augment.hip) and the writers of
// the resident layouts from it: the one place that has to agree bit for bit with MlpEngine.load_dataset().  Device
// code: only those two units include it.
//
// Both kernels are <T, VEC, VEC_T>, T = the element (1 / 2 / 4 / 8 bytes), on the grid
// (cdiv(N, 64), cdiv(P * sizeof(T), 256)): one 256-thread workgroup takes 64 destination samples d0 .. d0 + 63 and one
// 256-byte chunk of their rows, features f0 .. f0 + nf - 1.  The unit's own gather fills an LDS tile
// [64][256 B + 16 B pad] with those bytes, zeros for rows >= N and bytes >= the row's end, and after a barrier:
//   X    full rows, coalesced: VEC (rows 16-byte aligned and a multiple of 16 bytes: P * sizeof(T) % 16 == 0) 16 lanes
//        store one row chunk with 16-byte stores (Xw: the 32 bytes of the bf16 forms), else one element per lane.
//   XT   64-sample runs of one feature: VEC_T (N * sizeof(T) % 16 == 0, so a run is 16-byte aligned and a valid run
//        ends on a 16-byte boundary): each lane collects 16 / sizeof(T) samples of a feature from LDS and stores 16
//        bytes (XTw: the 32 bytes of their bf16 forms); else one element per lane, lane = sample.  Row P of XT / XTw
//        (the all-ones row) is never touched.
//   Xs   (mma_tile.h xs_off) per 16-sample tile and 64-feature pair one 1 KB block, lane l = (feature group g,
//        sample s) holding the 16 bytes of row s, features 16 g .. 16 g + 15: a 16-byte LDS read and a 16-byte
//        store per lane, 1 KB contiguous per wave.  Tiles up to cdiv(N, 16) and pairs up to cdiv(P, 64) only; the
//        padding inside them is rewritten as the tile's zeros.
// Every index is range-checked against N and P; stores are vector stores only.
#pragma once

#include <type_traits>

#include "common/hip_common.h"
#include "sample.h"
#include "shuffle.h"

namespace cme {
namespace gather {

constexpr int kRows = 64;            // destination samples per workgroup
constexpr int kChunk = 256;          // bytes of a row per workgroup
constexpr int kPitch = kChunk + 16;  // LDS row pitch (keeps 16-byte alignment, spreads the column reads)
constexpr int kThreads = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint16_t bf16_of_u8(uint32_t v) {
  // 0..255 is exact in fp32 and in bf16 (8 significand bits): the bf16 is the fp32's high half
  return static_cast<uint16_t>(__float_as_uint(static_cast<float>(v)) >> 16);
}
__device__ __forceinline__ uint32_t bf16x2(uint32_t lo, uint32_t hi) {
  return static_cast<uint32_t>(bf16_of_u8(lo)) | (static_cast<uint32_t>(bf16_of_u8(hi)) << 16);
}
// 16 u8 (a u32x4) -> 16 bf16 as two u32x4
__device__ __forceinline__ void widen16(const u32x4 v, u32x4& a, u32x4& b) {
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = v[w];
    o[2 * w] = bf16x2(x & 255u, (x >> 8) & 255u);
    o[2 * w + 1] = bf16x2((x >> 16) & 255u, x >> 24);
  }
  a = u32x4{o[0], o[1], o[2], o[3]};
  b = u32x4{o[4], o[5], o[6], o[7]};
}

// 16 bytes of elements at element offset o of D (X or XT) and, for 1-byte elements, their bf16 forms in Dw (Xw, XTw)
template <typename T>
__device__ __forceinline__ void store16(T* D, uint16_t* Dw, int64_t o, const u32x4 v) {
  if (D) *reinterpret_cast<u32x4*>(D + o) = v;
  if constexpr (sizeof(T) == 1) {
    if (Dw) {
      u32x4 lo, hi;
      widen16(v, lo, hi);
      *reinterpret_cast<u32x4*>(Dw + o) = lo;
      *reinterpret_cast<u32x4*>(Dw + o + 8) = hi;
    }
  }
}
// the same for one element
template <typename T>
__device__ __forceinline__ void store1(T* D, uint16_t* Dw, int64_t o, const T v) {
  if (D) D[o] = v;
  if constexpr (sizeof(T) == 1) {
    if (Dw) Dw[o] = bf16_of_u8(v);
  }
}

// The row prologue of thread d < 64: destination sample d (< N; past N the row is -1) -> its source row, d itself
// for the identity, a draw with replacement where a sampler's table is given (sample.h), else the keyed permutation.
// The test of the table pointer is uniform over the launch; against the parent's kernels the table-less shuffle
// launch measured the same with it (docs/PERFORMANCE.md "Weighted sampling") ...
__device__ __forceinline__ int source_of(const ShuffleArgs& a, int64_t d) {
  if (a.identity) return static_cast<int>(d);
  if (a.sample_table)
    return static_cast<int>(sample_draw(static_cast<uint32_t>(d), static_cast<uint32_t>(a.N), a.sample_key,
                                        a.sample_table));
  return static_cast<int>(shuffle_index(static_cast<uint32_t>(d), static_cast<uint32_t>(a.N), a.key));
}
// ... the identity the augmentations hash for it: the source row s, so that the order does not change what a sample
// gets; with a sampler the destination d, since one source row may then sit at many destinations of an epoch and each
// of them is to get its own shift, table entry and lattice ...
__device__ __forceinline__ uint32_t augment_id(const ShuffleArgs& a, int64_t d, int s) {
  return a.sample_table ? static_cast<uint32_t>(d) : static_cast<uint32_t>(s);
}
// ... and the chunk-0 workgroup's stores of perm[d] and the gathered label.  (One function that also tested d < N
// and chunk == 0 made the augment repeat both tests around its shift: + 9 instructions per kernel.)
__device__ __forceinline__ void store_order(const ShuffleArgs& a, int64_t d, int s) {
  if (a.perm) a.perm[d] = s;
  if (a.labels) a.labels[d] = a.labels0[s];
}

// XT (and XTw): runs of 64 samples of one feature
template <typename T, bool VEC_T>
__device__ __forceinline__ void write_xt(const unsigned char* tile, T* XT, uint16_t* XTw, int t, int64_t d0, int f0,
                                         int nf, int N) {
  constexpr int ES = sizeof(T);
  if (!XT && !XTw) return;
  if constexpr (VEC_T) {
    constexpr int EV = 16 / ES;     // samples per 16-byte store
    constexpr int GR = kRows / EV;  // 16-byte groups per run
    for (int idx = t; idx < nf * GR; idx += kThreads) {
      const int c = idx / GR, g = idx - c * GR;
      const int r0 = g * EV;
      if (d0 + r0 >= N) continue;  // N % EV == 0: a group is wholly valid or wholly past the end
      T e[EV];
#pragma unroll
      for (int j = 0; j < EV; ++j) e[j] = *reinterpret_cast<const T*>(tile + (r0 + j) * kPitch + c * ES);
      u32x4 v;
      __builtin_memcpy(&v, e, 16);
      store16(XT, XTw, static_cast<int64_t>(f0 + c) * N + d0 + r0, v);
    }
  } else {
    const int r = t & 63;
    if (d0 + r < N) {
      for (int c = t >> 6; c < nf; c += kThreads / 64) {
        const T v = *reinterpret_cast<const T*>(tile + r * kPitch + c * ES);
        store1(XT, XTw, static_cast<int64_t>(f0 + c) * N + d0 + r, v);
      }
    }
  }
}

// Xs: the forward's fragment order, 1 KB blocks [feature group][sample][16 B] (1-byte elements)
__device__ __forceinline__ void write_xs(const unsigned char* tile, void* Xs_, int t, int64_t d0, int chunk, int N,
                                         int P) {
  if (!Xs_) return;
  unsigned char* Xs = static_cast<unsigned char*>(Xs_);
  const int npair = (P + 63) >> 6;
  const int64_t ntile = (static_cast<int64_t>(N) + 15) >> 4;
  const int lane = t & 63, wave = t >> 6;
  const int s = lane & 15, grp = lane >> 4;
  // 4 sample tiles x 4 pairs per workgroup; wave w takes sample tile w
  const int64_t st = (d0 >> 4) + wave;
  if (st < ntile) {
#pragma unroll
    for (int pl = 0; pl < kChunk / 64; ++pl) {
      const int p = chunk * (kChunk / 64) + pl;
      if (p < npair) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(tile + (wave * 16 + s) * kPitch + pl * 64 + grp * 16);
        *reinterpret_cast<u32x4*>(Xs + ((st * npair + p) * 64 + lane) * 16) = v;
      }
    }
  }
}

// ---- host side: what the two launchers share
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// VEC as far as the destinations go (the shuffle also loads 16 bytes from X0), and VEC_T
inline bool vec_rows(const ShuffleArgs& a) {
  return static_cast<int64_t>(a.P) * a.es % 16 == 0 && al16(a.X) && al16(a.Xw);
}
inline bool vec_runs(const ShuffleArgs& a) {
  return static_cast<int64_t>(a.N) * a.es % 16 == 0 && al16(a.XT) && al16(a.XTw);
}
inline dim3 grid_of(const ShuffleArgs& a) {
  return dim3(static_cast<unsigned>((a.N + kRows - 1) / kRows),
              static_cast<unsigned>((static_cast<int64_t>(a.P) * a.es + kChunk - 1) / kChunk));
}

inline void check_gather_args(const ShuffleArgs& a, const char* who) {
  const std::string w = std::string(who) + ": ";
  CME_REQUIRE(a.N >= 1 && a.P >= 1, w + "N and P must be >= 1");
  CME_REQUIRE(a.X0 && a.labels0, w + "the pristine source (X0, labels0) is required");
  CME_REQUIRE(a.X0 != a.X, w + "source and destination must be distinct buffers");
  CME_REQUIRE(a.es == 1 || !(a.Xs || a.Xw || a.XTw), w + "Xs / Xw / XTw derive from uint8 pixels");
  CME_REQUIRE(a.Xs == nullptr || al16(a.Xs), w + "Xs must be 16-byte aligned");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(a.sample_table) & 7) == 0, w + "the sampler's table must be 8-byte aligned");
  CME_REQUIRE(a.sample_table != nullptr || a.sample_key == 0, w + "a sampler key needs the sampler's table");
}

// f(T{}, VEC, VEC_T): T the unsigned integer of `es` bytes, the two forms as std::bool_constant values.  False, and no
// call, for an `es` that is none of 1, 2, 4, 8.
template <typename F>
bool with_form(int es, bool vec, bool vec_t, F&& f) {
  const auto forms = [&](auto t) {
    if (vec && vec_t) f(t, std::true_type{}, std::true_type{});
    else if (vec) f(t, std::true_type{}, std::false_type{});
    else if (vec_t) f(t, std::false_type{}, std::true_type{});
    else f(t, std::false_type{}, std::false_type{});
    return true;
  };
  switch (es) {
    case 1: return forms(uint8_t{});
    case 2: return forms(uint16_t{});
    case 4: return forms(uint32_t{});
    case 8: return forms(uint64_t{});
    default: return false;
  }
}

}  // namespace gather
}  // namespace cme
