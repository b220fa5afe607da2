// The per-epoch shuffle of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0 in
// the order of the keyed permutation (shuffle.h shuffle_index) and rewrites every layout the step kernels read -- X,
// labels, XT, Xs, Xw, XTw -- in place, so every pointer an MlpStep has bound and every captured graph stays valid.
//
// shuffle_kernel<T, VEC, VEC_T>, T = the element (1 / 2 / 4 / 8 bytes).  Grid (cdiv(N, 64), cdiv(P * sizeof(T), 256)): one
// 256-thread workgroup takes 64 destination samples d0 .. d0 + 63 and one 256-byte chunk of their rows.
//   perm    thread d < 64 computes its destination sample's source row (or d itself: identity) into LDS; the
//           chunk-0 workgroup also stores perm[] and the gathered label.
//   gather  the 64 source-row chunks -> LDS tile [64][256 B + 16 B pad]; rows >= N and bytes >= the row's end are
//           written as zeros (the Xs padding is rewritten from them).  VEC (rows 16-byte aligned and a multiple of 16
//           bytes: P * sizeof(T) % 16 == 0): 16 lanes read one row chunk with 16-byte loads, 16 rows per pass; else
//           one element per lane.  The same registers go straight to X (and, converted, to Xw): full rows, coalesced.
//   XT      64-sample runs of one feature: VEC_T (N * sizeof(T) % 16 == 0, so a run is 16-byte aligned and a valid
//           run ends on a 16-byte boundary): each lane collects 16 / sizeof(T) samples of a feature from LDS and
//           stores 16 bytes (XTw: the 32 bytes of their bf16 forms); else one element per lane, lane = sample.
//   Xs      (mma_tile.h xs_off) per 16-sample tile and 64-feature pair one 1 KB block, lane l = (feature group g,
//           sample s) holding the 16 bytes of row s, features 16 g .. 16 g + 15: a 16-byte LDS read and a 16-byte
//           store per lane, 1 KB contiguous per wave.  Tiles up to cdiv(N, 16) and pairs up to cdiv(P, 64) only.
// Every index is range-checked against N and P; stores are vector stores only.  LDS 17.3 KB per workgroup, 14-26
// VGPRs, no scratch, 8 waves per SIMD.
// Measured (bench/shuffle_cost.py, docs/PERFORMANCE.md "Per-epoch shuffle"): 60 000 x 784 pixels in 38-43 us with X, XT
// and Xs (1.8 x a copy of the same bytes), 117-122 us with the bf16 copies.  A variant of the XT step that read the
// tile as four-byte words and transposed 4 x 4 byte blocks in registers (a quarter of the LDS reads) measured the
// same, so the one-byte LDS reads do not bound the kernel; the simpler form stays.  128 samples per workgroup (128-byte
// XT runs, 34 KB of LDS) measured 45-50 us and 106-109 us: slower where it counts, so 64 stays.
#include "shuffle.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kShRows = 64;            // destination samples per workgroup
constexpr int kShChunk = 256;          // bytes of a row per workgroup
constexpr int kShPitch = kShChunk + 16;  // LDS row pitch (keeps 16-byte alignment, spreads the column reads)
constexpr int kShThreads = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint16_t sh_bf16_of_u8(uint32_t v) {
  // 0..255 is exact in fp32 and in bf16 (8 significand bits): the bf16 is the fp32's high half
  return static_cast<uint16_t>(__float_as_uint(static_cast<float>(v)) >> 16);
}
__device__ __forceinline__ uint32_t sh_bf16x2(uint32_t lo, uint32_t hi) {
  return static_cast<uint32_t>(sh_bf16_of_u8(lo)) | (static_cast<uint32_t>(sh_bf16_of_u8(hi)) << 16);
}
// 16 u8 (a u32x4) -> 16 bf16 as two u32x4
__device__ __forceinline__ void sh_widen16(const u32x4 v, u32x4& a, u32x4& b) {
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = v[w];
    o[2 * w] = sh_bf16x2(x & 255u, (x >> 8) & 255u);
    o[2 * w + 1] = sh_bf16x2((x >> 16) & 255u, x >> 24);
  }
  a = u32x4{o[0], o[1], o[2], o[3]};
  b = u32x4{o[4], o[5], o[6], o[7]};
}

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kShThreads) void shuffle_kernel(ShuffleArgs a) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kShChunk / ES;  // features per chunk
  __shared__ __attribute__((aligned(16))) unsigned char tile[kShRows * kShPitch];
  __shared__ int src[kShRows];
  const int t = threadIdx.x;
  const int64_t d0 = static_cast<int64_t>(blockIdx.x) * kShRows;
  const int chunk = blockIdx.y;
  const int f0 = chunk * FC;  // first feature of the chunk
  const int N = a.N, P = a.P;
  const int nf = min(FC, P - f0);  // valid features of the chunk (>= 1 by the grid)

  if (t < kShRows) {
    const int64_t d = d0 + t;
    int s = -1;
    if (d < N) {
      s = a.identity ? static_cast<int>(d)
                     : static_cast<int>(shuffle_index(static_cast<uint32_t>(d), static_cast<uint32_t>(N), a.key));
      if (chunk == 0) {
        if (a.perm) a.perm[d] = s;
        if (a.labels) a.labels[d] = a.labels0[s];
      }
    }
    src[t] = s;
  }
  __syncthreads();

  const T* X0 = static_cast<const T*>(a.X0);
  T* X = static_cast<T*>(a.X);
  uint16_t* Xw = static_cast<uint16_t*>(a.Xw);
  // ---- gather: source rows -> LDS (+ X, Xw straight from the registers)
  if constexpr (VEC) {
    constexpr int EV = 16 / ES;  // elements per 16-byte load
    const int g = t & 15;        // 16-byte granule of the chunk
    const int fg = f0 + g * EV;  // its first feature; P % EV == 0, so a granule is wholly inside the row or outside
#pragma unroll
    for (int pass = 0; pass < kShRows / 16; ++pass) {
      const int r = pass * 16 + (t >> 4);
      const int s = src[r];
      u32x4 v = {0u, 0u, 0u, 0u};
      if (s >= 0 && fg < P) {
        v = *reinterpret_cast<const u32x4*>(X0 + static_cast<int64_t>(s) * P + fg);
        const int64_t o = (d0 + r) * P + fg;
        if (X) *reinterpret_cast<u32x4*>(X + o) = v;
        if constexpr (ES == 1) {
          if (Xw) {
            u32x4 lo, hi;
            sh_widen16(v, lo, hi);
            *reinterpret_cast<u32x4*>(Xw + o) = lo;
            *reinterpret_cast<u32x4*>(Xw + o + 8) = hi;
          }
        }
      }
      *reinterpret_cast<u32x4*>(tile + r * kShPitch + g * 16) = v;
    }
  } else {
    for (int idx = t; idx < kShRows * FC; idx += kShThreads) {
      const int r = idx / FC, c = idx - r * FC;
      const int s = src[r];
      T v = 0;
      if (s >= 0 && c < nf) {
        v = X0[static_cast<int64_t>(s) * P + f0 + c];
        const int64_t o = (d0 + r) * P + f0 + c;
        if (X) X[o] = v;
        if constexpr (ES == 1) {
          if (Xw) Xw[o] = sh_bf16_of_u8(v);
        }
      }
      *reinterpret_cast<T*>(tile + r * kShPitch + c * ES) = v;
    }
  }
  __syncthreads();

  // ---- XT (and XTw): runs of 64 samples of one feature
  T* XT = static_cast<T*>(a.XT);
  uint16_t* XTw = static_cast<uint16_t*>(a.XTw);
  if (XT || XTw) {
    if constexpr (VEC_T) {
      constexpr int EV = 16 / ES;        // samples per 16-byte store
      constexpr int GR = kShRows / EV;   // 16-byte groups per run
      for (int idx = t; idx < nf * GR; idx += kShThreads) {
        const int c = idx / GR, g = idx - c * GR;
        const int r0 = g * EV;
        if (d0 + r0 >= N) continue;  // N % EV == 0: a group is wholly valid or wholly past the end
        T e[EV];
#pragma unroll
        for (int j = 0; j < EV; ++j) e[j] = *reinterpret_cast<const T*>(tile + (r0 + j) * kShPitch + c * ES);
        const int64_t o = static_cast<int64_t>(f0 + c) * N + d0 + r0;
        u32x4 v;
        __builtin_memcpy(&v, e, 16);
        if (XT) *reinterpret_cast<u32x4*>(XT + o) = v;
        if constexpr (ES == 1) {
          if (XTw) {
            u32x4 lo, hi;
            sh_widen16(v, lo, hi);
            *reinterpret_cast<u32x4*>(XTw + o) = lo;
            *reinterpret_cast<u32x4*>(XTw + o + 8) = hi;
          }
        }
      }
    } else {
      const int r = t & 63;
      if (d0 + r < N) {
        for (int c = t >> 6; c < nf; c += kShThreads / 64) {
          const T v = *reinterpret_cast<const T*>(tile + r * kShPitch + c * ES);
          const int64_t o = static_cast<int64_t>(f0 + c) * N + d0 + r;
          if (XT) XT[o] = v;
          if constexpr (ES == 1) {
            if (XTw) XTw[o] = sh_bf16_of_u8(v);
          }
        }
      }
    }
  }

  // ---- Xs: the forward's fragment order, 1 KB blocks [feature group][sample][16 B]
  if constexpr (ES == 1) {
    if (a.Xs) {
      unsigned char* Xs = static_cast<unsigned char*>(a.Xs);
      const int npair = (P + 63) >> 6;
      const int64_t ntile = (static_cast<int64_t>(N) + 15) >> 4;
      const int lane = t & 63, wave = t >> 6;
      const int s = lane & 15, grp = lane >> 4;
      // 4 sample tiles x 4 pairs per workgroup; wave w takes sample tile w
      const int64_t st = (d0 >> 4) + wave;
      if (st < ntile) {
#pragma unroll
        for (int pl = 0; pl < kShChunk / 64; ++pl) {
          const int p = chunk * (kShChunk / 64) + pl;
          if (p < npair) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(tile + (wave * 16 + s) * kShPitch + pl * 64 + grp * 16);
            *reinterpret_cast<u32x4*>(Xs + ((st * npair + p) * 64 + lane) * 16) = v;
          }
        }
      }
    }
  }
}

inline bool sh_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
void launch(const ShuffleArgs& a, hipStream_t st) {
  constexpr int ES = sizeof(T);
  const int64_t rowb = static_cast<int64_t>(a.P) * ES, colb = static_cast<int64_t>(a.N) * ES;
  const bool vec = rowb % 16 == 0 && sh_al16(a.X0) && sh_al16(a.X) && sh_al16(a.Xw);
  const bool vec_t = colb % 16 == 0 && sh_al16(a.XT) && sh_al16(a.XTw);
  const dim3 grid(static_cast<unsigned>((a.N + kShRows - 1) / kShRows),
                  static_cast<unsigned>((rowb + kShChunk - 1) / kShChunk));
  if (vec && vec_t) hipLaunchKernelGGL((shuffle_kernel<T, true, true>), grid, dim3(kShThreads), 0, st, a);
  else if (vec) hipLaunchKernelGGL((shuffle_kernel<T, true, false>), grid, dim3(kShThreads), 0, st, a);
  else if (vec_t) hipLaunchKernelGGL((shuffle_kernel<T, false, true>), grid, dim3(kShThreads), 0, st, a);
  else hipLaunchKernelGGL((shuffle_kernel<T, false, false>), grid, dim3(kShThreads), 0, st, a);
  CME_LAUNCH_CHECK(st);
}

}  // namespace

void mlp_shuffle(const ShuffleArgs& a, void* stream) {
  CME_REQUIRE(a.N >= 1 && a.P >= 1, "mlp_shuffle: N and P must be >= 1");
  CME_REQUIRE(a.X0 && a.labels0, "mlp_shuffle: the pristine source (X0, labels0) is required");
  CME_REQUIRE(a.X0 != a.X, "mlp_shuffle: source and destination must be distinct buffers");
  CME_REQUIRE(a.es == 1 || !(a.Xs || a.Xw || a.XTw), "mlp_shuffle: Xs / Xw / XTw derive from uint8 pixels");
  CME_REQUIRE(a.Xs == nullptr || sh_al16(a.Xs), "mlp_shuffle: Xs must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a.es) {
    case 1: launch<uint8_t>(a, st); break;
    case 2: launch<uint16_t>(a, st); break;
    case 4: launch<uint32_t>(a, st); break;
    case 8: launch<uint64_t>(a, st); break;
    default: throw std::invalid_argument("mlp_shuffle: element size must be 1, 2, 4 or 8");
  }
}

}  // namespace cme
