// Random-shift augmentation of the resident training set for MI355X (gfx950): one launch gathers the pristine rows X0
// in the order of the keyed permutation (shuffle.h shuffle_index, or the loaded order), moves every image by its own
// (dx, dy) (augment.h augment_shift / augment_src_yx) and rewrites every layout the step kernels read -- X, labels,
// XT, Xs, Xw, XTw -- in place, so every pointer an MlpStep has bound and every captured graph stays valid.  The layout
// writers repeat shuffle.hip's (that unit is left as it is; merging the two is a follow-up).
//
// augment_kernel<T, VEC, VEC_T>, T = the element (1 / 2 / 4 / 8 bytes).  Grid (cdiv(N, 64), cdiv(P * sizeof(T), 256)): one
// 256-thread workgroup takes 64 destination samples d0 .. d0 + 63 and one 256-byte chunk of their rows.
//   rows    thread d < 64 computes its destination sample's source row (or d itself: identity; -1 past N) and that
//           row's shift into LDS as {source, dx, dy, dy * w + dx}; the chunk-0 workgroup also stores perm[], the
//           gathered label and shifts[].
//   gather  LDS tile [64][256 B + 16 B pad] of the SHIFTED bytes, one element per lane: a thread keeps one destination
//           feature (its (y, x) is divided out once) and walks the rows, so a wave reads 64 adjacent elements of one
//           source row, displaced by dy * w + dx; every lane is masked by the index rule for itself, so no address
//           outside row s of X0 is ever formed and every load is an aligned element load.  Pixels without a source,
//           rows >= N and bytes >= the row's end are written as zeros (the Xs padding is rewritten from them).
//   X       full rows from the tile, coalesced: VEC (rows 16-byte aligned and a multiple of 16 bytes) 16-byte LDS
//           reads and stores (Xw: the 32 bytes of the bf16 forms), else one element per lane.
//   XT, Xs  as in shuffle.hip: 64-sample runs per feature (VEC_T: N * sizeof(T) % 16 == 0, 16-byte stores), and the
//           forward's fragment order in 1 KB blocks.  Row P of XT / XTw (the all-ones row) is never touched.
// Every index is range-checked against N and P; stores are vector stores only; no atomics.  LDS 18 432 B per workgroup,
// 14-23 VGPRs, no scratch, 8 waves per SIMD (the compiler's resource report of the gfx950 build).
// Measured (bench/augment_cost.py, docs/PERFORMANCE.md "Augmentation"): 60 000 x 784 pixels in 73 us with X, XT and Xs
// against 44 us for the shuffle launch in the same run (1.66 x), 156 us against 122 us with the bf16 copies (1.28 x).
// The staged form of the gather (aligned 16-byte loads of the covering span into a second LDS buffer) was not built.
#include "augment.h"

#include "common/hip_common.h"

namespace cme {

namespace {

constexpr int kAuRows = 64;              // destination samples per workgroup
constexpr int kAuChunk = 256;            // bytes of a row per workgroup
constexpr int kAuPitch = kAuChunk + 16;  // LDS row pitch (keeps 16-byte alignment, spreads the column reads)
constexpr int kAuThreads = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint16_t au_bf16_of_u8(uint32_t v) {
  // 0..255 is exact in fp32 and in bf16 (8 significand bits): the bf16 is the fp32's high half
  return static_cast<uint16_t>(__float_as_uint(static_cast<float>(v)) >> 16);
}
__device__ __forceinline__ uint32_t au_bf16x2(uint32_t lo, uint32_t hi) {
  return static_cast<uint32_t>(au_bf16_of_u8(lo)) | (static_cast<uint32_t>(au_bf16_of_u8(hi)) << 16);
}
// 16 u8 (a u32x4) -> 16 bf16 as two u32x4
__device__ __forceinline__ void au_widen16(const u32x4 v, u32x4& a, u32x4& b) {
  uint32_t o[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t x = v[w];
    o[2 * w] = au_bf16x2(x & 255u, (x >> 8) & 255u);
    o[2 * w + 1] = au_bf16x2((x >> 16) & 255u, x >> 24);
  }
  a = u32x4{o[0], o[1], o[2], o[3]};
  b = u32x4{o[4], o[5], o[6], o[7]};
}

template <typename T, bool VEC, bool VEC_T>
__global__ __launch_bounds__(kAuThreads) void augment_kernel(AugmentArgs aa) {
  constexpr int ES = sizeof(T);
  constexpr int FC = kAuChunk / ES;  // features per chunk
  static_assert(kAuThreads % FC == 0, "a thread keeps one feature of the chunk");
  constexpr int RP = kAuThreads / FC;  // rows per pass of the gather
  __shared__ __attribute__((aligned(16))) unsigned char tile[kAuRows * kAuPitch];
  __shared__ __attribute__((aligned(16))) int rows[kAuRows * 4];  // {source row or -1, dx, dy, dy * w + dx}
  const ShuffleArgs& a = aa.base;
  const int t = threadIdx.x;
  const int64_t d0 = static_cast<int64_t>(blockIdx.x) * kAuRows;
  const int chunk = blockIdx.y;
  const int f0 = chunk * FC;  // first feature of the chunk
  const int N = a.N, P = a.P;
  const int nf = min(FC, P - f0);  // valid features of the chunk (>= 1 by the grid)
  const int ih = aa.h, iw = aa.w;

  if (t < kAuRows) {
    const int64_t d = d0 + t;
    int s = -1;
    AugmentShift sh{0, 0};
    if (d < N) {
      s = a.identity ? static_cast<int>(d)
                     : static_cast<int>(shuffle_index(static_cast<uint32_t>(d), static_cast<uint32_t>(N), a.key));
      sh = augment_shift(static_cast<uint32_t>(s), aa.akey, aa.max_dx, aa.max_dy);
      if (chunk == 0) {
        if (a.perm) a.perm[d] = s;
        if (a.labels) a.labels[d] = a.labels0[s];
        if (aa.shifts) {
          aa.shifts[2 * d] = sh.dx;
          aa.shifts[2 * d + 1] = sh.dy;
        }
      }
    }
    *reinterpret_cast<i32x4*>(rows + 4 * t) = i32x4{s, sh.dx, sh.dy, sh.dy * iw + sh.dx};
  }
  __syncthreads();

  // ---- gather: the shifted source rows -> LDS, one element per lane; the thread's feature is fixed
  const T* X0 = static_cast<const T*>(a.X0);
  {
    const int c = t & (FC - 1);
    const int f = f0 + c;
    const bool inrow = c < nf;  // f < P
    const int y = inrow ? f / iw : 0, x = inrow ? f - y * iw : 0;
#pragma unroll 8
    for (int r = t / FC; r < kAuRows; r += RP) {
      const i32x4 rw = *reinterpret_cast<const i32x4*>(rows + 4 * r);
      T v = 0;
      if (rw[0] >= 0 && inrow) {
        const int sf = augment_src_yx(y, x, rw[1], rw[2], ih, iw);  // in [0, P), or -1
        if (sf >= 0) v = X0[static_cast<int64_t>(rw[0]) * P + sf];
      }
      *reinterpret_cast<T*>(tile + r * kAuPitch + c * ES) = v;
    }
  }
  __syncthreads();

  // ---- X (and Xw): full rows from the tile
  T* X = static_cast<T*>(a.X);
  uint16_t* Xw = static_cast<uint16_t*>(a.Xw);
  if (X || Xw) {
    if constexpr (VEC) {
      constexpr int EV = 16 / ES;  // elements per 16-byte store
      const int g = t & 15;        // 16-byte granule of the chunk
      const int fg = f0 + g * EV;  // its first feature; P % EV == 0, so a granule is wholly inside the row or outside
#pragma unroll
      for (int pass = 0; pass < kAuRows / 16; ++pass) {
        const int r = pass * 16 + (t >> 4);
        if (d0 + r < N && fg < P) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(tile + r * kAuPitch + g * 16);
          const int64_t o = (d0 + r) * P + fg;
          if (X) *reinterpret_cast<u32x4*>(X + o) = v;
          if constexpr (ES == 1) {
            if (Xw) {
              u32x4 lo, hi;
              au_widen16(v, lo, hi);
              *reinterpret_cast<u32x4*>(Xw + o) = lo;
              *reinterpret_cast<u32x4*>(Xw + o + 8) = hi;
            }
          }
        }
      }
    } else {
      for (int idx = t; idx < kAuRows * FC; idx += kAuThreads) {
        const int r = idx / FC, c = idx - r * FC;
        if (d0 + r < N && c < nf) {
          const T v = *reinterpret_cast<const T*>(tile + r * kAuPitch + c * ES);
          const int64_t o = (d0 + r) * P + f0 + c;
          if (X) X[o] = v;
          if constexpr (ES == 1) {
            if (Xw) Xw[o] = au_bf16_of_u8(v);
          }
        }
      }
    }
  }

  // ---- XT (and XTw): runs of 64 samples of one feature
  T* XT = static_cast<T*>(a.XT);
  uint16_t* XTw = static_cast<uint16_t*>(a.XTw);
  if (XT || XTw) {
    if constexpr (VEC_T) {
      constexpr int EV = 16 / ES;       // samples per 16-byte store
      constexpr int GR = kAuRows / EV;  // 16-byte groups per run
      for (int idx = t; idx < nf * GR; idx += kAuThreads) {
        const int c = idx / GR, g = idx - c * GR;
        const int r0 = g * EV;
        if (d0 + r0 >= N) continue;  // N % EV == 0: a group is wholly valid or wholly past the end
        T e[EV];
#pragma unroll
        for (int j = 0; j < EV; ++j) e[j] = *reinterpret_cast<const T*>(tile + (r0 + j) * kAuPitch + c * ES);
        const int64_t o = static_cast<int64_t>(f0 + c) * N + d0 + r0;
        u32x4 v;
        __builtin_memcpy(&v, e, 16);
        if (XT) *reinterpret_cast<u32x4*>(XT + o) = v;
        if constexpr (ES == 1) {
          if (XTw) {
            u32x4 lo, hi;
            au_widen16(v, lo, hi);
            *reinterpret_cast<u32x4*>(XTw + o) = lo;
            *reinterpret_cast<u32x4*>(XTw + o + 8) = hi;
          }
        }
      }
    } else {
      const int r = t & 63;
      if (d0 + r < N) {
        for (int c = t >> 6; c < nf; c += kAuThreads / 64) {
          const T v = *reinterpret_cast<const T*>(tile + r * kAuPitch + c * ES);
          const int64_t o = static_cast<int64_t>(f0 + c) * N + d0 + r;
          if (XT) XT[o] = v;
          if constexpr (ES == 1) {
            if (XTw) XTw[o] = au_bf16_of_u8(v);
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
        for (int pl = 0; pl < kAuChunk / 64; ++pl) {
          const int p = chunk * (kAuChunk / 64) + pl;
          if (p < npair) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(tile + (wave * 16 + s) * kAuPitch + pl * 64 + grp * 16);
            *reinterpret_cast<u32x4*>(Xs + ((st * npair + p) * 64 + lane) * 16) = v;
          }
        }
      }
    }
  }
}

inline bool au_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
void launch(const AugmentArgs& aa, hipStream_t st) {
  constexpr int ES = sizeof(T);
  const ShuffleArgs& a = aa.base;
  const int64_t rowb = static_cast<int64_t>(a.P) * ES, colb = static_cast<int64_t>(a.N) * ES;
  const bool vec = rowb % 16 == 0 && au_al16(a.X) && au_al16(a.Xw);
  const bool vec_t = colb % 16 == 0 && au_al16(a.XT) && au_al16(a.XTw);
  const dim3 grid(static_cast<unsigned>((a.N + kAuRows - 1) / kAuRows),
                  static_cast<unsigned>((rowb + kAuChunk - 1) / kAuChunk));
  if (vec && vec_t) hipLaunchKernelGGL((augment_kernel<T, true, true>), grid, dim3(kAuThreads), 0, st, aa);
  else if (vec) hipLaunchKernelGGL((augment_kernel<T, true, false>), grid, dim3(kAuThreads), 0, st, aa);
  else if (vec_t) hipLaunchKernelGGL((augment_kernel<T, false, true>), grid, dim3(kAuThreads), 0, st, aa);
  else hipLaunchKernelGGL((augment_kernel<T, false, false>), grid, dim3(kAuThreads), 0, st, aa);
  CME_LAUNCH_CHECK(st);
}

}  // namespace

void mlp_augment(const AugmentArgs& aa, void* stream) {
  const ShuffleArgs& a = aa.base;
  CME_REQUIRE(a.N >= 1 && a.P >= 1, "mlp_augment: N and P must be >= 1");
  CME_REQUIRE(a.X0 && a.labels0, "mlp_augment: the pristine source (X0, labels0) is required");
  CME_REQUIRE(a.X0 != a.X, "mlp_augment: source and destination must be distinct buffers");
  CME_REQUIRE(a.es == 1 || a.es == 2 || a.es == 4 || a.es == 8, "mlp_augment: element size must be 1, 2, 4 or 8");
  CME_REQUIRE(a.es == 1 || !(a.Xs || a.Xw || a.XTw), "mlp_augment: Xs / Xw / XTw derive from uint8 pixels");
  CME_REQUIRE(a.Xs == nullptr || au_al16(a.Xs), "mlp_augment: Xs must be 16-byte aligned");
  CME_REQUIRE(aa.h >= 1 && aa.w >= 1 && static_cast<int64_t>(aa.h) * aa.w == a.P,
              "mlp_augment: the image shape h x w must have h * w == P");
  CME_REQUIRE(aa.max_dx >= 0 && aa.max_dx < aa.w && aa.max_dy >= 0 && aa.max_dy < aa.h,
              "mlp_augment: the shift bounds must satisfy 0 <= max_dx < w and 0 <= max_dy < h");
  CME_REQUIRE((reinterpret_cast<uintptr_t>(aa.shifts) & 3) == 0, "mlp_augment: shifts must be 4-byte aligned");
  const uintptr_t ea = static_cast<uintptr_t>(a.es) - 1;  // elements are loaded and stored at their natural alignment
  CME_REQUIRE(((reinterpret_cast<uintptr_t>(a.X0) | reinterpret_cast<uintptr_t>(a.X) |
                reinterpret_cast<uintptr_t>(a.XT)) & ea) == 0,
              "mlp_augment: X0, X and XT must be aligned to the element size");
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a.es) {
    case 1: launch<uint8_t>(aa, st); break;
    case 2: launch<uint16_t>(aa, st); break;
    case 4: launch<uint32_t>(aa, st); break;
    default: launch<uint64_t>(aa, st); break;
  }
}

}  // namespace cme
