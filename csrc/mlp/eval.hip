// The evaluation head for MI355X (gfx950), 1 <= C <= 64 classes, any H (eval.h): z2 = W2 a1 + b2 per sample column,
// then the first-maximum class, the stable nll, and per workgroup a loss partial, the hit / sample counts and an
// LDS-privatised confusion matrix -- instead of the pred[n] that mlp_head's predict mode stores.
//
// eval_head_kernel<P, NCT, VEC>, P = float / double, NCT = cdiv(C, 16) class tiles (1-4).  One 256-thread workgroup
// = 4 waves; it walks the 16-column blocks blockIdx.x, + gridDim.x, ... (at most kEvalMaxWgs workgroups per chunk):
//   z2      exact MFMA in the parameter dtype (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64).  Every wave takes a
//           quarter of the K = H chunks of 16 and keeps NCT accumulators; the fragment maps are mma_tile.h's (lane
//           group g owns hidden units kc + 4 g .. + 3, so W2 is one 16-byte K-contiguous load per lane and class
//           tile when H % 4 == 0, VEC).  The four partial sets go through LDS; wave 0 sums them in wave order and
//           adds b2.  W2 / b2 / a1 / label loads are range-checked buffer loads: tails in C, H and n read 0.
//   column  a column's classes are NCT x 4 accumulator registers in each of the 4 lane groups: first maximum in
//           registers in (tile, register) order (classes ascend), then across the lane groups with __shfl_xor 16 and
//           32, ties to the lower class, classes >= C masked (never compared); sum of exp(z - m) and z[label] (a
//           comparison with the label, never an index) the same way.
//   totals  lane c of lane group 0 keeps its columns' nll (fp64), hits and count over the walk; ONE LDS atomic per
//           sample on cm[label][pred].  After the walk: the loss partial = wave_sum in fixed xor order -> partials[wg]
//           (plain store), two 64-bit integer atomics for n and correct, and the non-zero cells of cm as 64-bit
//           integer atomics.
// eval_finish_kernel (one workgroup) sums the partials in index order and adds the sum to the slot's loss_sum with a
// plain load + store: chunks are stream-ordered.  eval_zero_kernel clears a slot.  No floating-point atomics.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 everywhere:
//   eval_head_kernel<float, 1/2/3/4, 0 or 1>   57-58 / 75-76 / 102 / 118 VGPRs + 4 / 8 / 16 / 20 AGPRs,
//                                              LDS 5 / 12 / 21 / 32 KB, 8 / 5 / 4 / 3 waves per SIMD
//   eval_head_kernel<double, 1/2/3/4, 0 or 1>  118-120 / 154-158 / 194-196 / 235 VGPRs + 8 / 16 / 24 / 32 AGPRs,
//                                              LDS 9 / 20 / 33 / 48 KB, 4 / 2 / 2 / 1 waves per SIMD
// Measured (bench/eval_cost.py, docs/PERFORMANCE.md "Resident evaluation"): 10 000 samples at 784-100-10 in 82-87 us,
// forward GEMMs included.
#include "eval.h"

#include "mma_tile.h"

#include <type_traits>

namespace cme {

namespace {

constexpr int kEvCols = 16;  // sample columns per block
constexpr int kEvWaves = 4;
constexpr int kEvThreads = 64 * kEvWaves;
constexpr int kEvCMax = 64;
constexpr int kEvU = 2;  // chunks of 16 hidden units per load burst (head_mc.hip's measured choice)

inline bool ev_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename P>
__device__ __forceinline__ P ev_exp(P x) {
  if constexpr (std::is_same_v<P, float>) return expf(x);
  else return exp(x);
}
template <typename P>
__device__ __forceinline__ P ev_log(P x) {
  if constexpr (std::is_same_v<P, float>) return logf(x);
  else return log(x);
}
__device__ __forceinline__ int ev_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void eval_zero_kernel(unsigned long long* stats, int words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < words) stats[i] = 0ull;
}

template <typename P, int NCT, int VEC>
__global__ __launch_bounds__(kEvThreads) void eval_head_kernel(EvalArgs a) {
  using Tr = MmaTraits<P>;
  using accv_t = typename Tr::accv_t;
  constexpr int SZ = (int)sizeof(P);
  constexpr int CP = 16 * NCT;  // classes the tiles cover (>= C)
  __shared__ __attribute__((aligned(16))) P zp[kEvWaves][NCT][4][64];  // z2 partial tiles, per wave
  __shared__ int cm[CP * CP];                                          // confusion counts [label][pred], pitch C
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c16 = lane & 15, g = lane >> 4;
  const int H = a.H, C = a.C;
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.W2), ra = make_rsrc(a.a1), rl = make_rsrc(a.labels);

  for (int i = t; i < C * C; i += kEvThreads) cm[i] = 0;  // (ordered before its first atomic by the walk's barrier)
  P bias[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cls = 16 * ct + Tr::row(g, i);
      bias[ct][i] = buf_load1<P>(make_rsrc(a.b2), cls < C ? cls * SZ : kOOB);
    }

  const int nch = (H + 15) >> 4, cpw = (nch + kEvWaves - 1) / kEvWaves;
  const int kbeg = w * cpw * 16, kend = min(H, (w + 1) * cpw * 16);
  const int ncb = (a.n + kEvCols - 1) / kEvCols;
  double lsum = 0.0;  // this lane's columns over the walk (lane group 0 of wave 0)
  int hits = 0, cnt = 0;

  // (every thread of the workgroup takes the same number of turns: the barriers inside are reached by all)
  for (int vb = blockIdx.x; vb < ncb; vb += gridDim.x) {
    const int col = vb * kEvCols + c16;
    const bool cval = col < a.n;
    const int lab = (int)__builtin_amdgcn_raw_buffer_load_b32(rl, cval ? col * 4 : kOOB, 0, 0);

    // ---- this wave's quarter of K = H
    accv_t acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = accv_t{0, 0, 0, 0};
    for (int kc = kbeg; kc < kend; kc += 16 * kEvU) {
      P xa[kEvU][4], wa[kEvU][NCT][4];
#pragma unroll
      for (int u = 0; u < kEvU; ++u) {
        const int k = kc + 16 * u + 4 * g;
        load_frag<P, 4, false, 0>(ra, a.lda, col, a.n, k, kend, xa[u]);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) load_frag<P, 4, true, VEC>(rw, H, 16 * ct + c16, C, k, kend, wa[u][ct]);
      }
      __builtin_amdgcn_sched_barrier(0);  // the burst's loads stay ahead of its first MFMA (mma_tile.h)
#pragma unroll
      for (int u = 0; u < kEvU; ++u)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) Tr::mma(wa[u][ct], xa[u], acc[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) zp[w][ct][i][lane] = acc[ct][i];
    __syncthreads();

    if (w == 0) {
      // ---- z2: the four partial sets in wave order, then b2; the first maximum on the way (classes ascend with
      //      (ct, i) in a lane)
      P z[NCT][4];
      P bv = P(0);
      int best = kEvCMax;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          P v = zp[0][ct][i][lane];
#pragma unroll
          for (int q = 1; q < kEvWaves; ++q) v += zp[q][ct][i][lane];
          v += bias[ct][i];
          z[ct][i] = v;
          const int cls = 16 * ct + Tr::row(g, i);
          const bool take = cls < C && (best == kEvCMax || v > bv || (v == bv && cls < best));
          bv = take ? v : bv;
          best = take ? cls : best;
        }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const P ov = __shfl_xor(bv, o, 64);
        const int ob = __shfl_xor(best, o, 64);
        const bool take = ob < kEvCMax && (best == kEvCMax || ov > bv || (ov == bv && ob < best));
        bv = take ? ov : bv;
        best = take ? ob : best;
      }
      // (class 0 is in lane group 0: every lane now holds its column's maximum bv and its first class best < C)
      P ssum = P(0), zl = P(0);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cls = 16 * ct + Tr::row(g, i);
          ssum += cls < C ? ev_exp<P>(z[ct][i] - bv) : P(0);
          zl += (cls < C && cls == lab) ? z[ct][i] : P(0);  // (one class of one lane group: the sum is that z2)
        }
      ssum += __shfl_xor(ssum, 16, 64);
      ssum += __shfl_xor(ssum, 32, 64);
      zl += __shfl_xor(zl, 16, 64);
      zl += __shfl_xor(zl, 32, 64);
      if (g == 0 && cval) {
        lsum += (double)(ev_log<P>(ssum) - (zl - bv));
        hits += best == lab ? 1 : 0;
        cnt += 1;
        // (a label outside [0, C) -- the callers check them once at upload -- is counted in n, never indexed)
        if ((unsigned)lab < (unsigned)C) atomicAdd(&cm[lab * C + best], 1);
      }
    }
    __syncthreads();  // zp is rewritten by the next turn; after the last one: cm is complete
  }

  if (w == 0) {
    const double ls = wave_sum(lsum);  // (0 outside lane group 0)
    const int hs = ev_wave_sum(hits), cs = ev_wave_sum(cnt);
    if (lane == 0) {
      a.partials[blockIdx.x] = ls;  // (blockIdx.x < gridDim.x = mlp_eval_num_partials(n))
      atomicAdd(a.stats + 0, (unsigned long long)cs);
      atomicAdd(a.stats + 1, (unsigned long long)hs);
    }
  }
  for (int i = t; i < C * C; i += kEvThreads) {
    const int v = cm[i];
    if (v != 0) atomicAdd(a.stats + 3 + i, (unsigned long long)v);
  }
}

// np <= kEvalMaxWgs partials in index order, added to the slot's loss_sum
__global__ __launch_bounds__(kEvalMaxWgs) void eval_finish_kernel(const double* partials, int np,
                                                                  unsigned long long* stats) {
  __shared__ double sp[kEvalMaxWgs];
  const int t = threadIdx.x;
  if (t < np) sp[t] = partials[t];
  __syncthreads();
  if (t != 0) return;
  double s = 0.0;
  for (int i = 0; i < np; ++i) s += sp[i];
  double* loss_sum = reinterpret_cast<double*>(stats + 2);
  *loss_sum = *loss_sum + s;
}

template <typename P>
void launch_eval_head(const EvalArgs& a, hipStream_t s) {
  const int grid = mlp_eval_num_partials(a.n);
  const int nct = (a.C + 15) / 16;
  // W2 rows as 16-byte vectors, each whole or out of range: H % 4 == 0 and a 16-byte aligned W2 (else element loads)
  const bool vec = a.H % 4 == 0 && ev_al16(a.W2);
#define CME_EVAL_HEAD(nc)                                                   \
  if (vec) eval_head_kernel<P, nc, 1><<<grid, kEvThreads, 0, s>>>(a); \
  else eval_head_kernel<P, nc, 0><<<grid, kEvThreads, 0, s>>>(a);
  if (nct == 1) { CME_EVAL_HEAD(1) } else if (nct == 2) { CME_EVAL_HEAD(2) } else if (nct == 3) { CME_EVAL_HEAD(3) }
  else { CME_EVAL_HEAD(4) }
#undef CME_EVAL_HEAD
  CME_LAUNCH_CHECK(s);
  eval_finish_kernel<<<1, kEvalMaxWgs, 0, s>>>(a.partials, grid, a.stats);
  CME_LAUNCH_CHECK(s);
}

}  // namespace

void mlp_eval_head(DType dt, const EvalArgs& a, hipStream_t s) {
  CME_REQUIRE(a.C >= 1 && a.C <= kEvCMax && a.H >= 1, "mlp_eval_head: 1 <= C <= 64 and H >= 1 required");
  CME_REQUIRE(a.stats != nullptr && (reinterpret_cast<uintptr_t>(a.stats) & 7) == 0,
              "mlp_eval_head: an 8-byte aligned stats slot required");
  if (a.zero) {
    const int words = (int)mlp_eval_slot_words(a.C);
    eval_zero_kernel<<<(words + 255) / 256, 256, 0, s>>>(a.stats, words);
    CME_LAUNCH_CHECK(s);
  }
  if (a.n <= 0) return;
  CME_REQUIRE(a.a1 && a.W2 && a.b2 && a.labels && a.partials,
              "mlp_eval_head: a1, W2, b2, labels and partials required");
  CME_REQUIRE(a.lda >= a.n, "mlp_eval_head: lda < n");
  const int64_t sz = dt == DType::F64 ? 8 : 4;
  CME_REQUIRE((int64_t)a.H * a.lda * sz < (int64_t)kOOB && (int64_t)a.C * a.H * sz < (int64_t)kOOB &&
                  (int64_t)a.n * 4 < (int64_t)kOOB,
              "mlp_eval_head: operand too large for 32-bit buffer offsets");
  if (dt == DType::F64) launch_eval_head<double>(a, s);
  else launch_eval_head<float>(a, s);
}

}  // namespace cme
