// The many-class output layer (17 <= C <= 64, any H) for MI355X (gfx950): the head and the output layer's weight
// gradients for class counts the 16-class kernels of mlp_kernels.hip / mlp_split.hip do not take.  Nothing here is
// fused into another launch: a step at C > 16 is forward GEMM, mlp_head_mc, dW1 launch, mlp_out_wgrad_mc.
//
// mlp_head_mc -- head_mc_kernel<P, NCT, VEC>, P = float / double (bf16 mode: fp32 parameters, the float form),
// NCT = cdiv(C, 16) class tiles.  One 256-thread workgroup = 16 sample columns x 4 waves, exact MFMA in the
// parameter dtype (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64):
//   pass 1  z2 (16 NCT x 16) = W2 . a1: every wave takes a quarter of the K = H chunks of 16 and keeps NCT
//           accumulators (W2 as 16-byte K-contiguous fragments when H % 4 == 0, VEC); the four partial sets go
//           through LDS and EVERY wave sums them in wave order and adds b2, so every wave holds the same z2 bits
//           (no second hand-off for D).
//   softmax a column's classes are NCT x 4 accumulator registers in each of the 4 lane groups: max and sum in
//           registers in (tile, register) order, then across the lane groups with __shfl_xor 16 and 32.  Classes
//           >= C are masked; the one-hot is a comparison with the label, never an index.
//   pass 2  dA1 (H x 16) = W2^T . D with K = C: accumulator register i of lane group g holds class row
//           16 ct + Tr::row(g, i), which IS the B operand of MFMA step i when the A operand supplies
//           W2[16 ct + Tr::row(g, i)][h0 + (lane & 15)] (head32_kernel's trick; Tr::row makes it hold for the f64
//           g + 4 i map too).  The waves stride over the 16-row tiles; dz = da . a1 (1 - a1) at the C/D positions.
//   With few column blocks the row tiles of pass 2 are spread over gridDim.y workgroups per column block (each
//   redoes pass 1, which is the same arithmetic in the same order: the bits do not depend on the grid); only row
//   block 0 writes D, the loss partial, pred and probs.
// Every W2 / b2 / a1 / label load is a range-checked buffer load (tails in C, H and n read 0, no branches around
// loads); W2 is never staged in LDS (H is unbounded).  Sums have a fixed order and there are no atomics: reruns
// are bitwise equal.
//
// mlp_out_wgrad_mc -- out_wgrad_mc_kernel<VEC>: what the split path's wgrad_roles produce at C <= 16.  cdiv(C, 16)
// x cdiv(H, 16) workgroups each form one 16 x 16 tile of dW2 = D . a1^T over K = n (wsk_tile<float, 1, 1, 8>,
// EpiW2: reg . W2 added, SGD in place or the gradient into gW2), then one wave per bias row (db2, and db1 from dZ1
// without the all-ones XT feature) in the roles' row_sum + wave_sum order.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 everywhere:
//   head_mc_kernel<float, 2/3/4, 0 or 1>   72 / 97 / 121 VGPRs + 8 / 12 / 16 AGPRs, LDS 8 / 12 / 16 KB, 6 / 4 / 3
//                                          waves per SIMD
//   head_mc_kernel<double, 2/3/4, 1>       114 / 150 / 189 VGPRs + 16 / 24 / 32 AGPRs, LDS 16 / 24 / 32 KB, 3 / 2 / 2
//                                          waves per SIMD (VEC 0: 112 / 148 / 189 VGPRs)
//   out_wgrad_mc_kernel<0/1>       90 / 84 VGPRs, LDS 8 KB, 5 waves per SIMD
#include "mlp_kernels.h"
#include "mlp_split.h"

#include "head_math.h"
#include "mma_tile.h"
#include "wgrad_epi.h"

#include <type_traits>

namespace cme {

namespace {

using namespace wg;  // (wgrad_epi.h: row_sum, EpiW2, ag_err_load, poisoned)

constexpr int kMcCols = 16;    // sample columns per workgroup
constexpr int kMcWaves = 4;
constexpr int kMcThreads = 64 * kMcWaves;
constexpr int kMcCMax = 64;
// pass-1 chunks of 16 hidden units per load burst (4 measured no faster at H = 1024 and 0.3-0.7 us slower at H = 100)
constexpr int kMcU = 2;

inline int mc_cdiv(int a, int b) { return (a + b - 1) / b; }
inline bool mc_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename P>
__device__ __forceinline__ void mfma4(P a, P b, typename MmaTraits<P>::accv_t& c) {
  if constexpr (std::is_same_v<P, float>) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  else c = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

template <typename P>
__device__ __forceinline__ P mc_exp(P x) {
  if constexpr (std::is_same_v<P, float>) return __expf(x);
  else return exp(x);
}
template <typename P>
__device__ __forceinline__ P mc_max(P a, P b) { return a > b ? a : b; }

template <typename P, int NCT, int VEC>
__global__ __launch_bounds__(kMcThreads) void head_mc_kernel(HeadArgs a) {
  using Tr = MmaTraits<P>;
  using accv_t = typename Tr::accv_t;
  constexpr int SZ = (int)sizeof(P);
  __shared__ __attribute__((aligned(16))) P zp[kMcWaves][NCT][4][64];  // pass-1 partial tiles, per wave
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, c16 = lane & 15, g = lane >> 4;
  const int H = a.H, C = a.C;
  const int vb = blockIdx.x, col = vb * kMcCols + c16;
  const bool cval = col < a.n;
  const bool first = blockIdx.y == 0;
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.W2), ra = make_rsrc(a.a1);

  // the label and this lane's biases ride with the first burst
  const int lab = a.mode == HEAD_TRAIN
                      ? (int)__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a.labels), cval ? col * 4 : kOOB, 0, 0)
                      : -1;
  P bias[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cls = 16 * ct + Tr::row(g, i);
      bias[ct][i] = buf_load1<P>(make_rsrc(a.b2), cls < C ? cls * SZ : kOOB);
    }

  // ---- pass 1: this wave's quarter of the K = H chunks of 16.  Inside a chunk K is permuted as in mma_tile.h:
  //      lane group g owns hidden units kc + 4 g .. kc + 4 g + 3 and MFMA j consumes element j, so a lane's four W2
  //      values are CONTIGUOUS -- one 16-byte load (VEC) instead of four 4-byte loads 16 rows apart.  (With step j
  //      taking unit kc + 4 j + g every load touched 16 bytes of 16 different W2 rows; at H = 1024 a row's 128-byte
  //      line left the L1 before its next 16 bytes were read: the head took 49 us there at n = 800, 21 us in this
  //      form; 784-100-47: 7.4 -> 5.7 us -- docs/PERFORMANCE.md "Many classes")
  accv_t acc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = accv_t{0, 0, 0, 0};
  const int nch = (H + 15) >> 4, cpw = (nch + kMcWaves - 1) / kMcWaves;
  const int kbeg = w * cpw * 16, kend = min(H, (w + 1) * cpw * 16);
  for (int kc = kbeg; kc < kend; kc += 16 * kMcU) {
    P xa[kMcU][4], wa[kMcU][NCT][4];
#pragma unroll
    for (int u = 0; u < kMcU; ++u) {
      const int k = kc + 16 * u + 4 * g;
      load_frag<P, 4, false, 0>(ra, a.lda, col, a.n, k, kend, xa[u]);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) load_frag<P, 4, true, VEC>(rw, H, 16 * ct + c16, C, k, kend, wa[u][ct]);
    }
    __builtin_amdgcn_sched_barrier(0);  // the burst's loads stay ahead of its first MFMA (mma_tile.h)
#pragma unroll
    for (int u = 0; u < kMcU; ++u)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) Tr::mma(wa[u][ct], xa[u], acc[ct]);
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) zp[w][ct][i][lane] = acc[ct][i];
  __syncthreads();  // (the only barrier: every thread of the workgroup reaches it)

  // ---- z2 in every wave: the four partial sets in wave order, then b2
  P z[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      P v = zp[0][ct][i][lane];
#pragma unroll
      for (int q = 1; q < kMcWaves; ++q) v += zp[q][ct][i][lane];
      z[ct][i] = v + bias[ct][i];
    }

  if (a.mode == HEAD_PREDICT) {  // the first maximum: classes ascend with (ct, i) in a lane, ties -> the lower class
    if (w != 0 || !first) return;
    P bv = P(0);
    int best = kMcCMax;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cls = 16 * ct + Tr::row(g, i);
        const bool take = cls < C && (best == kMcCMax || z[ct][i] > bv || (z[ct][i] == bv && cls < best));
        bv = take ? z[ct][i] : bv;
        best = take ? cls : best;
      }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const P ov = __shfl_xor(bv, o, 64);
      const int ob = __shfl_xor(best, o, 64);
      const bool take = ob < kMcCMax && (best == kMcCMax || ov > bv || (ov == bv && ob < best));
      bv = take ? ov : bv;
      best = take ? ob : best;
    }
    if (g == 0 && cval) a.pred[col] = best;
    return;
  }

  // ---- softmax over the C classes of column c16 (4 lane groups x NCT x 4 registers)
  P m = P(0);
  if (a.shift) {
    bool any = false;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (16 * ct + Tr::row(g, i) < C) {
          m = any ? mc_max<P>(m, z[ct][i]) : z[ct][i];
          any = true;
        }
    // (class 0 is in lane group 0: every column has a valid entry there)
    P mo = any ? m : (std::is_same_v<P, float> ? P(-3.402823466e38f) : P(-1.7976931348623157e308));
    mo = mc_max<P>(mo, __shfl_xor(mo, 16, 64));
    mo = mc_max<P>(mo, __shfl_xor(mo, 32, 64));
    m = mo;
  }
  P ssum = P(0), zl = P(0);  // zl: the label's shifted logit, in the lane that holds it (head_nll)
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cls = 16 * ct + Tr::row(g, i);
      const P zm = z[ct][i] - m;
      zl = cls == lab ? zm : zl;
      z[ct][i] = cls < C ? mc_exp<P>(zm) : P(0);
      ssum += z[ct][i];
    }
  ssum += __shfl_xor(ssum, 16, 64);
  ssum += __shfl_xor(ssum, 32, 64);
  const P inv = P(1) / ssum;

  if (a.mode == HEAD_PROBS) {
    if (w != 0 || !first || !cval) return;
    P* probs = static_cast<P*>(a.probs);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cls = 16 * ct + Tr::row(g, i);
        if (cls < C) probs[(size_t)cls * a.ldp + col] = z[ct][i] * inv;
      }
    return;
  }

  // ---- train: D = (yhat - onehot) * scale, the loss partial of these 16 columns
  const P sc = P(a.scale);
  float lp = 0.f;
  P d[NCT][4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cls = 16 * ct + Tr::row(g, i);
      const P yh = z[ct][i] * inv;
      const bool hit = cval && cls == lab;
      if (hit) lp = (float)head_nll(ssum, zl);
      d[ct][i] = (cval && cls < C) ? (yh - (hit ? P(1) : P(0))) * sc : P(0);
    }
  if (w == 0 && first) {
    P* Dg = static_cast<P*>(a.D);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cls = 16 * ct + Tr::row(g, i);
        if (cval && cls < C) Dg[(size_t)cls * a.ldd + col] = d[ct][i];
      }
    if (a.loss_partial) {
      const float v = wave_sum(lp);
      if (lane == 0) a.loss_partial[vb] = v;  // (vb * 16 < n: the grid has cdiv(n, 16) column blocks)
    }
  }

  // ---- pass 2: dZ1 = (W2^T D) .* a1 .* (1 - a1); row tiles blockIdx.y * 4 + w, then every 4 * gridDim.y
  P* dZ1 = static_cast<P*>(a.dZ1);
  __hip_bfloat16* dZlo = static_cast<__hip_bfloat16*>(a.dZ1_bf16);
  __hip_bfloat16* dZp = static_cast<__hip_bfloat16*>(a.dZ1_planes);
  const size_t pstride = (size_t)H * a.ldz;
  const int ntile = (H + 15) >> 4;
  for (int mt = (int)blockIdx.y * kMcWaves + w; mt < ntile; mt += kMcWaves * (int)gridDim.y) {
    const int hA = mt * 16 + c16;
    P wv[NCT][4], xe[4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cls = 16 * ct + Tr::row(g, i);
        wv[ct][i] = buf_load1<P>(rw, (cls < C && hA < H) ? (cls * H + hA) * SZ : kOOB);
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = mt * 16 + Tr::row(g, j);
      xe[j] = buf_load1<P>(ra, (h < H && cval) ? (h * a.lda + col) * SZ : kOOB);
    }
    __builtin_amdgcn_sched_barrier(0);
    accv_t r = accv_t{0, 0, 0, 0};
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) mfma4<P>(wv[ct][i], d[ct][i], r);
    if (!cval) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = mt * 16 + Tr::row(g, j);
      if (h >= H) continue;
      const P x = xe[j];
      const P dz = r[j] * x * (P(1) - x);
      const size_t zi = (size_t)h * a.ldz + col;
      if (dZ1) dZ1[zi] = dz;  // nullptr: fp32 dZ1 not needed (planes only)
      if (dZlo) dZlo[zi] = __float2bfloat16((float)dz);
      if (dZp) {  // exact split into npz bf16 planes (mlp_split.h)
        float rr = (float)dz;
        for (int p = 0; p < a.npz; ++p) {
          const __hip_bfloat16 q = __float2bfloat16(rr);
          dZp[p * pstride + zi] = q;
          rr -= __bfloat162float(q);
        }
      }
    }
  }
}

template <typename P>
void launch_head_mc(const HeadArgs& a, hipStream_t s) {
  const int ncb = mc_cdiv(a.n, kMcCols);
  // pass 2's row tiles over enough workgroups to cover the device when the column blocks alone do not
  int nrb = 1;
  if (a.mode == HEAD_TRAIN) {
    const int want = mc_cdiv(device_cu_count(), ncb), most = mc_cdiv(mc_cdiv(a.H, 16), kMcWaves);
    nrb = want < 1 ? 1 : (want > most ? most : want);
  }
  const dim3 grid(ncb, nrb);
  const int nct = mc_cdiv(a.C, 16);
  // W2 rows as 16-byte vectors, each whole or out of range: H % 4 == 0 and a 16-byte aligned W2 (else element loads)
  const bool vec = a.H % 4 == 0 && mc_al16(a.W2);
#define CME_MC_HEAD(nc)                                                  \
  if (vec) head_mc_kernel<P, nc, 1><<<grid, kMcThreads, 0, s>>>(a); \
  else head_mc_kernel<P, nc, 0><<<grid, kMcThreads, 0, s>>>(a);
  if (nct <= 2) { CME_MC_HEAD(2) } else if (nct == 3) { CME_MC_HEAD(3) } else { CME_MC_HEAD(4) }
#undef CME_MC_HEAD
  CME_LAUNCH_CHECK(s);
}

// ------------------------------------------------ the output layer's weight gradients (split path, C > 16)
constexpr int kMcKS = 8, kMcWT = 64 * kMcKS;  // wgrad_roles' kWKS / kWT

template <int VEC>
__global__ __launch_bounds__(kMcWT) void out_wgrad_mc_kernel(SplitStepArgs a, int t2, int t2n) {
  __shared__ __attribute__((aligned(16))) float red[kMcKS * 4 * 64];
  const float reg = (float)a.reg, lr = (float)a.lr;
  const int bid = blockIdx.x;
  if (bid < t2) {  // ---- dW2 = D a1^T: one 16 x 16 tile per workgroup, the 8 waves split K = batch
    TileGeom g{a.C, a.H, a.n, (bid / t2n) * 16, (bid % t2n) * 16};
    EpiW2 epi{a.W2, a.gW2, a.H, a.sgd, 0, reg, lr, {}, a.ag_err};
    wsk_tile<float, 1, 1, kMcKS, true, true, VEC, 8>(a.D, a.ld, a.a1, a.ld, g, epi, red);
    return;
  }
  // ---- bias gradients: one wave per row; rows [0, H) -> db1 from dZ1, [H, H + C) -> db2 from D
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = (bid - t2) * kMcKS + wv + (a.bias_col ? a.H : 0);  // db1 fused into dW1: db2 rows only
  if (row >= a.H + a.C) return;
  const bool first = row < a.H;
  const float* src = first ? a.dZ1 + (size_t)row * a.ld : a.D + (size_t)(row - a.H) * a.ld;
  const float bpre = buf_load1<float>(make_rsrc(first ? a.b1 : a.b2), (first ? row : row - a.H) * 4);
  const int perr = ag_err_load(a.ag_err);
  const float s = wave_sum(row_sum(src, a.n, lane));
  if (lane == 0) {
    float* bp = first ? a.b1 : a.b2;
    const int r = first ? row : row - a.H;
    if (a.sgd && !poisoned(perr)) bp[r] = bpre - lr * s;
    else (first ? a.gb1 : a.gb2)[r] = s;
  }
}

}  // namespace

void mlp_head_mc(DType dt, const HeadArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  CME_REQUIRE(a.C > 16 && a.C <= kMcCMax && a.H >= 1, "mlp_head_mc: 17 <= C <= 64 and H >= 1 required");
  CME_REQUIRE(a.dz_swz == 0 && a.z2_chunks == 0 && a.dw2part == nullptr,
              "mlp_head_mc: the fused forms (fragment-ordered dZ1, z2 partials from the forward, dW2 partials) "
              "exist for C <= 16 only");
  CME_REQUIRE(a.lda >= a.n, "mlp_head_mc: lda < n");
  const int64_t sz = dt == DType::F64 ? 8 : 4;
  CME_REQUIRE((int64_t)a.H * a.lda * sz < (int64_t)kOOB && (int64_t)a.C * a.H * sz < (int64_t)kOOB &&
                  (int64_t)a.n * 4 < (int64_t)kOOB,
              "mlp_head_mc: operand too large for 32-bit buffer offsets");
  if (a.mode == HEAD_TRAIN)
    CME_REQUIRE(a.labels && a.D && a.ldd >= a.n && (a.dZ1 || a.dZ1_bf16 || a.dZ1_planes) && a.ldz >= a.n,
                "mlp_head_mc: train mode needs labels, D and a dZ1 output with ldd, ldz >= n");
  else if (a.mode == HEAD_PREDICT) CME_REQUIRE(a.pred != nullptr, "mlp_head_mc: predict mode needs pred");
  else CME_REQUIRE(a.mode == HEAD_PROBS && a.probs && a.ldp >= a.n, "mlp_head_mc: probs mode needs probs, ldp >= n");
  if (dt == DType::F64) launch_head_mc<double>(a, s);
  else launch_head_mc<float>(a, s);
}

void mlp_out_wgrad_mc(const SplitStepArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  CME_REQUIRE(a.C > 16 && a.C <= kMcCMax, "mlp_out_wgrad_mc: 17 <= C <= 64 required");
  CME_REQUIRE(a.xf_world == 0 && !a.dw2part,
              "mlp_out_wgrad_mc: the all-reduce fused into the weight-gradient launch and the head's dW2 partials "
              "exist for C <= 16 only");
  CME_REQUIRE((int64_t)a.H * a.ld * 4 < (int64_t)kOOB && (int64_t)a.C * a.ld * 4 < (int64_t)kOOB &&
                  (int64_t)a.C * a.H * 4 < (int64_t)kOOB,
              "mlp_out_wgrad_mc: operand too large for 32-bit buffer offsets");
  CME_REQUIRE(a.ld >= a.n && a.D && a.a1 && (a.bias_col || a.dZ1), "mlp_out_wgrad_mc: D, a1 (and dZ1) with ld >= n");
  const int t2n = mc_cdiv(a.H, 16), t2 = mc_cdiv(a.C, 16) * t2n;
  const int tb = mc_cdiv((a.bias_col ? 0 : a.H) + a.C, kMcKS);
  // 16-byte K-contiguous vectors of D and a1 (whole or out of range: n % 4 == 0, 16-byte aligned rows)
  const bool vec = a.n % 4 == 0 && a.ld % 4 == 0 && mc_al16(a.D) && mc_al16(a.a1);
  if (vec) out_wgrad_mc_kernel<1><<<t2 + tb, kMcWT, 0, s>>>(a, t2, t2n);
  else out_wgrad_mc_kernel<0><<<t2 + tb, kMcWT, 0, s>>>(a, t2, t2n);
  CME_LAUNCH_CHECK(s);
}

}  // namespace cme
