// The XCD-local step pipeline (H <= 128, split3, one process): every step of a native step-loop plan in ONE
// persistent launch, with no grid-wide seam anywhere.
//
// The two-launch step (forward + head, then weight gradient) pays at both kernel boundaries of every step: the XCDs
// start a launch 0.6-1.5 us apart and every z2 all-gather waits for the last one (profiles/r5/stamps_fha_per_xcd.jsonl),
// and whatever the previous launch WROTE -- the updated W1, dZ1, the dW2 partials -- is read back at the die-level
// cache's rate, 2.44 us against 0.92 us for an L2-resident 2 MiB (docs/PERFORMANCE.md "Data written by one kernel is
// cold for the next").  Under the XCD-row placement, row tile rt of W1 is both forward-read and updated on XCD rt,
// dZ1 rows rt are written and read there, and so are W2[:, rt rows] and their dW2 partials.  The only cross-XCD
// dependency of a step is the z2 all-gather of the head, already an in-launch hand-off.  So here:
//
//   * every workgroup reads its XCD from HW_REG_XCC_ID and takes a ticket on that XCD's counter: row tile rt = XCD,
//     slot j = ticket (placement decides only which XCD serves which row tile: every hand-off below is between
//     workgroups that read the same XCC id, i.e. that share one L2);
//   * slot j < nw is a worker: the forward + head of tile (rt, column tile j) -- fha_body, the two-launch forward's
//     own body, in its PS form: z2 partials out as data-tagged granules (tag = the plan's step number, slab by step
//     parity), the all-gather, softmax, D, the dW2 partials and dZ1 -- then, each wave once the column tiles it reads
//     have arrived, the dW1 tile (rt, feature tile j) over the whole batch with the fused reg + SGD update of W1 /
//     W1s / b1 (EpiW1, the two-launch epilogue) -- its pixel operand out of the forward's fragment-ordered copy, which
//     this XCD's L2 holds, not the feature-major copy (PIX below);
//   * slot nw is the XCD's role workgroup: once every column tile has arrived it sums the dW2 partials of
//     W2[:, rt rows] (EpiW2) and reduces D into db2 -- redundantly on every XCD, in the same order, into that XCD's own
//     copy of b2 (XCD 0 also writes the master b2 at the plan's last step);
//   * the other slots return at once.  (Idle CUs pulling the pixels each XCD reads next into its L2 -- this step's XT,
//     the next step's X -- measured slower, +1.5 us per step, and so did the workers' own LDS-DMA pull during the z2
//     wait and an LDS-DMA of the dW1 tile's pixels ahead of its GEMM (the DMAs share the in-order vmcnt with the
//     critical loads): profiles/r6/xstep_ab_r6b.jsonl, xstep_ab_r6c_prefetch_rejected.jsonl, xpf_rejected/.)
//
// Synchronisation is XCD-local and has no barrier across workgroups, only the XCD's FLAG LINE (fha_body.h XcdFlags,
// XsBar below): one 32-bit word per slot in a single 128-byte line, written with a PLAIN store -- the line stays in
// this XCD's L2, no trip to the memory-side atomic unit -- holding the tag of the slot's last arrival, 2 (ep0 + s) + b
// for arrival b of step s (tags only grow over the buffer's life, so nothing is ever reset).  Word 31 is the stop word:
// launch + 1 once this launch has stopped.  Valid because every participant of a line is on the XCD whose L2 holds it
// (they all read the same XCC id).  A workgroup arrives twice per step, after its forward + head (b = 0) and after its
// dW1 tile or role (b = 1): it drains its stores (s_waitcnt vmcnt(0) + workgroup barrier) and writes its word.  A
// waiter is one wave polling the line with sc1 loads for just the words it depends on: each dW1 wave the column tiles
// its K range reads (EpiW1Gate), the role every column tile, and each forward wave of the next step the dW1 tiles its
// K range reads (fha_body PsGate; its wave 7, which has no K range, waits for all of them and the role and stages
// b1 / W2 / b2).  (Two full XCD barriers per step on the same line measured 11.0 us per walking step at n = 800, only
// the first of them fine-grained 10.8, this form 9.85, and an atomic counter per XCD in place of the line ~14:
// profiles/r6/xstep_ab_r6i.jsonl.)  Every read of data another workgroup of the launch wrote goes through sc1
// (L1-bypassing, L2-served) loads, so a CU never reuses a stale L1 line, and the producer's plain stores stay in the
// XCD's L2 (bench/micro/xcd_barrier.hip: the same-XCD read-back checked word by word, and priced,
// profiles/r6/xcd_barrier_micro*.jsonl).  Arithmetic and summation orders are those of the two-launch step, so the
// parameters are bitwise equal to it (tests/test_gpu_xstep.py).
// Walking step at n = 800: 9.4-9.5 us against the two-launch loop's 14.0 (profiles/r6/flags/, docs/ROUND6_STATUS.md);
// n = 100 (the row-major form, RM below): 8.90 us against 12.33 (profiles/r6/rm_form/).
//
// Failure semantics: a z2 hand-off wait that outlasts SplitStepArgs::ag_wait_us sets *err and makes its workgroup
// arrive "bad" (it writes the stop word first); every XCD's workgroup of that column tile waits for the same missing
// granule, so every XCD stops there and the step applies nothing (the launch ends; the steps before it stay applied).
// A flag wait that times out (a workgroup that never arrives) sets *err and stops the launch.
// Reference: the hot loop of fpcode/neural_network.cpp:449-555 (forward/backward :281-394) -- here one launch.
#include "mlp_split.h"
#include "mlp_kernels.h"

#include "fha_body.h"
#include "granule.h"
#include "mma_tile.h"
#include "wgrad_epi.h"

namespace cme {

namespace {

using bf16 = __hip_bfloat16;
using namespace wg;

constexpr int kXsWgsPerXcd = 32;                 // 256 CUs / 8 XCDs: one workgroup per CU
constexpr int kXsCols = 32;                      // the forward's column tile (fha_body)

inline int xs_cdiv(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ unsigned xcc_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 15u;
}

// control words: [2 banks][8 XCDs][32] uint64 -- the XCD's ticket at [0] (one 256-byte line each; the launch that
// takes ticket 0 of its bank zeroes the other bank's, for the next launch) ...
__device__ __forceinline__ unsigned long long* xs_ticket(unsigned long long* ctl, int bank, int x) {
  return ctl + ((size_t)bank * 8 + x) * 32;
}
// ... then [8 XCDs][16] uint64: one 128-byte flag line per XCD, never reset
__device__ __forceinline__ unsigned* xs_flags(unsigned long long* ctl, int x) {
  return reinterpret_cast<unsigned*>(ctl + 2 * 8 * 32 + (size_t)x * 16);
}

// One workgroup's end of its XCD's flag line: arrival q of the plan is 2 s + b (step s, b = 0 after the forward +
// head, 1 after the dW1 tile / the role).
struct XsBar {
  XcdFlags flags;
  unsigned ep0;  // the first step's granule tag
  int slot;
  __device__ unsigned tag_of(int q) const { return 2u * (ep0 + (unsigned)(q >> 1)) + (unsigned)(q & 1); }
  // this workgroup's stores drained (every wave), then lane 0 publishes its flag (and the stop word first when its
  // step is bad).  Returns after the workgroup barrier that follows the drain: the flag may still be in flight.
  __device__ void arrive(int q, bool bad) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      if (bad) flags.line[31] = flags.stop_tag;
      flags.line[slot] = tag_of(q);
    }
  }
  // one WAVE (all its lanes): wait until participants [lo, hi) have made arrival q (XcdFlags::wait)
  __device__ bool poll(int q, int lo, int hi) const { return flags.wait(tag_of(q), lo, hi); }
};

// The dW1 tile's epilogue, gated.  Each wave of the tile waits only for the forward + head workgroups whose dZ1
// column tiles its K range reads (samples [kbeg, kend) = column tiles [kbeg / 32, ceil(kend / 32))), not for the
// whole XCD; a wave that sees the launch stop marks the workgroup and the update is then not applied (the K loop's
// reduction barrier orders that mark before the epilogue).
struct EpiW1Gate : EpiW1 {
  const XsBar* bar;
  int q, tn;
  __device__ void before_kloop(int kbeg, int kend) {
    if (kend > kbeg) bar->poll(q, kbeg / kXsCols, min(tn, (kend + kXsCols - 1) / kXsCols));
  }
  __device__ __forceinline__ void operator()(int qq, int row, int col, float v) {
    if (!*bar->flags.s_stop) EpiW1::operator()(qq, row, col, v);
  }
};

// The diagnostics build's gated epilogue: per-wave stamps (s_memrealtime, lane 0) when the wave's gate has passed and
// when its first burst's operands are all back (it waits for them: the stamp perturbs what it measures); wsk_tile's
// own stamps give the tile's entry, K loop done, reduced and epilogue done (XStepPlan::w1stamps).
struct EpiW1GateDiag : EpiW1Gate {
  unsigned long long* ws;  // this wave's two stamps (nullptr: none)
  __device__ void put(int i) {
    const unsigned long long tt = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) ws[i] = tt;
  }
  __device__ void before_kloop(int kbeg, int kend) {
    EpiW1Gate::before_kloop(kbeg, kend);
    if (ws) put(0);
  }
  __device__ void first_operands_back() {
    if (ws) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      put(1);
    }
  }
};

// The samples of a run_steps plan's steps: consecutive global batches of B from gstart0, wrapping to 0 when one
// would pass N_end (MlpStep::run_steps), this rank's shard at +shard_off.  off() is the current step's first sample;
// advance() moves on by one step.
struct XsWalk {
  int64_t gs;
  const XStepPlan& p;
  __device__ explicit XsWalk(const XStepPlan& q) : gs(q.gstart0 + q.B > q.N_end ? 0 : q.gstart0), p(q) {}
  __device__ int64_t off() const { return gs + p.shard_off; }
  __device__ void advance() { gs = gs + 2 * p.B > p.N_end ? 0 : gs + p.B; }
};

// DIAG: the diagnostics instantiation that honours the stamp buffers (XStepPlan::stamps, SplitStepArgs::stamps,
// HeadArgs::stamps) and the hand-off test hook (SplitStepArgs::ag_test_skip); the production one has none of their
// branches (dropping the stamps' took the walking step 9.86 -> 9.55 us, profiles/r6/xstep_ab_r6k_diag_templated.jsonl) (a runtime diagnostics branch in a production
// kernel cost a launch 0.8 us in round 5, profiles/r5/regression_bisect.md).
// RM: the operand form.  0: the fragment-ordered pixels and dZ1 (steps on the 16-sample grid, n % 16 == 0, n >= 257);
// 1 / 2 / 3: the row-major form for every other step -- the forward reads the pixels row-major (fha_body SWZ = 1),
// the head writes fp32 dZ1 row-major and the dW1 tile reads it with sc1 loads, 2 x 16-byte vectors (RM 1, n % 8 == 0)
// or 16-byte pixel pairs (RM 3: a plan on the 16-sample grid, n % 16 == 0) -- the two-launch step's own forms for such
// a step (mlp_split_wgrad vec 1 / 3) -- or, n % 4 == 0, 2 x 16-byte vectors with the tail past n zeroed in registers
// (RM 4: the same MFMA operands as the two-launch step's element loads, vec 2; n = 100 walking step 9.25 -> 8.90 us,
// profiles/r6/rm_form/), so the bits are its bits.
// PIX (RM 0): where the dW1 tile's pixel operand comes from (XStepPlan::pix).  0: the feature-major
// copy XT, as the two-launch step reads it -- the same pixels the forward just pulled, at other addresses, so every
// XCD fetches the batch a second time through the fabric.  1: the forward's fragment-ordered copy, which this XCD's
// L2 holds, transposed through a wave-private LDS region (wsk_tile BLDS; the MFMA operands are the same registers,
// so the bits are the same) -- the default: fabric read requests per step 97.5k -> 60.1k, L2 hit rate 76.6 -> 86.9 %,
// the wave's first operands back 0.64 us sooner, walking step at n = 800 9.42-9.45 -> 9.30-9.34 us
// (profiles/r7/README.md).
template <bool DIAG, int HK, int RM, int PIX>
__global__ __launch_bounds__(512) void xstep_kernel(SplitStepArgs a, HeadArgs h, XStepPlan p, int tm, int tn,
                                                    int t1n) {
  static_assert(PIX == 0 || RM == 0, "the pixels through LDS: the fragment-ordered form");
  constexpr int kSwz = RM == 0 ? 7 : 1;  // fha_body: fragment-ordered W1 (+ pixels and dZ1 in form 0)
  __shared__ __attribute__((aligned(16))) float red[8 * 1 * 2 * 4 * 64];  // both GEMM tiles' K reductions
  __shared__ __attribute__((aligned(16))) unsigned char pixl[PIX ? 8 * 4 * 1024 : 16];  // PIX: 4 KB per dW1 wave
  __shared__ int s_slot, s_stop;
  __shared__ unsigned s_x;
  const int t = threadIdx.x;
  const int bank = (int)(p.launch & 1u);
  if (t == 0) {
    const unsigned x = xcc_id();
    int slot = -1;
    if (x < 8) {
      slot = (int)__hip_atomic_fetch_add(xs_ticket(p.ctl, bank, (int)x), 1ull, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
      if (slot == 0)  // the other bank, for the next launch (the previous launch that used it has ended)
        __hip_atomic_store(xs_ticket(p.ctl, bank ^ 1, (int)x), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_x = x;
    s_slot = slot;
    s_stop = 0;
  }
  __syncthreads();
  const int x = (int)s_x, slot = s_slot;
  if (x >= tm || slot < 0 || slot > p.nw) return;  // (uniform) XCDs past the last row tile, spare CUs
  // the flag line's participants: the workers + the role
  XsBar bar{{xs_flags(p.ctl, x), p.launch + 1u, &s_stop, p.err, (uint32_t)a.ag_wait_us}, p.ep0, slot};
  const int n = a.n, ld = a.ld;
  const float reg = (float)a.reg, lr = (float)a.lr;
  unsigned long long* st = DIAG ? p.stamps : nullptr;  // diagnostics: [step][8][32][4]
  auto stamp = [&](int s, int i) {
    if (st && t == 0 && s < p.stamp_steps)
      st[(((size_t)s * 8 + x) * kXsWgsPerXcd + slot) * 4 + i] = __builtin_amdgcn_s_memrealtime();
  };

  XsWalk w(p);
  for (int s = 0; s < p.count; ++s, w.advance()) {
    const int64_t off = w.off();
    stamp(s, 0);
    // ---- forward + head of tile (x, slot)
    bool bad = false;
    if (slot < p.nw && slot < tn) {
      SplitStepArgs f = a;
      if constexpr (!DIAG) f.stamps = nullptr;  // (fha_body's per-workgroup stamps)
      f.X = p.X0 + off * a.P;
      if constexpr (RM == 0) f.Xs = p.Xs0 + off / 16 * p.xs_tile;
      f.XT = p.XT0 + off;
      HeadArgs hh = h;
      if constexpr (!DIAG) hh.stamps = nullptr;  // (the forward K loop's per-wave stamps)
      hh.labels = p.lab0 + off;
      hh.D = p.Dx + (size_t)x * 16 * ld;  // this XCD's copy of D (the role's db2 reads it)
      hh.b2 = s == 0 ? (const void*)a.b2 : (const void*)(p.b2x + x * 16);
      gran_t* slabs = p.gran + (size_t)(s & 1) * 32 * 8 * 16 * kXsCols;
      // (the previous step's dW1 tiles and role, waited for per wave inside the GEMM)
      const PsGate gate{s > 0 ? &bar.flags : nullptr, bar.tag_of(2 * s - 1), t1n, p.nw};
      bad = !fha_body<3, 3, true, kSwz, true, DIAG, HK>(f, hh, nullptr, slabs, p.err, tm, tn, slot * 8 + x, red, x, slot,
                                                        p.ep0 + (unsigned)s, &gate, &s_stop);
    }  // (a worker without a forward tile: the heads that overwrite what its dW1 tile read waited for it)
    stamp(s, 1);
    bar.arrive(2 * s, bad);  // (the dW1 waves wait for their own column tiles, the role for all of them)
    stamp(s, 2);
    if (slot < p.nw) {
      if (slot < t1n) {  // ---- dW1 tile (x, slot) over the whole batch + reg + SGD (W1, W1s, b1)
        TileGeom g{a.H, a.P + a.bias_col, n, x * 16, slot * 32};
        const EpiW1 e1{a.W1, a.gW1, static_cast<bf16*>(a.W1p), (size_t)a.H * a.P, a.P, 1, 0, reg, lr, a.xscale, {},
                       a.b1, a.gb1, 0, nullptr};
        auto dw1 = [&](auto& epi, unsigned long long* wst) {
          epi.W1s = a.W1s;
          if constexpr (RM == 0 && PIX != 0)
            wsk_tile<bf16, 1, 2, 8, true, true, 3, 4, 3, uint8_t, float, true, false, kSc1, true>(
                a.dZ1, (ld + 63) / 64, p.Xs0 + off / 16 * p.xs_tile, (int)(p.xs_tile / 1024), g, epi, red, 0, wst, pixl,
                a.P);
          else if constexpr (RM == 0)
            wsk_tile<bf16, 1, 2, 8, true, true, 3, 4, 3, uint8_t, float, true, false, kSc1>(
                a.dZ1, (ld + 63) / 64, static_cast<const uint8_t*>(p.XT0) + off, a.ldxt, g, epi, red, 0, wst);
          else
            wsk_tile<bf16, 1, 2, 8, true, true, RM, 4, 3, uint8_t, float, false, false, kSc1>(
                a.dZ1, ld, static_cast<const uint8_t*>(p.XT0) + off, a.ldxt, g, epi, red, 0, wst);
        };
        if constexpr (DIAG) {  // (the last step's stamps stay: [256 workgroups][8 waves][4], then [256][8][2])
          EpiW1GateDiag epi{{e1, &bar, 2 * s, tn},
                            p.w1stamps ? p.w1stamps + 256 * 8 * 4 + ((size_t)blockIdx.x * 8 + (t >> 6)) * 2 : nullptr};
          dw1(epi, p.w1stamps);
        } else {
          EpiW1Gate epi{e1, &bar, 2 * s, tn};
          dw1(epi, nullptr);
        }
      }
    } else {  // (the role reads every column tile's dW2 partials and D: it waits for all of them)
      if (t < 64) bar.poll(2 * s, 0, tn);
      __syncthreads();
    }
    if (slot == p.nw && !s_stop) {  // ---- the role: W2[:, x rows] from the dW2 partials and db2 into this XCD's b2
      // copy, side by side
      // (waves [0, dw): dW2, one element per lane; waves [dw, 8): db2, up to 4 classes per wave with every row's
      // loads in flight at once -- one after the other they were this workgroup's 4.2 us critical path,
      // profiles/r6/xstep_ab_r6a.jsonl)
      const int lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
      const int dw = (16 * a.C + 63) / 64;
      if (wv < dw) {
        const int nct = (n + 15) / 16, e = t, c = e >> 4, hr = x * 16 + (e & 15);
        const bool ok = c < a.C && hr < a.H;
        EpiW2 epi{a.W2, a.gW2, a.H, 1, 0, reg, lr, {}, nullptr};
        epi.prefetch(0, c, hr, ok);
        const __amdgpu_buffer_rsrc_t rp = make_rsrc(a.dw2part);
        float v = 0.f;
        for (int k0 = 0; k0 < nct; k0 += 32) {  // (the two-launch role's summation order: k ascending)
          float pv[32];
#pragma unroll
          for (int u = 0; u < 32; ++u)
            pv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                  rp, (ok && k0 + u < nct) ? (((k0 + u) * 16 + c) * a.H + hr) * 4 : kOOB,
                                                  0, kSc1));
#pragma unroll
          for (int u = 0; u < 32; ++u) v += pv[u];
        }
        if (ok) epi(0, c, hr, v);
      } else {
        // db2 as the two-launch step's bias-row workgroups compute it (row_sum's lane-strided order, then wave_sum)
        const int nd = 8 - dw, c0 = wv - dw;
        const float* b2src = s == 0 ? a.b2 : p.b2x + x * 16;
        const __amdgpu_buffer_rsrc_t rb = make_rsrc(b2src);
        float bpre[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cc = c0 + k * nd;
          bpre[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, cc < a.C ? cc * 4 : kOOB, 0,
                                                                                   kSc1));
        }
        for (int j0 = 0; j0 < n; j0 += 64 * 16) {
          float v[4][16];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int cc = c0 + k * nd;
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.Dx + ((size_t)x * 16 + (cc < a.C ? cc : 0)) * ld);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
              const int jj = j0 + u * 64 + lane;
              v[k][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                      rs, (cc < a.C && jj < n) ? jj * 4 : kOOB, 0, kSc1));
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[k] += v[k][u];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cc = c0 + k * nd;
          const float sum = wave_sum(acc[k]);
          if (cc < a.C && lane == 0) {
            const float nb = bpre[k] - lr * sum;
            p.b2x[x * 16 + cc] = nb;
            if (x == 0 && s + 1 == p.count) a.b2[cc] = nb;
          }
        }
      }
    }
    stamp(s, 3);
    bar.arrive(2 * s + 1, s_stop != 0);  // (the next forward's waves wait for the flags they need)
    if (s_stop) return;
  }
}

}  // namespace

// The row-major form's dW1 vector form (xstep_kernel RM): 1 (n % 8 == 0), 2 (n % 4 == 0), 0 none -- fp32 dZ1 and
// 4-byte pixel rows, as the two-launch weight gradient takes them (mlp_split_wgrad: base_ok, vec)
int mlp_xstep_rm(const SplitStepArgs& a) {
  const bool ok = a.npz == 3 && (a.a_fp32 & 2) && a.dZ1 && ((uintptr_t)a.dZ1 & 15) == 0 && a.ld % 8 == 0 &&
                  ((uintptr_t)a.XT & 3) == 0 && a.ldxt % 4 == 0;
  const bool pairs = ((uintptr_t)a.XT & 15) == 0 && a.ldxt % 16 == 0 && a.n % 16 == 0;
  return !ok ? 0 : a.n % 8 == 0 ? (pairs ? 3 : 1) : a.n % 4 == 0 ? 4 : 0;
}

bool mlp_xstep_ok(const SplitStepArgs& a, const HeadArgs& h) {
  const int tm = xs_cdiv(a.H, 16), tn = xs_cdiv(a.n, kXsCols), t1n = xs_cdiv(a.P + a.bias_col, 32);
  const int nw = std::max(tn, t1n);
  const bool common =
      a.H <= 128 && tm <= 8 && a.C <= 16 && a.bias_col && a.sgd == 1 && a.xf_world == 0 && a.npw == 3 &&
      a.npz == 3 && a.w1_swz && a.W1s && a.dZ1 && h.dZ1 == a.dZ1 && !h.dZ1_planes && a.dw2part &&
      h.dw2part == a.dw2part && a.dw2_cols == 16 && !h.a1 && !a.a1 && !h.loss_partial && a.n > 0 &&
      nw + 1 <= kXsWgsPerXcd && nw + 1 <= 31 && device_cu_count() == 8 * kXsWgsPerXcd &&
      // (the forward GEMM's wave 7 has no K range: the gated forward stages b1 / W2 / b2 there, fha_body PsGate)
      xs_cdiv(xs_cdiv(a.P, 32), 8) * 7 * 32 >= a.P && (int64_t)a.P * a.ldxt < (int64_t)kOOB &&
      (int64_t)xs_cdiv(a.H, 16) * 16 * a.ld < (int64_t)kOOB / 4;
  if (!common) return false;
  if (a.dz_swz == 1)  // the fragment-ordered form
    return a.x_swz && a.Xs && h.dz_swz == 1 && a.n % 16 == 0 && mlp_wgrad_dz_swz_ok(a);
  return a.dz_swz == 0 && h.dz_swz == 0 && !a.x_swz && mlp_xstep_rm(a) > 0;  // the row-major form
}

int mlp_xstep_workers(const SplitStepArgs& a) { return std::max(xs_cdiv(a.n, kXsCols), xs_cdiv(a.P + a.bias_col, 32)); }

void mlp_xstep(const SplitStepArgs& a, const HeadArgs& h, const XStepPlan& p, hipStream_t s) {
  if (p.count <= 0) return;
  CME_REQUIRE(mlp_xstep_ok(a, h), "xstep: the plan's step is not the XCD-local pipeline's shape");
  const int tm = xs_cdiv(a.H, 16), tn = xs_cdiv(a.n, kXsCols), t1n = xs_cdiv(a.P + a.bias_col, 32);
  CME_REQUIRE(p.nw == mlp_xstep_workers(a) && p.nw + 1 <= kXsWgsPerXcd && p.nw + 1 <= 31,
              "xstep: the workers + the role must fit one XCD's CUs and its flag line");
  CME_REQUIRE(p.gran && p.ctl && p.Dx && p.b2x && p.err && p.X0 && p.XT0 && p.Xs0 && p.lab0 && p.xs_tile > 0,
              "xstep: scratch buffers missing");
  const bool grid16 = p.gstart0 % 16 == 0 && p.B % 16 == 0 && p.shard_off % 16 == 0;
  int rm = a.dz_swz ? 0 : mlp_xstep_rm(a);
  if (rm == 3 && !grid16) rm = 1;  // (16-byte pixel pairs need every step's columns 16-byte aligned)
  const int grid = rm ? 4 : 16;
  CME_REQUIRE(p.gstart0 % grid == 0 && p.B % grid == 0 && p.shard_off % grid == 0 && p.B >= a.n && p.N_end >= p.B,
              "xstep: every step must start a 16-sample tile of the fragment-ordered pixels (row-major form: 4-byte "
              "aligned pixel columns)");
  CME_REQUIRE(a.ld >= a.n && a.ld % 16 == 0, "xstep: activation pitch");
  const bool diag = p.stamps || p.w1stamps || a.stamps || h.stamps || a.ag_test_skip >= 0;
  CME_REQUIRE(!rm || !diag, "xstep: the row-major form has no diagnostics build");
  // (pix is honoured by the fragment-ordered form and its diagnostics build; the row-major form reads XT)
  CME_REQUIRE(p.pix == 0 || p.pix == 1, "xstep: the dW1 pixel operand's form is 0 (XT) or 1 (the forward's copy)");
  const dim3 grid_dim(8 * kXsWgsPerXcd), block(512);
  if (rm == 1) xstep_kernel<false, 7, 1, 0><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  else if (rm == 4) xstep_kernel<false, 7, 4, 0><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  else if (rm == 3) xstep_kernel<false, 7, 3, 0><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  else if (diag && p.pix == 1) xstep_kernel<true, 0, 0, 1><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  else if (diag) xstep_kernel<true, 0, 0, 0><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  // (the production form keeps fha_body's three no-op runtime tests, HK = 7: measured 9.55-9.61 us against 9.81-9.86
  // without them and 9.62-9.94 with any one or two -- the compiler schedules the body differently; alternated four
  // and three times on two boxes, profiles/r6/hk/)
  else if (p.pix == 1) xstep_kernel<false, 7, 0, 1><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  else xstep_kernel<false, 7, 0, 0><<<grid_dim, block, 0, s>>>(a, h, p, tm, tn, t1n);
  CME_LAUNCH_CHECK(s);
}

}  // namespace cme
