// Evaluation of a resident validation set on the device (eval.hip): loss, hit count and confusion matrix of the
// samples whose a1 a forward GEMM just left, accumulated into a stats slot in device memory.  Nothing is read back
// and nothing is synchronised: an evaluation is kernels on the training stream, legal under graph capture.
//
// A stats slot is mlp_eval_slot_words(C) 8-byte words:
//   [0] n          samples counted                    (uint64)
//   [1] correct    samples with pred == label         (uint64)
//   [2] loss_sum   sum of nll over the samples        (fp64)
//   [3 + label * C + pred]  confusion counts          (uint64; rows are labels, columns are predictions)
// pred is the first maximum of z2 = W2 a1 + b2 over the classes < C (ties -> the lower class) and
// nll = log sum_c exp(z2_c - m) - (z2_label - m), m = max_c z2_c: the same number as -log yhat[label] without the
// log of an underflowed probability -- the form of the training heads' loss partials too (head_math.h head_nll).
//
// One evaluation is one or more chunks enqueued in order on ONE stream; the first (zero = 1) clears the slot, so
// re-enqueueing into a slot overwrites it.  Counts are integer atomics, the loss is fp64 partials summed in index
// order by a one-workgroup kernel: no floating-point atomics, the result is bitwise reproducible.
#pragma once

#include "mlp_kernels.h"

namespace cme {

struct EvalArgs {
  const void* a1;  int lda;          // [H][lda], param dtype (bf16 mode: fp32)
  const void* W2;  const void* b2;   // [C][H], [C]
  const int* labels;                 // [n], each in [0, C)
  int H, C, n;                       // 1 <= C <= 64, any H >= 1
  unsigned long long* stats;         // the slot, mlp_eval_slot_words(C) words
  double* partials;                  // >= mlp_eval_num_partials(n) loss partials (scratch, one per workgroup)
  int zero;                          // 1: the evaluation's first chunk -- the slot is cleared first
};

constexpr int kEvalMaxWgs = 256;  // workgroups (= loss partials) per chunk at most; each walks its column blocks
inline int mlp_eval_num_partials(int n) {
  const int ncb = (n + 15) / 16;
  return ncb < 1 ? 1 : (ncb > kEvalMaxWgs ? kEvalMaxWgs : ncb);
}
inline int64_t mlp_eval_slot_words(int C) { return 3 + (int64_t)C * C; }

// dt: F32 or F64 (BF16 is taken as F32: bf16 mode's a1, W2 and b2 are fp32).  n <= 0 with zero = 1 only clears.
void mlp_eval_head(DType dt, const EvalArgs& a, hipStream_t stream);

}  // namespace cme
