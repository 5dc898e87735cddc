// Class-aware row cross-entropy (fp32 throughout): the multi-positive sibling of xent_rows_kernel (loss.hip).
//
//   xent_rows_classes : row r carries class row_class[r], column c carries class col_class[c]; the positives of the row are
//                       P = { c : col_class[c] == row_class[r] }, empty when row_class[r] < 0 (a negative column class never
//                       equals a non-negative row class, so such a column is a plain negative).  With uniform soft targets
//                       over P:
//                         loss_row = lse(row) - mean_{c in P} row[c]                  (0 when P is empty)
//                         pred     = argmax(row) (first maximum);  hit = row_class[r] >= 0 && col_class[pred] == row_class[r]
//                         dlogits  = (softmax(row) - [c in P] / |P|) * grad_scale     (all zero when P is empty)
//                         rowdot   = sum_c dlogits[c] * row[c]
//                       Used for both halves of the class-aware contrastive loss (clip/loss.py, labels=...).
//
// col_class is read through L2 next to the logits, not staged in LDS: a block owns four rows per trip of the grid-stride loop
// (ONE trip at R <= 16384), so a staged copy would be read four times per element after every wave has waited at a barrier for
// the whole vector - and at C = 8192 its 32 KB would cap the CU at five blocks instead of eight.  Read directly, lane l takes
// col_class[c] with the same coalesced index as row[c]; the four waves of a block and every block on the CU hit the same lines.
#include "row_kernels.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

// `dlogits` may alias `logits` (row_kernels.h, sweep_row4_store): the positives' sum is taken in sweep one, before any store.
__global__ __launch_bounds__(256) void xent_rows_classes_kernel(const float* logits, long ld, int R, int C,
                                                                const int* __restrict__ row_class,
                                                                const int* __restrict__ col_class, float grad_scale,
                                                                float* __restrict__ loss_row, int* __restrict__ pred,
                                                                float* __restrict__ hit, float* dlogits, long ldd,
                                                                float* __restrict__ rowdot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
    const float* row = logits + (long)r * ld;
    const int cls = row_class[r];
    const bool labelled = cls >= 0;
    float m = -__builtin_inff(), s = 0.f, psum = 0.f;
    int arg = 0x7fffffff, pcnt = 0;
    // one column: online (max, sum, argmax) exactly as xent_rows_kernel, plus the positives' sum and count
    sweep_row4(row, col_class, lane, C, [&](float v, int k, int c) {
      online_softmax_step<false>(v, c, m, s, arg);
      const bool p = labelled && k == cls;
      psum += p ? v : 0.f;
      pcnt += p ? 1 : 0;
    });
    wave_softmax_argmax(m, s, arg);
    psum = wave_sum(psum);
    pcnt = wave_sum_int(pcnt);
    const float lse = m + __logf(s);
    const bool has = pcnt > 0;
    const float inv = has ? 1.f / (float)pcnt : 0.f;
    if (lane == 0) {
      if (loss_row) loss_row[r] = has ? lse - psum * inv : 0.f;
      store_pred_hit(r, arg, C, pred, hit, [=] { return labelled && col_class[arg] == cls; });
    }
    if (dlogits) {
      float* drow = dlogits + (long)r * ldd;
      const float gs = has ? grad_scale : 0.f;
      float dot = 0.f;
      // d = (softmax - [positive] / |P|) * gs;  has => cls >= 0, and without positives inv = gs = 0
      sweep_row4_store<true>(row, col_class, drow, lane, C, [&](float v, int k, int) {
        const float d = (__expf(v - lse) - (k == cls ? inv : 0.f)) * gs;
        dot += d * v;
        return d;
      });
      if (rowdot) { dot = wave_sum(dot); if (lane == 0) rowdot[r] = dot; }
    }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_xent_rows_classes(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* row_class,
                                       const int32_t* col_class, float grad_scale, float* loss_row, int32_t* pred,
                                       float* hit, float* dlogits, int64_t ldd, float* rowdot, hipStream_t stream) {
  if (!row_loss_shape_ok(logits, R, C, ld, dlogits, ldd) || !row_class || !col_class) return CCLIP_ERR_ARG;
  return launch_rows4(xent_rows_classes_kernel, R, stream, logits, ld, R, C, row_class, col_class, grad_scale, loss_row, pred, hit,
                      dlogits, ldd, rowdot);
}
