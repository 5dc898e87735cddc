// Distillation row loss (fp32 throughout): the sibling of xent_rows_classes_kernel (class_loss.hip) and sigmoid_rows_kernel
// (sigmoid_loss.hip) whose target is not a set of positives but a second row of logits, a frozen teacher's.
//
//   kl_rows : l = row r of the student's logits, g = row r of the teacher's (a leading dimension of its own), lse = logsumexp:
//               p_t[c]   = exp(g[c] - lse(g))          p_s[c] = exp(l[c] - lse(l))
//               loss_row = sum_c p_t[c] * ((g[c] - lse(g)) - (l[c] - lse(l)))      KL(teacher || student); p_t == 0 adds 0
//               dlogits  = (p_s - p_t) * grad_scale
//               rowdot   = sum_c dlogits[c] * l[c]
//               pred     = argmax(l) (first maximum);  agree = argmax(l) == argmax(g)
//             Used for both halves of the distillation loss (clip/loss.py, distill_loss).
//
// Two sweeps.  The first takes both rows' online (max, sum of exp, argmax), exactly as xent_rows_classes_kernel takes one; the
// second reads both rows again (from L2 at the head's sizes) for the loss, the gradient and rowdot.  Shape, grid cap and the
// sweep are row_kernels.h's; the teacher row is the sweep's companion vector, where the class kernels have col_class.
//
// Numerics.  Both log-probabilities are formed as (v - m) - log(s), not v - (m + log(s)): at logits of a few hundred the sum
// m + log(s) rounds to 3e-5, which every probability of the row would carry as a relative error and the loss a hundredfold;
// v - m is exact near the maximum, where the probabilities are.  The two rows go through the same operations, so a teacher row
// equal to the student's gives a == b bit for bit: loss and gradient exactly 0.  A teacher cell of -inf has p_t = exp(-inf) = 0
// and is skipped (0 * inf would be NaN); online_softmax_step<true> also keeps it out of the running sum (row_kernels.h).  The
// skip tests p_t == 0, which NaN fails: a NaN anywhere in either row reaches lse, hence every cell, hence loss_row of that row
// alone.  A row without a maximum (all NaN, all -inf) keeps arg = INT_MAX >= C, as in the siblings; such a row agrees with
// nothing.
#include "row_kernels.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

// `dlogits` may alias `logits` (row_kernels.h, sweep_row4_store): a wave owns its row, sweep one stores nothing, and nothing of
// the row is read after sweep two.  `teacher` is never written.
template <bool GRAD>
__global__ __launch_bounds__(256) void kl_rows_kernel(const float* logits, long ld, const float* __restrict__ teacher, long ldt,
                                                      int R, int C, float grad_scale, float* __restrict__ loss_row,
                                                      int* __restrict__ pred, float* __restrict__ agree, float* dlogits,
                                                      long ldd, float* __restrict__ rowdot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
    const float* row = logits + (long)r * ld;
    const float* trow = teacher + (long)r * ldt;
    float ml = -__builtin_inff(), sl = 0.f, mg = -__builtin_inff(), sg = 0.f;
    int argl = 0x7fffffff, argg = 0x7fffffff;
    // two independent online (max, sum, argmax) states, the student's and the teacher's
    sweep_row4(row, trow, lane, C, [&](float v, float g, int c) {
      online_softmax_step<true>(v, c, ml, sl, argl);
      online_softmax_step<true>(g, c, mg, sg, argg);
    });
    wave_softmax_argmax(ml, sl, argl);
    wave_softmax_argmax(mg, sg, argg);
    if (lane == 0) store_pred_hit(r, argl, C, pred, agree, [=] { return argl == argg; });
    if (!GRAD && !loss_row) continue;
    const float logsl = __logf(sl), logsg = __logf(sg);
    float* drow = GRAD ? dlogits + (long)r * ldd : nullptr;
    float loss = 0.f, dot = 0.f;
    // one cell: its loss term, and its gradient (returned; summed into dot)
    sweep_row4_store<GRAD>(row, trow, drow, lane, C, [&](float v, float g, int) {
      const float a = (g - mg) - logsg, b = (v - ml) - logsl;               // v - lse, without rounding lse to the size of m
      const float pt = __expf(a);
      loss += pt == 0.f ? 0.f : pt * (a - b);
      const float d = (__expf(b) - pt) * grad_scale;
      dot += d * v;
      return d;
    });
    if (loss_row) { loss = wave_sum(loss); if (lane == 0) loss_row[r] = loss; }
    if (GRAD && rowdot) { dot = wave_sum(dot); if (lane == 0) rowdot[r] = dot; }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_kl_rows(const float* logits, int64_t ld, const float* teacher, int64_t ldt, int32_t R, int32_t C,
                             float grad_scale, float* loss_row, int32_t* pred, float* agree, float* dlogits, int64_t ldd,
                             float* rowdot, hipStream_t stream) {
  if (!row_loss_shape_ok(logits, R, C, ld, dlogits, ldd) || !teacher || ldt < C) return CCLIP_ERR_ARG;
  // without a gradient the kernel reads none of dlogits, ldd, rowdot
  return launch_rows4(dlogits ? kl_rows_kernel<true> : kl_rows_kernel<false>, R, stream, logits, ld, teacher, ldt, R, C, grad_scale,
                      loss_row, pred, agree, dlogits, ldd, rowdot);
}
