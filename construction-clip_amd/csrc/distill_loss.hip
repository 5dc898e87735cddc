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
// second reads both rows again (from L2 at the head's sizes) for the loss, the gradient and rowdot.  Shape and grid cap are
// class_loss.hip's; the teacher row stands where its col_class vector stood: lane l reads g[c] with the coalesced index of l[c],
// four columns per trip with all eight loads issued before the first use.
//
// Numerics.  Both log-probabilities are formed as (v - m) - log(s), not v - (m + log(s)): at logits of a few hundred the sum
// m + log(s) rounds to 3e-5, which every probability of the row would carry as a relative error and the loss a hundredfold;
// v - m is exact near the maximum, where the probabilities are.  The two rows go through the same operations, so a teacher row
// equal to the student's gives a == b bit for bit: loss and gradient exactly 0.  A teacher cell of -inf has p_t = exp(-inf) = 0 and is skipped (0 * inf
// would be NaN); it is also kept out of the running sum while the maximum is still -inf (exp(-inf - -inf) likewise).  The skip
// tests p_t == 0, which NaN fails: a NaN anywhere in either row reaches lse, hence every cell, hence loss_row of that row alone.
// A row without a maximum (all NaN, all -inf) keeps arg = INT_MAX >= C, as in the siblings; such a row agrees with nothing.
#include "row_kernels.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

// `dlogits` may alias `logits` (clip/loss.py overwrites the logits with their gradient in place), so neither carries
// __restrict__: a wave owns its row, sweep one stores nothing, and in sweep two every element is read by the lane that later
// writes it and nothing of the row is read again.  `teacher` is never written.
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
    // one cell of a row's online (max, sum, argmax), as xent_rows_classes_kernel; v == -inf adds exp(-inf) = 0 whatever m is
    auto online = [](float v, int c, float& m, float& s, int& arg) {
      if (v > m) { s = s * __expf(m - v) + 1.f; m = v; arg = c; }
      else if (!(v == -__builtin_inff())) s += __expf(v - m);
    };
    int c = lane;
    for (; c + 192 < C; c += 256) {
      const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
      const float g0 = trow[c], g1 = trow[c + 64], g2 = trow[c + 128], g3 = trow[c + 192];
      online(v0, c, ml, sl, argl); online(v1, c + 64, ml, sl, argl); online(v2, c + 128, ml, sl, argl); online(v3, c + 192, ml, sl, argl);
      online(g0, c, mg, sg, argg); online(g1, c + 64, mg, sg, argg); online(g2, c + 128, mg, sg, argg); online(g3, c + 192, mg, sg, argg);
    }
    for (; c < C; c += 64) { online(row[c], c, ml, sl, argl); online(trow[c], c, mg, sg, argg); }
    wave_softmax_argmax(ml, sl, argl);
    wave_softmax_argmax(mg, sg, argg);
    if (lane == 0) {
      if (pred) pred[r] = argl;
      if (agree) agree[r] = (argl < C && argl == argg) ? 1.f : 0.f;          // arg >= C: a row without a maximum (all NaN)
    }
    if (!GRAD && !loss_row) continue;
    const float logsl = __logf(sl), logsg = __logf(sg);
    float* drow = GRAD ? dlogits + (long)r * ldd : nullptr;
    float loss = 0.f, dot = 0.f;
    // one cell: its loss term, and its gradient (returned; summed into dot)
    auto step = [&](float v, float g) {
      const float a = (g - mg) - logsg, b = (v - ml) - logsl;               // v - lse, without rounding lse to the size of m
      const float pt = __expf(a);
      loss += pt == 0.f ? 0.f : pt * (a - b);
      const float d = (__expf(b) - pt) * grad_scale;
      dot += d * v;
      return d;
    };
    c = lane;
    for (; c + 192 < C; c += 256) {             // every element is read before the (possibly aliasing) write of the same element
      const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
      const float g0 = trow[c], g1 = trow[c + 64], g2 = trow[c + 128], g3 = trow[c + 192];
      const float d0 = step(v0, g0), d1 = step(v1, g1), d2 = step(v2, g2), d3 = step(v3, g3);
      if (GRAD) { drow[c] = d0; drow[c + 64] = d1; drow[c + 128] = d2; drow[c + 192] = d3; }
    }
    for (; c < C; c += 64) {
      const float d = step(row[c], trow[c]);
      if (GRAD) drow[c] = d;
    }
    if (loss_row) { loss = wave_sum(loss); if (lane == 0) loss_row[r] = loss; }
    if (GRAD && rowdot) { dot = wave_sum(dot); if (lane == 0) rowdot[r] = dot; }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_kl_rows(const float* logits, int64_t ld, const float* teacher, int64_t ldt, int32_t R, int32_t C,
                             float grad_scale, float* loss_row, int32_t* pred, float* agree, float* dlogits, int64_t ldd,
                             float* rowdot, hipStream_t stream) {
  if (!logits || !teacher || R <= 0 || C <= 0) return CCLIP_ERR_ARG;
  if (ld < C || ldt < C || (dlogits && ldd < C)) return CCLIP_ERR_ARG;
  if (dlogits)
    hipLaunchKernelGGL(kl_rows_kernel<true>, dim3(grid_rows4(R)), dim3(256), 0, stream, logits, (long)ld, teacher, (long)ldt, R,
                       C, grad_scale, loss_row, pred, agree, dlogits, (long)ldd, rowdot);
  else
    hipLaunchKernelGGL(kl_rows_kernel<false>, dim3(grid_rows4(R)), dim3(256), 0, stream, logits, (long)ld, teacher, (long)ldt, R,
                       C, grad_scale, loss_row, pred, agree, (float*)nullptr, 0L, (float*)nullptr);
  return cclip_launch_status();
}
