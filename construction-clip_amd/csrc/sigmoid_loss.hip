// Pairwise sigmoid (SigLIP) row loss (fp32 throughout): the sibling of xent_rows_classes_kernel (class_loss.hip) for the
// objective that scores every (row, column) cell on its own.
//
//   sigmoid_rows : row r carries class row_class[r], column c carries class col_class[c], b = *bias_dev, u = row[c] + b and
//                  y = +1 when row_class[r] >= 0 and col_class[c] == row_class[r], else -1 (a negative column class never
//                  equals a non-negative row class, so such a column is a plain negative).  For a labelled row:
//                    loss_row = sum_c softplus(-y u)
//                    dlogits  = -y sigmoid(-y u) * grad_scale
//                    rowdot   = sum_c dlogits[c] * row[c]        (row, not u: the bias does not scale with logit_scale)
//                    rowsum   = sum_c dlogits[c]                 (the row's part of d/d bias)
//                  and for an unlabelled one (row_class[r] < 0) all four are zero.  For every row:
//                    pred = argmax(row) (first maximum);  hit = row_class[r] >= 0 && col_class[pred] == row_class[r]
//                  The pairwise form is the same kernel with row ids rank * N_loc + r and column ids 0 .. C-1.
//
// Unlike the softmax kernels there is no row statistic to wait for: loss, gradient and the row sums come out of ONE sweep, each
// element read once and written once.  Shape, grid cap and the sweep are row_kernels.h's; why col_class is read directly
// (through L2) is in class_loss.hip.
//
// Numerics.  With x = -y u, e = exp(-|x|) in (0, 1] and w = 1 + e:
//   softplus(x) = max(x, 0) + log1p(e),    sigmoid(x) = x >= 0 ? 1 / w : e / w
// so nothing overflows at either end (|u| = 100: loss terms |u| and 0, gradients grad_scale and 0).  log1p(e) is taken as
// log(w) + (e - (w - 1)) / w: w - 1 and e - (w - 1) are exact, and the second term is the first order of log((1 + e) / w), the
// part of e that rounding 1 + e to w dropped (all of e once e < 2^-24, where log(w) = 0).
#include "row_kernels.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

// `dlogits` may alias `logits` (row_kernels.h, sweep_row4_store): nothing of a row is read twice.
template <bool GRAD>
__global__ __launch_bounds__(256) void sigmoid_rows_kernel(const float* logits, long ld, int R, int C,
                                                           const int* __restrict__ row_class,
                                                           const int* __restrict__ col_class,
                                                           const float* __restrict__ bias_dev, float grad_scale,
                                                           float* __restrict__ loss_row, int* __restrict__ pred,
                                                           float* __restrict__ hit, float* dlogits, long ldd,
                                                           float* __restrict__ rowdot, float* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float bias = *bias_dev;
  for (int r = blockIdx.x * 4 + wave; r < R; r += gridDim.x * 4) {
    const float* row = logits + (long)r * ld;
    float* drow = GRAD ? dlogits + (long)r * ldd : nullptr;
    const int cls = row_class[r];
    const bool labelled = cls >= 0;
    float m = -__builtin_inff(), loss = 0.f, dot = 0.f, sum = 0.f;
    int arg = 0x7fffffff;
    // one cell: the running (max, argmax) of the row, its loss term, and its gradient (returned; summed into dot and sum)
    sweep_row4_store<GRAD>(row, col_class, drow, lane, C, [&](float v, int k, int c) {
      if (v > m) { m = v; arg = c; }
      const bool pos = labelled && k == cls;
      const float u = v + bias, ax = fabsf(u);
      const float e = __expf(-ax), w = 1.f + e, rw = __builtin_amdgcn_rcpf(w);
      const float l1p = __logf(w) + (e - (w - 1.f)) * rw;
      const bool up = pos ? u < 0.f : u > 0.f;                  // x = -y u > 0 (at x == 0 both branches agree)
      loss += (up ? ax : 0.f) + l1p;
      const float sg = up ? rw : e * rw;                        // sigmoid(x)
      const float d = labelled ? (pos ? -sg : sg) * grad_scale : 0.f;
      dot += d * v;
      sum += d;
      return d;
    });
    wave_argmax(m, arg);
    if (loss_row) { loss = wave_sum(loss); if (lane == 0) loss_row[r] = labelled ? loss : 0.f; }
    if (lane == 0) store_pred_hit(r, arg, C, pred, hit, [=] { return labelled && col_class[arg] == cls; });
    if (GRAD) {
      if (rowdot) { dot = wave_sum(dot); if (lane == 0) rowdot[r] = dot; }
      if (rowsum) { sum = wave_sum(sum); if (lane == 0) rowsum[r] = sum; }
    }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_sigmoid_rows(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* row_class,
                                  const int32_t* col_class, const float* bias_dev, float grad_scale, float* loss_row,
                                  int32_t* pred, float* hit, float* dlogits, int64_t ldd, float* rowdot, float* rowsum,
                                  hipStream_t stream) {
  if (!row_loss_shape_ok(logits, R, C, ld, dlogits, ldd) || !row_class || !col_class || !bias_dev) return CCLIP_ERR_ARG;
  // without a gradient the kernel reads none of dlogits, ldd, rowdot, rowsum
  return launch_rows4(dlogits ? sigmoid_rows_kernel<true> : sigmoid_rows_kernel<false>, R, stream, logits, ld, R, C, row_class,
                      col_class, bias_dev, grad_scale, loss_row, pred, hit, dlogits, ldd, rowdot, rowsum);
}
