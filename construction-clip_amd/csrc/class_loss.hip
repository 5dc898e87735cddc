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

// `dlogits` may alias `logits` (clip/loss.py overwrites the logits with their gradient in place), so neither carries
// __restrict__: every element is read by the lane that later writes it, and the positives' sum is taken in pass one,
// before any store.
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
    // one column of the sweep: online (max, sum, argmax) exactly as xent_rows_kernel, plus the positives' sum and count
    auto step = [&](float v, int k, int c) {
      if (v > m) { s = s * __expf(m - v) + 1.f; m = v; arg = c; }
      else s += __expf(v - m);
      const bool p = labelled && k == cls;
      psum += p ? v : 0.f;
      pcnt += p ? 1 : 0;
    };
    int c = lane;
    // four columns per trip, all eight loads issued before the first use: at one wave per SIMD (R = 1024 is four waves per CU)
    // nothing else hides a load's latency, and a column's class fetched only after its logit had arrived cost a second one
    for (; c + 192 < C; c += 256) {
      const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
      const int k0 = col_class[c], k1 = col_class[c + 64], k2 = col_class[c + 128], k3 = col_class[c + 192];
      step(v0, k0, c); step(v1, k1, c + 64); step(v2, k2, c + 128); step(v3, k3, c + 192);
    }
    for (; c < C; c += 64) step(row[c], col_class[c], c);
    wave_softmax_argmax(m, s, arg);
    psum = wave_sum(psum);
    pcnt = wave_sum_int(pcnt);
    const float lse = m + __logf(s);
    const bool has = pcnt > 0;
    const float inv = has ? 1.f / (float)pcnt : 0.f;
    if (lane == 0) {
      if (loss_row) loss_row[r] = has ? lse - psum * inv : 0.f;
      if (pred) pred[r] = arg;
      if (hit) hit[r] = (cls >= 0 && arg < C && col_class[arg] == cls) ? 1.f : 0.f;   // arg >= C: a row without a maximum (all NaN)
    }
    if (dlogits) {
      float* drow = dlogits + (long)r * ldd;
      const float gs = has ? grad_scale : 0.f;
      float dot = 0.f;
      // d = (softmax - [positive] / |P|) * gs;  has => cls >= 0, and without positives inv = gs = 0
      auto grad = [&](float lv, int k) { return (__expf(lv - lse) - (k == cls ? inv : 0.f)) * gs; };
      int c = lane;
      for (; c + 192 < C; c += 256) {           // every element is read before the (possibly aliasing) write of the same element
        const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
        const int k0 = col_class[c], k1 = col_class[c + 64], k2 = col_class[c + 128], k3 = col_class[c + 192];
        const float d0 = grad(v0, k0), d1 = grad(v1, k1), d2 = grad(v2, k2), d3 = grad(v3, k3);
        dot += d0 * v0; dot += d1 * v1; dot += d2 * v2; dot += d3 * v3;
        drow[c] = d0; drow[c + 64] = d1; drow[c + 128] = d2; drow[c + 192] = d3;
      }
      for (; c < C; c += 64) {
        const float lv = row[c];
        const float d = grad(lv, col_class[c]);
        dot += d * lv;
        drow[c] = d;
      }
      if (rowdot) { dot = wave_sum(dot); if (lane == 0) rowdot[r] = dot; }
    }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_xent_rows_classes(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* row_class,
                                       const int32_t* col_class, float grad_scale, float* loss_row, int32_t* pred,
                                       float* hit, float* dlogits, int64_t ldd, float* rowdot, hipStream_t stream) {
  if (!logits || !row_class || !col_class || R <= 0 || C <= 0) return CCLIP_ERR_ARG;
  if (ld < C || (dlogits && ldd < C)) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(xent_rows_classes_kernel, dim3(grid_rows4(R)), dim3(256), 0, stream, logits, (long)ld, R, C, row_class,
                     col_class, grad_scale, loss_row, pred, hit, dlogits, (long)ldd, rowdot);
  return cclip_launch_status();
}
