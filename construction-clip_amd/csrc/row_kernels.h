// What the fp32 one-wave-per-row kernels share (loss.hip, class_loss.hip, sigmoid_loss.hip; embed.hip for the grid alone):
// the grid of a four-rows-per-block grid-stride launch and the wave reductions of a row's running (max, sum, argmax).
#pragma once
#include "cclip_common.h"

namespace CCLIP_NS {

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// combine the lanes' (max, first index of it) of one row; ties -> smallest index (torch.argmax returns the first max)
__device__ __forceinline__ void wave_argmax(float& m, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int a2 = __shfl_xor(arg, o, 64);
    if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
  }
}

// combine the lanes' online softmax state (m, s = sum of exp(x - m), arg) of one row; ties -> smallest index
__device__ __forceinline__ void wave_softmax_argmax(float& m, float& s, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const int a2 = __shfl_xor(arg, o, 64);
    const float mn = fmaxf(m, m2);
    s = s * (m == mn ? 1.f : __expf(m - mn)) + s2 * (m2 == mn ? 1.f : __expf(m2 - mn));
    if (m2 > m || (m2 == m && a2 < arg)) arg = a2;
    m = mn;
  }
}

}  // namespace CCLIP_NS

// blocks of a launch in which each of a block's four waves strides over the rows
static inline int grid_rows4(int rows) { int g = (rows + 3) / 4; return g > 4096 ? 4096 : (g < 1 ? 1 : g); }
