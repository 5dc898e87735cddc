// The ordering key of the scoring kernels: an fp32 score as an unsigned whose integer order is the score's order.
// embed_topk.hip and lm_score.hip (through score_tiles.h) rank by score_key, NaN below every number; caption_select.hip and
// sample_rows.hip rank by mono_bits alone, a total order on every bit pattern in which a NaN keeps the place of its bits.
#pragma once
#include "cclip_common.h"

namespace CCLIP_NS {

__device__ __forceinline__ unsigned mono_bits(float x) {
  x += 0.0f;                                      // -0 -> +0: equal fp32 scores share one key
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned score_key(float s) { return s != s ? 0u : mono_bits(s); }   // NaN -> 0, the lowest
__device__ __forceinline__ float key_score(unsigned key) {
  const unsigned b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  return key == 0u ? __uint_as_float(0x7fc00000u) : __uint_as_float(b);
}

}  // namespace CCLIP_NS
