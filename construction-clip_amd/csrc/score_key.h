// The ordering key of the scoring kernels: an fp32 score as an unsigned whose integer order is the score's order.
// embed_topk.hip and lm_score.hip (through score_tiles.h) rank by score_key, NaN below every number; caption_select.hip and
// sample_rows.hip rank by mono_bits alone, a total order on every bit pattern in which a NaN keeps the place of its bits.
// Also the cross-lane steps on such keys and on per-row sums: the 64-bit xor shuffle, and the butterfly over the 16 lanes
// li = 0 .. 15 of a lane group in the fixed order xor 1, 2, 4, 8 (both partners compute the same bits; float sums depend on it),
// and the sum over a 256-thread work-group.  (Not in cclip_common.h: the tuned GEMM table is keyed by that file's bytes.)
#pragma once
#include "cclip_common.h"

namespace CCLIP_NS {

typedef unsigned long long u64;

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


__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 group_max_key(u64 v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) { const u64 p = shfl_xor64(v, o); v = v > p ? v : p; }
  return v;
}
template <class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The sum of one value per thread of a 256-thread work-group, in every thread, in a fixed tree: the xor butterfly inside a wave
// (every lane holds the same bits), then the four waves in ascending order through red (4 floats of LDS).  A second call on the
// same red needs a barrier in between.
__device__ __forceinline__ float block_sum4(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace CCLIP_NS
