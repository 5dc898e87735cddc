// The LDS image of a [rows][64] 16-bit head slice and its staging, shared by the head_dim-64 attention kernels
// (attention.hip, attention_relevance.hip, attention_relevance_row.hip, attention_probs.hip): 128-byte rows, 16-byte chunk c
// of row r stored at chunk c ^ (r & 7) - conflict-free for both ds_read_b128 row reads and the transposed reads.
#pragma once
#include "cclip_common.h"

namespace CCLIP_NS {

__device__ __forceinline__ int at_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// A-operand fragment of X^T (16 columns d0..d0+15 as MFMA rows) over 8 rows given as two 4-row blocks
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int rowblk0, int rowblk1, int dt, int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3;
  const int chunk = 2 * dt + (p >> 1), sub = 8 * (p & 1);
  const bf16x4 lo = lds_read_tr16(img + at_off(rowblk0 + q, chunk) + sub);
  const bf16x4 hi = lds_read_tr16(img + at_off(rowblk1 + q, chunk) + sub);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 frag_row(const char* img, int row, int chunk) {
  return *(const bf16x8*)(img + at_off(row, chunk));
}

// Staging of a [T][64] head slice into LDS in two halves: head_load issues every 16-byte global load of the slice (IT per
// thread, rows clamped so that no load is predicated) and head_store writes them to the swizzled image, zeroing rows >= T.
// All loads of all operands go out before the first wait: a predicated load -> wait -> ds_write loop costs one HBM round
// trip per iteration (8-10 serial round trips were most of a T=50 workgroup's life, rocprofv3 + ISA).
// g is the head's base pointer (the caller adds h * 64); 256 threads.
template <int IT>
__device__ __forceinline__ void head_load(const bf16* g, long ld, long row0, int T, uint4 (&r)[IT], int tid) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = tid + 256 * it, row = idx >> 3, c = idx & 7;
    r[it] = *(const uint4*)(g + (row0 + (row < T ? row : T - 1)) * ld + c * 8);
  }
}
template <int IT>
__device__ __forceinline__ void head_store(char* img, int T, int rows_total, const uint4 (&r)[IT], int tid) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int idx = tid + 256 * it, row = idx >> 3, c = idx & 7;
    if (row < rows_total) *(uint4*)(img + at_off(row, c)) = row < T ? r[it] : make_uint4(0, 0, 0, 0);
  }
}

// Staging of 64 rows [r0, r0+64) of a [T][64] head slice, split the same way: blk_load requests the thread's
// two 16-byte chunks (rows clamped: no predicated load), blk_store writes them to the swizzled image (zero rows >= T).
// Between the two a kernel keeps the NEXT block's chunks in registers while the current block is multiplied.
__device__ __forceinline__ void blk_load(const bf16* g, long ld, long row0, int r0, int T, uint4 (&r)[2], int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = r0 + (tid >> 3) + 32 * i;
    r[i] = *(const uint4*)(g + (row0 + (row < T ? row : T - 1)) * ld + (tid & 7) * 8);
  }
}
__device__ __forceinline__ void blk_store(char* img, int r0, int T, const uint4 (&r)[2], int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (tid >> 3) + 32 * i;
    *(uint4*)(img + at_off(row, tid & 7)) = r0 + row < T ? r[i] : make_uint4(0, 0, 0, 0);
  }
}

}  // namespace CCLIP_NS
