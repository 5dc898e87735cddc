// What the two-product kernels on score_tiles.h share: embed_cache_bwd, embed_probe's backward, concept_codes and embed_moments
// multiply one streamed LDS tile of 32 rows twice, once in row order and once through the transposed read ds_read_b64_tr_b16,
// and most of their fp32 operands enter the MFMA as a 16-bit hi + lo pair.
//   split16            hi = round16(v), lo = round16(v - hi)                                    (all four, gauss_scores' image)
//   tile_frag_tr       the transposed A-fragment read of a tile image                           (all four)
//   pair_image_kernel  an fp32 matrix as the padded hi / lo image of 32-row tiles               (embed_probe, gauss_scores)
//   opaque_lane, tile_scores_t, tr_accumulate, store_dt_columns
//                      the inner step of a tile where the streamed rows are the k index of the second product and a wave's
//                      16 register-held rows meet them on the lane                              (embed_cache_bwd, embed_probe backward)
// Functions only.  Each kernel keeps its own tile loop: the four fetch, rewrite the staged tile and store at different points
// (dead-row masks, the late fetch above D = 512, label staging, concept_codes' second barrier), and a shared loop cost the
// forward kernels time and registers (score_sweep.h).  The first products of concept_codes (permuted k, bf16x4 pair reads) and
// embed_moments (one-hot operand) are their own.
#pragma once
#include "score_sweep.h"

// every file that includes this sets the same below its includes; what is inlined from here must round as it does there
#pragma clang fp contract(off)

namespace CCLIP_NS {

// v as a pair of 16-bit operands: two MFMAs into one accumulator then lose only the rounding of lo - 2^-16 relative for bf16
// (unit roundoff 2^-8, squared), 2^-22 for fp16
__device__ __forceinline__ void split16(float v, bf16& hi, bf16& lo) {
  hi = (bf16)v;
  lo = (bf16)(v - (float)hi);
}
// the same into element j of an operand pair (a vector element cannot be bound to a reference)
__device__ __forceinline__ void split16(float v, bf16x8& hi, bf16x8& lo, int j) {
  bf16 h, l;
  split16(v, h, l);
  hi[j] = h;
  lo[j] = l;
}

// A-operand fragment of X^T (columns 16 dt .. 16 dt + 15 of the tile image as MFMA rows) over 8 tile rows given as two 4-row
// blocks: attention_tiles.h's frag_tr on score_tiles.h's image.  With rowblk0 = 4 g, rowblk1 = 16 + 4 g element j of lane (li, g)
// is row 16 (j >> 2) + 4 g + (j & 3), column 16 dt + li: the k order of an accumulator of the first product taken as B operand.
// Every address is a chunk offset (a multiple of 16) plus 0 or 8: 8-byte aligned.  Needs EXEC all ones.
__device__ __forceinline__ bf16x8 tile_frag_tr(const char* tile, const TileGeom& geo, int rowblk0, int rowblk1, int dt, int lane) {
  const int qq = (lane >> 2) & 3, p = lane & 3;
  const int chunk = 2 * dt + (p >> 1), sub = 8 * (p & 1);
  const bf16x4 lo = lds_read_tr16(tile + geo.off(rowblk0 + qq, chunk) + sub);
  const bf16x4 hi = lds_read_tr16(tile + geo.off(rowblk1 + qq, chunk) + sub);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The image of an fp32 matrix M [R, D] as MFMA operand pair: rows padded to Rp = 16 ceil(R / 16) and laid out in tiles of 16,
// image rows 32 t .. 32 t + 15 are hi of the rows 16 t .., rows 32 t + 16 .. 32 t + 31 their lo; padding rows are zero.  A tile of
// 32 image rows is one streamed tile of score_tiles.h whose two sub-tiles are the hi chain and the lo chain.  [2 Rp][D] 16-bit.
// (static: every translation unit that launches it has its own copy and the library links them side by side; kernel and
// launcher are templates so that a file that includes this and never calls the launcher carries no copy)
template <int = 0>
static __global__ __launch_bounds__(256) void pair_image_kernel(const float* __restrict__ M, int R, int D, int rpad,
                                                                bf16* __restrict__ img) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)rpad * D) return;
  const int r = (int)(idx / D), d = (int)(idx - (long)r * D);
  bf16 hi, lo;
  split16(r < R ? M[idx] : 0.0f, hi, lo);
  const long row = (long)(r >> 4) * 32 + (r & 15);
  img[row * D + d] = hi;
  img[(row + 16) * D + d] = lo;
}

static inline int pair_image_rows(int R) { return (R + 15) / 16 * 16; }           // Rp; the image takes 4 Rp D bytes

template <int = 0>
static inline void pair_image_launch(const float* M, int R, int D, void* img, hipStream_t stream) {
  const int rpad = pair_image_rows(R);
  const long cells = (long)rpad * D;
  hipLaunchKernelGGL(pair_image_kernel<>, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, M, R, D, rpad, (bf16*)img);
}

// The LDS addresses of a tile are recomputed per tile from an opaque copy of the lane number: hoisted out of the tile loop
// (2 KSMAX + 2 NDT swizzled addresses) they would cost more registers than the accumulator
__device__ __forceinline__ int opaque_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// s[nb][st] = (sub-tile st of the tile)^T-side scores: the tile's row 16 st + 4 g + r on the accumulator row, the wave's
// register-held row li of fragment set nb on the lane; each ONE chain over d = 0, 32, 64 ..  The tile is the A operand.
template <int KSMAX, int NB>
__device__ __forceinline__ void tile_scores_t(f32x4 (&s)[NB][2], const bf16x8 (&bf)[NB][KSMAX], const char* tile, const TileGeom& geo,
                                              int lane) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) s[nb][0] = s[nb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KSMAX; ++ks) {
    if (ks >= geo.nks) continue;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 xf = *(const bf16x8*)(tile + geo.off(16 * st + li, 4 * ks + g));
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) s[nb][st] = CCLIP_MFMA_16x16x32(xf, bf[nb][ks], s[nb][st]);
    }
  }
}

// acc[dt]^T[d, n] += tile^T[d, q] w[q, n] over the 32 rows q of the tile, w = hi + lo with element 4 st + r of a lane the weight
// of tile row 16 st + 4 g + r: k index = (st, g, r) on both operands.  Column tiles dt0 .. dt0 + NDT - 1, those below D.
template <int NDT>
__device__ __forceinline__ void tr_accumulate(f32x4 (&acc)[NDT], const char* tile, const TileGeom& geo, int dt0, int D, bf16x8 hi,
                                              bf16x8 lo, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    if (16 * (dt0 + dt) >= D) continue;           // (wave-uniform)
    const bf16x8 xt = tile_frag_tr(tile, geo, 4 * g, 16 + 4 * g, dt0 + dt, lane);
    acc[dt] = CCLIP_MFMA_16x16x32(xt, hi, acc[dt]);
    acc[dt] = CCLIP_MFMA_16x16x32(xt, lo, acc[dt]);
  }
}

// lane (li, g) holds the columns 16 (dt0 + dt) + 4 g .. + 3 of its row; out = the row + 4 g, value(dt) what is stored of acc[dt]
template <int NDT, class F>
__device__ __forceinline__ void store_dt_columns(float* out, int dt0, int D, F&& value) {
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) {
    const int d = 16 * (dt0 + dt);
    if (d >= D) continue;
    *(f32x4*)(out + d) = value(dt);
  }
}

}  // namespace CCLIP_NS
