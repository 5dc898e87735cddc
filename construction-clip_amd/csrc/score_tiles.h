// The streamed-tile parts of the scoring kernels (every kernel on score_sweep.h, plus the two-product kernels on
// score_pair.h, which run their own tile loops on these parts).  A work-group of four waves keeps 64 * MT
// operand rows as MFMA A fragments in registers and streams a [rows][D] 16-bit matrix through LDS in tiles of GT rows:
// row-major, 16-byte chunk c of row r stored at chunk c ^ (r & mask) - the swizzle of attention_tiles.h at row length D,
// conflict-free for the B-fragment reads.  Lane (li, g) of a wave holds the operand rows 4g .. 4g+3 against tile row
// 16 st + li of sub-tile st, and every score is ONE accumulator chain over d = 0, 32, 64 .. in that order.
// The tile loop, its buffers and its barriers are score_sweep.h's; what a kernel does with acc[][] is its own.
//   KSMAX: k-steps of 32 the A fragments are sized for (D <= 32 KSMAX); MT: operand tiles of 16 rows per wave; GT: rows per tile
#pragma once
#include "cclip_common.h"
#include "score_key.h"

namespace CCLIP_NS {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // one 16-byte chunk

struct TileGeom {
  int nks, cpr, rowbytes, swz;                    // k-steps; 16-byte chunks per row; bytes per row; swizzle mask
  __device__ __forceinline__ explicit TileGeom(int D) : nks(D >> 5), cpr(D >> 3), rowbytes(D * 2) {
    const int low = cpr & -cpr;                   // swizzle over the largest power of two (<= 16) dividing a row's chunks
    swz = (low > 16 ? 16 : low) - 1;
  }
  // byte offset of chunk ch of tile row `row`: the one place the store and the B-fragment read take it from
  __device__ __forceinline__ int off(int row, int ch) const { return row * rowbytes + ((ch ^ (row & swz)) << 4); }
};

// A fragments of the wave's rows row0 .., clamped to last_row: a row beyond it is loaded, never out of bounds
template <int KSMAX, int MT>
__device__ __forceinline__ void load_a_frags(bf16x8 (&af)[MT][KSMAX], const bf16* base, long ld, int row0, int last_row, int nks,
                                             int lane) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = min(row0 + 16 * mt + li, last_row);
    const bf16* p = base + (long)row * ld + 8 * g;
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks)
      if (ks < nks) af[mt][ks] = *(const bf16x8*)(p + 32 * ks);
  }
}

// Moves tiles global -> registers -> LDS, so that the next tile's 16-byte loads are in flight while the current one is multiplied
template <int KSMAX, int GT>
struct TileMover {
  static constexpr int IT = GT * KSMAX * 4 / 256; // 16-byte chunks of a tile per thread, at most
  int where[IT];                                  // (row << 8) | chunk of the it-th chunk this thread moves (beyond the tile: loaded, not kept)
  u32x4 stage[IT];
  const TileGeom geo; const int tid;
  __device__ __forceinline__ TileMover(const TileGeom& geo_, int tid_) : geo(geo_), tid(tid_) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = tid + 256 * it;
      where[it] = idx < GT * geo.cpr ? ((idx / geo.cpr) << 8) | (idx % geo.cpr) : 0;
    }
  }
  // the tile that starts at row row_base; rows beyond last_row are clamped, never read out of bounds
  __device__ __forceinline__ void fetch(const bf16* base, long ld, int row_base, int last_row) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int row = min(row_base + (where[it] >> 8), last_row);
      stage[it] = *(const u32x4*)(base + (long)row * ld + (where[it] & 255) * 8);
    }
  }
  __device__ __forceinline__ void store(char* tile) const {
#pragma unroll
    for (int it = 0; it < IT; ++it)
      if (tid + 256 * it < GT * geo.cpr) *(u32x4*)(tile + geo.off(where[it] >> 8, where[it] & 255)) = stage[it];
  }
};

// acc[mt][st] = the wave's operand tile mt against sub-tile st of the tile
template <int KSMAX, int MT, int GT>
__device__ __forceinline__ void tile_multiply(f32x4 (&acc)[MT][GT / 16], const bf16x8 (&af)[MT][KSMAX], const char* tile,
                                              const TileGeom& geo, int lane) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int st = 0; st < GT / 16; ++st) acc[mt][st] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KSMAX; ++ks) {
    if (ks >= geo.nks) continue;
#pragma unroll
    for (int st = 0; st < GT / 16; ++st) {
      const bf16x8 bfrag = *(const bf16x8*)(tile + geo.off(16 * st + li, 4 * ks + g));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt][st] = CCLIP_MFMA_16x16x32(af[mt][ks], bfrag, acc[mt][st]);
    }
  }
}

// Launch of a 256-thread partial kernel with `lds` bytes of dynamic LDS; above 64 KB the kernel has to be told first
template <class Args>
static int score_launch(void (*kernel)(const Args), dim3 grid, size_t lds, const Args& a, hipStream_t stream) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return CCLIP_ERR_LAUNCH;
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, a);
  return CCLIP_OK;
}

// The contract every C entry checks: the row length D, one 16-bit operand [rows][D] with row stride ldx (elements), two of them
static inline bool score_dim_ok(int32_t D) { return !(D < 32 || (D & 31) || D > 1024); }
static inline bool score_operand_ok(const void* x, int64_t ldx, int32_t D) { return !((ldx & 7) || ldx < D || ((uintptr_t)x & 15)); }
static inline bool score_operands_ok(const void* a, int64_t lda, const void* b, int64_t ldb, int32_t D) {
  return score_dim_ok(D) && score_operand_ok(a, lda, D) && score_operand_ok(b, ldb, D);
}
// a scalar parameter that is a number: neither NaN nor an infinity
static inline bool score_finite(float v) { return v == v && v < __builtin_huge_valf() && v > -__builtin_huge_valf(); }

}  // namespace CCLIP_NS
