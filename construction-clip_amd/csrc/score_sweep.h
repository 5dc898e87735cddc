// What the streamed-score kernels on score_tiles.h share beyond its parts.
// Host side, used by every one of them (embed_topk, embed_range, embed_kmeans assign, embed_hub, embed_cache, embed_probe
// forward, lm_score, mst nearest; the two-product kernels on score_pair.h take the checks):
//   gallery_splits  how the streamed rows are cut into splits
//   row_parts       how the streamed rows are cut into parts with one fp32 partial each (embed_probe backward, embed_moments)
//   score_dispatch  (D, wide) -> <KSMAX, MT, GT>, with or without the 768 rung
//   sweep_launch    grid = row blocks x splits, its 2^31 guard, LDS for the tile buffers
//   segment_of, clamp_index, score_rows_ok   the small change of the same kernels
// (the 16-lane group butterflies are in score_key.h.)
// Device side, used by the two kernels that score the rows of a matrix of up to 2^31 - 1 rows against a streamed one through
// two tile buffers, embed_kmeans' assign kernel, embed_hub's partial kernel and mst's nearest kernel:
//   SweepCtx        lane coordinates, geometry, the work-group's operand rows and its split [n0, n1) of the streamed rows
//   stream_tiles    the tile loop with its one barrier per tile and the fetch hook
//   for_subtiles    the walk over a tile's sub-tiles of 16 streamed rows
// The other kernels keep their own tile loops.  embed_topk, embed_range (one tile buffer, two barriers), embed_cache and
// lm_score (two buffers, rows counted in int from zero) were written on a stream_tiles that also served them and measured
// slower there than on their own loops - range 4 %, top-k about 1 %, lm_score 0.5 %, cache 4 % at its small shape - with no
// spill and no lost occupancy; embed_probe's forward took up to 47 more registers.  embed_cache_bwd and embed_probe's backward
// stream the OTHER operand with their own products, fetch in another place and rewrite the staged tile before the store; what
// they, concept_codes and embed_moments share is functions, not a loop: score_pair.h.
//
// Rows are counted in long from the work-group's first row (row0), so that no sum of a row index comes near 2^31 whatever N is.
// Rows beyond the last are loaded clamped - never out of bounds - and row_live says which to store.
#pragma once
#include "score_tiles.h"

#define CCLIP_SWEEP_INLINE __attribute__((always_inline))   // on every lambda handed to stream_tiles / for_subtiles

namespace CCLIP_NS {

template <int MT>
struct SweepCtx {
  const int tid, lane, wave, li, g;
  const TileGeom geo;
  int split;                                      // of the streamed rows; n0 < n1: a launcher leaves no split empty
  long n0, n1;
  long row0;                                      // the work-group's first operand row (row0 < rows: no empty block)
  int q0, last;                                   // block-relative: the wave's first row, the block's last live row
  bool active;                                    // (wave-uniform) a wave without rows only helps to load
  __device__ __forceinline__ SweepCtx(int D, long rows, long streamed, int splits, long rows_per_split)
      : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), li(lane & 15), g(lane >> 4), geo(D) {
    split = blockIdx.x % splits;
    n0 = split * rows_per_split;
    n1 = min(streamed, n0 + rows_per_split);
    row0 = (long)(blockIdx.x / splits) * (64 * MT);
    last = (int)min(rows - 1 - row0, (long)(64 * MT - 1));
    q0 = wave * (16 * MT);
    active = q0 <= last;
  }
  // row r of operand tile mt of this lane: lane (li, g) holds the rows 4g .. 4g+3 of each tile
  __device__ __forceinline__ int rel(int mt, int r) const { return q0 + 16 * mt + 4 * g + r; }
  __device__ __forceinline__ bool row_live(int mt, int r) const { return rel(mt, r) <= last; }
  __device__ __forceinline__ long row(int mt, int r) const { return row0 + rel(mt, r); }
  __device__ __forceinline__ long row_clamped(int mt, int r) const { return row0 + min(rel(mt, r), last); }
  template <int KSMAX>
  __device__ __forceinline__ void load_a(bf16x8 (&af)[MT][KSMAX], const bf16* base, long ld) const {
    load_a_frags<KSMAX, MT>(af, base + row0 * ld, ld, q0, last, geo.nks, lane);
  }
};

struct NoFetchHook { __device__ __forceinline__ void operator()(long) const {} };

// Streams the rows [first, n1) of src (row stride ld, last valid row last_row; first a multiple of 16) through two LDS tile
// buffers in tiles of GT and calls body(base, acc) per tile, on the active waves only: acc[mt][st] = operand tile mt x
// sub-tile st of the tile that starts at row `base`.  Inactive waves help to load and meet every barrier.  A tile is stored
// into the buffer the tile before last was read from, ONE barrier publishes it, and the next tile's global loads are issued
// right behind that barrier, so they fly under the multiply; on_fetch(next_base) runs beside them.
template <int KSMAX, int MT, int GT, class Body, class OnFetch = NoFetchHook>
__device__ __forceinline__ void stream_tiles(const SweepCtx<MT>& ctx, const bf16x8 (&af)[MT][KSMAX], const bf16* src, long ld,
                                             long first, long n1, long last_row, char* lds, Body&& body,
                                             OnFetch&& on_fetch = OnFetch()) {
  const long ntiles = (n1 - first + GT - 1) / GT;
  const int tilebytes = GT * ctx.geo.rowbytes;
  TileMover<KSMAX, GT> mover(ctx.geo, ctx.tid);
  // the tile is addressed from its own first row: no row index is formed beyond GT - 1
  auto fetch = [&](long base) CCLIP_SWEEP_INLINE {
    mover.fetch(src + base * ld, ld, 0, (int)min(last_row - base, (long)(GT - 1)));
  };
  fetch(first);
  int buf = 0;
  for (long t = 0; t < ntiles; ++t, buf ^= 1) {
    const long base = first + t * GT;
    char* tile = lds + buf * tilebytes;
    mover.store(tile);
    __syncthreads();                              // tile `base` is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < ntiles) { fetch(base + GT); on_fetch(base + GT); }
    if (!ctx.active) continue;
    f32x4 acc[MT][GT / 16];
    tile_multiply<KSMAX, MT, GT>(acc, af, tile, ctx.geo, ctx.lane);
    body(base, acc);
  }
}

// f(st, nb, okn) for every sub-tile st of the tile at `base` that starts below n1: nb its first streamed row, okn whether this
// lane's row nb + li lies below n1
template <int GT, int MT, class F>
__device__ __forceinline__ void for_subtiles(const SweepCtx<MT>& ctx, long base, long n1, F&& f) {
#pragma unroll
  for (int st = 0; st < GT / 16; ++st) {
    const long nb = base + 16 * st;
    if (nb >= n1) continue;                       // (wave-uniform)
    f(st, nb, nb + ctx.li < n1);
  }
}

// the segment that holds position p of an offsets array off[0 .. n]: the last s with off[s] <= p (s < n whatever the array holds)
template <class T>
__device__ __forceinline__ int segment_of(const int* __restrict__ off, int n, T p) {
  int lo = 1, hi = n;                             // the smallest j in 1 .. n with off[j] > p
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] > p) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

template <class T>
__device__ __forceinline__ T clamp_index(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }

static inline bool score_rows_ok(int64_t n) { return n > 0 && n <= 0x7fffffffLL; }

// Splits of N streamed rows for a grid of `blocks` row blocks: enough for about `groups` work-groups while a split keeps at
// least min_rows rows; rows per split a multiple of 64; no empty split
static inline void gallery_splits(int64_t N, int64_t blocks, int64_t groups, int64_t min_rows, int* splits, int* rows_per_split) {
  const int64_t want = (groups + blocks - 1) / blocks, most = (N + min_rows - 1) / min_rows;
  int64_t s = want < most ? want : most;
  if (s < 1) s = 1;
  const int64_t rows = ((N + s - 1) / s + 63) / 64 * 64;
  s = (N + rows - 1) / rows;
  *splits = (int)s; *rows_per_split = (int)rows;
}

// Row parts of the kernels that split the streamed rows over the grid and write one fp32 partial per part (embed_probe's
// backward, embed_moments): N rows in tiles of 32, a part is tpp consecutive tiles.  As many parts as keep the partials within
// 32 MB at bytes_per_part each, at most 1024, and a part at least 8 tiles = 256 rows; no empty part.  Of its arguments alone.
static inline void row_parts(int64_t N, int64_t bytes_per_part, int* ntiles, int* tpp, int* parts) {
  *ntiles = (int)((N + 31) / 32);
  int64_t pmax = (32ll << 20) / bytes_per_part;
  pmax = pmax < 1 ? 1 : pmax > 1024 ? 1024 : pmax;
  const int64_t need = (*ntiles + pmax - 1) / pmax;
  *tpp = (int)(need < 8 ? 8 : need);
  *parts = (*ntiles + *tpp - 1) / *tpp;
}

// The variants: k-steps the A fragments are sized for, operand tiles per wave (two halve the LDS reads per MFMA, same bits
// either way), streamed rows per tile.  f is called with one SweepShape; RUNG768 = false leaves the <24, ., 32> pair out, so
// that a kernel has exactly the instantiations of its ladder.
template <int KSMAX_, int MT_, int GT_>
struct SweepShape { static constexpr int KSMAX = KSMAX_, MT = MT_, GT = GT_; };

template <bool RUNG768, class F>
static int score_dispatch(int D, bool wide, F&& f) {
  if (D <= 128) return wide ? f(SweepShape<4, 2, 64>()) : f(SweepShape<4, 1, 64>());
  if (D <= 512) return wide ? f(SweepShape<16, 2, 64>()) : f(SweepShape<16, 1, 64>());
  if constexpr (RUNG768)
    if (D <= 768) return wide ? f(SweepShape<24, 2, 32>()) : f(SweepShape<24, 1, 32>());
  return f(SweepShape<32, 1, 32>());
}

// grid = blocks of 64 * MT rows x splits; lds_tiles tile buffers of GT rows and extra_lds bytes behind them
template <class Args>
static int sweep_launch(void (*kernel)(const Args), const Args& a, int64_t rows, int MT, int GT, int D, int splits, int lds_tiles,
                        size_t extra_lds, hipStream_t stream) {
  const int64_t blocks = (rows + 64 * MT - 1) / (64 * MT);
  if (blocks * splits > 0x7fffffffLL) return CCLIP_ERR_ARG;
  return score_launch(kernel, (unsigned)(blocks * splits), (size_t)lds_tiles * GT * D * 2 + extra_lds, a, stream);
}

}  // namespace CCLIP_NS
