// Class affinities of a few-shot cache model for gfx950 (Tip-Adapter, Zhang et al., ECCV 2022): for queries Qm [Q, D] and
// stored rows G [Np, D] (16-bit rows) that are grouped by class,
//     s[q, n]   = sum_d Qm[q, d] G[n, d]          (fp32 accumulation on v_mfma_f32_16x16x32)
//     out[q, c] = sum over the live rows n of class c, n != exclude[q], of exp(beta * (s[q, n] - 1))
// The Q x Np matrix is never written: what reaches memory is one float per (query, split, class the split meets), then out.
//
// Layout.  Class c owns the rows class_off[c] .. class_off[c + 1]; the first class_len[c] of them are live, the rest is
// padding (allocated, loaded, never selected: a NaN there does not reach the output).  Every class_off is a multiple of 16,
// so a sub-tile of 16 stored rows belongs to one class and a lane's mask is `row < live end && row != exclude`.
//
// Score independent of position.  Every score is ONE accumulator chain over d = 0, 32, 64 .. in that order (the tile multiply
// of score_tiles.h), whichever tile, split, lane or kernel variant its rows land on.
// Sum independent of Q.  The stored rows are cut into splits by a rule that depends on Np alone (gallery_splits of
// score_sweep.h at one query block; rows per split a multiple of 64).  Inside a split, lane li of a 16-lane group meets the
// rows n0 + li, n0 + li + 16, .. of a class in ascending order and adds their terms to one register per query row; when the
// class ends the 16 lanes are combined by a fixed xor butterfly (both partners compute the same bits) and phase 2 adds the
// splits that hold live rows of the class in ascending order.  None of this depends on how many queries are scored, on which
// accumulator row a query sits, or on the variant (rows per wave, tile height) the launcher picks from Q and D: a query's row
// of `out` is bit-identical scored alone or inside any batch.  No atomics: two launches are bitwise equal.
// An empty class has no split to add and gives exactly 0.0f; so does a class whose only live row is excluded (its term is 0.0f).
//
// Phase 1 (cache_partial_kernel): grid = query blocks x splits.  A work-group (4 waves) owns 64 * MT query rows, wave w the
// rows 16 MT w ..; their A fragments stay in registers.  G streams through two LDS buffers in tiles of GT rows (the swizzled
// [row][D] image, the tile mover and the multiply of score_tiles.h; one barrier per tile).  The class of a sub-tile is a
// wave-uniform cursor into class_off.  Rows beyond Q and beyond Np are loaded clamped (never out of bounds) and never stored.
// Phase 2 (cache_merge_kernel): one thread per (query, class).
// The kernels index class_off / class_len with clamped cursors only: whatever the two arrays hold, no access leaves g, the
// workspace or out.  That their content is a legal layout is checked where they are still host data (cclip_hip/ops.py).
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them, so that every
// instantiation of the kernel rounds alike
#pragma clang fp contract(off)

#define CACHE_MAX_C 256

namespace CCLIP_NS {

struct CacheArgs {
  const bf16* q; const bf16* g;
  long ldq, ldg;
  int Q, Np, D, C;
  int splits, rows_per_split;                     // rows_per_split is a multiple of 64
  const int* class_off; const int* class_len; const int* exclude;
  float beta;
  float* ws;                                      // [Q][splits][C]
};

// <KSMAX, MT, GT> as in score_tiles.h: MT query tiles of 16 rows per wave, GT stored rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void cache_partial_kernel(const CacheArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 stored rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int Q = a.Q, Np = a.Np, C = a.C;
  const TileGeom geo(a.D);
  const int tilebytes = GT * geo.rowbytes;

  const int split = blockIdx.x % a.splits, qb = blockIdx.x / a.splits;
  const int n0 = split * a.rows_per_split;        // (n0 < Np: the launcher leaves no split empty)
  const int n1 = (int)min((long)Np, (long)n0 + a.rows_per_split);
  const int ntiles = (n1 - n0 + GT - 1) / GT;
  const int q0 = (qb * 4 + wave) * (16 * MT);
  const bool active = q0 < Q;                     // (wave-uniform) a wave without rows only helps to load

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, a.q, a.ldq, q0, Q - 1, geo.nks, lane);
  // per-row state of this lane: query rows q0 + 16 mt + 4 g + r against the stored rows nb + li of the open class
  float rs[MT][4];
  int excl[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = q0 + 16 * mt + 4 * g + r;
      rs[mt][r] = 0.0f;
      excl[mt][r] = (a.exclude && row < Q) ? a.exclude[row] : -1;
    }

  // (all wave-uniform) the class cursor: segment [.., seg_end), live rows [.., live_end); open = rs holds terms of class c
  int c = segment_of(a.class_off, C, n0);
  int seg_end = a.class_off[c + 1], live_end = a.class_off[c] + a.class_len[c];
  bool open = false;

  // the 16 lanes of a group -> one partial per query row of class `cls` (xor butterfly: both partners compute the same bits)
  auto flush = [&](int cls) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = rs[mt][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
        const int row = q0 + 16 * mt + 4 * g + r;
        if (li == 0 && row < Q) a.ws[((long)row * a.splits + split) * C + cls] = s;
        rs[mt][r] = 0.0f;
      }
  };

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.g, a.ldg, n0, Np - 1);            // rows >= Np are clamped (their sub-tiles are skipped below)
  int buf = 0;
  for (int t = 0; t < ntiles; ++t, buf ^= 1) {
    const int base = n0 + t * GT;
    char* Gs = lds + buf * tilebytes;
    mover.store(Gs);
    __syncthreads();                              // tile `base` is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < ntiles) mover.fetch(a.g, a.ldg, base + GT, Np - 1);
    if (!active) continue;

    f32x4 acc[MT][NST];
    tile_multiply<KSMAX, MT, GT>(acc, af, Gs, geo, lane);

#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int nb = base + 16 * st;
      if (nb >= n1) continue;                     // (wave-uniform)
      if (nb >= seg_end) {                        // the sub-tile starts another class
        if (open) flush(c);
        open = false;
        while (c + 1 < C && a.class_off[c + 1] <= nb) ++c;
        seg_end = a.class_off[c + 1]; live_end = a.class_off[c] + a.class_len[c];
      }
      if (nb >= live_end) continue;               // padding only
      open = true;
      const int row = nb + li;
      const bool live = row < live_end;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = (acc[mt][st][r] - 1.0f) * a.beta;
          rs[mt][r] += (live && row != excl[mt][r]) ? __expf(x) : 0.0f;   // selected, not multiplied: a masked NaN stays out
        }
    }
  }
  if (active && open) flush(c);
}

// One thread per (query, class): the partials of the splits that hold live rows of the class, in ascending order.
__global__ __launch_bounds__(256) void cache_merge_kernel(const float* __restrict__ ws, int Q, int C, int splits, int rows_per_split,
                                                          const int* __restrict__ class_off, const int* __restrict__ class_len,
                                                          float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Q * C) return;
  const long q = i / C;
  const int c = (int)(i - q * C);
  const long o = class_off[c], n = class_len[c];
  float s = 0.0f;
  if (n > 0) {
    const long first = max(0L, o / rows_per_split), last = min((long)splits - 1, (o + n - 1) / rows_per_split);
    for (long sp = first; sp <= last; ++sp) s += ws[(q * splits + sp) * C + c];
  }
  out[i] = s;
}

// splits from Np alone (a query's sums must not depend on Q): the rule of cclip_similarity_topk at one query block, i.e. up to
// 512 work-groups per query block while a split keeps at least 256 rows
static inline void cache_splits(int64_t Np, int* splits, int* rows_per_split) { gallery_splits(Np, 1, 512, 256, splits, rows_per_split); }

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_cache_affinity_workspace(int32_t Q, int64_t Np, int32_t C) {
  if (Q <= 0 || !score_rows_ok(Np) || (Np & 15) || C < 1 || C > CACHE_MAX_C) return 0;
  int splits, rows;
  cache_splits(Np, &splits, &rows);
  return (int64_t)Q * splits * C * 4;
}
#endif

extern "C" int CCLIP_FN(cclip_cache_affinity)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np, int32_t D,
                                               const int32_t* class_off, const int32_t* class_len, int32_t C, float beta,
                                               const int32_t* exclude, float* out, void* workspace, int64_t workspace_bytes,
                                               hipStream_t stream) {
  if (!q || !g || !class_off || !class_len || !out || !workspace) return CCLIP_ERR_ARG;
  if (Q <= 0 || !score_rows_ok(Np) || (Np & 15) || C < 1 || C > CACHE_MAX_C) return CCLIP_ERR_ARG;
  if (!score_operands_ok(q, ldq, g, ldg, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)workspace & 3) || ((uintptr_t)out & 3) || ((uintptr_t)class_off & 3) || ((uintptr_t)class_len & 3) ||
      ((uintptr_t)exclude & 3))
    return CCLIP_ERR_ARG;
  CacheArgs a;
  a.q = (const bf16*)q; a.g = (const bf16*)g; a.ldq = ldq; a.ldg = ldg;
  a.Q = Q; a.Np = (int)Np; a.D = D; a.C = C;
  cache_splits(Np, &a.splits, &a.rows_per_split);
  a.class_off = class_off; a.class_len = class_len; a.exclude = exclude;
  a.beta = beta;
  a.ws = (float*)workspace;
  if (workspace_bytes < (int64_t)Q * a.splits * C * 4) return CCLIP_ERR_ARG;
  const int st = score_dispatch<true>(D, Q > 64, [&](auto s) {
    using S = decltype(s);                        // two tiles; the class sums live in registers, so C costs no LDS
    return sweep_launch(cache_partial_kernel<S::KSMAX, S::MT, S::GT>, a, Q, S::MT, S::GT, D, a.splits, 2, 0, stream);
  });
  if (st != CCLIP_OK) return st;
  const long cells = (long)Q * C;
  hipLaunchKernelGGL(cache_merge_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, (const float*)a.ws, Q, C,
                     a.splits, a.rows_per_split, class_off, class_len, out);
  return cclip_launch_status();
}
