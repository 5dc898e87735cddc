// Fixed-radius search for gfx950: for queries Qm [Q, D] and a gallery G [N, D] (16-bit rows), every pair whose
//     s[q, n] = sum_d Qm[q, d] G[n, d]            (fp32 accumulation on v_mfma_f32_16x16x32)
// is >= threshold, as CSR: the gallery rows of query i (ascending) and their scores at offsets[i] .. offsets[i+1].
// The Q x N matrix is never written.  A NaN score is never a hit (s >= t is false); +inf is one.
//
// Score.  The tile loop, the instantiations and the split rule of embed_topk.hip on the parts of score_tiles.h: ONE
// accumulator chain over d = 0, 32, 64 .. per pair, so a pair's score bits equal those cclip_similarity_topk returns for it.
//
// Two passes over one grid (query blocks x gallery splits), no atomics, no LDS lists:
//   count: every (query row, split) counts its hits into counts[Q][splits]           (range_kernel<.., false>)
//   scan:  the caller's exclusive scan over the Q * splits counts, row-major: a row's splits are adjacent, so the scanned
//          value of (row, split) is where that segment starts and that of (row, 0) is offsets[row]
//   emit:  the same tiles again; every (row, split) writes its segment from its start  (range_kernel<.., true>)
// Lane (li, g) holds query rows 4g .. 4g+3 against gallery row 16 st + li of sub-tile st: the 16 lanes of group g meet a
// row's gallery rows in ascending order, so a hit's place is the row's running count (equal in the group's lanes) plus the
// number of hits of the row's ballot mask below the lane.  Tiles and sub-tiles ascend: the segment is in gallery order.
// Both passes take the hit decision from the same expression on the same bits, so counts and segments agree.
//
// Self-join (q == g, Q == N): only pairs n > i.  A tile whose rows all lie at or below the work-group's first query row
// is not loaded; a work-group whose whole split does writes zero counts and leaves.
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct RangeArgs {
  const bf16* q; const bf16* g;
  long ldq, ldg;
  int Q, N, D;
  int splits, rows_per_split;                     // rows_per_split is a multiple of 64
  int self_join;
  float thr;
  int* counts;                                    // count: [Q][splits]
  const long long* start;                         // emit: [Q][splits], the exclusive scan of counts
  long long cap;                                  // emit: entries index / scores hold; nothing is written at or beyond it
  int* index; float* scores;
};

template <int KSMAX, int MT, int GT, bool EMIT>
__global__ __launch_bounds__(256) void range_kernel(const RangeArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 gallery rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int Q = a.Q, N = a.N;
  const TileGeom geo(a.D);
  char* Gs = lds;

  const int split = blockIdx.x % a.splits, qb = blockIdx.x / a.splits;
  const int n0 = split * a.rows_per_split;
  const int n1 = min(N, n0 + a.rows_per_split);   // (n0 < N: the launcher leaves no split empty)
  const int qblock = qb * (64 * MT);              // the work-group's first query row
  const int q0 = qblock + wave * (16 * MT);
  const bool active = q0 < Q;                     // (wave-uniform) a wave without rows only helps to load
  // self-join: the first tile that holds a row above qblock (tiles start at multiples of GT, as n0 does)
  const int first = a.self_join ? max(n0, (qblock + 1) / GT * GT) : n0;
  // self-join: n > row  <=>  n - 16 mt - r > q0 + 4 g; otherwise always true
  const int lim = a.self_join ? q0 + 4 * g : -0x7fffffff - 1;

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, a.q, a.ldq, q0, Q - 1, geo.nks, lane);
  // threshold of the rows this lane holds; NaN for a row beyond Q: nothing is >= NaN
  float tf[MT][4];
  int cnt[MT][4];                                 // count: this lane's hits; emit: unused
  long long pos[MT][4];                           // emit: where the row's next hit goes
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = q0 + 16 * mt + 4 * g + r;
      tf[mt][r] = row < Q ? a.thr : __uint_as_float(0x7fc00000u);
      cnt[mt][r] = 0;
      pos[mt][r] = 0;
      if constexpr (EMIT)
        if (row < Q) pos[mt][r] = a.start[(long)row * a.splits + split];
    }

  if (first < n1) {                               // (work-group-uniform)
    TileMover<KSMAX, GT> mover(geo, tid);
    mover.fetch(a.g, a.ldg, first, N - 1);        // rows >= N are clamped (never a hit)
    for (int base = first; base < n1; base += GT) {
      __syncthreads();                            // the previous tile has been read
      mover.store(Gs);
      __syncthreads();
      if (base + GT < n1) mover.fetch(a.g, a.ldg, base + GT, N - 1);
      if (!active) continue;

      f32x4 acc[MT][NST];
      tile_multiply<KSMAX, MT, GT>(acc, af, Gs, geo, lane);

#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const int nb = base + 16 * st;
        if (nb >= n1) continue;                   // (wave-uniform)
        const int n = nb + li;
        const bool okn = n < n1;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          bool hit[4];
          bool any = false;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            hit[r] = okn && acc[mt][st][r] >= tf[mt][r] && n - 16 * mt - r > lim;
            any |= hit[r];
          }
          if constexpr (!EMIT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cnt[mt][r] += hit[r] ? 1 : 0;
          } else {
            if (!__ballot(any)) continue;         // the usual case at a high threshold: no hit in this sub-tile
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const unsigned grp = (unsigned)(__ballot(hit[r]) >> (16 * g)) & 0xffffu;   // the row's hits, bit = li
              if (hit[r]) {
                const long long p = pos[mt][r] + __popc(grp & ((1u << li) - 1u));
                if (p < a.cap) { a.index[p] = n; a.scores[p] = acc[mt][st][r]; }
              }
              pos[mt][r] += __popc(grp);
            }
          }
        }
      }
    }
  }

  if constexpr (!EMIT) {
    if (!active) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int c = cnt[mt][r];                       // sum over the 16 lanes of the group (xor 1 .. 8 stays inside it)
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) c += __shfl_xor(c, s, 64);
        const int row = q0 + 16 * mt + 4 * g + r;
        if (li == 0 && row < Q) a.counts[(long)row * a.splits + split] = c;
      }
  }
}

// gallery splits from (Q, N) alone: the rule of cclip_similarity_topk
static inline void range_splits(int64_t Q, int64_t N, int* splits, int* rows_per_split) {
  gallery_splits(N, (Q + 63) / 64, 512, 256, splits, rows_per_split);
}

template <bool EMIT>
static int range_dispatch(const RangeArgs& a, hipStream_t stream) {
  const int st = score_dispatch<false>(a.D, a.Q > 64, [&](auto s) {             // the instantiations of cclip_similarity_topk
    using S = decltype(s);
    return sweep_launch(range_kernel<S::KSMAX, S::MT, S::GT, EMIT>, a, a.Q, S::MT, S::GT, a.D, a.splits, 1, 0, stream);
  });
  return st != CCLIP_OK ? st : cclip_launch_status();
}

// the checks the two entries share; fills everything of `a` but the outputs
static bool range_args(RangeArgs& a, const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                       float threshold, int32_t self_join) {
  if (!q || !g) return false;
  if (Q <= 0 || !score_rows_ok(N)) return false;
  if (!score_operands_ok(q, ldq, g, ldg, D)) return false;
  if (self_join != 0 && self_join != 1) return false;
  if (self_join && (q != g || ldq != ldg || (int64_t)Q != N)) return false;
  a.q = (const bf16*)q; a.g = (const bf16*)g; a.ldq = ldq; a.ldg = ldg;
  a.Q = Q; a.N = (int)N; a.D = D; a.self_join = self_join; a.thr = threshold;
  range_splits(Q, N, &a.splits, &a.rows_per_split);
  a.counts = nullptr; a.start = nullptr; a.cap = 0; a.index = nullptr; a.scores = nullptr;
  return true;
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_similarity_range_workspace(int32_t Q, int64_t N) {
  if (Q <= 0 || !score_rows_ok(N)) return 0;
  int splits, rows;
  range_splits(Q, N, &splits, &rows);
  return (int64_t)Q * splits * 4;
}
#endif

extern "C" int CCLIP_FN(cclip_similarity_range_count)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N,
                                                       int32_t D, float threshold, int32_t self_join, int32_t* counts,
                                                       int64_t workspace_bytes, hipStream_t stream) {
  RangeArgs a;
  if (!counts || ((uintptr_t)counts & 3)) return CCLIP_ERR_ARG;
  if (!range_args(a, q, ldq, Q, g, ldg, N, D, threshold, self_join)) return CCLIP_ERR_ARG;
  if (workspace_bytes < (int64_t)Q * a.splits * 4) return CCLIP_ERR_ARG;
  a.counts = counts;
  return range_dispatch<false>(a, stream);
}

extern "C" int CCLIP_FN(cclip_similarity_range_emit)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N,
                                                      int32_t D, float threshold, int32_t self_join, const int64_t* starts,
                                                      int64_t total, int64_t H, int32_t* index, float* scores,
                                                      hipStream_t stream) {
  RangeArgs a;
  if (!starts || ((uintptr_t)starts & 7) || !index || !scores || ((uintptr_t)index & 3) || ((uintptr_t)scores & 3))
    return CCLIP_ERR_ARG;
  if (total < 0 || H < 0 || total > H) return CCLIP_ERR_ARG;
  if (!range_args(a, q, ldq, Q, g, ldg, N, D, threshold, self_join)) return CCLIP_ERR_ARG;
  if (total == 0) return CCLIP_OK;                // nothing to write, nothing launched
  a.start = (const long long*)starts; a.cap = H; a.index = index; a.scores = scores;
  return range_dispatch<true>(a, stream);
}
