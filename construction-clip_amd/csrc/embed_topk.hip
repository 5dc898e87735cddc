// Exact top-k retrieval for gfx950: for queries Qm [Q, D] and a gallery G [N, D] (16-bit rows), the k largest
//     s[q, n] = sum_d Qm[q, d] G[n, d]            (fp32 accumulation on v_mfma_f32_16x16x32)
// of every query, as (score fp32, gallery index int32) in descending order.  The Q x N matrix is never written.
//
// Order.  A candidate is one 64-bit key: the high word is score_key (score_key.h: the bits made monotone, NaN -> 0, -0 -> +0),
// the low word is ~index.  Larger key = better: higher score first, equal fp32 scores by the LOWER gallery index, NaN below
// every number.  Keys of distinct gallery rows are distinct, so "the k largest keys" is one well-defined set whatever the
// order candidates are met in: the result does not depend on how the gallery is split.  No atomics; two launches are bitwise equal.
//
// Score independent of position.  Every score is ONE accumulator chain over d = 0, 32, 64 .. in that order, whichever tile,
// split or lane the gallery row lands on, and whichever kernel variant runs; identical gallery rows give identical bits.
//
// Phase 1 (topk_partial_kernel): grid = query blocks x gallery splits; the parts of score_tiles.h in the kernel's own loop
// with one tile buffer and two barriers per tile (see score_sweep.h for why not its loop).
// The query is on the accumulator rows: lane (li, g) holds query rows 4g .. 4g+3 against gallery row 16 st + li of sub-tile st.
// Each lane keeps its rows' running k-th-best score; a sub-tile none of whose scores beats it costs four compares and one
// wave-uniform branch.  A score that does goes, one at a time, into the row's sorted list in LDS (all 64 lanes shift the list
// in one step); about k ln(N / k) such inserts per row.  The lists go to the workspace: [Q][splits][k] keys.
// Phase 2 (topk_merge_kernel): one work-group per query runs the same insert over its splits * k keys and decodes them.
//
// Biased form (cclip_similarity_topk_biased): the same two phases on t[q, n] = fmaf(scale, s[q, n], bias[n]) with bias fp32 [N] -
// the hubness corrections of clip/hubness.py, and with bias = -inf filtered search.  Phase 1 is a compile-time variant of the same
// kernel, chosen by its argument struct; the merge is shared.  A -inf t keys below every finite one and above NaN, so an
// excluded row can only trail, by ascending index.  scale = 1, bias = 0 is the unbiased result bit for bit.
#include <type_traits>
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct TopkArgs {
  const bf16* q; const bf16* g;
  long ldq, ldg;
  int Q, N, D, k;
  int splits, rows_per_split;                     // rows_per_split is a multiple of 64
  u64* ws;
};
struct TopkBiasedArgs : TopkArgs {
  const float* bias; float scale;                 // bias fp32 [N]
};

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}

// Insert the wave-uniform key c into the descending list L[0 .. k) (k <= 64, lane j owns entry j).  Returns the high word of
// the new k-th entry to every lane.
__device__ __forceinline__ unsigned list_insert(volatile u64* L, int k, int lane, u64 c) {
  const bool in = lane < k;
  const u64 e = in ? L[lane] : 0ull;
  const u64 prev = (in && lane > 0) ? L[lane - 1] : ~0ull;
  const u64 nw = c > e ? (c > prev ? prev : c) : e;
  if (in && c > e) L[lane] = nw;
  return __shfl((unsigned)(nw >> 32), k - 1, 64);
}

// <KSMAX, MT, GT> as in score_tiles.h: MT query tiles of 16 rows per wave, GT gallery rows per tile
// Args = TopkArgs: the kernel of cclip_similarity_topk.  Args = TopkBiasedArgs ranks t = fmaf(scale, s, bias[n]) instead of s;
// every `if constexpr (BIASED)` below compiles to nothing in the unbiased kernel.
template <int KSMAX, int MT, int GT, class Args>
__global__ __launch_bounds__(256) void topk_partial_kernel(const Args a) {
  constexpr bool BIASED = std::is_same<Args, TopkBiasedArgs>::value;
  constexpr int NST = GT / 16;                    // sub-tiles of 16 gallery rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int k = a.k, Q = a.Q, N = a.N;
  const TileGeom geo(a.D);
  char* Gs = lds;
  volatile u64* lists = (volatile u64*)(lds + GT * geo.rowbytes) + (long)wave * (16 * MT) * k;

  const int split = blockIdx.x % a.splits, qb = blockIdx.x / a.splits;
  const int n0 = split * a.rows_per_split;
  const int n1 = min(N, n0 + a.rows_per_split);   // (n0 < N: the launcher leaves no split empty)
  const int q0 = (qb * 4 + wave) * (16 * MT);
  const bool active = q0 < Q;                     // (wave-uniform) a wave without rows only helps to load

  for (int i = lane; i < 16 * MT * k; i += 64) lists[i] = 0ull;

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, a.q, a.ldq, q0, Q - 1, geo.nks, lane);
  // running k-th-best score of the rows this lane holds: NaN = list not full yet (everything passes), +inf = row beyond Q
  float tf[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      tf[mt][r] = q0 + 16 * mt + 4 * g + r < Q ? __uint_as_float(0x7fc00000u) : __builtin_huge_valf();

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.g, a.ldg, n0, N - 1);             // rows >= N are clamped (never selected)
  for (int base = n0; base < n1; base += GT) {
    __syncthreads();                              // the previous tile has been read (and, first time, the lists are zero)
    mover.store(Gs);
    __syncthreads();
    if (base + GT < n1) mover.fetch(a.g, a.ldg, base + GT, N - 1);
    if (!active) continue;

    float bs[NST];                                // the bias of this lane's gallery row of every sub-tile, loaded under the multiply
    if constexpr (BIASED) {
#pragma unroll
      for (int st = 0; st < NST; ++st) bs[st] = a.bias[min(base + 16 * st + li, N - 1)];    // clamped (never selected)
    }
    f32x4 acc[MT][NST];
    tile_multiply<KSMAX, MT, GT>(acc, af, Gs, geo, lane);
    if constexpr (BIASED) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int st = 0; st < NST; ++st)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][st][r] = __builtin_fmaf(a.scale, acc[mt][st][r], bs[st]);
    }

#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int nb = base + 16 * st;
      if (nb >= n1) continue;                     // (wave-uniform)
      const bool okn = nb + li < n1;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bool pass[4];
        bool any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pass[r] = okn && !(acc[mt][st][r] <= tf[mt][r]); any |= pass[r]; }
        if (!__ballot(any)) continue;             // the usual case: nothing in this sub-tile beats any row's k-th best
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          u64 mask = __ballot(pass[r]);
          while (mask) {                          // ascending lanes: a row meets its candidates in ascending gallery order
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float sc = __shfl(acc[mt][st][r], src, 64);
            const u64 c = ((u64)score_key(sc) << 32) | (unsigned)~(unsigned)(nb + (src & 15));
            const int row = 16 * mt + 4 * (src >> 4) + r;
            const unsigned kth = list_insert(lists + row * k, k, lane, c);
            if (g == (src >> 4)) tf[mt][r] = key_score(kth);
          }
        }
      }
    }
  }

  if (!active) return;
  // the wave's lists -> workspace [Q][splits][k]
  for (int i = lane; i < 16 * MT * k; i += 64) {
    const int row = i / k, j = i - row * k;
    if (q0 + row < Q) a.ws[((long)(q0 + row) * a.splits + split) * k + j] = lists[i];
  }
}

// One work-group per query: the k largest of its splits * k keys, decoded.  Empty entries (key 0) never enter.
__global__ __launch_bounds__(256) void topk_merge_kernel(const u64* __restrict__ ws, int splits, int k, float* __restrict__ scores,
                                                         int* __restrict__ index) {
  __shared__ u64 Ls[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long q = blockIdx.x;
  const int C = splits * k;
  const u64* src = ws + q * C;
  volatile u64* L = Ls[wave];
  L[lane] = 0ull;
  u64 kth = 0ull;                                 // the wave's k-th best so far (wave-uniform)
  auto offer = [&](u64 c) {
    u64 mask = __ballot(c > kth);
    while (mask) {
      const int s = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const u64 cc = shfl64(c, s);
      if (cc > kth) {                             // (wave-uniform) kth may have risen since the ballot
        list_insert(L, k, lane, cc);
        kth = L[k - 1];
      }
    }
  };
  for (int base = wave * 64; base < C; base += 1024) {          // four independent loads in flight per lane
    u64 c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = base + 256 * u + lane; c[u] = i < C ? src[i] : 0ull; }
#pragma unroll
    for (int u = 0; u < 4; ++u) offer(c[u]);
  }
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < 4; ++w) offer(lane < k ? Ls[w][lane] : 0ull);
  if (lane < k) {
    const u64 e = L[lane];
    scores[q * k + lane] = key_score((unsigned)(e >> 32));
    index[q * k + lane] = (int)~(unsigned)e;
  }
}

// gallery splits from (Q, N) alone: enough work-groups for two per CU while a split keeps at least 256 rows
static inline void topk_splits(int64_t Q, int64_t N, int* splits, int* rows_per_split) {
  gallery_splits(N, (Q + 63) / 64, 512, 256, splits, rows_per_split);
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_similarity_topk_workspace(int32_t Q, int64_t N, int32_t k) {
  if (Q <= 0 || !score_rows_ok(N) || k <= 0) return 0;
  int splits, rows;
  topk_splits(Q, N, &splits, &rows);
  return (int64_t)Q * splits * k * 8;
}
#endif

// the checks the two entries share; fills a
static int topk_args(TopkArgs& a, const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D, int32_t k,
                     float* scores, int32_t* index, void* workspace, int64_t workspace_bytes) {
  if (!q || !g || !scores || !index || !workspace) return CCLIP_ERR_ARG;
  if (Q <= 0 || !score_rows_ok(N) || k < 1 || k > 64 || k > N) return CCLIP_ERR_ARG;
  if (!score_operands_ok(q, ldq, g, ldg, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)scores & 3) || ((uintptr_t)index & 3)) return CCLIP_ERR_ARG;
  a.q = (const bf16*)q; a.g = (const bf16*)g; a.ldq = ldq; a.ldg = ldg;
  a.Q = Q; a.N = (int)N; a.D = D; a.k = k;
  topk_splits(Q, N, &a.splits, &a.rows_per_split);
  a.ws = (u64*)workspace;
  if (workspace_bytes < (int64_t)Q * a.splits * k * 8) return CCLIP_ERR_ARG;
  return CCLIP_OK;
}

extern "C" int CCLIP_FN(cclip_similarity_topk)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N,
                                                int32_t D, int32_t k, float* scores, int32_t* index, void* workspace,
                                                int64_t workspace_bytes, hipStream_t stream) {
  TopkArgs a;
  if (topk_args(a, q, ldq, Q, g, ldg, N, D, k, scores, index, workspace, workspace_bytes) != CCLIP_OK) return CCLIP_ERR_ARG;
  const int st = score_dispatch<false>(D, Q > 64, [&](auto s) {
    using S = decltype(s);                        // one tile, then the four waves' lists
    return sweep_launch(topk_partial_kernel<S::KSMAX, S::MT, S::GT, TopkArgs>, a, Q, S::MT, S::GT, D, a.splits, 1, (size_t)4 * 16 * S::MT * k * 8, stream);
  });
  if (st != CCLIP_OK) return st;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, stream, (const u64*)a.ws, a.splits, k, scores, index);
  return cclip_launch_status();
}

extern "C" int CCLIP_FN(cclip_similarity_topk_biased)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N,
                                                       int32_t D, int32_t k, const float* bias, float scale, float* scores,
                                                       int32_t* index, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  TopkBiasedArgs b;
  if (!bias || ((uintptr_t)bias & 3)) return CCLIP_ERR_ARG;
  if (topk_args(b, q, ldq, Q, g, ldg, N, D, k, scores, index, workspace, workspace_bytes) != CCLIP_OK) return CCLIP_ERR_ARG;
  b.bias = bias; b.scale = scale;
  const TopkArgs& a = b;
  const int st = score_dispatch<false>(D, Q > 64, [&](auto s) {
    using S = decltype(s);
    return sweep_launch(topk_partial_kernel<S::KSMAX, S::MT, S::GT, TopkBiasedArgs>, b, Q, S::MT, S::GT, D, a.splits, 1, (size_t)4 * 16 * S::MT * k * 8, stream);
  });
  if (st != CCLIP_OK) return st;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, stream, (const u64*)a.ws, a.splits, k, scores, index);
  return cclip_launch_status();
}
