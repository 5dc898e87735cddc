// Gradient of the class affinities of embed_cache.hip with respect to the stored rows, for gfx950.  With queries Qm [Q, D],
// stored rows G [Np, D] (16-bit, grouped by class as embed_cache.hip describes) and dA [Q, C] fp32,
//     s[q, n]  = sum_d Qm[q, d] G[n, d]                       (fp32 on v_mfma_f32_16x16x32, ONE chain over d = 0, 32, 64 ..)
//     w[q, n]  = dA[q, c(n)] * exp(beta * (s[q, n] - 1))      for live n, n != exclude[q];  0 otherwise (selected, never multiplied)
//     dG[n, :] = beta * sum_q w[q, n] * Qm[q, :]              for live n;  exactly +0.0f for padding rows
// Every row of dG is written (no zero fill by the caller), and the Q x Np matrix never reaches memory.
//
// Roles.  The forward kernel's, swapped: a work-group (4 waves) owns 64 stored rows, wave w the 16 rows 16 w .. of them as MFMA
// fragments in registers, and streams the QUERIES through two LDS buffers in tiles of 32 rows with score_tiles.h's tile mover
// and image (one barrier per tile).  A block of 16 stored rows belongs to one class, so the class - the column of dA a wave
// gathers - is wave-uniform.  Rows beyond Q and beyond Np are loaded clamped (never out of bounds) and selected away.
//
// Two products, no transpose of w.  The scores are taken with the query tile as the A operand and the stored rows as B, so a
// 16 x 16 score tile has the query on the accumulator row (4 g + r) and the stored row on the lane (li).  That is the B operand
// layout of the second product  dG^T[d, n] = sum_q Qm^T[d, q] w[q, n]  over k = the 32 queries of the tile (element j of lane
// group g: query 16 (j >> 2) + 4 g + (j & 3), the same k order on both operands), whose A operand Qm^T comes from the SAME LDS
// image through the transposed read ds_read_b64_tr_b16 (score_pair.h's tile_frag_tr; the scheme of attention.hip's
// dV^T = dO^T P).  All branches around it are wave-uniform.
//
// w as a 16-bit operand.  w is fp32 in the accumulators.  It is scaled by a power of two 2^-e taken from max|dA| (a small
// reduction launch in front; e = the exponent of the maximum, so |dA| 2^-e < 1 and fp16 does not go subnormal where dA is of
// order 1 / Q), then split into hi = round16(w) and lo = round16(w - hi): two MFMAs into the same accumulator.  What is lost
// is the rounding of lo: 2^-16 relative for bf16 (unit roundoff 2^-8, squared), 2^-22 for fp16, plus for fp16 an absolute
// 2^-25 (half its smallest subnormal) in scaled units.  (A single rounding would leave 2^-8 / 2^-11 per term.)  The scale is undone together with beta in the epilogue:
// dG = acc * (beta * 2^e), e exact.
//
// Registers.  A wave's accumulator is [16 rows x D] fp32 = D / 4 registers per lane, next to D / 8 for its stored-row fragments
// and D / 16 for the tile mover's staging.  Up to D = 512 that is 128 + 64 + 32; above, the columns are cut in two halves over
// the grid (each half recomputes the scores, 1/3 more MFMA work, and keeps 128 accumulator registers) so that no variant
// spills.  The queries are NOT split over the grid: a work-group adds its queries in ascending tile order into one
// accumulator, there is no workspace pass and no merge, at the price of ceil(Np / 64) work-groups only (a cache of a few
// hundred rows fills a few CUs; that launch is latency-bound either way).
//
// Determinism.  No atomics; a row's sum runs over the query tiles in ascending order inside one wave, and neither the grid nor
// the variant depends on anything but Np and D: two launches are bitwise equal.
// The kernels index class_off / class_len with clamped cursors only: whatever the two arrays hold, no access leaves q, g, dA,
// the workspace or dG.
#include "score_pair.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them, so that every
// instantiation of the kernel rounds alike
#pragma clang fp contract(off)

#define CACHE_MAX_C 256
#define CACHE_BWD_MAXPARTS 64                     // partial maxima of |dA| (the workspace: CACHE_BWD_MAXPARTS floats)
#define CACHE_BWD_QT 32                           // queries per streamed tile: one k-step of the second product

namespace CCLIP_NS {

struct CacheBwdArgs {
  const bf16* q; const bf16* g;
  long ldq, ldg;
  int Q, Np, D, C;
  const int* class_off; const int* class_len; const int* exclude;
  const float* dA;
  float beta;
  const float* amax; int nparts;                  // partial maxima of |dA|
  float* dG;                                      // [Np][D]
};

// partial maxima of |dA| (NaN is ignored by fmaxf); block b writes part[b]
__global__ __launch_bounds__(256) void cache_bwd_amax_kernel(const float* __restrict__ dA, long n, float* __restrict__ part) {
  __shared__ float red[4];
  float m = 0.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(dA[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// <KSMAX, DS>: k-steps of 32 the stored-row fragments are sized for (D <= 32 KSMAX); DS column parts over the grid
template <int KSMAX, int DS>
__global__ __launch_bounds__(256) void cache_bwd_kernel(const CacheBwdArgs a) {
  constexpr int GT = CACHE_BWD_QT;
  constexpr int NDT = 2 * KSMAX / DS;             // column tiles of 16 this work-group accumulates
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int Q = a.Q, Np = a.Np, C = a.C, D = a.D;
  const TileGeom geo(D);
  const int tilebytes = GT * geo.rowbytes;

  const int part = blockIdx.x % DS, blk = blockIdx.x / DS;
  const int dt0 = part * NDT;                     // first column tile of this part
  const int n0 = blk * 64 + 16 * wave;            // this wave's 16 stored rows (a multiple of 16: one class)
  const int ntiles = (Q + GT - 1) / GT;

  // the power-of-two scale from max|dA|
  float amax = 0.0f;
  for (int i = 0; i < a.nparts; ++i) amax = fmaxf(amax, a.amax[i]);
  int e = 0;
  if (amax > 0.0f && amax <= 3.0e38f) { (void)frexpf(amax, &e); e = min(max(e, -120), 120); }
  const float down = ldexpf(1.0f, -e), up = a.beta * ldexpf(1.0f, e);

  // (all wave-uniform) the class of the wave's rows and its live end; a wave without live rows only helps to load
  int c = 0, live_end = 0;
  if (n0 < Np) {
    c = segment_of(a.class_off, C, n0);
    const int first = a.class_off[c];
    live_end = (n0 >= first) ? first + a.class_len[c] : 0;
  }
  const bool active = n0 < Np && n0 < live_end && 16 * dt0 < D;
  const int row = n0 + li;                        // this lane's stored row
  const bool live = row < live_end;

  bf16x8 gf[1][KSMAX];
  load_a_frags<KSMAX, 1>(gf, a.g, a.ldg, n0, Np - 1, geo.nks, lane);

  f32x4 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.q, a.ldq, 0, Q - 1);              // rows >= Q are clamped (their terms are selected away below)
  int buf = 0;
  for (int t = 0; t < ntiles; ++t, buf ^= 1) {
    const int base = t * GT;
    char* Qs = lds + buf * tilebytes;
    mover.store(Qs);
    __syncthreads();                              // tile `base` is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < ntiles) mover.fetch(a.q, a.ldq, base + GT, Q - 1);
    if (!active) continue;                        // (wave-uniform)
    const int lane_t = opaque_lane(lane);         // the tile's LDS addresses are formed per tile (score_pair.h)

    // this lane's queries base + 16 st + 4 g + r: their dA (scaled, exact) and excluded rows
    float da[2][4];
    int excl[2][4];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = min(base + 16 * st + 4 * g + r, Q - 1);
        da[st][r] = a.dA[(long)qi * C + c] * down;
        excl[st][r] = a.exclude ? a.exclude[qi] : -1;
      }

    // s^T: query on the accumulator row, stored row on the lane; one chain over d
    f32x4 s[1][2];
    tile_scores_t<KSMAX, 1>(s, gf, Qs, geo, lane_t);

    bf16x8 whi, wlo;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = base + 16 * st + 4 * g + r;
        const float x = (s[0][st][r] - 1.0f) * a.beta;
        const bool take = live && qi < Q && row != excl[st][r];
        const float w = take ? da[st][r] * __expf(x) : 0.0f;      // selected, not multiplied: a masked NaN stays out
        split16(w, whi, wlo, 4 * st + r);
      }

    // dG^T[d, n] += Qm^T[d, q] w[q, n] over the 32 queries of the tile: k index = (st, g, r) on both operands
    tr_accumulate<NDT>(acc, Qs, geo, dt0, D, whi, wlo, lane_t);
  }

  // lane (li, g) holds dG[row][16 dt + 4 g .. + 3]; a padding row is +0.0f whatever the accumulator's sign
  if (row < Np) {
    store_dt_columns<NDT>(a.dG + (long)row * D + 4 * g, dt0, D, [&](int dt) CCLIP_SWEEP_INLINE {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = live ? acc[dt][r] * up : 0.0f;
      return v;
    });
  }
}

static inline int cache_bwd_parts(int64_t cells) {
  int64_t p = (cells + 4095) / 4096;
  return (int)(p < 1 ? 1 : p > CACHE_BWD_MAXPARTS ? CACHE_BWD_MAXPARTS : p);
}

template <int KSMAX, int DS>
static int cache_bwd_launch(const CacheBwdArgs& a, hipStream_t stream) {
  const long nblk = ((long)a.Np + 63) / 64;       // Np < 2^31: at most 2^25 blocks
  const size_t lds = (size_t)2 * CACHE_BWD_QT * a.D * 2;
  return score_launch(cache_bwd_kernel<KSMAX, DS>, (unsigned)(nblk * DS), lds, a, stream);
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_cache_affinity_bwd_workspace(int32_t Q, int32_t C) {
  if (Q <= 0 || C < 1 || C > CACHE_MAX_C) return 0;
  return (int64_t)CACHE_BWD_MAXPARTS * 4;
}
#endif

extern "C" int CCLIP_FN(cclip_cache_affinity_bwd)(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np,
                                                   int32_t D, const int32_t* class_off, const int32_t* class_len, int32_t C,
                                                   float beta, const int32_t* exclude, const float* dA, float* dG, void* workspace,
                                                   int64_t workspace_bytes, hipStream_t stream) {
  if (!q || !g || !class_off || !class_len || !dA || !dG || !workspace) return CCLIP_ERR_ARG;
  if (Q <= 0 || !score_rows_ok(Np) || (Np & 15) || C < 1 || C > CACHE_MAX_C) return CCLIP_ERR_ARG;
  if (!score_operands_ok(q, ldq, g, ldg, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)workspace & 3) || ((uintptr_t)dA & 3) || ((uintptr_t)dG & 15) || ((uintptr_t)class_off & 3) ||
      ((uintptr_t)class_len & 3) || ((uintptr_t)exclude & 3))
    return CCLIP_ERR_ARG;
  if (workspace_bytes < (int64_t)CACHE_BWD_MAXPARTS * 4) return CCLIP_ERR_ARG;
  CacheBwdArgs a;
  a.q = (const bf16*)q; a.g = (const bf16*)g; a.ldq = ldq; a.ldg = ldg;
  a.Q = Q; a.Np = (int)Np; a.D = D; a.C = C;
  a.class_off = class_off; a.class_len = class_len; a.exclude = exclude;
  a.dA = dA; a.beta = beta; a.dG = dG;
  a.amax = (const float*)workspace; a.nparts = cache_bwd_parts((int64_t)Q * C);
  hipLaunchKernelGGL(cache_bwd_amax_kernel, dim3((unsigned)a.nparts), dim3(256), 0, stream, dA, (long)Q * C, (float*)workspace);
  int st;
  if (D <= 128) st = cache_bwd_launch<4, 1>(a, stream);
  else if (D <= 512) st = cache_bwd_launch<16, 1>(a, stream);
  else st = cache_bwd_launch<32, 2>(a, stream);
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}
