// Spherical k-means over stored embeddings for gfx950: the two steps of a Lloyd iteration on 16-bit rows x [N, D] and
// centroids c [K, D].
//     assign:  s[n, k] = sum_d x[n, d] c[k, d]   (fp32 accumulation on v_mfma_f32_16x16x32); per row the best centroid, its
//              score and the second-best score.  The N x K matrix is never written.
//     update:  out_c[k] = S / |S| with S = sum of the rows of cluster k in fp32, rounded once to the 16-bit type; |S| alongside.
//
// Assign (kmeans_assign_kernel): one launch, no workspace, grid = blocks of 64 * MT rows of x.  A work-group (4 waves) keeps its
// rows as A fragments in registers and streams ALL K centroid rows through two LDS tiles (the swizzled [row][D] image, the tile
// mover and the multiply of score_tiles.h; one barrier per tile) - the small side is the streamed one, so nothing is split and
// nothing merged.  Every score is ONE accumulator chain over d = 0, 32, 64 .. (tile_multiply): it carries the bits
// cclip_similarity_topk returns for the pair.  Lane (li, g) meets the centroids 16 st + li of every tile and keeps, per row it
// owns, the best candidate as a 64-bit key (score_key in the high word, ~index in the low one: larger = better, equal scores to
// the LOWER index, NaN below every number - the order of embed_topk.hip) and the score key of the runner-up.  The maximum of a
// set of distinct keys does not depend on the order they are met in; the 16 lanes of a group are combined by a fixed xor
// butterfly and lane 0 writes.  So a row's three outputs do not depend on N, on where the row sits or on the variant.
// Rows beyond N and centroids beyond K are loaded clamped (never out of bounds), never selected and never stored.
//
// Update.  `order` lists the rows of x grouped by cluster (ascending row inside a cluster), seg_off[k] .. seg_off[k + 1] are the
// positions of cluster k.  Phase 1 (kmeans_partial_kernel): grid = slabs of KM_SLAB positions, so one huge cluster costs what a
// balanced set costs.  A slab is cut at the cluster boundaries inside it (a wave-uniform cursor into seg_off).  The members of a
// piece are dealt to 4 R streams (wave w, sub-row j: stream w R + j takes the members stream, stream + 4 R, ..), each lane adds
// its 8 columns of its stream's members in that order into fp32 registers, the streams are added through LDS in ascending
// stream order, and the piece's [D] sums go to workspace slot slab + cluster - unique, because along `order` the pair (slab,
// cluster) never decreases in either coordinate and consecutive distinct pairs increase in at least one.
// Phase 2 (kmeans_finish_kernel): one work-group per cluster adds the slots of its slabs in ascending slab order, reduces the
// squared norm by a fixed tree (thread, xor butterfly, waves in order), divides, rounds and writes.  An empty cluster, or one
// whose |S| is 0 or not finite, copies prev_c[k] bit for bit and reports norm 0.
// No atomics anywhere and no fused multiply-add in the sums: the outputs are a pure function of (x, order, seg_off, prev_c),
// two launches are bitwise equal.  The kernels use order / seg_off through clamped values only: whatever the two arrays hold,
// no access leaves x, the workspace or the outputs (garbage there gives garbage sums, nothing else).  That order is a
// permutation and seg_off its monotone boundaries is the caller's to ensure (cclip_hip/ops.py builds both by a stable sort).
#include "score_tiles.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them
#pragma clang fp contract(off)

#define KM_SLAB 256                               // positions of `order` per phase-1 work-group

namespace CCLIP_NS {

struct AssignArgs {
  const bf16* x; const bf16* c;
  long ldx, ldc;
  int N, K, D;
  int* assign; float* best; float* second;        // second may be null
};

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

// <KSMAX, MT, GT> as in score_tiles.h: MT tiles of 16 rows of x per wave, GT centroid rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const AssignArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 centroid rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const long K = a.K;
  const TileGeom geo(a.D);
  const int tilebytes = GT * geo.rowbytes;
  const long ntiles = (K + GT - 1) / GT;

  // rows are counted from the block's first row, so that no int sum comes near 2^31 whatever N is
  const long row0 = (long)blockIdx.x * (64 * MT);                 // (row0 < N: the grid has no empty block)
  const int last = (int)min((long)a.N - 1 - row0, (long)(64 * MT - 1));   // the block's last live row, block-relative
  const bf16* xb = a.x + row0 * a.ldx;
  const int q0 = wave * (16 * MT);
  const bool active = q0 <= last;                 // (wave-uniform) a wave without rows only helps to load

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, xb, a.ldx, q0, last, geo.nks, lane);
  // per-row state of this lane, rows q0 + 16 mt + 4 g + r: the best key and the runner-up's score key (0 = none yet)
  u64 b1[MT][4];
  unsigned b2[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { b1[mt][r] = 0ull; b2[mt][r] = 0u; }

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.c, a.ldc, 0, (int)min(K - 1, (long)(GT - 1)));    // rows >= K are clamped (never selected below)
  int buf = 0;
  for (long t = 0; t < ntiles; ++t, buf ^= 1) {
    const long base = t * GT;
    char* Cs = lds + buf * tilebytes;
    mover.store(Cs);
    __syncthreads();                              // tile `base` is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < ntiles)
      mover.fetch(a.c + (base + GT) * a.ldc, a.ldc, 0, (int)min(K - 1 - (base + GT), (long)(GT - 1)));
    if (!active) continue;

    f32x4 acc[MT][NST];
    tile_multiply<KSMAX, MT, GT>(acc, af, Cs, geo, lane);

#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const long nb = base + 16 * st;
      if (nb >= K) continue;                      // (wave-uniform)
      const bool okc = nb + li < K;
      const unsigned low = ~(unsigned)(nb + li);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const u64 cand = okc ? (((u64)score_key(acc[mt][st][r]) << 32) | low) : 0ull;   // selected, not multiplied
          const u64 b = b1[mt][r];
          const bool better = cand > b;
          const unsigned loser = (unsigned)((better ? b : cand) >> 32);
          b2[mt][r] = max(b2[mt][r], loser);
          b1[mt][r] = better ? cand : b;
        }
    }
  }
  if (!active) return;

  // the 16 lanes of a group hold disjoint centroids: a fixed xor butterfly (both partners compute the same bits), lane 0 writes
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u64 m1 = b1[mt][r];
      unsigned m2 = b2[mt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const u64 p1 = shfl_xor64(m1, o);
        const unsigned p2 = __shfl_xor(m2, o, 64);
        const unsigned loser = (unsigned)((m1 > p1 ? p1 : m1) >> 32);
        m2 = max(max(m2, p2), loser);
        m1 = m1 > p1 ? m1 : p1;
      }
      const int rel = q0 + 16 * mt + 4 * g + r;
      if (li == 0 && rel <= last) {
        const long row = row0 + rel;
        a.assign[row] = (int)~(unsigned)m1;
        a.best[row] = key_score((unsigned)(m1 >> 32));
        if (a.second) a.second[row] = key_score(m2);              // key 0 (K == 1, or a NaN score) decodes to NaN
      }
    }
}

template <int KSMAX, int MT, int GT>
static int assign_launch(const AssignArgs& a, hipStream_t stream) {
  const long nblk = ((long)a.N + 64 * MT - 1) / (64 * MT);        // < 2^26
  const size_t lds = (size_t)2 * GT * a.D * 2;                    // two tiles
  return score_launch(kmeans_assign_kernel<KSMAX, MT, GT>, (unsigned)nblk, lds, a, stream);
}

// ------------------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
  const bf16* x; long ldx;
  int N, D, K;
  const int* order; const int* seg_off;
  float* ws;                                      // [nslabs + K][D]
};

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the cluster whose segment holds position p: the last k with seg_off[k] <= p (k < K whatever the array holds)
__device__ __forceinline__ int cluster_of_pos(const int* __restrict__ off, int K, long p) {
  int lo = 1, hi = K;                             // the smallest j in 1 .. K with off[j] > p
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] > p) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

__global__ __launch_bounds__(256) void kmeans_partial_kernel(const UpdateArgs a) {
  __shared__ float part[4096];                    // [streams][D]: 4 R D <= 2048 floats below 64 chunks a row, 4 D <= 4096 above
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, D = a.D, K = a.K;
  const int cpr = D >> 3;                         // 16-byte chunks per row
  const int R = cpr >= 64 ? 1 : 64 / cpr;         // rows a wave gathers side by side
  const int sub = cpr >= 64 ? 0 : lane / cpr;
  const int ch = cpr >= 64 ? lane : lane - sub * cpr;
  const bool lane_on = sub < R;                   // (the lanes past R cpr idle)
  const bool two = ch + 64 < cpr;                 // a second chunk of the row (D > 512)
  const int nstreams = 4 * R, stream = wave * R + sub;

  const long p0 = (long)blockIdx.x * KM_SLAB, p1 = min((long)N, p0 + KM_SLAB);
  int c = cluster_of_pos(a.seg_off, K, p0);       // (all wave- and block-uniform from here)
  long p = p0;
  while (p < p1) {
    while (c + 1 < K && a.seg_off[c + 1] <= p) ++c;               // skip the clusters that end here (empty ones among them)
    long e = c + 1 < K ? (long)a.seg_off[c + 1] : p1;
    if (e > p1 || e <= p) e = p1;                 // the piece [p, e) of cluster c inside this slab

    float acc[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
    if (lane_on) {
      for (long i = p + stream; i < e; i += 4L * nstreams) {      // four members in flight; added in ascending order
        bf16x8 v[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long pos = min(i + (long)u * nstreams, e - 1);    // (a clamped position is loaded, not added)
          const long row = clampl(a.order[pos], 0, N - 1);
          const bf16* src = a.x + row * a.ldx + ch * 8;
          v[u][0] = *(const bf16x8*)src;
          if (two) v[u][1] = *(const bf16x8*)(src + 512);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (i + (long)u * nstreams >= e) break;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[0][j] += (float)v[u][0][j];
          if (two) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[1][j] += (float)v[u][1][j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) part[stream * D + ch * 8 + j] = acc[0][j];
      if (two) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part[stream * D + 512 + ch * 8 + j] = acc[1][j];
      }
    }
    __syncthreads();
    float* slot = a.ws + ((long)blockIdx.x + c) * D;              // slab + cluster < nslabs + K
    for (int d = tid; d < D; d += 256) {
      float s = part[d];
      for (int st = 1; st < nstreams; ++st) s += part[st * D + d];
      slot[d] = s;
    }
    __syncthreads();                              // part is free again
    p = e;
  }
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(const UpdateArgs a, const bf16* __restrict__ prev, long ldp, bf16* out,
                                                            long ldo, float* __restrict__ out_norm) {
  __shared__ float wsum[4];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int D = a.D;
  const long k = blockIdx.x;
  const long o0 = clampl(a.seg_off[k], 0, a.N), o1 = clampl(a.seg_off[k + 1], 0, a.N);
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};          // columns tid + 256 j
  if (o1 > o0) {
    const long first = o0 / KM_SLAB, lastsl = (o1 - 1) / KM_SLAB; // slabs that hold positions of the cluster: < nslabs
    for (long sl = first; sl <= lastsl; ++sl) {
      const float* slot = a.ws + (sl + k) * D;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (tid + 256 * j < D) s[j] += slot[tid + 256 * j];
    }
  }
  float ss = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (tid + 256 * j < D) ss += s[j] * s[j];
  ss = wave_sum(ss);                              // xor butterfly: every lane holds the same bits
  if ((tid & 63) == 0) wsum[wave] = ss;
  __syncthreads();
  const float norm = sqrtf(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
  const bool keep = !(o1 > o0) || !(norm > 0.0f) || !(norm < __builtin_huge_valf());   // empty, cancelled to zero, or not finite
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = tid + 256 * j;
    if (d < D) out[k * ldo + d] = keep ? prev[k * ldp + d] : (bf16)(s[j] / norm);
  }
  if (tid == 0) out_norm[k] = keep ? 0.0f : norm;
}

static inline int64_t update_slabs(int64_t N) { return (N + KM_SLAB - 1) / KM_SLAB; }

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_kmeans_assign)(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t K, int32_t D,
                                              int32_t* assign, float* best, float* second, hipStream_t stream) {
  if (!x || !c || !assign || !best) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || K <= 0 || K > 0x7fffffffLL) return CCLIP_ERR_ARG;
  if (D < 32 || !score_operands_ok(x, ldx, c, ldc, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)assign & 3) || ((uintptr_t)best & 3) || ((uintptr_t)second & 3)) return CCLIP_ERR_ARG;
  AssignArgs a;
  a.x = (const bf16*)x; a.c = (const bf16*)c; a.ldx = ldx; a.ldc = ldc;
  a.N = (int)N; a.K = (int)K; a.D = D;
  a.assign = assign; a.best = best; a.second = second;
  const bool wide = N > 64;                       // two row tiles per wave halve the LDS reads per MFMA (same bits either way)
  int st;
  if (D <= 128) st = wide ? assign_launch<4, 2, 64>(a, stream) : assign_launch<4, 1, 64>(a, stream);
  else if (D <= 512) st = wide ? assign_launch<16, 2, 64>(a, stream) : assign_launch<16, 1, 64>(a, stream);
  else if (D <= 768) st = wide ? assign_launch<24, 2, 32>(a, stream) : assign_launch<24, 1, 32>(a, stream);
  else st = assign_launch<32, 1, 32>(a, stream);
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}

#ifndef CCLIP_F16
extern "C" int64_t cclip_kmeans_update_workspace(int64_t N, int64_t K, int32_t D) {
  if (N <= 0 || N > 0x7fffffffLL || K <= 0 || K > 0x7fffffffLL || D < 32 || (D & 31) || D > 1024) return 0;
  return (update_slabs(N) + K) * D * 4;
}
#endif

extern "C" int CCLIP_FN(cclip_kmeans_update)(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* order,
                                              const int32_t* seg_off, int64_t K, const void* prev_c, int64_t ldp, void* out_c,
                                              int64_t ldo, float* out_norm, void* workspace, int64_t workspace_bytes,
                                              hipStream_t stream) {
  if (!x || !order || !seg_off || !prev_c || !out_c || !out_norm || !workspace) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || K <= 0 || K > 0x7fffffffLL) return CCLIP_ERR_ARG;
  if (D < 32 || (D & 31) || D > 1024 || (ldx & 7) || ldx < D || ((uintptr_t)x & 15)) return CCLIP_ERR_ARG;
  if (ldp < D || ldo < D || ((uintptr_t)prev_c & 1) || ((uintptr_t)out_c & 1)) return CCLIP_ERR_ARG;
  if (((uintptr_t)order & 3) || ((uintptr_t)seg_off & 3) || ((uintptr_t)out_norm & 3) || ((uintptr_t)workspace & 3)) return CCLIP_ERR_ARG;
  const int64_t nslabs = update_slabs(N);
  if (workspace_bytes < (nslabs + K) * D * 4) return CCLIP_ERR_ARG;
  UpdateArgs a;
  a.x = (const bf16*)x; a.ldx = ldx; a.N = (int)N; a.D = D; a.K = (int)K;
  a.order = order; a.seg_off = seg_off; a.ws = (float*)workspace;
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)nslabs), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)K), dim3(256), 0, stream, a, (const bf16*)prev_c, (long)ldp, (bf16*)out_c,
                     (long)ldo, out_norm);
  return cclip_launch_status();
}
