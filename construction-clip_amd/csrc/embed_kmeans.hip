// Spherical k-means over stored embeddings for gfx950: the two steps of a Lloyd iteration on 16-bit rows x [N, D] and
// centroids c [K, D].
//     assign:  s[n, k] = sum_d x[n, d] c[k, d]   (fp32 accumulation on v_mfma_f32_16x16x32); per row the best centroid, its
//              score and the second-best score.  The N x K matrix is never written.
//     update:  out_c[k] = S / |S| with S = sum of the rows of cluster k in fp32, rounded once to the 16-bit type; |S| alongside.
//
// Assign (kmeans_assign_kernel): one launch, no workspace: the sweep of score_sweep.h (two tile buffers) over blocks of 64 * MT
// rows of x with ALL K centroid rows as its one split - the small side is the streamed one, so nothing is split and nothing
// merged.  Every score carries the bits cclip_similarity_topk returns for the pair.  Lane (li, g) meets the centroids
// 16 st + li of every tile and keeps, per row it
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
#include "score_sweep.h"
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

// <KSMAX, MT, GT> as in score_tiles.h: MT tiles of 16 rows of x per wave, GT centroid rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const AssignArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const SweepCtx<MT> ctx(a.D, a.N, a.K, 1, a.K);
  const int li = ctx.li;
  const long K = a.K;

  bf16x8 af[MT][KSMAX];
  ctx.load_a(af, a.x, a.ldx);
  // per-row state of this lane: the best key and the runner-up's score key (0 = none yet)
  u64 b1[MT][4];
  unsigned b2[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { b1[mt][r] = 0ull; b2[mt][r] = 0u; }

  // rows >= K are clamped (never selected below)
  stream_tiles<KSMAX, MT, GT>(ctx, af, a.c, a.ldc, 0L, K, K - 1, lds, [&](long base, f32x4 (&acc)[MT][GT / 16]) CCLIP_SWEEP_INLINE {
    for_subtiles<GT>(ctx, base, K, [&](int st, long nb, bool okc) CCLIP_SWEEP_INLINE {
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
    });
  });
  if (!ctx.active) return;

  // the 16 lanes of a group hold disjoint centroids: the butterfly of group_max_key (score_key.h) with the runner-up carried along
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
      if (li == 0 && ctx.row_live(mt, r)) {
        const long row = ctx.row(mt, r);
        a.assign[row] = (int)~(unsigned)m1;
        a.best[row] = key_score((unsigned)(m1 >> 32));
        if (a.second) a.second[row] = key_score(m2);              // key 0 (K == 1, or a NaN score) decodes to NaN
      }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
  const bf16* x; long ldx;
  int N, D, K;
  const int* order; const int* seg_off;
  float* ws;                                      // [nslabs + K][D]
};

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
  int c = segment_of(a.seg_off, K, p0);       // (all wave- and block-uniform from here)
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
          const long row = clamp_index<long>(a.order[pos], 0, N - 1);
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
  const long o0 = clamp_index<long>(a.seg_off[k], 0, a.N), o1 = clamp_index<long>(a.seg_off[k + 1], 0, a.N);
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
  // (score_key.h's block_sum4, kept open-coded here: profiles/score_pair_refactor_ab.txt)
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
  if (!score_rows_ok(N) || !score_rows_ok(K)) return CCLIP_ERR_ARG;
  if (!score_operands_ok(x, ldx, c, ldc, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)assign & 3) || ((uintptr_t)best & 3) || ((uintptr_t)second & 3)) return CCLIP_ERR_ARG;
  AssignArgs a;
  a.x = (const bf16*)x; a.c = (const bf16*)c; a.ldx = ldx; a.ldc = ldc;
  a.N = (int)N; a.K = (int)K; a.D = D;
  a.assign = assign; a.best = best; a.second = second;
  const int st = score_dispatch<true>(D, N > 64, [&](auto s) {
    using S = decltype(s);
    return sweep_launch(kmeans_assign_kernel<S::KSMAX, S::MT, S::GT>, a, N, S::MT, S::GT, D, 1, 2, 0, stream);
  });
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}

#ifndef CCLIP_F16
extern "C" int64_t cclip_kmeans_update_workspace(int64_t N, int64_t K, int32_t D) {
  if (!score_rows_ok(N) || !score_rows_ok(K) || !score_dim_ok(D)) return 0;
  return (update_slabs(N) + K) * D * 4;
}
#endif

extern "C" int CCLIP_FN(cclip_kmeans_update)(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* order,
                                              const int32_t* seg_off, int64_t K, const void* prev_c, int64_t ldp, void* out_c,
                                              int64_t ldo, float* out_norm, void* workspace, int64_t workspace_bytes,
                                              hipStream_t stream) {
  if (!x || !order || !seg_off || !prev_c || !out_c || !out_norm || !workspace) return CCLIP_ERR_ARG;
  if (!score_rows_ok(N) || !score_rows_ok(K)) return CCLIP_ERR_ARG;
  if (!score_dim_ok(D) || !score_operand_ok(x, ldx, D)) return CCLIP_ERR_ARG;
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
