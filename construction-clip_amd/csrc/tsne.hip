// t-SNE of stored embeddings for gfx950: the three device steps of clip/tsne.py, all fp32 (the 16-bit rows never come here).
//
//   affinities: from the similarities of a row's k nearest other rows the conditional probabilities p_j ~ exp(-beta diff_j),
//               diff_j = d2_j - min_j d2_j, d2 = max(0, 2 - 2 s), with beta found by a FIXED number of bisection steps.
//   repulsion:  the N-body sums zrow[i] = sum_{j != i} w_ij and rep[i] = sum_{j != i} w_ij^2 (y_i - y_j), w = 1 / (1 + |y_i - y_j|^2),
//               and Z = sum_i zrow[i] in a device scalar.
//   step:       attraction over a CSR row, gradient, gains, momentum, y_out = y + vel, and the row's KL term.
//
// Affinities (tsne_affinity_kernel): one thread per row, TA_BLOCK rows per work-group; the row's k diffs sit in LDS column
// [j][thread] (no bank conflict) and are read once per step.  TSNE_BISECT_STEPS entropy evaluations, each S = sum e_j,
// T = sum diff_j e_j in ascending j, H = log S + beta T / S; H > target doubles beta (no upper bound yet) or moves the lower
// bound, else moves the upper bound; no exit depends on the data.
//
// Repulsion, three launches.  (1) tsne_repulsion_kernel: grid (row blocks of 256, splits).  A thread owns row i; its
// work-group streams the y of its split's tiles (TSNE_TILE points, 4 KiB) through LDS, every lane reads the same y_j (a
// broadcast, two points per 16-byte read).  Per pair: 2 subtractions, d2 by a multiply and an fma, 1 + d2, v_rcp_f32 (1 ulp),
// w^2, z += w and two fmas - about 10 vector operations and no MFMA.  Four accumulator sets take j = 0, 1, 2, 3 mod 4 of a
// tile and are added ((a0 + a1) + (a2 + a3)) once at the end of the split; the rest of a last short tile goes to set 0.
// Only the tile that holds the work-group's own rows tests j == i (block-uniform), and selects 0 there.  One partial
// (z, fx, fy) per (split, row) slot.  (2) tsne_merge_kernel adds a row's slots in ascending split order, writes zrow and rep
// and one sum of zrow per block of 256 rows (fixed tree).  (3) tsne_total_kernel: one work-group adds the block sums (thread t
// takes t, t + 256, .. ascending, then the same tree) into the scalar.  The split count is a function of N alone, there are
// no atomics, and every order above is fixed: two launches on the same y are bitwise equal.
//
// Step (tsne_step_kernel): one thread per row walks its CSR entries in ascending order.  Nothing here is contracted by the
// compiler; the fmas are written out.
#include "score_key.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)

#define TSNE_TILE 512                             // points of y per LDS tile
#define TSNE_ROWS 256                             // rows (threads) per repulsion work-group
#define TSNE_SPLIT_MAX 16                         // the j range is cut into at most this many splits
#define TSNE_TARGET_BLOCKS 1024                   // 256 CUs x 4 work-groups
#define TSNE_BISECT_STEPS 100
#define TA_BLOCK 128
#define TSNE_MAX_K 63

namespace cclip_tsne {

using CCLIP_NS::block_sum4;                       // the fixed-tree sum of 256 values (score_key.h)

// ---- affinities -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TA_BLOCK) void tsne_affinity_kernel(const float* __restrict__ scores, long ld, int N, int k,
                                                                 float target, float* __restrict__ P, float* __restrict__ beta_out) {
  __shared__ float diff[TSNE_MAX_K * TA_BLOCK];
  const int tid = threadIdx.x;
  const long row = (long)blockIdx.x * TA_BLOCK + tid;
  if (row >= N) return;                           // (no barrier below: a thread only reads what it wrote)
  const float* s = scores + row * ld;
  bool bad = false;
  float dmin = __builtin_huge_valf();
  for (int j = 0; j < k; ++j) {
    const float v = 2.0f - 2.0f * s[j];
    const float d2 = v < 0.0f ? 0.0f : v;         // NaN stays NaN
    bad |= d2 != d2;
    dmin = d2 < dmin ? d2 : dmin;
    diff[j * TA_BLOCK + tid] = d2;
  }
  for (int j = 0; j < k; ++j) diff[j * TA_BLOCK + tid] -= dmin;

  float beta = 1.0f, lo = 0.0f, hi = 0.0f;
  bool have_hi = false;
  for (int step = 0; step < TSNE_BISECT_STEPS; ++step) {
    float S = 0.0f, T = 0.0f;
    for (int j = 0; j < k; ++j) {
      const float d = diff[j * TA_BLOCK + tid];
      const float e = expf(-(beta * d));
      S += e;
      T += d * e;
    }
    const float H = logf(S) + beta * T / S;
    if (H > target) {
      lo = beta;
      beta = have_hi ? 0.5f * (lo + hi) : beta * 2.0f;
    } else {
      hi = beta;
      have_hi = true;
      beta = 0.5f * (lo + hi);
    }
  }
  float S = 0.0f;
  for (int j = 0; j < k; ++j) S += expf(-(beta * diff[j * TA_BLOCK + tid]));
  const float nan = __builtin_nanf("");
  for (int j = 0; j < k; ++j) P[row * k + j] = bad ? nan : expf(-(beta * diff[j * TA_BLOCK + tid])) / S;
  beta_out[row] = bad ? nan : beta;
}

// ---- repulsion --------------------------------------------------------------------------------------------------------
struct Acc { float z, fx, fy; };

__device__ __forceinline__ void pair(Acc& a, float xi, float yi, float xj, float yj) {
  const float dx = xi - xj, dy = yi - yj;
  const float w = __builtin_amdgcn_rcpf(1.0f + __builtin_fmaf(dx, dx, dy * dy));
  const float w2 = w * w;
  a.z += w;
  a.fx = __builtin_fmaf(w2, dx, a.fx);
  a.fy = __builtin_fmaf(w2, dy, a.fy);
}

// the pair (i, j) with j possibly i itself: the diagonal is selected away, not multiplied
__device__ __forceinline__ void pair_checked(Acc& a, float xi, float yi, float xj, float yj, bool self) {
  const float dx = xi - xj, dy = yi - yj;
  const float w0 = __builtin_amdgcn_rcpf(1.0f + __builtin_fmaf(dx, dx, dy * dy));
  const float w = self ? 0.0f : w0;
  const float w2 = w * w;
  a.z += w;
  a.fx = __builtin_fmaf(w2, dx, a.fx);
  a.fy = __builtin_fmaf(w2, dy, a.fy);
}

template <bool DIAG>
__device__ __forceinline__ void tile_pairs(Acc (&a)[4], float xi, float yi, const float* __restrict__ tile, int n, long self_rel) {
  const int n4 = n & ~3;
  for (int j = 0; j < n4; j += 4) {
    const f32x4 p = *(const f32x4*)(tile + 2 * j), q = *(const f32x4*)(tile + 2 * j + 4);
    if (DIAG) {
      pair_checked(a[0], xi, yi, p[0], p[1], self_rel == j);
      pair_checked(a[1], xi, yi, p[2], p[3], self_rel == j + 1);
      pair_checked(a[2], xi, yi, q[0], q[1], self_rel == j + 2);
      pair_checked(a[3], xi, yi, q[2], q[3], self_rel == j + 3);
    } else {
      pair(a[0], xi, yi, p[0], p[1]);
      pair(a[1], xi, yi, p[2], p[3]);
      pair(a[2], xi, yi, q[0], q[1]);
      pair(a[3], xi, yi, q[2], q[3]);
    }
  }
  for (int j = n4; j < n; ++j) pair_checked(a[0], xi, yi, tile[2 * j], tile[2 * j + 1], DIAG && self_rel == j);
}

// ws: [splits][3][N]
__global__ __launch_bounds__(TSNE_ROWS) void tsne_repulsion_kernel(const float* __restrict__ y, int N, int tiles_per_split,
                                                                   float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float tile[2 * TSNE_TILE];
  const int tid = threadIdx.x;
  const long row0 = (long)blockIdx.x * TSNE_ROWS;
  const long row = row0 + tid;
  const long rc = row < N ? row : (long)N - 1;    // a thread past N computes a clamped row and stores nothing
  const float xi = y[2 * rc], yi = y[2 * rc + 1];
  Acc a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u].z = a[u].fx = a[u].fy = 0.0f;

  const long ntiles = ((long)N + TSNE_TILE - 1) / TSNE_TILE;
  const long t0 = (long)blockIdx.y * tiles_per_split;
  const long t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  for (long t = t0; t < t1; ++t) {
    const long base = t * TSNE_TILE;
    const int n = (int)((long)N - base < TSNE_TILE ? (long)N - base : TSNE_TILE);
    __syncthreads();                              // every thread has left the previous tile
    for (int e = tid; e < 2 * n; e += TSNE_ROWS) tile[e] = y[2 * base + e];
    __syncthreads();
    const bool diag = base < row0 + TSNE_ROWS && row0 < base + n;      // (block-uniform) the tile holds rows of this block
    if (diag) tile_pairs<true>(a, xi, yi, tile, n, rc - base);
    else tile_pairs<false>(a, xi, yi, tile, n, -1);
  }
  if (row < N) {
    float* slot = ws + (long)blockIdx.y * 3 * N;
    slot[row] = (a[0].z + a[1].z) + (a[2].z + a[3].z);
    slot[(long)N + row] = (a[0].fx + a[1].fx) + (a[2].fx + a[3].fx);
    slot[2L * N + row] = (a[0].fy + a[1].fy) + (a[2].fy + a[3].fy);
  }
}

__global__ __launch_bounds__(256) void tsne_merge_kernel(const float* __restrict__ ws, int N, int splits, float* __restrict__ zrow,
                                                         float* __restrict__ rep, float* __restrict__ zblock) {
  __shared__ float wsum[4];
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  float z = 0.0f;
  if (row < N) {
    float fx = 0.0f, fy = 0.0f;
    for (int s = 0; s < splits; ++s) {
      const float* slot = ws + (long)s * 3 * N;
      z += slot[row];
      fx += slot[(long)N + row];
      fy += slot[2L * N + row];
    }
    zrow[row] = z;
    rep[2 * row] = fx;
    rep[2 * row + 1] = fy;
  }
  const float b = block_sum4(z, wsum);
  if (threadIdx.x == 0) zblock[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void tsne_total_kernel(const float* __restrict__ zblock, int nblocks, float* __restrict__ z_sum) {
  __shared__ float wsum[4];
  float v = 0.0f;
  for (int b = threadIdx.x; b < nblocks; b += 256) v += zblock[b];
  const float t = block_sum4(v, wsum);
  if (threadIdx.x == 0) z_sum[0] = t;
}

static inline int64_t row_blocks(int64_t N) { return (N + TSNE_ROWS - 1) / TSNE_ROWS; }

// (tiles per split, splits): a function of N alone
static inline void split_plan(int64_t N, int64_t* tps, int64_t* splits) {
  const int64_t ntiles = (N + TSNE_TILE - 1) / TSNE_TILE, rb = row_blocks(N);
  int64_t want = (TSNE_TARGET_BLOCKS + rb - 1) / rb;
  if (want > TSNE_SPLIT_MAX) want = TSNE_SPLIT_MAX;
  if (want > ntiles) want = ntiles;
  *tps = (ntiles + want - 1) / want;
  *splits = (ntiles + *tps - 1) / *tps;
}

// ---- step -------------------------------------------------------------------------------------------------------------
struct StepArgs {
  const float* y; float* vel; float* gains;
  const int64_t* offsets; const int32_t* cols; const float* vals;
  const float* rep; const float* z_sum;
  float ex, momentum, lr, min_gain;
  float* y_out; float* kl_row;
  int N; int64_t nnz;
};

__global__ __launch_bounds__(64) void tsne_step_kernel(const StepArgs a) {
  const long row = (long)blockIdx.x * 64 + threadIdx.x;
  if (row >= a.N) return;
  const float Z = a.z_sum[0];
  const float logZ = logf(Z);
  const float xi = a.y[2 * row], yi = a.y[2 * row + 1];
  int64_t e0 = a.offsets[row], e1 = a.offsets[row + 1];
  e0 = e0 < 0 ? 0 : (e0 > a.nnz ? a.nnz : e0);    // whatever the arrays hold, no access leaves cols / vals / y
  e1 = e1 < e0 ? e0 : (e1 > a.nnz ? a.nnz : e1);
  float ax = 0.0f, ay = 0.0f, kl = 0.0f;
  for (int64_t e = e0; e < e1; ++e) {
    int c = a.cols[e];
    c = c < 0 ? 0 : (c >= a.N ? a.N - 1 : c);
    const float p = a.vals[e];
    const float dx = xi - a.y[2 * (long)c], dy = yi - a.y[2 * (long)c + 1];
    const float q = 1.0f + (dx * dx + dy * dy);
    const float pw = a.ex * p / q;
    ax += pw * dx;
    ay += pw * dy;
    if (p > 0.0f) kl += p * ((logf(p) + logf(q)) + logZ);       // -log w = log(1 + d2)
  }
  if (a.kl_row) a.kl_row[row] = kl;
  if (!a.y_out) return;                           // evaluation only
  const float g[2] = {4.0f * (ax - a.rep[2 * row] / Z), 4.0f * (ay - a.rep[2 * row + 1] / Z)};
  const float pos[2] = {xi, yi};
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float v = a.vel[2 * row + d];
    float gn = a.gains[2 * row + d];
    gn = ((v > 0.0f) != (g[d] > 0.0f)) ? gn + 0.2f : gn * 0.8f;
    gn = gn < a.min_gain ? a.min_gain : gn;
    const float vn = a.momentum * v - a.lr * gn * g[d];
    a.gains[2 * row + d] = gn;
    a.vel[2 * row + d] = vn;
    a.y_out[2 * row + d] = pos[d] + vn;
  }
}

}  // namespace cclip_tsne
using namespace cclip_tsne;

extern "C" int cclip_tsne_affinities(const float* scores, int64_t ld, int64_t N, int32_t k, float perplexity, float* P, float* beta,
                                     hipStream_t stream) {
  if (!scores || !P || !beta) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || k < 1 || k > TSNE_MAX_K || ld < k) return CCLIP_ERR_ARG;
  if (!(perplexity > 1.0f) || !(perplexity < (float)k)) return CCLIP_ERR_ARG;
  if (((uintptr_t)scores & 3) || ((uintptr_t)P & 3) || ((uintptr_t)beta & 3)) return CCLIP_ERR_ARG;
  const unsigned nblk = (unsigned)((N + TA_BLOCK - 1) / TA_BLOCK);
  hipLaunchKernelGGL(tsne_affinity_kernel, dim3(nblk), dim3(TA_BLOCK), 0, stream, scores, (long)ld, (int)N, (int)k,
                     (float)log((double)perplexity), P, beta);
  return cclip_launch_status();
}

extern "C" int32_t cclip_tsne_repulsion_splits(int64_t N) {
  if (N <= 0 || N > 0x7fffffffLL) return 0;
  int64_t tps, splits;
  split_plan(N, &tps, &splits);
  return (int32_t)splits;
}

extern "C" int64_t cclip_tsne_repulsion_workspace(int64_t N) {
  if (N <= 0 || N > 0x7fffffffLL) return 0;
  int64_t tps, splits;
  split_plan(N, &tps, &splits);
  return (splits * 3 * N + row_blocks(N)) * 4;
}

extern "C" int cclip_tsne_repulsion(const float* y, int64_t N, float* zrow, float* rep, float* z_sum, void* workspace,
                                    int64_t workspace_bytes, hipStream_t stream) {
  if (!y || !zrow || !rep || !z_sum || !workspace) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL) return CCLIP_ERR_ARG;
  if (((uintptr_t)y & 7) || ((uintptr_t)zrow & 3) || ((uintptr_t)rep & 7) || ((uintptr_t)z_sum & 3) || ((uintptr_t)workspace & 3))
    return CCLIP_ERR_ARG;
  int64_t tps, splits;
  split_plan(N, &tps, &splits);
  const int64_t rb = row_blocks(N);
  if (workspace_bytes < (splits * 3 * N + rb) * 4) return CCLIP_ERR_ARG;
  float* ws = (float*)workspace;
  float* zblock = ws + splits * 3 * N;
  hipLaunchKernelGGL(tsne_repulsion_kernel, dim3((unsigned)rb, (unsigned)splits), dim3(TSNE_ROWS), 0, stream, y, (int)N, (int)tps, ws);
  hipLaunchKernelGGL(tsne_merge_kernel, dim3((unsigned)rb), dim3(256), 0, stream, ws, (int)N, (int)splits, zrow, rep, zblock);
  hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(256), 0, stream, zblock, (int)rb, z_sum);
  return cclip_launch_status();
}

extern "C" int cclip_tsne_step(const float* y, float* vel, float* gains, int64_t N, const int64_t* offsets, const int32_t* cols,
                               const float* vals, int64_t nnz, const float* rep, const float* z_sum, float exaggeration,
                               float momentum, float learning_rate, float min_gain, float* y_out, float* kl_row,
                               hipStream_t stream) {
  if (!y || !offsets || !z_sum) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || nnz < 0) return CCLIP_ERR_ARG;
  if (nnz > 0 && (!cols || !vals)) return CCLIP_ERR_ARG;
  if (!y_out && !kl_row) return CCLIP_ERR_ARG;
  if (y_out && (!vel || !gains || !rep || y_out == y)) return CCLIP_ERR_ARG;
  if (((uintptr_t)y & 3) || ((uintptr_t)vel & 3) || ((uintptr_t)gains & 3) || ((uintptr_t)offsets & 7) || ((uintptr_t)cols & 3) ||
      ((uintptr_t)vals & 3) || ((uintptr_t)rep & 3) || ((uintptr_t)z_sum & 3) || ((uintptr_t)y_out & 3) || ((uintptr_t)kl_row & 3))
    return CCLIP_ERR_ARG;
  StepArgs a;
  a.y = y; a.vel = vel; a.gains = gains; a.offsets = offsets; a.cols = cols; a.vals = vals; a.rep = rep; a.z_sum = z_sum;
  a.ex = exaggeration; a.momentum = momentum; a.lr = learning_rate; a.min_gain = min_gain;
  a.y_out = y_out; a.kl_row = kl_row; a.N = (int)N; a.nnz = nnz;
  hipLaunchKernelGGL(tsne_step_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, a);
  return cclip_launch_status();
}
