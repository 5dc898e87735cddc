// Second moments of stored embeddings for gfx950: from 16-bit rows x [N, D] and labels in [0, C),
//     count[c] = #{n : y_n = c}        sum[c, :] = sum_{y_n = c} x[n, :]        gram = sum_{live n} x[n, :]^T x[n, :]
// A row whose label lies outside [0, C) is dropped from all three (embed_probe.hip's convention); without labels every row is
// class 0.  No N x D fp32 copy, no float atomics.
//
// Both products are [onehot(y) | X]^T X.  The k index of the MFMA is the ROW of x on both operands, so both are transposed reads
// (ds_read_b64_tr_b16) of one row-major LDS tile of 32 rows - score_pair.h's tile_frag_tr on a [32][128] image.  Products of two 16-bit
// values are exact in fp32: no hi + lo pair.  The one-hot operand is built in registers from the tile's labels (compared, never
// used as an address).
//
// Jobs.  The D columns are cut into blocks of 128.  A work-group owns one 128 x 128 block of the output for one part of the
// rows: a pair (bi <= bj) of column blocks of the Gram matrix - the lower block triangle is never computed - or a (class block,
// column block) pair of the sums.  Its four waves are 2 x 2 sub-blocks of 64 x 64 = 4 x 4 MFMA tiles (64 accumulator
// registers); on a diagonal block the wave below the diagonal only helps to load.  The two column blocks of a tile of 32 rows
// go through two LDS buffers (one barrier per tile, the next tile's loads in flight under the products); a dropped row and a
// row beyond N enter LDS as zeros, so they add exactly +0.
// Non-finite values.  NaN x 0 is NaN: inside the Gram matrix that IS the row's outer product (row and column a of gram for a
// NaN in column a).  In the one-hot product it would poison column a of EVERY class, so there a non-finite element enters LDS
// as zero and is recorded instead, by an integer atomic OR into flags[y_n, a] (1 NaN, 2 +Inf, 4 -Inf); the merge turns the flags
// back into the value an fp32 sum would have had.  count is an LDS histogram per part, added by integer atomics.
//
// Order.  The rows are split into cclip_moments_parts(N, C, D) parts of tpp consecutive tiles (score_sweep.h's row_parts); a part is ONE accumulator chain
// in ascending row order, written as an fp32 partial block.  moments_merge_kernel adds the parts in a fixed two-level tree
// (runs of 8 in ascending order, the runs in ascending order) and writes gram[a, b] and gram[b, a] from the same value.  Every
// choice is a function of (N, C, D) alone; two calls are bitwise equal.
// Launches: zero (count, flags), partials, merge.
#include "score_pair.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)

#define MOM_RT 32                                 // rows per tile: one k-step
#define MOM_CB 128                                // columns (or classes) per block
#define MOM_MAX_C 256
#define MOM_BLOCK_FLOATS (MOM_CB * MOM_CB)

namespace CCLIP_NS {

struct MomGeom {
  int nb, npairs, ncb, jobs, ntiles, tpp, parts;
  int64_t off_flags, total;
};

static inline bool mom_geom(int64_t N, int64_t C, int32_t D, MomGeom& g) {
  if (!score_rows_ok(N) || C < 1 || C > MOM_MAX_C || !score_dim_ok(D)) return false;
  g.nb = (D + MOM_CB - 1) / MOM_CB;
  g.npairs = g.nb * (g.nb + 1) / 2;
  g.ncb = (int)((C + MOM_CB - 1) / MOM_CB);
  g.jobs = g.npairs + g.ncb * g.nb;
  row_parts(N, (int64_t)g.jobs * MOM_BLOCK_FLOATS * 4, &g.ntiles, &g.tpp, &g.parts);   // a part holds one fp32 block per job
  g.off_flags = (int64_t)4 * g.parts * g.jobs * MOM_BLOCK_FLOATS;
  g.total = g.off_flags + (int64_t)4 * C * D;
  return true;
}

struct MomArgs {
  const bf16* x; long ldx;
  const int* labels;                              // may be null
  int N, C, D, nb, npairs, jobs, tpp, ntiles;
  float* part;                                    // [parts][jobs][128][128]
  int* flags;                                     // [C][D]
  int* count;                                     // [C]
};

// the column-block pair (bi <= bj) of pair index p, rows of the upper block triangle in ascending order
__host__ __device__ __forceinline__ void mom_pair(int p, int nb, int& bi, int& bj) {
  bi = 0;
  while (p >= nb - bi) { p -= nb - bi; ++bi; }
  bj = bi + p;
}

__global__ __launch_bounds__(256) void moments_zero_kernel(int* __restrict__ count, int C, int* __restrict__ flags, long nflags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < C) count[i] = 0;
  if (i < nflags) flags[i] = 0;
}

// score_pair.h's tile_frag_tr on a [32][128] image at the row blocks 4 g, 16 + 4 g: element j of lane (li, g) is row
// 16 (j >> 2) + 4 g + (j & 3), column 16 dt + li - the k order both operands share
__device__ __forceinline__ bf16x8 mom_frag_tr(const char* tile, const TileGeom& geo, int dt, int lane) {
  const int g = lane >> 4;
  return tile_frag_tr(tile, geo, 4 * g, 16 + 4 * g, dt, lane);
}

__global__ __launch_bounds__(256) void moments_partial_kernel(const MomArgs a) {
  constexpr int IMG = MOM_RT * MOM_CB * 2;        // bytes of one column block of a tile
  __shared__ __attribute__((aligned(16))) char lds[2 * 2 * IMG];  // [buffer][block A, block B]
  __shared__ __attribute__((aligned(16))) int labs[2][MOM_RT];    // the tile's labels, -1 for a dropped row
  __shared__ int hist[MOM_MAX_C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int N = a.N, C = a.C, D = a.D;
  const TileGeom geo(MOM_CB);
  const int job = blockIdx.x, part = blockIdx.y;
  const bool gram = job < a.npairs;               // (uniform)
  int bi, bj;                                     // gram: the column blocks; sums: class block bi, column block bj
  if (gram) mom_pair(job, a.nb, bi, bj);
  else { bi = (job - a.npairs) / a.nb; bj = (job - a.npairs) - bi * a.nb; }
  const bool two = gram && bi != bj;              // block A is staged only where it differs from block B
  const int t0 = part * a.tpp, t1 = min(t0 + a.tpp, a.ntiles);    // (t0 < ntiles: the grid has no empty part)

  // count: job 0 of every part takes its rows' labels through an LDS histogram
  if (job == 0) {
    const long r0 = (long)t0 * MOM_RT, r1 = min((long)t1 * MOM_RT, (long)N);
    if (!a.labels) {
      if (tid == 0) atomicAdd(a.count, (int)(r1 - r0));
    } else {
      hist[tid] = 0;
      __syncthreads();
      for (long r = r0 + tid; r < r1; r += 256) {
        const int y = a.labels[r];
        if (y >= 0 && y < C) atomicAdd(&hist[y], 1);
      }
      __syncthreads();
      if (tid < C && hist[tid]) atomicAdd(a.count + tid, hist[tid]);
    }
  }

  // this thread moves chunk ch of the rows rr and rr + 16 of either block
  const int rr = tid >> 4, ch = tid & 15;
  const bool ina = 128 * bi + 8 * ch < D, inb = 128 * bj + 8 * ch < D;     // D % 8 == 0: a chunk is inside or outside
  u32x4 sa[2], sb[2];
  int ylab[2];
  auto fetch = [&](int t) CCLIP_SWEEP_INLINE {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const long row = (long)t * MOM_RT + rr + 16 * it;
      const long rc = min(row, (long)N - 1);
      const int y = a.labels ? a.labels[rc] : 0;
      ylab[it] = (row < N && y >= 0 && y < C) ? y : -1;
      const bf16* p = a.x + rc * a.ldx + 8 * ch;
      sb[it] = inb ? *(const u32x4*)(p + 128 * bj) : (u32x4){0u, 0u, 0u, 0u};
      if (two) sa[it] = ina ? *(const u32x4*)(p + 128 * bi) : (u32x4){0u, 0u, 0u, 0u};
    }
  };
#ifdef CCLIP_F16
  constexpr unsigned EXPM = 0x7c00u, MANT = 0x03ffu;
#else
  constexpr unsigned EXPM = 0x7f80u, MANT = 0x007fu;
#endif
  auto store = [&](int buf) CCLIP_SWEEP_INLINE {
    char* A = lds + buf * 2 * IMG;
    char* B = A + IMG;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = rr + 16 * it;
      if (ylab[it] < 0) { sa[it] = (u32x4){0u, 0u, 0u, 0u}; sb[it] = (u32x4){0u, 0u, 0u, 0u}; }
      else if (!gram) {
        // the one-hot product: a non-finite element is recorded and enters as zero (0 x NaN would reach every class)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          unsigned word = sb[it][w];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned e = (word >> (16 * h)) & 0xffffu;
            if ((e & EXPM) == EXPM) {
              const int code = (e & MANT) ? 1 : ((e & 0x8000u) ? 4 : 2);
              if (bi == 0) atomicOr(a.flags + (long)ylab[it] * D + 128 * bj + 8 * ch + 2 * w + h, code);
              word &= ~(0xffffu << (16 * h));
            }
          }
          sb[it][w] = word;
        }
      }
      *(u32x4*)(B + geo.off(row, ch)) = sb[it];
      if (two) *(u32x4*)(A + geo.off(row, ch)) = sa[it];
      if (ch == 0) labs[buf][row] = ylab[it];
    }
  };

  const int wi = wave >> 1, wj = wave & 1;        // the wave's 64 x 64 sub-block
  const bool active = !(gram && bi == bj && wi > wj);             // (wave-uniform) below the diagonal: only helps to load
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  fetch(t0);
  int buf = 0;
  for (int t = t0; t < t1; ++t, buf ^= 1) {
    store(buf);
    __syncthreads();                              // tile t is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < t1) fetch(t + 1);
    if (!active) continue;                        // (wave-uniform)
    const char* B = lds + buf * 2 * IMG + IMG;
    const char* A = two ? B - IMG : B;
    bf16x8 bf[4], af[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = mom_frag_tr(B, geo, 4 * wj + j, lane);
    if (gram) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = mom_frag_tr(A, geo, 4 * wi + i, lane);
    } else {
      const int4 y0 = *(const int4*)&labs[buf][4 * g], y1 = *(const int4*)&labs[buf][16 + 4 * g];
      const int yy[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cls = MOM_CB * bi + 64 * wi + 16 * i + li;
#pragma unroll
        for (int j = 0; j < 8; ++j) af[i][j] = (bf16)(yy[j] == cls ? 1.0f : 0.0f);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = CCLIP_MFMA_16x16x32(af[i], bf[j], acc[i][j]);
  }
  if (!active) return;

  // lane (li, g) holds [64 wi + 16 i + 4 g + r][64 wj + 16 j + li] of the block
  float* out = a.part + ((long)part * a.jobs + job) * MOM_BLOCK_FLOATS;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(64 * wi + 16 * i + 4 * g + r) * MOM_CB + 64 * wj + 16 * j + li] = acc[i][j][r];
}

// the parts of one entry: runs of 8 in ascending order, the runs in ascending order
__device__ __forceinline__ float mom_tree(const float* p, long stride, int parts) {
  float total = 0.0f;
  for (int s0 = 0; s0 < parts; s0 += 8) {
    float run = p[s0 * stride];
    const int s1 = min(s0 + 8, parts);
    for (int s = s0 + 1; s < s1; ++s) run += p[s * stride];
    total = s0 == 0 ? run : total + run;
  }
  return total;
}

struct MomMergeArgs {
  const float* part; const int* flags;
  int C, D, nb, npairs, jobs, parts;
  float* sum; float* gram;
};

__global__ __launch_bounds__(256) void moments_merge_kernel(const MomMergeArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long ngram = (long)a.D * a.D;
  const long stride = (long)a.jobs * MOM_BLOCK_FLOATS;
  if (idx < ngram) {
    const int r = (int)(idx / a.D), c = (int)(idx - (long)r * a.D);
    if (r > c) return;                            // written by its mirror
    const int bi = r >> 7, bj = c >> 7;
    const int job = bi * a.nb - bi * (bi - 1) / 2 + (bj - bi);
    const float v = mom_tree(a.part + (long)job * MOM_BLOCK_FLOATS + (r & 127) * MOM_CB + (c & 127), stride, a.parts);
    a.gram[(long)r * a.D + c] = v;
    a.gram[(long)c * a.D + r] = v;
    return;
  }
  const long k = idx - ngram;
  if (k >= (long)a.C * a.D) return;
  const int cls = (int)(k / a.D), d = (int)(k - (long)cls * a.D);
  const int job = a.npairs + (cls >> 7) * a.nb + (d >> 7);
  float v = mom_tree(a.part + (long)job * MOM_BLOCK_FLOATS + (cls & 127) * MOM_CB + (d & 127), stride, a.parts);
  const int f = a.flags[k];
  if (f) {                                        // what the fp32 sum of the recorded values would have been
    const float inf = __builtin_huge_valf();
    v = ((f & 1) || (f & 6) == 6) ? __uint_as_float(0x7fc00000u) : ((f & 2) ? inf : -inf);
  }
  a.sum[k] = v;
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_moments_workspace(int64_t N, int32_t C, int32_t D) {
  MomGeom g;
  return mom_geom(N, C, D, g) ? g.total : 0;
}

extern "C" int32_t cclip_moments_parts(int64_t N, int32_t C, int32_t D) {
  MomGeom g;
  return mom_geom(N, C, D, g) ? g.parts : 0;
}
#endif

extern "C" int CCLIP_FN(cclip_class_moments)(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* labels, int32_t C,
                                              int32_t* count, float* sum, float* gram, void* workspace, int64_t workspace_bytes,
                                              hipStream_t stream) {
  MomGeom g;
  if (!x || !count || !sum || !gram || !workspace) return CCLIP_ERR_ARG;
  if (!mom_geom(N, C, D, g)) return CCLIP_ERR_ARG;
  if (!labels && C != 1) return CCLIP_ERR_ARG;
  if (!score_operand_ok(x, ldx, D) || ((uintptr_t)workspace & 15)) return CCLIP_ERR_ARG;
  if (((uintptr_t)labels & 3) || ((uintptr_t)count & 3) || ((uintptr_t)sum & 3) || ((uintptr_t)gram & 3)) return CCLIP_ERR_ARG;
  if (workspace_bytes < g.total) return CCLIP_ERR_ARG;
  char* ws = (char*)workspace;
  MomArgs a;
  a.x = (const bf16*)x; a.ldx = ldx; a.labels = labels;
  a.N = (int)N; a.C = C; a.D = D; a.nb = g.nb; a.npairs = g.npairs; a.jobs = g.jobs; a.tpp = g.tpp; a.ntiles = g.ntiles;
  a.part = (float*)ws; a.flags = (int*)(ws + g.off_flags); a.count = count;
  const long nflags = (long)C * D;
  hipLaunchKernelGGL(moments_zero_kernel, dim3((unsigned)((nflags + 255) / 256)), dim3(256), 0, stream, count, C, a.flags, nflags);
  hipLaunchKernelGGL(moments_partial_kernel, dim3(g.jobs, g.parts), dim3(256), 0, stream, a);
  MomMergeArgs m;
  m.part = a.part; m.flags = a.flags; m.C = C; m.D = D; m.nb = g.nb; m.npairs = g.npairs; m.jobs = g.jobs; m.parts = g.parts;
  m.sum = sum; m.gram = gram;
  const long cells = (long)D * D + nflags;
  hipLaunchKernelGGL(moments_merge_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, m);
  return cclip_launch_status();
}
