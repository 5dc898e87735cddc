// Label spreading over the kNN graph for gfx950 (Zhou et al. 2004): the three device steps of clip/propagate.py, all fp32.
//
//   normalize: d_i = sum of row i's weights, r_i = 1 / sqrt(d_i) (0 where d_i is not > 0), S_ij = (W_ij r_i) r_j.
//   step:      F_out = alpha S F_in + (1 - alpha) Y, Y the (weighted) one-hot labels; optionally the row's largest change.
//   finish:    per row z = sum_c F_ic, p = F / z, the argmax of F, max p and the certainty 1 - H(p) / log C.
//
// Step (spread_step_kernel<CW, G, NQ>).  The kernel is a gather: per CSR entry it reads one row of F_in, 4 C bytes, at a random
// place.  The classes that matter are C = 2 and C = 9, so a row is not given a wave but a TEAM of T = G * CW lanes, CW = the
// power of two >= min(C, 64) and G = min(8, 64 / CW) - a function of C alone (spread_plan):
//       C      2   3..4   5..8   9..16   17..32   33..64   65..128   129..1024
//       CW     2     4      8     16       32       64       64         64
//       G      8     8      8      4        2        1        1          1
//       NQ     1     1      1      1        1        1        2          4
// 64 / T rows share a wave and 4 * 64 / T a work-group of 256 threads (16 rows per wave at C = 2).  Lane l of a team is edge
// group g = l / CW and class slot c = l % CW.  Order of a sum: group g takes the row's entries at positions g, g + G, g + 2G, ..
// of the row in ascending order as one fma chain starting from 0 (a hub row is a long chain in its team; nothing is scheduled
// by the data), then the G chains are added in the xor tree over lane offsets CW, 2 CW, .., T / 2, i.e.
// ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)); both operands of every level are the same pair in every lane, so every
// lane of the team ends with the same bits.  For C > 64 a lane owns the NQ classes c, c + 64, .., in registers, and C > 256
// takes ceil(C / 256) passes over the row's entries, one per chunk of 256 classes.  The label term is cw - alpha cw rounded
// once (fma), the result fma(alpha, sum, label term).  No atomics: two launches are bitwise equal.
//
// Normalize: two launches, one thread per row, the row's entries in ascending order.  Finish: one team of CW lanes per row,
// lane c adds classes c, c + CW, .. ascending, then the xor tree over offsets 1 .. CW / 2; the argmax takes the larger value
// and, at equal values, the lower class.
//
// offsets and cols are clamped before use in every kernel: no CSR content makes a kernel leave its arrays.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)

#define LS_MAX_C 1024
#define LS_BLOCK 256

namespace cclip_label_spread {

__device__ __forceinline__ void row_range(const int64_t* __restrict__ offsets, long row, int64_t nnz, int64_t& e0, int64_t& e1) {
  e0 = offsets[row];
  e1 = offsets[row + 1];
  e0 = e0 < 0 ? 0 : (e0 > nnz ? nnz : e0);        // whatever the arrays hold, no access leaves cols / vals
  e1 = e1 < e0 ? e0 : (e1 > nnz ? nnz : e1);
}

__device__ __forceinline__ int clamp_col(int c, int N) { return c < 0 ? 0 : (c >= N ? N - 1 : c); }

// ---- normalize --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LS_BLOCK) void degree_kernel(const int64_t* __restrict__ offsets, const float* __restrict__ vals, int N,
                                                          int64_t nnz, float* __restrict__ deg) {
  const long row = (long)blockIdx.x * LS_BLOCK + threadIdx.x;
  if (row >= N) return;
  int64_t e0, e1;
  row_range(offsets, row, nnz, e0, e1);
  float d = 0.0f;
  for (int64_t e = e0; e < e1; ++e) d += vals[e];
  deg[row] = d;
}

__device__ __forceinline__ float inv_sqrt_deg(float d) { return d > 0.0f ? 1.0f / sqrtf(d) : 0.0f; }   // NaN -> 0 as well

// vals_out may be vals: an entry is read and written by the one thread that owns its row
__global__ __launch_bounds__(LS_BLOCK) void scale_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ cols,
                                                         const float* vals, int N, int64_t nnz, const float* __restrict__ deg,
                                                         float* vals_out) {
  const long row = (long)blockIdx.x * LS_BLOCK + threadIdx.x;
  if (row >= N) return;
  int64_t e0, e1;
  row_range(offsets, row, nnz, e0, e1);
  const float ri = inv_sqrt_deg(deg[row]);
  for (int64_t e = e0; e < e1; ++e) {
    const float rj = inv_sqrt_deg(deg[clamp_col(cols[e], N)]);
    vals_out[e] = (vals[e] * ri) * rj;
  }
}

// ---- step -------------------------------------------------------------------------------------------------------------
struct StepArgs {
  const float* F_in; float* F_out;
  const int32_t* labels; const float* class_weight;
  const int64_t* offsets; const int32_t* cols; const float* vals;
  float* delta_row;
  float alpha;
  int N, C; int64_t nnz;
};

// NaN-sticky maximum: the result is NaN if any operand is
__device__ __forceinline__ float nan_max(float m, float d) { return (d > m || d != d) ? d : m; }

template <int CW, int G, int NQ>
__global__ __launch_bounds__(LS_BLOCK) void spread_step_kernel(const StepArgs a) {
  constexpr int T = CW * G;                       // lanes of a row's team
  constexpr int ROWS = LS_BLOCK / T;              // rows of a work-group
  const int tid = threadIdx.x;
  const int l = tid % T, g = l / CW, cl = l % CW;
  const long row = (long)blockIdx.x * ROWS + tid / T;
  const bool live = row < a.N;                    // a team is live or not as a whole; nobody leaves before the shuffles
  const long rc = live ? row : (long)a.N - 1;
  int64_t e0, e1;
  row_range(a.offsets, rc, a.nnz, e0, e1);
  const int lab = a.labels[rc];
  float delta = 0.0f;
  for (int cbase = 0; cbase < a.C; cbase += CW * NQ) {                           // one pass unless C > 256
    float acc[NQ];
    bool on[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      acc[q] = 0.0f;
      on[q] = cbase + cl + CW * q < a.C;
    }
    const float* Fc = a.F_in + cbase + cl;
    int64_t e = e0 + g;
    for (; e + 3 * G < e1; e += 4 * G) {                                         // four entries' loads in flight, one chain
      int col[4];
      float v[4], f[4][NQ];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        col[u] = clamp_col(a.cols[e + u * G], a.N);
        v[u] = a.vals[e + u * G];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < NQ; ++q) f[u][q] = on[q] ? Fc[(long)col[u] * a.C + CW * q] : 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = __builtin_fmaf(v[u], f[u][q], acc[q]);
    }
    for (; e < e1; e += G) {
      const int col = clamp_col(a.cols[e], a.N);
      const float v = a.vals[e];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = __builtin_fmaf(v, on[q] ? Fc[(long)col * a.C + CW * q] : 0.0f, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
      for (int o = CW; o < T; o <<= 1) acc[q] += __shfl_xor(acc[q], o, 64);      // the fixed tree over the edge groups
      const int c = cbase + cl + CW * q;
      if (on[q]) {
        const float cw = a.class_weight ? a.class_weight[c] : 1.0f;
        const float y = lab == c ? __builtin_fmaf(-a.alpha, cw, cw) : 0.0f;      // (1 - alpha) cw, rounded once
        const float out = __builtin_fmaf(a.alpha, acc[q], y);
        if (a.delta_row) delta = nan_max(delta, fabsf(out - a.F_in[rc * a.C + c]));
        if (live && g == 0) a.F_out[row * a.C + c] = out;
      }
    }
  }
  if (a.delta_row) {
#pragma unroll
    for (int o = 1; o < CW; o <<= 1) delta = nan_max(delta, __shfl_xor(delta, o, 64));
    if (live && l == 0) a.delta_row[row] = delta;
  }
}

// ---- finish -----------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(LS_BLOCK) void spread_finish_kernel(const float* __restrict__ F, int N, int C, float* __restrict__ dist,
                                                                 int32_t* __restrict__ pred, float* __restrict__ conf,
                                                                 float* __restrict__ cert) {
  constexpr int ROWS = LS_BLOCK / CW;
  const int tid = threadIdx.x, cl = tid % CW;
  const long row = (long)blockIdx.x * ROWS + tid / CW;
  const bool live = row < N;
  const float* f = F + (live ? row : (long)N - 1) * C;
  float z = 0.0f, best = -__builtin_huge_valf();
  int arg = 0x7fffffff;
  for (int c = cl; c < C; c += CW) {
    const float v = f[c];
    z += v;
    if (v > best) { best = v; arg = c; }          // ascending c: the lowest class of equal values stays
  }
#pragma unroll
  for (int o = 1; o < CW; o <<= 1) {
    z += __shfl_xor(z, o, 64);
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  const bool pos = z > 0.0f, bad = z != z;        // neither: z == 0 (or below), a row no label reaches
  const float nan = __builtin_nanf("");
  float h = 0.0f;
  for (int c = cl; c < C; c += CW) {
    const float p = pos ? f[c] / z : (bad ? nan : 0.0f);
    if (p > 0.0f) h += p * logf(p);               // 0 log 0 = 0
    if (live && dist) dist[row * C + c] = p;
  }
#pragma unroll
  for (int o = 1; o < CW; o <<= 1) h += __shfl_xor(h, o, 64);
  if (live && cl == 0) {
    pred[row] = pos ? arg : -1;
    conf[row] = pos ? best / z : (bad ? nan : 0.0f);
    cert[row] = pos ? 1.0f + h / logf((float)C) : (bad ? nan : 0.0f);
  }
}

// (class lanes CW, edge groups G, classes per lane NQ): a function of C alone
static inline void spread_plan(int C, int* cw, int* g, int* nq) {
  int w = 2;
  while (w < C && w < 64) w <<= 1;
  *cw = w;
  *g = 64 / w < 8 ? 64 / w : 8;
  *nq = C <= 64 ? 1 : (C <= 128 ? 2 : 4);
}

template <int CW, int G, int NQ>
static inline void launch_step(const StepArgs& a, hipStream_t stream) {
  const int rows = LS_BLOCK / (CW * G);
  hipLaunchKernelGGL((spread_step_kernel<CW, G, NQ>), dim3((unsigned)(((int64_t)a.N + rows - 1) / rows)), dim3(LS_BLOCK), 0, stream, a);
}

template <int CW>
static inline void launch_finish(const float* F, int N, int C, float* dist, int32_t* pred, float* conf, float* cert, hipStream_t stream) {
  const int rows = LS_BLOCK / CW;
  hipLaunchKernelGGL((spread_finish_kernel<CW>), dim3((unsigned)(((int64_t)N + rows - 1) / rows)), dim3(LS_BLOCK), 0, stream, F, N, C,
                     dist, pred, conf, cert);
}

}  // namespace cclip_label_spread
using namespace cclip_label_spread;

extern "C" int cclip_label_graph_normalize(const int64_t* offsets, const int32_t* cols, const float* vals, int64_t N, int64_t nnz,
                                           float* deg, float* vals_out, hipStream_t stream) {
  if (!offsets || !deg) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || nnz < 0 || nnz > 0x7fffffffLL) return CCLIP_ERR_ARG;
  if (nnz > 0 && (!cols || !vals || !vals_out)) return CCLIP_ERR_ARG;
  if (((uintptr_t)offsets & 7) || ((uintptr_t)cols & 3) || ((uintptr_t)vals & 3) || ((uintptr_t)deg & 3) || ((uintptr_t)vals_out & 3))
    return CCLIP_ERR_ARG;
  const unsigned nblk = (unsigned)((N + LS_BLOCK - 1) / LS_BLOCK);
  hipLaunchKernelGGL(degree_kernel, dim3(nblk), dim3(LS_BLOCK), 0, stream, offsets, vals, (int)N, nnz, deg);
  hipLaunchKernelGGL(scale_kernel, dim3(nblk), dim3(LS_BLOCK), 0, stream, offsets, cols, vals, (int)N, nnz, (const float*)deg, vals_out);
  return cclip_launch_status();
}

extern "C" int32_t cclip_label_spread_groups(int32_t C) {
  if (C < 2 || C > LS_MAX_C) return 0;
  int cw, g, nq;
  spread_plan(C, &cw, &g, &nq);
  return g;
}

extern "C" int cclip_label_spread_step(const float* F_in, float* F_out, int64_t N, int32_t C, const int32_t* labels,
                                       const float* class_weight, const int64_t* offsets, const int32_t* cols, const float* vals,
                                       int64_t nnz, float alpha, float* delta_row, hipStream_t stream) {
  if (!F_in || !F_out || !labels || !offsets || F_in == F_out) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || nnz < 0 || nnz > 0x7fffffffLL || C < 2 || C > LS_MAX_C) return CCLIP_ERR_ARG;
  if (nnz > 0 && (!cols || !vals)) return CCLIP_ERR_ARG;
  if (!(alpha >= 0.0f) || !(alpha <= 1.0f)) return CCLIP_ERR_ARG;
  if (((uintptr_t)F_in & 3) || ((uintptr_t)F_out & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)class_weight & 3) ||
      ((uintptr_t)offsets & 7) || ((uintptr_t)cols & 3) || ((uintptr_t)vals & 3) || ((uintptr_t)delta_row & 3))
    return CCLIP_ERR_ARG;
  StepArgs a;
  a.F_in = F_in; a.F_out = F_out; a.labels = labels; a.class_weight = class_weight; a.offsets = offsets; a.cols = cols;
  a.vals = vals; a.delta_row = delta_row; a.alpha = alpha; a.N = (int)N; a.C = (int)C; a.nnz = nnz;
  int cw, g, nq;
  spread_plan((int)C, &cw, &g, &nq);
  if (nq == 4) launch_step<64, 1, 4>(a, stream);
  else if (nq == 2) launch_step<64, 1, 2>(a, stream);
  else if (cw == 64) launch_step<64, 1, 1>(a, stream);
  else if (cw == 32) launch_step<32, 2, 1>(a, stream);
  else if (cw == 16) launch_step<16, 4, 1>(a, stream);
  else if (cw == 8) launch_step<8, 8, 1>(a, stream);
  else if (cw == 4) launch_step<4, 8, 1>(a, stream);
  else launch_step<2, 8, 1>(a, stream);
  return cclip_launch_status();
}

extern "C" int cclip_label_spread_finish(const float* F, int64_t N, int32_t C, float* dist, int32_t* pred, float* conf, float* cert,
                                         hipStream_t stream) {
  if (!F || !pred || !conf || !cert) return CCLIP_ERR_ARG;
  if (N <= 0 || N > 0x7fffffffLL || C < 2 || C > LS_MAX_C) return CCLIP_ERR_ARG;
  if (((uintptr_t)F & 3) || ((uintptr_t)dist & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)conf & 3) || ((uintptr_t)cert & 3))
    return CCLIP_ERR_ARG;
  int cw, g, nq;
  spread_plan((int)C, &cw, &g, &nq);
  if (cw == 64) launch_finish<64>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  else if (cw == 32) launch_finish<32>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  else if (cw == 16) launch_finish<16>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  else if (cw == 8) launch_finish<8>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  else if (cw == 4) launch_finish<4>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  else launch_finish<2>(F, (int)N, (int)C, dist, pred, conf, cert, stream);
  return cclip_launch_status();
}
