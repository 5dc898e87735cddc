// Attention relevance (Chefer et al.) of one layer for gfx950, T <= 128, head_dim 64: the per-layer step of the reference's
// `interpret()` (attention.py:14-69), fused so that neither the attention probabilities P nor their gradient
// dP ever reach HBM.  For every sequence b (length T_b):
//     P_h  = exp(scale Q_h K_h^T - lse_h)            (causal: 0 above the diagonal; rows / keys >= T_b: 0)
//     dP_h = dA_h V_h^T                              (dA: gradient at the attention output, from the dgrad chain)
//     C    = 1 / (H grad_scale) * sum_h max(P_h (.) dP_h, 0)
//     R[:T_b, :T_b] <- R[:T_b, :T_b] + R[:T_b, :T_b] C     (R fp32 [B, T, T], updated in place; the rest of R is not touched)
// The backward visits the layers top-down, so right-multiplying reaches the reference's bottom-up product
// (I + C_{L-1}) ... (I + C_s) without storing the L per-layer maps.
//
// One workgroup (4 waves) per sequence.  Heads are looped; each wave keeps the same query tiles for every head, so C sums
// across heads in registers (fixed order: no atomics, bitwise reproducible).  K and V of the head are staged in LDS with
// head_load / head_store (attention_tiles.h), the next head's loads in flight under this head's MFMAs; the tile itself -
// S = Q K^T, dP = dA V^T, the mask and max(P dP, 0) - is rel_tile of attention_relevance_core.h, shared with the row kernel.
// After the head loop C goes to LDS as fp32 (reusing the head operands' space); each wave then forms rows
// of R C from R rows it holds in registers (one row's columns across the lanes, broadcast with readlane) and writes them back.
#include "attention_relevance_core.h"

namespace CCLIP_NS {

struct RelArgs : RelCommon { float* R; };         // R: [B, T, T]

// (second bound = waves per SIMD: unbounded, <5> - T <= 80, the text tower's 77 - allocates 172 registers, which is two waves, not three)
template <int NKT>
__global__ __launch_bounds__(256, NKT <= 5 ? 3 : 2) void attn_relevance_kernel(const RelArgs a) {
  constexpr int TP = 16 * NKT;                    // padded tokens
  constexpr int NQW = (NKT + 3) / 4;              // query tiles per wave
  constexpr int CLD = TP + 4;                     // row stride of C in LDS (floats; even: 8-byte aligned column pairs)
  constexpr int IT = (TP * 8 + 255) / 256;        // 16-byte chunks of one head operand per thread
  constexpr int OPB = 2 * TP * 128, CB = TP * CLD * 4;
  __shared__ __attribute__((aligned(16))) char smem[OPB > CB ? OPB : CB];
  char* Ks = smem;
  char* Vs = smem + TP * 128;
  float* Cs = (float*)smem;                       // after the head loop
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  long row0;
  const int T = rel_seq(a, b, row0);
  if (T <= 0) return;                             // (workgroup-uniform)
  const int nqt = (T + 15) >> 4;

  f32x4 c[NQW][NKT];
#pragma unroll
  for (int i = 0; i < NQW; ++i)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) c[i][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 rk[IT], rv[IT];
  auto kv_load = [&](int h) {
    head_load<IT>(a.k + h * 64, a.ldk, row0, T, rk, tid);
    head_load<IT>(a.v + h * 64, a.ldv, row0, T, rv, tid);
  };
  kv_load(0);
  for (int h = 0; h < a.H; ++h) {
    __syncthreads();                              // everyone is done with the previous head's K / V
    head_store<IT>(Ks, T, TP, rk, tid);
    head_store<IT>(Vs, T, TP, rv, tid);
    if (h + 1 < a.H) kv_load(h + 1);              // in flight under this head's MFMAs
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NQW; ++i) {
      const int qt = wave + 4 * i;
      if (qt >= nqt) continue;                    // (wave-uniform)
      const RelQTile q = rel_qtile(a, row0, b, h, qt, T, lane);
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt >= nqt || (a.causal && kt > qt)) continue;
        c[i][kt] += rel_tile(a, q, Ks, Vs, qt, kt, 0, T, lane);
      }
    }
  }
  __syncthreads();                                // K / V images are dead: C takes their place
#pragma unroll
  for (int i = 0; i < NQW; ++i) {
    const int qt = wave + 4 * i;
    if (qt >= NKT) continue;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[(16 * qt + 4 * g + r) * CLD + 16 * kt + li] = c[i][kt][r] * a.cscale;
  }
  __syncthreads();

  // R[i, :T] += R[i, :T] C for the rows i < T: wave w takes rows 8w + 32n + u (u < 8); lane l holds columns 2l, 2l + 1.
  // The wave reads its rows whole before it writes any of them, and no other wave touches them.
  constexpr int RB = 8;
  float* Rb = a.R + (long)b * a.T * a.T;
  const int j0 = 2 * lane, jc = j0 < TP ? j0 : 0;   // (lanes past the padded width read a valid column and store nothing)
  for (int ib = RB * wave; ib < T; ib += 4 * RB) {
    float rx[RB], ry[RB], ax[RB], ay[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int i = ib + u;
      const float* rp = Rb + (long)(i < T ? i : 0) * a.T;
      rx[u] = (i < T && j0 < T) ? rp[j0] : 0.f;
      ry[u] = (i < T && j0 + 1 < T) ? rp[j0 + 1] : 0.f;
      ax[u] = 0.f; ay[u] = 0.f;
    }
    for (int k2 = 0; 2 * k2 < T; ++k2) {          // rows 2 k2, 2 k2 + 1 of C (row T of C, if read, is zero)
      const float2 c0 = *(const float2*)(Cs + (2 * k2) * CLD + jc);
      const float2 c1 = *(const float2*)(Cs + (2 * k2 + 1) * CLD + jc);
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rx[u]), k2));
        const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ry[u]), k2));
        ax[u] = fmaf(r0, c0.x, ax[u]); ay[u] = fmaf(r0, c0.y, ay[u]);
        ax[u] = fmaf(r1, c1.x, ax[u]); ay[u] = fmaf(r1, c1.y, ay[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int i = ib + u;
      if (i >= T) break;
      float* rp = Rb + (long)i * a.T;
      if (j0 < T) rp[j0] = rx[u] + ax[u];
      if (j0 + 1 < T) rp[j0 + 1] = ry[u] + ay[u];
    }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_attention_relevance)(const cclip_attn_desc* d, float grad_scale, float* R, hipStream_t stream) {
  RelArgs a;
  if (rel_common_from_desc(d, grad_scale, 128, a) != CCLIP_OK || !R || ((uintptr_t)R & 3)) return CCLIP_ERR_ARG;
  a.R = R;
  const int nkt = (d->T + 15) / 16;
  dim3 grid(d->B), block(256);
  if (nkt <= 2) hipLaunchKernelGGL((attn_relevance_kernel<2>), grid, block, 0, stream, a);
  else if (nkt <= 4) hipLaunchKernelGGL((attn_relevance_kernel<4>), grid, block, 0, stream, a);
  else if (nkt <= 5) hipLaunchKernelGGL((attn_relevance_kernel<5>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((attn_relevance_kernel<8>), grid, block, 0, stream, a);
  return cclip_launch_status();
}
