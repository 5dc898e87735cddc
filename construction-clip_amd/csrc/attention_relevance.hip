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
// across heads in registers (fixed order: no atomics, bitwise reproducible).  Both products are v_mfma_f32_16x16x32 with the
// query on the accumulator rows, exactly as in attn_bwd_kernel (attention.hip): S = Q K^T and dP = dA V^T, K and V of the
// head staged in LDS ([row][64] 16-bit, 16-byte chunk c of row r at chunk c ^ (r & 7)), Q and dA rows read straight into
// the A fragments.  After the head loop C goes to LDS as fp32 (reusing the head operands' space); each wave then forms rows
// of R C from R rows it holds in registers (one row's columns across the lanes, broadcast with readlane) and writes them back.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct RelArgs {
  const bf16* q; const bf16* k; const bf16* v;   // row (b*T + t) (or cu[b] + t), head h at column h*64
  long ldq, ldk, ldv;
  const bf16* da; long ldda;                      // gradient at the attention output, same layout
  const float* lse;                               // [B, H, T]
  const int* cu;                                  // packed batch: sequence b is rows [cu[b], cu[b+1]); null: row b*T + t
  float* R;                                       // [B, T, T]
  int B, T, H, causal;
  float scale, cscale;                            // cscale = 1 / (H * grad_scale)
};

__device__ __forceinline__ int rel_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

template <int NKT>
__global__ __launch_bounds__(256) void attn_relevance_kernel(const RelArgs a) {
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
  int T = a.cu ? a.cu[b + 1] - a.cu[b] : a.T;
  T = T < a.T ? T : a.T;
  if (T <= 0) return;                             // (workgroup-uniform)
  const long row0 = a.cu ? (long)a.cu[b] : (long)b * a.T;
  const int nqt = (T + 15) >> 4;

  f32x4 c[NQW][NKT];
#pragma unroll
  for (int i = 0; i < NQW; ++i)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) c[i][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 rk[IT], rv[IT];
  auto head_load = [&](int h) {                   // every 16-byte load of head h's K and V, rows clamped (no predicated loads)
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = tid + 256 * it, row = idx >> 3, ch = idx & 7;
      const long gr = row0 + (row < T ? row : T - 1);
      rk[it] = *(const uint4*)(a.k + gr * a.ldk + h * 64 + ch * 8);
      rv[it] = *(const uint4*)(a.v + gr * a.ldv + h * 64 + ch * 8);
    }
  };
  head_load(0);
  for (int h = 0; h < a.H; ++h) {
    __syncthreads();                              // everyone is done with the previous head's K / V
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = tid + 256 * it, row = idx >> 3, ch = idx & 7;
      if (row < TP) {
        *(uint4*)(Ks + rel_off(row, ch)) = row < T ? rk[it] : make_uint4(0, 0, 0, 0);
        *(uint4*)(Vs + rel_off(row, ch)) = row < T ? rv[it] : make_uint4(0, 0, 0, 0);
      }
    }
    if (h + 1 < a.H) head_load(h + 1);            // in flight under this head's MFMAs
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NQW; ++i) {
      const int qt = wave + 4 * i;
      if (qt >= nqt) continue;                    // (wave-uniform)
      const int qr = 16 * qt + li < T ? 16 * qt + li : T - 1;
      const bf16* qp = a.q + (row0 + qr) * a.ldq + h * 64 + 8 * g;
      const bf16* dp_ = a.da + (row0 + qr) * a.ldda + h * 64 + 8 * g;
      const bf16x8 qf0 = *(const bf16x8*)qp, qf1 = *(const bf16x8*)(qp + 32);
      const bf16x8 df0 = *(const bf16x8*)dp_, df1 = *(const bf16x8*)(dp_ + 32);
      float lsv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = 16 * qt + 4 * g + r;
        lsv[r] = qi < T ? a.lse[((long)b * a.H + h) * a.T + qi] : 0.f;
      }
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt >= nqt || (a.causal && kt > qt)) continue;
        const int key = 16 * kt + li;
        f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        sv = CCLIP_MFMA_16x16x32(qf0, *(const bf16x8*)(Ks + rel_off(key, g)), sv);
        sv = CCLIP_MFMA_16x16x32(qf1, *(const bf16x8*)(Ks + rel_off(key, 4 + g)), sv);
        dp = CCLIP_MFMA_16x16x32(df0, *(const bf16x8*)(Vs + rel_off(key, g)), dp);
        dp = CCLIP_MFMA_16x16x32(df1, *(const bf16x8*)(Vs + rel_off(key, 4 + g)), dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = 16 * qt + 4 * g + r;
          const bool ok = qi < T && key < T && (!a.causal || key <= qi);
          const float pv = ok ? __expf(sv[r] * a.scale - lsv[r]) : 0.f;
          c[i][kt][r] += ok ? fmaxf(pv * dp[r], 0.f) : 0.f;
        }
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
  if (!d || !d->q || !d->k || !d->v || !d->lse || !d->dout || !R) return CCLIP_ERR_ARG;
  if (d->B <= 0 || d->H <= 0 || d->T <= 0 || d->T > 128 || d->head_dim != 64 || !(grad_scale > 0.f)) return CCLIP_ERR_ARG;
  if ((d->ldq & 7) || (d->ldk & 7) || (d->ldv & 7) || (d->lddo & 7)) return CCLIP_ERR_ARG;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->dout) & 15) return CCLIP_ERR_ARG;
  if (((uintptr_t)R & 3) || ((uintptr_t)d->lse & 3)) return CCLIP_ERR_ARG;
  RelArgs a;
  a.q = (const bf16*)d->q; a.k = (const bf16*)d->k; a.v = (const bf16*)d->v;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv;
  a.da = (const bf16*)d->dout; a.ldda = d->lddo;
  a.lse = d->lse; a.cu = d->cu_seqlens; a.R = R;
  a.B = d->B; a.T = d->T; a.H = d->H; a.causal = d->causal;
  a.scale = d->scale; a.cscale = 1.0f / ((float)d->H * grad_scale);
  const int nkt = (d->T + 15) / 16;
  dim3 grid(d->B), block(256);
  if (nkt <= 2) hipLaunchKernelGGL((attn_relevance_kernel<2>), grid, block, 0, stream, a);
  else if (nkt <= 4) hipLaunchKernelGGL((attn_relevance_kernel<4>), grid, block, 0, stream, a);
  else if (nkt <= 5) hipLaunchKernelGGL((attn_relevance_kernel<5>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((attn_relevance_kernel<8>), grid, block, 0, stream, a);
  return cclip_launch_status();
}
