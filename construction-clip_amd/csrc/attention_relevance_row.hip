// One row of the attention relevance (Chefer et al.) of one layer for gfx950, any T <= 8192, head_dim 64: the per-layer step of
// the reference's `interpret()` (attention.py:14-69) for the only rows its callers read - the class-token row of R_image and
// the EOT row of R_text.  The backward visits the layers top-down and right-multiplies (R <- R + R C_l), so one row of the final
// R obeys the same recurrence on a row vector; for every sequence b (length T_b):
//     P_h  = exp(scale Q_h K_h^T - lse_h)            (causal: 0 above the diagonal)
//     dP_h = dA_h V_h^T                              (dA: gradient at the attention output, from the dgrad chain)
//     r_out[j] = r_in[j] + 1 / (H grad_scale) * sum_{i < T_b} r_in[i] * sum_h max(P_h[i, j] dP_h[i, j], 0)     (j < T_b)
//     r_out[j] = r_in[j]                                                                                      (T_b <= j < T)
// A flash-style streaming reduction over the query rows: no T x T object exists, neither in LDS nor in HBM (attention_relevance.hip
// keeps the whole C in LDS, which ends at T = 128).
//
// One workgroup (4 waves) per sequence and per block of 64 keys.  Heads are looped; K_h and V_h of the key block are staged in LDS
// in the layout of attention_relevance.hip ([row][64] 16-bit, 16-byte chunk c of row r at chunk c ^ (r & 7)), the next head's loads
// in flight under this head's MFMAs.  Each wave walks the query tiles wave, wave + 4, ...: Q and dA rows go straight into the A
// fragments, v_mfma_f32_16x16x32 forms S and dP with the query on the accumulator rows (as in attn_bwd_kernel, attention.hip), and
// max(p dp, 0) r_in[i] accumulates in 4 key tiles x 4 registers per lane across all heads and query tiles.  A query tile whose 16
// r_in values are all zero is skipped (wave-uniform; it would add exactly zero), so a one-hot r - the default start_layer = -1 -
// touches one query tile per sequence.  The end is a fixed-order reduction: the 4 accumulator rows, the 4 lane groups (cross-lane
// moves), the 4 waves (LDS).  No atomics: two launches agree bit for bit.  No predicated global loads: rows are clamped.
//
// Correctness and determinism at every T are the goal here, not speed: the grid is B x ceil(T / 64), so one ViT-L/14@336px image
// (T = 577) is 10 workgroups, and every workgroup re-reads all of Q and dA of its sequence.  That is accepted - the step runs once
// per layer of a single explanation pass, next to a dgrad chain that costs far more.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct RelRowArgs {
  const bf16* q; const bf16* k; const bf16* v;   // row (b*T + t) (or cu[b] + t), head h at column h*64
  long ldq, ldk, ldv;
  const bf16* da; long ldda;                      // gradient at the attention output, same layout
  const float* lse;                               // [B, H, T]
  const int* cu;                                  // packed batch: sequence b is rows [cu[b], cu[b+1]); null: row b*T + t
  const float* r_in;                              // [B, T]
  float* r_out;                                   // [B, T], not r_in
  int B, T, H, causal, nkb;                       // nkb = ceil(T / 64) key blocks per sequence
  float scale, cscale;                            // cscale = 1 / (H * grad_scale)
};

__device__ __forceinline__ int relrow_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// dynamic LDS: K image (8 KiB) | V image (8 KiB) | r_in of the sequence, zero-padded to whole query tiles (16 ceil(T / 16) floats)
__global__ __launch_bounds__(256) void attn_relevance_row_kernel(const RelRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + 64 * 128;
  float* red = (float*)smem;                      // after the head loop: [4 waves][64 keys]
  float* rs = (float*)(smem + 2 * 64 * 128);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.nkb, k0 = 64 * (blockIdx.x - b * a.nkb);
  int T = a.cu ? a.cu[b + 1] - a.cu[b] : a.T;
  T = T < a.T ? T : a.T;
  const float* rin = a.r_in + (long)b * a.T;
  float* rout = a.r_out + (long)b * a.T;
  if (k0 >= T) {                                  // (workgroup-uniform) no live key in this block: the row passes through
    if (tid < 64 && k0 + tid < a.T) rout[k0 + tid] = rin[k0 + tid];
    return;
  }
  const long row0 = a.cu ? (long)a.cu[b] : (long)b * a.T;
  const int nqt = (T + 15) >> 4;
  for (int i = tid; i < 16 * nqt; i += 256) rs[i] = i < T ? rin[i] : 0.f;

  f32x4 c[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) c[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (T - k0 + 15) >> 4;             // live key tiles of this block (>= 1)
  const int qt0 = a.causal ? k0 >> 4 : 0;         // causal: every query before the block's first key sees none of its keys

  uint4 rk[2], rv[2];
  auto head_load = [&](int h) {                   // every 16-byte load of head h's K and V block, rows clamped (no predicated loads)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it, row = k0 + (idx >> 3), ch = idx & 7;
      const long gr = row0 + (row < T ? row : T - 1);
      rk[it] = *(const uint4*)(a.k + gr * a.ldk + h * 64 + ch * 8);
      rv[it] = *(const uint4*)(a.v + gr * a.ldv + h * 64 + ch * 8);
    }
  };
  head_load(0);
  for (int h = 0; h < a.H; ++h) {
    __syncthreads();                              // everyone is done with the previous head's K / V (first pass: rs is written)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it, row = idx >> 3, ch = idx & 7;
      *(uint4*)(Ks + relrow_off(row, ch)) = k0 + row < T ? rk[it] : make_uint4(0, 0, 0, 0);
      *(uint4*)(Vs + relrow_off(row, ch)) = k0 + row < T ? rv[it] : make_uint4(0, 0, 0, 0);
    }
    if (h + 1 < a.H) head_load(h + 1);            // in flight under this head's MFMAs
    __syncthreads();
    for (int qt = qt0 + wave; qt < nqt; qt += 4) {
      float rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rq[r] = rs[16 * qt + 4 * g + r];
      if (!__ballot(rq[0] != 0.f || rq[1] != 0.f || rq[2] != 0.f || rq[3] != 0.f)) continue;   // (wave-uniform) adds exactly zero
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
      for (int kt = 0; kt < 4; ++kt) {
        if (kt >= nkt || (a.causal && k0 + 16 * kt > 16 * qt + 15)) continue;
        const int key = 16 * kt + li;
        f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        sv = CCLIP_MFMA_16x16x32(qf0, *(const bf16x8*)(Ks + relrow_off(key, g)), sv);
        sv = CCLIP_MFMA_16x16x32(qf1, *(const bf16x8*)(Ks + relrow_off(key, 4 + g)), sv);
        dp = CCLIP_MFMA_16x16x32(df0, *(const bf16x8*)(Vs + relrow_off(key, g)), dp);
        dp = CCLIP_MFMA_16x16x32(df1, *(const bf16x8*)(Vs + relrow_off(key, 4 + g)), dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = 16 * qt + 4 * g + r;
          const bool ok = qi < T && k0 + key < T && (!a.causal || k0 + key <= qi);
          const float pv = ok ? __expf(sv[r] * a.scale - lsv[r]) : 0.f;
          c[kt][r] += ok ? fmaxf(pv * dp[r], 0.f) * rq[r] : 0.f;
        }
      }
    }
  }
  __syncthreads();                                // K / V images are dead: the waves' partial rows take their place
  // fixed order: the 4 accumulator rows, then the 4 lane groups, then (below) the 4 waves
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    float s = (c[kt][0] + c[kt][1]) + (c[kt][2] + c[kt][3]);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (g == 0) red[wave * 64 + 16 * kt + li] = s;
  }
  __syncthreads();
  if (tid < 64 && k0 + tid < a.T) {
    const int j = k0 + tid;
    const float s = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
    rout[j] = j < T ? rin[j] + s * a.cscale : rin[j];
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_attention_relevance_row)(const cclip_attn_desc* d, float grad_scale, const float* r_in, float* r_out,
                                                       hipStream_t stream) {
  if (!d || !d->q || !d->k || !d->v || !d->lse || !d->dout || !r_in || !r_out || r_in == r_out) return CCLIP_ERR_ARG;
  if (d->B <= 0 || d->H <= 0 || d->T <= 0 || d->T > 8192 || d->head_dim != 64 || !(grad_scale > 0.f)) return CCLIP_ERR_ARG;
  if ((d->ldq & 7) || (d->ldk & 7) || (d->ldv & 7) || (d->lddo & 7)) return CCLIP_ERR_ARG;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->dout) & 15) return CCLIP_ERR_ARG;
  if ((((uintptr_t)r_in | (uintptr_t)r_out) & 3) || ((uintptr_t)d->lse & 3)) return CCLIP_ERR_ARG;
  RelRowArgs a;
  a.q = (const bf16*)d->q; a.k = (const bf16*)d->k; a.v = (const bf16*)d->v;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv;
  a.da = (const bf16*)d->dout; a.ldda = d->lddo;
  a.lse = d->lse; a.cu = d->cu_seqlens; a.r_in = r_in; a.r_out = r_out;
  a.B = d->B; a.T = d->T; a.H = d->H; a.causal = d->causal; a.nkb = (d->T + 63) / 64;
  a.scale = d->scale; a.cscale = 1.0f / ((float)d->H * grad_scale);
  if ((long)a.B * a.nkb > 0x7fffffffL) return CCLIP_ERR_ARG;
  const size_t lds = 2 * 64 * 128 + sizeof(float) * 16 * ((d->T + 15) / 16);     // <= 48 KiB at T = 8192
  hipLaunchKernelGGL(attn_relevance_row_kernel, dim3(a.B * a.nkb), dim3(256), lds, stream, a);
  return cclip_launch_status();
}
