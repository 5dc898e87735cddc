// One tile of the attention relevance (Chefer et al.), shared by attention_relevance.hip (the whole T <= 128 matrix) and
// attention_relevance_row.hip (one row at any T): for 16 queries x 16 keys of one head,
//     t = max(exp(scale S - lse) (.) dP, 0),   S = Q K^T,   dP = dA V^T      (masked entries: exactly 0)
// Both products are v_mfma_f32_16x16x32 with the query on the accumulator rows, as in attn_bwd_kernel (attention.hip): lane
// (li, g) holds queries 4g .. 4g+3 of the tile against key li.  K and V come from LDS images in the layout of attention_tiles.h;
// Q and dA rows are read straight into the A fragments.  Each kernel keeps its own accumulation, tile skipping and epilogue.
#pragma once
#include "attention_tiles.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct RelCommon {
  const bf16* q; const bf16* k; const bf16* v;   // row (b*T + t) (or cu[b] + t), head h at column h*64
  long ldq, ldk, ldv;
  const bf16* da; long ldda;                      // gradient at the attention output, same layout
  const float* lse;                               // [B, H, T]
  const int* cu;                                  // packed batch: sequence b is rows [cu[b], cu[b+1]); null: row b*T + t
  int B, T, H, causal;
  float scale, cscale;                            // cscale = 1 / (H * grad_scale)
};

// length of sequence b (at most a.T) and its first row
__device__ __forceinline__ int rel_seq(const RelCommon& a, int b, long& row0) {
  const int T = a.cu ? a.cu[b + 1] - a.cu[b] : a.T;
  row0 = a.cu ? (long)a.cu[b] : (long)b * a.T;
  return T < a.T ? T : a.T;
}

// the A fragments and log-sum-exp of query tile qt of head h (rows clamped: no predicated loads)
struct RelQTile { bf16x8 qf0, qf1, df0, df1; float lsv[4]; };
__device__ __forceinline__ RelQTile rel_qtile(const RelCommon& a, long row0, int b, int h, int qt, int T, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int qr = 16 * qt + li < T ? 16 * qt + li : T - 1;
  const bf16* qp = a.q + (row0 + qr) * a.ldq + h * 64 + 8 * g;
  const bf16* dp_ = a.da + (row0 + qr) * a.ldda + h * 64 + 8 * g;
  RelQTile t;
  t.qf0 = *(const bf16x8*)qp; t.qf1 = *(const bf16x8*)(qp + 32);
  t.df0 = *(const bf16x8*)dp_; t.df1 = *(const bf16x8*)(dp_ + 32);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = 16 * qt + 4 * g + r;
    t.lsv[r] = qi < T ? a.lse[((long)b * a.H + h) * a.T + qi] : 0.f;
  }
  return t;
}

// does query qi see key `key` (both positions in the sequence)?
__device__ __forceinline__ bool rel_sees(const RelCommon& a, int T, int qi, int key) {
  return qi < T && key < T && (!a.causal || key <= qi);
}

// the tile of query tile qt against rows 16 kt .. 16 kt + 15 of the K / V images, whose row 0 is key k0 of the sequence; entries
// rel_sees() masks are exact zeros (a caller that scales an entry re-applies rel_sees with the same positions: no 0 * inf)
__device__ __forceinline__ f32x4 rel_tile(const RelCommon& a, const RelQTile& t, const char* Ks, const char* Vs, int qt, int kt,
                                          int k0, int T, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int key = 16 * kt + li;
  f32x4 sv = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
  sv = CCLIP_MFMA_16x16x32(t.qf0, frag_row(Ks, key, g), sv);
  sv = CCLIP_MFMA_16x16x32(t.qf1, frag_row(Ks, key, 4 + g), sv);
  dp = CCLIP_MFMA_16x16x32(t.df0, frag_row(Vs, key, g), dp);
  dp = CCLIP_MFMA_16x16x32(t.df1, frag_row(Vs, key, 4 + g), dp);
  f32x4 out;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = rel_sees(a, T, 16 * qt + 4 * g + r, k0 + key);
    const float pv = ok ? __expf(sv[r] * a.scale - t.lsv[r]) : 0.f;
    out[r] = ok ? fmaxf(pv * dp[r], 0.f) : 0.f;
  }
  return out;
}

// Host side: what both launchers require of the descriptor (T <= max_T; q / k / v / dout 16-byte aligned rows of 8-element
// multiples, lse fp32) - fills the common arguments, or returns CCLIP_ERR_ARG.
static inline int rel_common_from_desc(const cclip_attn_desc* d, float grad_scale, int max_T, RelCommon& a) {
  if (!d || !d->q || !d->k || !d->v || !d->lse || !d->dout) return CCLIP_ERR_ARG;
  if (d->B <= 0 || d->H <= 0 || d->T <= 0 || d->T > max_T || d->head_dim != 64 || !(grad_scale > 0.f)) return CCLIP_ERR_ARG;
  if ((d->ldq & 7) || (d->ldk & 7) || (d->ldv & 7) || (d->lddo & 7)) return CCLIP_ERR_ARG;
  if (((uintptr_t)d->q | (uintptr_t)d->k | (uintptr_t)d->v | (uintptr_t)d->dout) & 15) return CCLIP_ERR_ARG;
  if ((uintptr_t)d->lse & 3) return CCLIP_ERR_ARG;
  a.q = (const bf16*)d->q; a.k = (const bf16*)d->k; a.v = (const bf16*)d->v;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv;
  a.da = (const bf16*)d->dout; a.ldda = d->lddo;
  a.lse = d->lse; a.cu = d->cu_seqlens;
  a.B = d->B; a.T = d->T; a.H = d->H; a.causal = d->causal;
  a.scale = d->scale; a.cscale = 1.0f / ((float)d->H * grad_scale);
  return CCLIP_OK;
}

}  // namespace CCLIP_NS
