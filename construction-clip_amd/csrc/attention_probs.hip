// Attention probabilities of one layer for gfx950, T <= 256, head_dim 64: the one thing the fused attention kernels never
// write.  For every (sequence b, head h) and every requested query position t = q_rows[i] (all T positions when q_rows is null):
//     P[b, h, i, j] = softmax_j(scale q_t . k_j + mask)          fp32, j = 0 .. T-1
// mask: causal (j > t) and key_keep[b, j] == 0 entries are exactly 0; a row that sees no key at all is all zeros.  Every
// element 0 .. T-1 of a produced row is written (the caller passes uninitialised memory), nothing else is.
// This is what `output_attentions=True` of the reference's generate_beam (CLIP_prefix_caption/test.py:381-390) asks GPT-2 for.
//
// Normalisation: the TWO-PASS form (row max and row sum, then the normalised values) - but the scores of a wave's 16 query
// rows against all <= 256 keys fit in its registers (16 key tiles x 4 fp32), so Q K^T is formed ONCE and both passes run on
// registers.  The forward's lse is not read: the kernel needs nothing but q and k, and a row sums to 1 to fp32 rounding.
//
// One work-group (4 waves) per (b, h, block of 64 query rows); wave w owns rows 16w .. 16w+15 of the block.  K of the
// (b, h) is staged once in LDS in the swizzled [row][64] image of attention_tiles.h (at_off / frag_row, conflict-free for the
// B-fragment reads) by a loop of its own: through head_load / head_store the kernel measured 4 % slower per launch at
// B H = 36, T = 140, with everything after the barrier unchanged.  Q rows go straight from memory into the A fragments.
// S = Q K^T is v_mfma_f32_16x16x32 with the query on the accumulator rows: lane (li, g) holds rows 4g .. 4g+3, column
// (key) 16 kt + li of tile kt, so a row's reduction is over kt in registers and over the 16 lanes of a group by xor-shuffles.
// Fixed order, no atomics: two launches are bitwise equal.
#include "attention_tiles.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

struct ProbsArgs {
  const bf16* q; const bf16* k;                   // row (b*T + t), head h at column h*64
  long ldq, ldk;
  const float* keep;                              // [B, T] or null: 0 masks a key
  const int* q_rows;                              // [n_q] query positions (clamped to 0 .. T-1) or null: i -> i
  float* P; long ldb, ldh, ldi;                   // P[b*ldb + h*ldh + i*ldi + j]
  int B, T, H, n_q, causal;
  float scale;
};

__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NKT>
__global__ __launch_bounds__(256) void attn_probs_kernel(const ProbsArgs a) {
  constexpr int TP = 16 * NKT;                    // padded keys
  constexpr int IT = TP * 8 / 256;                // 16-byte chunks of K per thread (TP is a multiple of 32)
  static_assert(TP % 32 == 0, "whole rounds of 256 chunks");
  __shared__ __attribute__((aligned(16))) char Ks[TP * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int T = a.T, n_q = a.n_q;
  const int nqb = (n_q + 63) >> 6;
  int bid = blockIdx.x;
  const int qb = bid % nqb; bid /= nqb;
  const int h = bid % a.H, b = bid / a.H;
  const long row0 = (long)b * T;

#pragma unroll
  for (int it = 0; it < IT; ++it) {               // K of (b, h) -> LDS; rows >= T are zero (loads clamped, not predicated)
    const int idx = tid + 256 * it, row = idx >> 3, ch = idx & 7;
    const uint4 v = *(const uint4*)(a.k + (row0 + (row < T ? row : T - 1)) * a.ldk + h * 64 + ch * 8);
    *(uint4*)(Ks + at_off(row, ch)) = row < T ? v : make_uint4(0, 0, 0, 0);
  }
  __syncthreads();                                // the only barrier: waves without rows may leave after it
  const int i0 = 64 * qb + 16 * wave;
  if (i0 >= n_q) return;                          // (wave-uniform)

  auto qpos = [&](int i) {                        // query position of output row i; rows >= n_q repeat the last one, never stored
    const int ii = i < n_q ? i : n_q - 1;
    const int p = a.q_rows ? a.q_rows[ii] : ii;
    return p < 0 ? 0 : (p < T ? p : T - 1);
  };
  const int pa = qpos(i0 + li);                   // the row this lane feeds into the A fragment
  const bf16* qp = a.q + (row0 + pa) * a.ldq + h * 64 + 8 * g;
  const bf16x8 qf0 = *(const bf16x8*)qp, qf1 = *(const bf16x8*)(qp + 32);
  int pr[4];                                      // positions of the accumulator rows this lane holds
#pragma unroll
  for (int r = 0; r < 4; ++r) pr[r] = qpos(i0 + 4 * g + r);
  int pmax = pa;                                  // the furthest key any of the wave's 16 rows may see (causal tile skip)
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) { const int t = __shfl_xor(pmax, o, 64); pmax = t > pmax ? t : pmax; }
  const int nkt = (T + 15) >> 4;

  unsigned kmask = 0;                             // bit kt: key 16 kt + li exists and is kept
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const int key = 16 * kt + li;
    const bool ok = key < T && (!a.keep || a.keep[row0 + key] != 0.f);
    kmask |= ok ? 1u << kt : 0u;
  }

  f32x4 s[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (kt >= nkt || (a.causal && 16 * kt > pmax)) continue;     // (wave-uniform; every entry of such a tile is masked below)
    const int key = 16 * kt + li;
    s[kt] = CCLIP_MFMA_16x16x32(qf0, frag_row(Ks, key, g), s[kt]);
    s[kt] = CCLIP_MFMA_16x16x32(qf1, frag_row(Ks, key, 4 + g), s[kt]);
  }

  const float NEG = -__builtin_huge_valf();
  float m[4] = {NEG, NEG, NEG, NEG};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = ((kmask >> kt) & 1u) && (!a.causal || 16 * kt + li <= pr[r]);
      const float z = ok ? s[kt][r] * a.scale : NEG;
      s[kt][r] = z;
      m[r] = fmaxf(m[r], z);
    }
  float inv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = group16_max(m[r]);
    if (m[r] == NEG) m[r] = 0.f;                  // no visible key: the row becomes zeros
  }
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = s[kt][r] > NEG ? __expf(s[kt][r] - m[r]) : 0.f;
      s[kt][r] = e;
      sum[r] += e;
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sum[r] = group16_sum(sum[r]);
    inv[r] = sum[r] > 0.f ? 1.0f / sum[r] : 0.f;
  }

  float* Pb = a.P + (long)b * a.ldb + (long)h * a.ldh;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * g + r;
    if (i >= n_q) continue;
    float* pp = Pb + (long)i * a.ldi;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const int key = 16 * kt + li;
      if (key < T) pp[key] = s[kt][r] * inv[r];   // 16 lanes of a group: 64 contiguous bytes of one row
    }
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_attention_probs)(const cclip_attn_desc* d, const int32_t* q_rows, int32_t n_q, float* P,
                                               int64_t ld_p_b, int64_t ld_p_h, int64_t ld_p_q, hipStream_t stream) {
  if (!d || !d->q || !d->k || !P) return CCLIP_ERR_ARG;
  if (d->B <= 0 || d->H <= 0 || d->T <= 0 || d->T > 256 || d->head_dim != 64 || d->cu_seqlens) return CCLIP_ERR_ARG;
  if ((d->ldq & 7) || (d->ldk & 7) || d->ldq < (int64_t)d->H * 64 || d->ldk < (int64_t)d->H * 64) return CCLIP_ERR_ARG;
  if (((uintptr_t)d->q | (uintptr_t)d->k) & 15) return CCLIP_ERR_ARG;
  if (((uintptr_t)P & 3) || ((uintptr_t)d->key_keep & 3) || ((uintptr_t)q_rows & 3)) return CCLIP_ERR_ARG;
  if (!q_rows) n_q = d->T;
  if (n_q <= 0 || ld_p_q < d->T || (d->H > 1 && ld_p_h <= 0) || (d->B > 1 && ld_p_b <= 0)) return CCLIP_ERR_ARG;
  const int64_t nqb = (n_q + 63) / 64;
  if (nqb * d->H * d->B > 0x7fffffffLL) return CCLIP_ERR_ARG;
  ProbsArgs a;
  a.q = (const bf16*)d->q; a.k = (const bf16*)d->k;
  a.ldq = d->ldq; a.ldk = d->ldk;
  a.keep = d->key_keep; a.q_rows = q_rows;
  a.P = P; a.ldb = ld_p_b; a.ldh = ld_p_h; a.ldi = ld_p_q;
  a.B = d->B; a.T = d->T; a.H = d->H; a.n_q = n_q; a.causal = d->causal;
  a.scale = d->scale;
  const int nkt = (d->T + 15) / 16;
  dim3 grid((unsigned)(nqb * d->H * d->B)), block(256);
  if (nkt <= 2) hipLaunchKernelGGL((attn_probs_kernel<2>), grid, block, 0, stream, a);
  else if (nkt <= 4) hipLaunchKernelGGL((attn_probs_kernel<4>), grid, block, 0, stream, a);
  else if (nkt <= 8) hipLaunchKernelGGL((attn_probs_kernel<8>), grid, block, 0, stream, a);
  else if (nkt <= 12) hipLaunchKernelGGL((attn_probs_kernel<12>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((attn_probs_kernel<16>), grid, block, 0, stream, a);
  return cclip_launch_status();
}
