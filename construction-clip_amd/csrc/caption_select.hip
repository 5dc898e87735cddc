// CLIP-guided caption selection for gfx950: one launch scores K candidate captions against each of N images and ranks them.
// It replaces normalize -> bmm -> clamp -> (reference cosines -> max -> harmonic mean) -> argsort of a torch composition by one
// kernel, with nothing read by the host between the towers and the answer.
//
// Semantics (include/cclip_hip.h, cclip_caption_select; tests/caption_select_ref.py restates them in float64).  All buffers
// are fp32 - the towers' outputs after .float(), raw, not normalised - so there is no 16-bit operand and NO fp16 twin: the
// translation unit is built once.
//   cos[n,k]   = <i_n, t_nk> / (|i_n| |t_nk|), 0 when either norm is 0        (t_nk = txt row n K + k)
//   clip_score = w max(cos, 0)
//   rmax[n,k]  = max(0, max_r cos(t_nk, ref_r)) over image n's references ref_off[n] <= r < ref_off[n+1]; 0 without any
//   ref_score  = 2 clip_score rmax / (clip_score + rmax), 0 when the denominator is 0
//   score      = cos + lm_weight lm_mean[n K + k]                              (cos itself when lm_mean is NULL)
//   order[n,:] = the candidates by (score descending, k ascending);  best[n] = order[n,0]
// Scores are compared through a monotone integer image of their fp32 bits (mono_bits of score_key.h; -0 == +0), a total order
// on every bit pattern, so order[n,:] is a permutation of 0 .. K-1 for ANY input, NaN included.  Values computed from
// non-finite features are otherwise undefined; every access stays inside the buffers.
//
// Shape of the work.  One 256-thread work-group per image, four waves; wave v takes the candidates k = v, v + 4, ...  A row
// of E <= 1024 floats is E / 4 float4s: lane l owns the float4s l, l + 64, l + 128, l + 192 (those below E / 4), so a row is
// at most four 16-byte loads per lane, all issued before the first is used, and the image row stays in registers for the
// whole work-group's life.  The dot and the two squared norms are accumulated per lane in that fixed order (x, y, z, w of each
// float4 in turn) and reduced by the fixed xor butterfly of wave_sum; addition is commutative, so every lane ends with the
// same bits.  No floating-point atomic, no dependence on N or on the row's place: two launches agree bit for bit.  The
// reference pass is the same dot loop, wave v walking the pairs (k, r) of its candidates while t_nk is still in registers;
// a maximum does not depend on the order it is taken in.  After one barrier wave 0 ranks the K <= 64 keys by counting: lane k
// counts the candidates that come before candidate k and writes k at that rank.  256 bytes of LDS, no workspace, no global
// scratch, every loop bound known at launch.
//
// Error.  A lane adds at most E / 64 products one after the other and six butterfly levels follow, so each of the three sums
// errs by at most (E / 64 + 6) 2^-24 of sum |a_i b_i| <= |a| |b|; with the two square roots, the product and the division
// |cos - exact| <= 4 (E / 64 + 8) 2^-24.
#include "score_key.h"
#include "../../include/cclip_hip.h"

#define CS_Q 4                                    // float4s of a row a lane owns: CCLIP_CAPTION_SELECT_MAX_E / (4 * 64)

namespace CCLIP_NS {

struct CsRow { float4 v[CS_Q]; };

// the lane's float4s of a row of E4 float4s; beyond the row the value is zero (adds nothing to any sum) and nothing is loaded
__device__ __forceinline__ CsRow cs_load(const float* __restrict__ row, int E4, int lane) {
  CsRow r;
#pragma unroll
  for (int i = 0; i < CS_Q; ++i) {
    const int j = lane + 64 * i;
    r.v[i] = j < E4 ? ((const float4*)row)[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  return r;
}

__device__ __forceinline__ float cs_dot(const CsRow& a, const CsRow& b) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < CS_Q; ++i) {
    s += a.v[i].x * b.v[i].x;
    s += a.v[i].y * b.v[i].y;
    s += a.v[i].z * b.v[i].z;
    s += a.v[i].w * b.v[i].w;
  }
  return wave_sum(s);
}

// <a, b> / (|a| |b|) from the dot and the squared norms; 0 when either norm is 0
__device__ __forceinline__ float cs_cos(float dot, float na, float nb) {
  return na == 0.0f || nb == 0.0f ? 0.0f : dot / (sqrtf(na) * sqrtf(nb));
}

__global__ __launch_bounds__(256) void caption_select_kernel(const float* __restrict__ img, long ldi, const float* __restrict__ txt,
                                                             long ldt, int K, int E4, const float* __restrict__ lm_mean,
                                                             const float* __restrict__ ref, long ldr,
                                                             const int* __restrict__ ref_off, float w, float lm_weight,
                                                             float* __restrict__ cos_out, float* __restrict__ clip_out,
                                                             float* __restrict__ ref_out, float* __restrict__ score_out,
                                                             int* __restrict__ order, int* __restrict__ best) {
  __shared__ unsigned s_key[CCLIP_CAPTION_SELECT_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;
  const CsRow im = cs_load(img + n * ldi, E4, lane);
  const float ni = cs_dot(im, im);
  int r0 = 0, r1 = 0;
  if (ref) { r0 = ref_off[n]; r1 = ref_off[n + 1]; }

  for (int k = wave; k < K; k += 4) {             // (uniform over the wave)
    const long row = n * K + k;
    const CsRow t = cs_load(txt + row * ldt, E4, lane);
    const float nt = cs_dot(t, t);
    const float c = cs_cos(cs_dot(im, t), ni, nt);
    const float cs = w * fmaxf(c, 0.0f);
    const float sc = lm_mean ? c + lm_weight * lm_mean[row] : c;
    float rmax = 0.0f;
    for (int r = r0; r < r1; ++r) {
      const CsRow f = cs_load(ref + (long)r * ldr, E4, lane);
      rmax = fmaxf(rmax, cs_cos(cs_dot(t, f), nt, cs_dot(f, f)));
    }
    if (lane == 0) {
      cos_out[row] = c;
      clip_out[row] = cs;
      score_out[row] = sc;
      if (ref) {
        const float den = cs + rmax;
        ref_out[row] = den == 0.0f ? 0.0f : 2.0f * cs * rmax / den;
      }
      s_key[k] = mono_bits(sc);
    }
  }
  __syncthreads();

  if (wave == 0 && lane < K) {                    // rank by counting: lane k places candidate k
    const unsigned mine = s_key[lane];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const unsigned other = s_key[j];            // (one address for the whole wave: a broadcast)
      rank += other > mine || (other == mine && j < lane);
    }
    order[n * K + rank] = lane;
    if (rank == 0) best[n] = lane;
  }
}

// the launch of cclip_caption_select (capi.hip), which has checked every argument
int caption_select_launch(const float* img, long ldi, const float* txt, long ldt, int N, int K, int E, const float* lm_mean,
                          const float* ref, long ldr, const int* ref_off, float w, float lm_weight, float* cos_out, float* clip_out,
                          float* ref_out, float* score_out, int* order, int* best, hipStream_t stream) {
  static_assert(CCLIP_CAPTION_SELECT_MAX_E == 4 * 64 * CS_Q, "a lane owns CS_Q float4s of a row");
  static_assert(CCLIP_CAPTION_SELECT_MAX_K == 64, "one lane of wave 0 ranks one candidate");
  hipLaunchKernelGGL(caption_select_kernel, dim3((unsigned)N), dim3(256), 0, stream, img, ldi, txt, ldt, K, E / 4, lm_mean, ref, ldr,
                     ref_off, w, lm_weight, cos_out, clip_out, ref_out, score_out, order, best);
  return cclip_launch_status();
}

}  // namespace CCLIP_NS
