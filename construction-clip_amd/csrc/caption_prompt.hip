// The step between the CLIP image tower and the caption decoder (CLIP_prefix_caption/test.py:521-542, parse_coco.py:45-56):
// the zero-shot heads over an image's feature row and the attribute ids their arg-maxes select, in one launch and without
// the host looking at anything.
//
//   caption_prompt   per image row n and head g (prompt rows [head_start[g], head_start[g+1]) of `prompts`):
//                      logit[n,k] = exp(*logit_scale) * <feat_n, prompt_k> / (|feat_n| |prompt_k|)
//                      probs[n,k] = softmax of logit[n, :] over the prompts of k's head
//                      index[n,g] = arg-max of the head's logits, the lowest index on an exact tie
//                      ids[n,:]   = table[((index[n,0] * K_1) + index[n,1]) * K_2 + ...]        (head 0 slowest)
//
// One wave per image row, four rows per workgroup.  Every workgroup first L2-normalises the prompt rows into LDS (K * E
// floats: 33 KiB for 2 + 9 prompts of width 768).  fp32 throughout; every sum over E is a fixed per-lane order followed by the
// xor butterfly of wave_sum, every sum over a head's prompts is serial: two launches are bitwise equal.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#define PROMPT_MAX_HEADS 16
#define PROMPT_MAX_E 1024                 // 4 float4 per lane
#define PROMPT_MAX_LDS_BYTES 65536

namespace CCLIP_NS {

struct PromptHeads {
  int g;
  int start[PROMPT_MAX_HEADS + 1];
};

__global__ __launch_bounds__(256) void caption_prompt_kernel(const float* __restrict__ feat, long ldf, int N, int E,
                                                             const float* __restrict__ prompts, int K, PromptHeads heads,
                                                             const float* __restrict__ logit_scale,
                                                             const int* __restrict__ table, int A,
                                                             float* __restrict__ probs, int* __restrict__ index,
                                                             int* __restrict__ ids) {
  extern __shared__ float lds[];
  float* pn = lds;                                  // [K, E] normalised prompt rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* lg = lds + (long)K * E + wave * K;         // [K] this wave's logits
  for (int k = wave; k < K; k += 4) {
    float s = 0.f;
    for (int col = lane * 4; col < E; col += 256) {
      const float4 v = *(const float4*)(prompts + (long)k * E + col);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    const float inv = rsqrtf(wave_sum(s));
    for (int col = lane * 4; col < E; col += 256) {
      const float4 v = *(const float4*)(prompts + (long)k * E + col);
      *(float4*)(pn + (long)k * E + col) = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
    }
  }
  __syncthreads();
  const float scale = expf(*logit_scale);
  for (int r = blockIdx.x * 4 + wave; r < N; r += gridDim.x * 4) {
    float4 f[PROMPT_MAX_E / 256];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < PROMPT_MAX_E / 256; ++c) {
      const int col = c * 256 + lane * 4;
      f[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < E) f[c] = *(const float4*)(feat + (long)r * ldf + col);
      ss += f[c].x * f[c].x + f[c].y * f[c].y + f[c].z * f[c].z + f[c].w * f[c].w;
    }
    const float inv_f = rsqrtf(wave_sum(ss));
    for (int k = 0; k < K; ++k) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < PROMPT_MAX_E / 256; ++c) {
        const int col = c * 256 + lane * 4;
        if (col < E) {
          const float4 p = *(const float4*)(pn + (long)k * E + col);
          d += f[c].x * p.x + f[c].y * p.y + f[c].z * p.z + f[c].w * p.w;
        }
      }
      // the butterfly leaves the same sum in every lane: each lane stores it and later reads back its own store
      lg[k] = scale * (wave_sum(d) * inv_f);
    }
    int comb = 0;
    for (int g = 0; g < heads.g; ++g) {
      const int k0 = heads.start[g], k1 = heads.start[g + 1];
      float m = lg[k0];
      int best = k0;
      for (int k = k0 + 1; k < k1; ++k) {
        const float v = lg[k];
        if (v > m) { m = v; best = k; }             // strict: the lowest index wins an exact tie
      }
      float sum = 0.f;
      for (int k = k0; k < k1; ++k) sum += expf(lg[k] - m);
      const float inv_sum = 1.0f / sum;
      for (int k = k0 + lane; k < k1; k += 64) probs[(long)r * K + k] = expf(lg[k] - m) * inv_sum;
      if (lane == 0) index[(long)r * heads.g + g] = best - k0;
      comb = comb * (k1 - k0) + (best - k0);
    }
    for (int a = lane; a < A; a += 64) ids[(long)r * A + a] = table[(long)comb * A + a];
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_caption_prompt(const float* feat, int64_t ldf, int32_t N, int32_t E, const float* prompts, int32_t K,
                                    const int32_t* head_start, int32_t G, const float* logit_scale_dev, const int32_t* table,
                                    int32_t table_rows, int32_t A, float* probs, int32_t* index, int32_t* ids,
                                    hipStream_t stream) {
  if (!feat || !prompts || !head_start || !logit_scale_dev || !table || !probs || !index || !ids) return CCLIP_ERR_ARG;
  if (N <= 0 || E <= 0 || K <= 0 || G <= 0 || A <= 0 || G > PROMPT_MAX_HEADS) return CCLIP_ERR_ARG;
  if ((E & 3) || E > PROMPT_MAX_E || ldf < E || (ldf & 3) || ((uintptr_t)feat & 15) || ((uintptr_t)prompts & 15)) return CCLIP_ERR_ARG;
  const size_t lds_bytes = ((size_t)K * E + 4 * (size_t)K) * sizeof(float);
  if (lds_bytes > PROMPT_MAX_LDS_BYTES) return CCLIP_ERR_ARG;
  PromptHeads h;
  h.g = G;
  if (head_start[0] != 0 || head_start[G] != K) return CCLIP_ERR_ARG;
  int64_t rows = 1;
  for (int g = 0; g < G; ++g) {
    const int32_t kg = head_start[g + 1] - head_start[g];
    if (kg <= 0) return CCLIP_ERR_ARG;                         // a head with no prompts (or starts out of order)
    rows *= kg;
    if (rows > INT32_MAX) return CCLIP_ERR_ARG;
  }
  if (rows != table_rows) return CCLIP_ERR_ARG;                // every combination the arg-maxes can form has its row
  for (int g = 0; g <= G; ++g) h.start[g] = head_start[g];
  for (int g = G + 1; g <= PROMPT_MAX_HEADS; ++g) h.start[g] = K;
  int blocks = (N + 3) / 4;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(caption_prompt_kernel, dim3(blocks), dim3(256), lds_bytes, stream, feat, (long)ldf, N, E, prompts, K, h,
                     logit_scale_dev, table, A, probs, index, ids);
  return cclip_launch_status();
}
