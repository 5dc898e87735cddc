// ABI version + small utilities of libcclip_hip.so.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

extern "C" int cclip_abi_version(void) { return CCLIP_ABI_VERSION; }

// x[i] *= alpha over a flat fp32 range (HBM-bound: 8 B per element).  Used to undo the static loss scale of the fp16
// operand mode on the gradient arena: powers of two, so the scaling itself is exact.
__global__ __launch_bounds__(256) void scale_f32_kernel(float* __restrict__ x, long n4, float alpha) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256L) {
    float4 v = ((float4*)x)[i];
    v.x *= alpha; v.y *= alpha; v.z *= alpha; v.w *= alpha;
    ((float4*)x)[i] = v;
  }
}

extern "C" int cclip_scale_f32(float* x, int64_t n, float alpha, hipStream_t stream) {
  if (!x || n <= 0 || (n & 3) || ((uintptr_t)x & 15)) return CCLIP_ERR_ARG;
  long b = ((n >> 2) + 255) / 256;
  hipLaunchKernelGGL(scale_f32_kernel, dim3((int)(b > 8192 ? 8192 : b)), dim3(256), 0, stream, x, (long)(n >> 2), alpha);
  return cclip_launch_status();
}

// CLIP-guided caption selection (csrc/caption_select.hip; contract in include/cclip_hip.h).  The arguments are checked here
// and nothing is launched on a violation; ref_off lives on the device and is the caller's to validate.
namespace CCLIP_NS {
int caption_select_launch(const float* img, long ldi, const float* txt, long ldt, int N, int K, int E, const float* lm_mean,
                          const float* ref, long ldr, const int* ref_off, float w, float lm_weight, float* cos_out, float* clip_out,
                          float* ref_out, float* score_out, int* order, int* best, hipStream_t stream);
}

extern "C" int cclip_caption_select(const float* img, int64_t ldi, const float* txt, int64_t ldt, int32_t N, int32_t K, int32_t E,
                                    const float* lm_mean, const float* ref, int64_t ldr, const int32_t* ref_off, float w,
                                    float lm_weight, float* cos, float* clip_score, float* ref_score, float* score, int32_t* order,
                                    int32_t* best, hipStream_t stream) {
  if (!img || !txt || !cos || !clip_score || !score || !order || !best) return CCLIP_ERR_ARG;
  if (N <= 0 || K < 1 || K > CCLIP_CAPTION_SELECT_MAX_K) return CCLIP_ERR_ARG;
  if (E <= 0 || (E & 3) || E > CCLIP_CAPTION_SELECT_MAX_E) return CCLIP_ERR_ARG;
  if (ldi < E || (ldi & 3) || ldt < E || (ldt & 3)) return CCLIP_ERR_ARG;
  if (((uintptr_t)img & 15) || ((uintptr_t)txt & 15)) return CCLIP_ERR_ARG;
  if ((ref != nullptr) != (ref_off != nullptr)) return CCLIP_ERR_ARG;
  if (ref && (!ref_score || ldr < E || (ldr & 3) || ((uintptr_t)ref & 15))) return CCLIP_ERR_ARG;
  return CCLIP_NS::caption_select_launch(img, (long)ldi, txt, (long)ldt, N, K, E, lm_mean, ref, (long)ldr, ref_off, w, lm_weight, cos,
                                         clip_score, ref_score, score, order, best, stream);
}
