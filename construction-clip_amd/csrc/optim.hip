// Optimiser step + weight casting over the flat parameter arena (one launch for all 151 M
// parameters; HBM-bound: 16 B read + 14 B written per parameter).
//
// AdamW in the exact form the reference optimises with: `transformers.AdamW(lr, betas=(0.9,0.999),
// eps=1e-6, weight_decay=0.0, correct_bias=True)` at /root/reference/CLIP/train.py:143 and
// /root/reference/CLIP_prefix_caption/train.py:336 (class removed from transformers >= 5; its
// published update is restated in oracle/optim_oracle.py):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v)+eps) ;
//   then p -= lr*wd*p.
// mode 1 is torch.optim.AdamW's form (decay first, eps added after the bias-corrected sqrt).
// The bf16 compute copy of the weights is refreshed in the same pass.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

namespace CCLIP_NS {

// One thread-iteration = U float4 groups a grid stride apart: the 4 U loads go out before the first use (U = 2: eight read
// streams' worth of bytes in flight per thread; the single-group form sat at 4.4 TB/s of its 30 B per parameter).
__device__ __forceinline__ void adamw_update(float (&pa)[4], const float (&ga)[4], float (&ma)[4], float (&va)[4], float lr, float b1,
                                             float b2, float eps, float wd, float bc1, float sq2, float grad_scale, int mode) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gr = ga[j] * grad_scale;
    ma[j] = b1 * ma[j] + (1.f - b1) * gr;
    va[j] = b2 * va[j] + (1.f - b2) * gr * gr;
    if (mode == 0) {
      pa[j] -= (lr * sq2 / bc1) * ma[j] / (sqrtf(va[j]) + eps);
      if (wd > 0.f) pa[j] -= lr * wd * pa[j];
    } else {
      pa[j] *= 1.f - lr * wd;
      pa[j] -= (lr / bc1) * ma[j] / (sqrtf(va[j]) / sq2 + eps);
    }
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2,
                                                    float grad_scale, int mode, bf16* __restrict__ shadow) {
  constexpr int U = 2;
  const long n4 = n >> 2;
  const float sq2 = sqrtf(bc2);
  const long stride = gridDim.x * 256L;
  for (long i0 = blockIdx.x * 256L + threadIdx.x; i0 < n4; i0 += U * stride) {
    float4 pp[U], gg[U], mm[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i < n4) { pp[u] = ((float4*)p)[i]; gg[u] = ((const float4*)g)[i]; mm[u] = ((float4*)m)[i]; vv[u] = ((float4*)v)[i]; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i >= n4) break;
      float pa[4] = {pp[u].x, pp[u].y, pp[u].z, pp[u].w}, ga[4] = {gg[u].x, gg[u].y, gg[u].z, gg[u].w};
      float ma[4] = {mm[u].x, mm[u].y, mm[u].z, mm[u].w}, va[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
      adamw_update(pa, ga, ma, va, lr, b1, b2, eps, wd, bc1, sq2, grad_scale, mode);
      ((float4*)p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
      ((float4*)m)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
      ((float4*)v)[i] = make_float4(va[0], va[1], va[2], va[3]);
      if (shadow) {
        bf16x4 sdw = {(bf16)pa[0], (bf16)pa[1], (bf16)pa[2], (bf16)pa[3]};
        ((bf16x4*)shadow)[i] = sdw;
      }
    }
  }
}

// ---- grouped step: adamw_kernel's loop and arithmetic (adamw_update_groups below; one group without a scalar or an EMA gives its
// bits), with lr / weight decay looked up per 64-element chunk, the gradient scaled by a clip coefficient formed from a device
// scalar, and an EMA of the new masters written in the same pass (8 B more per parameter; EMA is a template parameter so that
// the form without it issues adamw_kernel's loads and stores and nothing else).
struct AdamwGroups {
  float lr[256];
  float wd[256];
};

// adamw_update with lr and wd per lane.  The text is adamw_update's except for mode 1's parameter line: with lr and wd uniform
// the compiler contracts `p * (1 - lr wd) - u` of adamw_kernel into fma(fma(-lr, wd, 1), p, -u); with them per lane it multiplied
// p separately (a packed multiply over two elements) and the last bit of p differed.  The two fmas are therefore written out.
// That the two kernels agree bit for bit, in both modes, is what tests/test_optim_groups_kernels_gpu.py (K1) checks on the device.
__device__ __forceinline__ void adamw_update_groups(float (&pa)[4], const float (&ga)[4], float (&ma)[4], float (&va)[4], float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float sq2, float grad_scale,
                                                    int mode) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gr = ga[j] * grad_scale;
    ma[j] = b1 * ma[j] + (1.f - b1) * gr;
    va[j] = b2 * va[j] + (1.f - b2) * gr * gr;
    if (mode == 0) {
      pa[j] -= (lr * sq2 / bc1) * ma[j] / (sqrtf(va[j]) + eps);
      if (wd > 0.f) pa[j] -= lr * wd * pa[j];
    } else {
      const float u = (lr / bc1) * ma[j] / (sqrtf(va[j]) / sq2 + eps);
      pa[j] = __builtin_fmaf(__builtin_fmaf(-lr, wd, 1.f), pa[j], -u);
    }
  }
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n, const uint8_t* __restrict__ chunk_group,
                                                           const AdamwGroups groups, float b1, float b2, float eps, float bc1,
                                                           float bc2, float grad_scale, int mode, bf16* __restrict__ shadow,
                                                           const float* __restrict__ sumsq_dev, float max_norm, int skip_nonfinite,
                                                           float* __restrict__ ema, float ema_decay) {
  constexpr int U = 2;
  const long n4 = n >> 2;
  const float sq2 = sqrtf(bc2);
  const long stride = gridDim.x * 256L;
  if (sumsq_dev) {
    const float ss = *sumsq_dev;
    if (skip_nonfinite && !(fabsf(ss) <= 3.402823466e38f)) return;        // inf or NaN: every thread leaves, nothing is written
    grad_scale = grad_scale * fminf(1.f, max_norm / (fabsf(grad_scale) * sqrtf(ss) + 1e-6f));
  }
  for (long i0 = blockIdx.x * 256L + threadIdx.x; i0 < n4; i0 += U * stride) {
    float4 pp[U], gg[U], mm[U], vv[U], ee[U];
    int grp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i < n4) {
        pp[u] = ((float4*)p)[i]; gg[u] = ((const float4*)g)[i]; mm[u] = ((float4*)m)[i]; vv[u] = ((float4*)v)[i];
        if constexpr (EMA) ee[u] = ((float4*)ema)[i];
        grp[u] = chunk_group[i >> 4];                                     // 16 float4 = one 64-element chunk
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (i >= n4) break;
      float pa[4] = {pp[u].x, pp[u].y, pp[u].z, pp[u].w}, ga[4] = {gg[u].x, gg[u].y, gg[u].z, gg[u].w};
      float ma[4] = {mm[u].x, mm[u].y, mm[u].z, mm[u].w}, va[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
      adamw_update_groups(pa, ga, ma, va, groups.lr[grp[u]], b1, b2, eps, groups.wd[grp[u]], bc1, sq2, grad_scale, mode);
      ((float4*)p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
      ((float4*)m)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
      ((float4*)v)[i] = make_float4(va[0], va[1], va[2], va[3]);
      if constexpr (EMA) {
        const float ea[4] = {ee[u].x, ee[u].y, ee[u].z, ee[u].w};
        float eo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) eo[j] = ema_decay * ea[j] + (1.f - ema_decay) * pa[j];
        ((float4*)ema)[i] = make_float4(eo[0], eo[1], eo[2], eo[3]);
      }
      if (shadow) {
        bf16x4 sdw = {(bf16)pa[0], (bf16)pa[1], (bf16)pa[2], (bf16)pa[3]};
        ((bf16x4*)shadow)[i] = sdw;
      }
    }
  }
}

#ifndef CCLIP_F16
// ---- sum of squares of a flat fp32 range, in two fixed trees (no float atomics: two launches give equal bits).
// Stage 1: a grid that depends on n alone; thread t of block b owns the float4 groups b*256 + t, + grid*256, ... and folds
// their 4 elements in order into one fma chain; the block folds its 256 chains with the 6-level wave butterfly and then its 4
// wave sums in ascending order, and writes one partial.  Stage 2: one block; its first thread folds the partials in ascending
// order.  A NaN or an inf anywhere reaches `out` through the chains; so does a square that overflows fp32.
constexpr int SUMSQ_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long n, float* __restrict__ partials) {
  __shared__ float red[4];
  const long n4 = n >> 2;
  const long stride = gridDim.x * 256L;
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += stride) {
    const float4 a = ((const float4*)x)[i];
    s = fmaf(a.x, a.x, s);
    s = fmaf(a.y, a.y, s);
    s = fmaf(a.z, a.z, s);
    s = fmaf(a.w, a.w, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void sumsq_fold_kernel(const float* __restrict__ partials, int n_partials, float* __restrict__ out,
                                                         int accumulate, int* __restrict__ nonfinite_count) {
  __shared__ float part[SUMSQ_MAX_BLOCKS];
  for (int i = threadIdx.x; i < n_partials; i += 256) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = accumulate ? *out : 0.f;
    for (int i = 0; i < n_partials; ++i) t += part[i];
    *out = t;
    if (nonfinite_count && !(fabsf(t) <= 3.402823466e38f)) *nonfinite_count = *nonfinite_count + 1;
  }
}
#endif

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, long n) {
  const long n4 = n >> 2;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += gridDim.x * 256L) {
    const float4 a = ((const float4*)in)[i];
    bf16x4 s = {(bf16)a.x, (bf16)a.y, (bf16)a.z, (bf16)a.w};
    ((bf16x4*)out)[i] = s;
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

static int flat_grid(long n4) { long b = (n4 + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

extern "C" int CCLIP_FN(cclip_adamw_step)(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int32_t step,
                                int32_t correct_bias, float grad_scale, int32_t mode, void* bf16_shadow,
                                hipStream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || (n & 3) || step < 1) return CCLIP_ERR_ARG;
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return CCLIP_ERR_ARG;
  float bc1 = 1.f, bc2 = 1.f;
  if (correct_bias) {
    bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  }
  hipLaunchKernelGGL(adamw_kernel, dim3(flat_grid(n >> 2)), dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq,
                     (long)n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, mode, (bf16*)bf16_shadow);
  return cclip_launch_status();
}

extern "C" int CCLIP_FN(cclip_adamw_step_groups)(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                                 const uint8_t* chunk_group, const float* lr, const float* weight_decay,
                                                 int32_t n_groups, float beta1, float beta2, float eps, int32_t step,
                                                 int32_t correct_bias, float grad_scale, int32_t mode, void* bf16_shadow,
                                                 const float* sumsq_dev, float max_norm, int32_t skip_nonfinite, float* ema,
                                                 float ema_decay, hipStream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || (n & 3) || step < 1) return CCLIP_ERR_ARG;
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) return CCLIP_ERR_ARG;
  if (!chunk_group || !lr || !weight_decay || n_groups < 1 || n_groups > 256) return CCLIP_ERR_ARG;
  if (sumsq_dev && !(max_norm > 0.f && max_norm <= 3.402823466e38f)) return CCLIP_ERR_ARG;
  if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return CCLIP_ERR_ARG;
  AdamwGroups groups = {};                   // entries >= n_groups: lr = wd = 0 (see the header)
  for (int i = 0; i < n_groups; ++i) { groups.lr[i] = lr[i]; groups.wd[i] = weight_decay[i]; }
  float bc1 = 1.f, bc2 = 1.f;
  if (correct_bias) {
    bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  }
  const dim3 grid(flat_grid(n >> 2));
  if (ema)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, grid, dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq, (long)n, chunk_group,
                       groups, beta1, beta2, eps, bc1, bc2, grad_scale, mode, (bf16*)bf16_shadow, sumsq_dev, max_norm, skip_nonfinite,
                       ema, ema_decay);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, grid, dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq, (long)n, chunk_group,
                       groups, beta1, beta2, eps, bc1, bc2, grad_scale, mode, (bf16*)bf16_shadow, sumsq_dev, max_norm, skip_nonfinite,
                       ema, ema_decay);
  return cclip_launch_status();
}

#ifndef CCLIP_F16
extern "C" int32_t cclip_adamw_grid(int64_t n) { return n > 0 && !(n & 3) ? flat_grid(n >> 2) : 0; }

static int sumsq_grid(int64_t n) {
  const int64_t b = ((n >> 2) + 255) / 256;
  return (int)(b > SUMSQ_MAX_BLOCKS ? SUMSQ_MAX_BLOCKS : b);
}

extern "C" int64_t cclip_sumsq_workspace(int64_t n) { return n > 0 && !(n & 3) ? 4 * (int64_t)sumsq_grid(n) : 0; }

extern "C" int cclip_sumsq_f32(const float* x, int64_t n, float* partials, float* out, int32_t accumulate, int32_t* nonfinite_count,
                               hipStream_t stream) {
  if (!x || !partials || !out || n <= 0 || (n & 3) || ((uintptr_t)x & 15) || ((uintptr_t)partials & 3)) return CCLIP_ERR_ARG;
  const int blocks = sumsq_grid(n);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(256), 0, stream, x, (long)n, partials);
  hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, out, accumulate, nonfinite_count);
  return cclip_launch_status();
}
#endif

extern "C" int CCLIP_CAST_FN(const float* in, void* out, int64_t n, hipStream_t stream) {
  if (!in || !out || n <= 0 || (n & 3) || ((uintptr_t)in & 15) || ((uintptr_t)out & 7)) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(flat_grid(n >> 2)), dim3(256), 0, stream, in, (bf16*)out, (long)n);
  return cclip_launch_status();
}
