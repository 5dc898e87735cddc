// Region preprocess: K boxes of decoded 8-bit RGB photos -> fp32 [K, 3, n, n], every box bit-identical to openai/CLIP's
// _transform(n) of the cropped box (Resize(n, BICUBIC) -> CenterCrop(n) -> ToTensor -> Normalize), in three launches
// whatever K is.  preprocess.hip does one whole image per call from coefficient tables built on the host; here the tables
// are built on the device as well, because every box has its own size and so its own tables:
//   1. roi_coeffs_kernel     one thread per (box, axis, surviving output sample): PIL's window and integer coefficients
//                            (preprocess_coeffs.h, double precision, no fused multiply-add);
//   2. roi_resample_h_kernel the horizontal pass of every box over the input rows its n surviving output rows touch, into one
//                            8-bit intermediate packed box after box (2^21 + sum p*k, >> 22, clamp - as resample_h_u8_kernel);
//   3. roi_resample_v_norm_kernel  the vertical pass + crop + ((u8 / 255) - mean) / std in fp32 (as resample_v_norm_kernel).
// A box addresses its photo through a byte offset and a row stride, so several photos of different sizes can share one
// packed source buffer.  The launchers check the HOST copy of every descriptor against the buffer sizes they are given before
// anything is launched (roi_check).  The kernels read the DEVICE copy, which a launcher cannot see without a read-back: that no
// kernel leaves [src, src + src_bytes) or [tmp, tmp + tmp_bytes) holds as long as the caller keeps the two copies identical.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"
#include "preprocess_coeffs.h"

// bounds[((k * 2 + axis) * n + j) * 2 + {0, 1}], kk[((k * 2 + axis) * n + j) * ksize_max + tap]; axis 0 = horizontal
__global__ __launch_bounds__(256) void roi_coeffs_kernel(const cclip_roi_desc* __restrict__ desc, long K, int n, int ksize_max,
                                                         int* __restrict__ bounds, int* __restrict__ kk) {
  const long total = K * 2 * n;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += gridDim.x * 256L) {
    const int j = (int)(t % n);
    const int axis = (int)((t / n) & 1);
    const cclip_roi_desc* d = desc + t / (2L * n);
    const int in_size = (int)(axis ? d->h : d->w), out_size = (int)(axis ? d->nh : d->nw);
    const int xx = j + (int)(axis ? d->top : d->left);
    int first;
    const int count = cclip_window_coeffs(in_size, out_size, xx, &first, kk + t * ksize_max, ksize_max);
    bounds[2 * t] = first;
    bounds[2 * t + 1] = count < ksize_max ? count : ksize_max;
  }
}

// tmp[tmp_off + (r * n + j) * 3 + c]: input row row0 + r of box k, surviving output column j.  blockIdx.y walks the boxes.
__global__ __launch_bounds__(256) void roi_resample_h_kernel(const unsigned char* __restrict__ src, const cclip_roi_desc* __restrict__ desc,
                                                             long K, int n, int ksize_max, const int* __restrict__ bounds,
                                                             const int* __restrict__ kk, unsigned char* __restrict__ tmp) {
  for (long b = blockIdx.y; b < K; b += gridDim.y) {
    const cclip_roi_desc* d = desc + b;
    const unsigned char* in = src + d->src_off + d->row0 * d->src_ld;
    const long in_ld = d->src_ld;
    unsigned char* out = tmp + d->tmp_off;
    const int* bnd = bounds + b * 2 * n * 2;                 // the horizontal tables of box b
    const int* kb = kk + b * 2 * n * ksize_max;
    const long total = d->rows * n;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
      const int j = (int)(i % n);
      const long r = i / n;
      const int xmin = bnd[2 * j], xn = bnd[2 * j + 1];
      const int* k = kb + (long)j * ksize_max;
      const unsigned char* p = in + r * in_ld + (long)xmin * 3;
      int s0 = 1 << (CCLIP_PRE_BITS - 1), s1 = s0, s2 = s0;
      for (int x = 0; x < xn; ++x) {
        const int w = k[x];
        s0 += p[3 * x] * w; s1 += p[3 * x + 1] * w; s2 += p[3 * x + 2] * w;
      }
      unsigned char* o = out + i * 3;
      s0 >>= CCLIP_PRE_BITS; s1 >>= CCLIP_PRE_BITS; s2 >>= CCLIP_PRE_BITS;
      o[0] = (unsigned char)(s0 < 0 ? 0 : (s0 > 255 ? 255 : s0));
      o[1] = (unsigned char)(s1 < 0 ? 0 : (s1 > 255 ? 255 : s1));
      o[2] = (unsigned char)(s2 < 0 ? 0 : (s2 > 255 ? 255 : s2));
    }
  }
}

// out[k][c][yy][xx] (fp32 CHW) from the rows of box k in the intermediate
__global__ __launch_bounds__(256) void roi_resample_v_norm_kernel(const unsigned char* __restrict__ tmp, const cclip_roi_desc* __restrict__ desc,
                                                                  long K, int n, int ksize_max, const int* __restrict__ bounds,
                                                                  const int* __restrict__ kk, float m0, float m1, float m2, float d0,
                                                                  float d1, float d2, float* __restrict__ out) {
  const long plane = (long)n * n, total = K * plane;
  const long tmp_ld = 3L * n;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += gridDim.x * 256L) {
    const long b = t / plane, i = t % plane;
    const int xx = (int)(i % n), yy = (int)(i / n);
    const cclip_roi_desc* d = desc + b;
    const long tb = (b * 2 + 1) * n + yy;                    // the vertical tables of box b, output row yy
    const int ymin = bounds[2 * tb], yn = bounds[2 * tb + 1];
    const int* k = kk + tb * ksize_max;
    const unsigned char* p = tmp + d->tmp_off + (ymin - d->row0) * tmp_ld + (long)xx * 3;
    int s0 = 1 << (CCLIP_PRE_BITS - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < yn; ++y) {
      const int w = k[y];
      s0 += p[0] * w; s1 += p[1] * w; s2 += p[2] * w;
      p += tmp_ld;
    }
    s0 >>= CCLIP_PRE_BITS; s1 >>= CCLIP_PRE_BITS; s2 >>= CCLIP_PRE_BITS;
    s0 = s0 < 0 ? 0 : (s0 > 255 ? 255 : s0);
    s1 = s1 < 0 ? 0 : (s1 > 255 ? 255 : s1);
    s2 = s2 < 0 ? 0 : (s2 > 255 ? 255 : s2);
    float* o = out + b * 3 * plane + i;
    o[0] = ((float)s0 / 255.0f - m0) / d0;
    o[plane] = ((float)s1 / 255.0f - m1) / d1;
    o[2 * plane] = ((float)s2 / 255.0f - m2) / d2;
  }
}

// One descriptor against the geometry the kernels derive from it; returns the ksize it needs, 0 if it is inconsistent.
static int roi_desc_ksize(const cclip_roi_desc* d, int n) {
  const int64_t lim = 1 << 24;                               // every size stays far inside int and exact in a double
  if (d->w < 1 || d->h < 1 || d->w > lim || d->h > lim || d->nw < n || d->nh < n || d->nw > lim || d->nh > lim) return 0;
  if (d->left < 0 || d->top < 0 || d->left + n > d->nw || d->top + n > d->nh) return 0;
  const int kh = cclip_window_ksize((int)d->w, (int)d->nw), kv = cclip_window_ksize((int)d->h, (int)d->nh);
  int first, last;
  cclip_window_bounds((int)d->h, (int)d->nh, (int)d->top, &first);
  const int cnt = cclip_window_bounds((int)d->h, (int)d->nh, (int)d->top + n - 1, &last);
  if (d->row0 != first || d->rows != last + cnt - first || d->rows < 1) return 0;    // window starts and ends rise with the row
  return kh > kv ? kh : kv;
}

// The one check all three launchers run on the host copy of the descriptors: geometry and ksize of every box, and - where the
// launch touches that buffer (bytes >= 0) - its source and intermediate extents.  *max_rows: the most input rows a box needs.
static int roi_check(const cclip_roi_desc* desc_host, int32_t K, int32_t n, int32_t ksize_max, int64_t src_bytes, int64_t tmp_bytes,
                     int64_t* max_rows) {
  if (!desc_host || K <= 0 || n <= 0 || ksize_max <= 0 || ksize_max > CCLIP_ROI_MAX_KSIZE) return CCLIP_ERR_ARG;
  const int64_t ld_lim = (int64_t)1 << 36;                   // (h - 1) * src_ld stays below 2^60
  *max_rows = 0;
  for (int32_t b = 0; b < K; ++b) {
    const cclip_roi_desc* d = desc_host + b;
    const int need = roi_desc_ksize(d, n);
    if (need == 0 || need > ksize_max) return CCLIP_ERR_ARG;
    if (src_bytes >= 0 && (d->src_off < 0 || d->src_off > src_bytes || d->src_ld < 3 * d->w || d->src_ld > ld_lim ||
                           (d->h - 1) * d->src_ld + 3 * d->w > src_bytes - d->src_off))
      return CCLIP_ERR_ARG;
    if (tmp_bytes >= 0 && (d->tmp_off < 0 || d->tmp_off > tmp_bytes || d->rows * 3 * n > tmp_bytes - d->tmp_off)) return CCLIP_ERR_ARG;
    if (d->rows > *max_rows) *max_rows = d->rows;
  }
  return CCLIP_OK;
}

static long roi_blocks(long items) {
  long blocks = (items + 255) / 256;
  return blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
}

extern "C" int cclip_roi_coeffs(const cclip_roi_desc* desc_host, const cclip_roi_desc* desc, int32_t K, int32_t n, int32_t ksize_max,
                                int32_t* bounds_out, int32_t* kk_out, hipStream_t stream) {
  int64_t max_rows;
  if (!desc || !bounds_out || !kk_out || roi_check(desc_host, K, n, ksize_max, -1, -1, &max_rows) != CCLIP_OK) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(roi_coeffs_kernel, dim3((int)roi_blocks((long)K * 2 * n)), dim3(256), 0, stream, desc, (long)K, n, ksize_max,
                     bounds_out, kk_out);
  return cclip_launch_status();
}

extern "C" int cclip_roi_resample_h(const uint8_t* src, int64_t src_bytes, const cclip_roi_desc* desc_host, const cclip_roi_desc* desc,
                                    int32_t K, int32_t n, int32_t ksize_max, const int32_t* bounds, const int32_t* kk, uint8_t* tmp,
                                    int64_t tmp_bytes, hipStream_t stream) {
  int64_t max_rows;
  if (!src || !desc || !bounds || !kk || !tmp || src_bytes <= 0 || tmp_bytes <= 0 ||
      roi_check(desc_host, K, n, ksize_max, src_bytes, tmp_bytes, &max_rows) != CCLIP_OK)
    return CCLIP_ERR_ARG;
  const long gx = roi_blocks(max_rows * n);
  long gy = 4096 / gx;                                       // at most 4096 work-groups; both loops stride
  if (gy > K) gy = K;
  if (gy < 1) gy = 1;
  hipLaunchKernelGGL(roi_resample_h_kernel, dim3((int)gx, (int)gy), dim3(256), 0, stream, src, desc, (long)K, n, ksize_max, bounds, kk, tmp);
  return cclip_launch_status();
}

extern "C" int cclip_roi_resample_v_norm(const uint8_t* tmp, int64_t tmp_bytes, const cclip_roi_desc* desc_host, const cclip_roi_desc* desc,
                                         int32_t K, int32_t n, int32_t ksize_max, const int32_t* bounds, const int32_t* kk,
                                         const float* mean3, const float* std3, float* out, hipStream_t stream) {
  int64_t max_rows;
  if (!tmp || !desc || !bounds || !kk || !mean3 || !std3 || !out || tmp_bytes <= 0 ||
      roi_check(desc_host, K, n, ksize_max, -1, tmp_bytes, &max_rows) != CCLIP_OK)
    return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(roi_resample_v_norm_kernel, dim3((int)roi_blocks((long)K * n * n)), dim3(256), 0, stream, tmp, desc, (long)K, n, ksize_max,
                     bounds, kk, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out);
  return cclip_launch_status();
}
