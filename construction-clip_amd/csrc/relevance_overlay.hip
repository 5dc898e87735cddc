// Relevance overlays: N patch-relevance vectors and their images -> N finished 8-bit RGB pictures (the reference's
// show_image_relevance / show_cam_on_image, attention.py:77-96) in ONE launch.  The upsampled map, the min-max normalised image
// and the blend never reach memory; what comes back per picture is 3 * S * S bytes.
//
// For overlay n, output pixel (y, x), output size S, relevance grid g x g, image [3, R, R] - all fp32:
//   bil(src, L, i)  F.interpolate(mode="bilinear", align_corners=False): s = max((i + 0.5) * L / S - 0.5, 0), i0 = floor(s),
//                   i1 = min(i0 + 1, L - 1), weight s - i0; separable in y and x; the identity when L == S
//   u     = bil of the relevance grid; lo, hi = min, max of u over the picture;        m = (u - lo) / (hi - lo)          (0 if hi == lo)
//   v_c   = bil of image channel c;    ilo, ihi = min, max of v over the 3 channels;   xn_c = (v_c - ilo) / (ihi - ilo)  (0 if ihi == ilo)
//   k     = min(floor(255 m), 255);    cam_c = lut[k][c] + xn_c;   M = max of cam over the 3 channels of the picture
//   out[n][y][x][c] = floor(255 * (cam_c / M))                                                                          (0 if M == 0)
//
// One work-group of 1024 threads per overlay walks its pixels three times - (1) lo, hi, ilo, ihi; (2) M (and the optional map
// output); (3) the bytes - and takes the samples again in every pass: a 224 x 224 image is 600 KB and stays in L2, the grid is a
// few hundred bytes.  The three reductions are wave shuffles plus 16 LDS words each; there is no atomic and no hand-over between
// work-groups, so two launches give the same bytes.  Contraction to fused multiply-adds is switched off for the whole file: a
// sample has to come out bit-identical in all three passes (a u one ulp below the lo of pass 1 would index the colour table at
// -1), and that must not hang on the compiler fusing the same expression the same way in three inlined copies.
//
// Pass 3 stores 12-byte runs of the picture's byte stream from dword-aligned addresses (three dwords per thread = four pixels,
// or parts of five when the run does not start on a pixel).  Overlay n starts at byte n * 3 * S * S, which is not dword-aligned
// for odd S: the bytes before the first aligned address and after the last whole run (at most 3 + 11) are stored one by one.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)
#include "bilinear.h"                                       // ov_axis, ov_coord, ov_bil (shared with dense_classes.hip)

#define OV_THREADS 1024
#define OV_WAVES (OV_THREADS / 64)

struct ov_geom {
  const float* rel; const float* img;                       // this overlay's grid and image
  int g, R, S;
  float sg, sr;                                             // g / S, R / S
  long plane;                                               // R * R
};

// u and the three v of pixel p (< S * S).  With R == S every weight is 0 and bil returns its first sample: read that one alone.
__device__ __forceinline__ void ov_sample(const ov_geom& G, int p, float& u, float (&v)[3]) {
  const int y = p / G.S, x = p - y * G.S;
  u = ov_bil(G.rel, G.g, ov_coord(y, G.sg, G.g), ov_coord(x, G.sg, G.g));
  if (G.R == G.S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = G.img[c * G.plane + p];
  } else {
    const ov_axis ay = ov_coord(y, G.sr, G.R), ax = ov_coord(x, G.sr, G.R);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ov_bil(G.img + c * G.plane, G.R, ay, ax);
  }
}

// the K maxima of the work-group, in every thread.  red: K * OV_WAVES words of LDS
template <int K>
__device__ __forceinline__ void ov_block_max(float (&v)[K], float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_max(v[k]);
  __syncthreads();                                          // the previous reduction's words have been read
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * OV_WAVES + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float m = red[k * OV_WAVES];
#pragma unroll
    for (int w = 1; w < OV_WAVES; ++w) m = fmaxf(m, red[k * OV_WAVES + w]);
    v[k] = m;
  }
}

struct ov_norm { float lo, rng, ilo, irng; };               // rng = hi - lo, irng = ihi - ilo

// m and cam of pixel p; lut is the LDS copy of the colour table
__device__ __forceinline__ void ov_cam(const ov_geom& G, const ov_norm& Z, const float* lut, int p, float& m, float (&cam)[3]) {
  float u, v[3];
  ov_sample(G, p, u, v);
  m = Z.rng > 0.0f ? (u - Z.lo) / Z.rng : 0.0f;
  const float t = 255.0f * m;
  const int k = t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);  // floor, and inside the table whatever u is (a NaN gives 0)
#pragma unroll
  for (int c = 0; c < 3; ++c) cam[c] = lut[k * 3 + c] + (Z.irng > 0.0f ? (v[c] - Z.ilo) / Z.irng : 0.0f);
}

// the three bytes of pixel p in bits 0..23
__device__ __forceinline__ unsigned ov_pixel(const ov_geom& G, const ov_norm& Z, const float* lut, float M, int p) {
  float m, cam[3];
  ov_cam(G, Z, lut, p, m, cam);
  unsigned px = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = M > 0.0f ? 255.0f * (cam[c] / M) : 0.0f;
    const unsigned b = t >= 255.0f ? 255u : (t > 0.0f ? (unsigned)t : 0u);
    px |= b << (8 * c);
  }
  return px;
}

__global__ __launch_bounds__(OV_THREADS) void relevance_overlay_kernel(const float* __restrict__ rel, int g, const float* __restrict__ images,
                                                                       long image_stride, int R, const float* __restrict__ lut_g, int S,
                                                                       unsigned char* __restrict__ out, float* __restrict__ map_out) {
  __shared__ float lut[256 * 3];
  __shared__ float red[4 * OV_WAVES];
  const long n = blockIdx.x;
  const int tid = threadIdx.x;
  const int npix = S * S;
  ov_geom G;
  G.rel = rel + n * g * g;
  G.img = images + n * image_stride;
  G.g = g; G.R = R; G.S = S;
  G.sg = (float)g / (float)S;
  G.sr = (float)R / (float)S;
  G.plane = (long)R * R;
  if (tid < 256 * 3) lut[tid] = lut_g[tid];                 // (first read after the barriers of pass 1's reduction)

  // pass 1: -lo, hi, -ilo, ihi
  float r[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int p = tid; p < npix; p += OV_THREADS) {
    float u, v[3];
    ov_sample(G, p, u, v);
    r[0] = fmaxf(r[0], -u);
    r[1] = fmaxf(r[1], u);
    const float vmin = fminf(fminf(v[0], v[1]), v[2]), vmax = fmaxf(fmaxf(v[0], v[1]), v[2]);
    r[2] = fmaxf(r[2], -vmin);
    r[3] = fmaxf(r[3], vmax);
  }
  ov_block_max<4>(r, red);
  ov_norm Z;
  Z.lo = -r[0]; Z.rng = r[1] - Z.lo;
  Z.ilo = -r[2]; Z.irng = r[3] - Z.ilo;

  // pass 2: M, and the map where it is asked for
  float mx[1] = {-INFINITY};
  float* mo = map_out ? map_out + n * npix : nullptr;
  for (int p = tid; p < npix; p += OV_THREADS) {
    float m, cam[3];
    ov_cam(G, Z, lut, p, m, cam);
    if (mo) mo[p] = m;
    mx[0] = fmaxf(mx[0], fmaxf(fmaxf(cam[0], cam[1]), cam[2]));
  }
  ov_block_max<1>(mx, red);
  const float M = mx[0];

  // pass 3: the bytes.  [0, head) and [head + 12 * runs, total) one by one, the runs between as three dwords each
  unsigned char* o = out + n * 3 * npix;
  const int total = 3 * npix;
  int head = (int)((4 - ((uintptr_t)o & 3)) & 3);
  if (head > total) head = total;
  const int runs = (total - head) / 12;
  const int tail0 = head + 12 * runs;
  const int edge = head + (total - tail0);                  // <= 14
  if (tid < edge) {
    const int j = tid < head ? tid : tail0 + (tid - head);
    o[j] = (unsigned char)(ov_pixel(G, Z, lut, M, j / 3) >> (8 * (j % 3)));
  }
  const int skip = head % 3;                                // bytes of pixel p0 that belong to the run before (12 = 4 pixels)
  const int p_head = head / 3;
  for (int c = tid; c < runs; c += OV_THREADS) {
    const int p0 = p_head + 4 * c;                          // pixel of byte head + 12 c
    // 16 bytes of the stream from pixel p0 on; the fifth pixel exists whenever skip > 0 (the run ends inside it)
    const unsigned a = ov_pixel(G, Z, lut, M, p0), b = ov_pixel(G, Z, lut, M, p0 + 1), d = ov_pixel(G, Z, lut, M, p0 + 2),
                   e = ov_pixel(G, Z, lut, M, p0 + 3), f = skip ? ov_pixel(G, Z, lut, M, p0 + 4) : 0u;
    const unsigned w0 = a | (b << 24), w1 = (b >> 8) | (d << 16), w2 = (d >> 16) | (e << 8), w3 = f;
    const int sh = 8 * skip;
    unsigned* q = (unsigned*)(o + head + 12 * (long)c);
    q[0] = (unsigned)(((((unsigned long long)w1) << 32) | w0) >> sh);
    q[1] = (unsigned)(((((unsigned long long)w2) << 32) | w1) >> sh);
    q[2] = (unsigned)(((((unsigned long long)w3) << 32) | w2) >> sh);
  }
}

extern "C" int cclip_relevance_overlay(const float* rel, int32_t N, int32_t g, const float* images, int64_t image_stride, int32_t R,
                                       const float* lut, int32_t S, uint8_t* out, float* map_out, hipStream_t stream) {
  if (!rel || !images || !lut || !out || N < 1 || g < 1 || g > CCLIP_OVERLAY_MAX_SIDE || R < 1 || R > CCLIP_OVERLAY_MAX_SIDE ||
      S < 1 || S > CCLIP_OVERLAY_MAX_SIDE)
    return CCLIP_ERR_ARG;
  if (image_stride != 0 && image_stride < 3 * (int64_t)R * R) return CCLIP_ERR_ARG;
  if (((uintptr_t)rel | (uintptr_t)images | (uintptr_t)lut | (uintptr_t)map_out) & 3) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(relevance_overlay_kernel, dim3((unsigned)N), dim3(OV_THREADS), 0, stream, rel, g, images, (long)image_stride, R, lut,
                     S, out, map_out);
  return cclip_launch_status();
}
