// The writer of the per-pixel label kernels (dense_classes.hip: dense_label_map_kernel, dense_maps_label_kernel; dense_stitch.hip:
// dense_stitch_kernel): which pixels a thread owns, which class a pixel gets, and how labels, conf, cover and the picture reach
// memory.  The kernels form a pixel's per-class values their own way and hand the four results to lp_store_quad, so they agree
// byte for byte by construction.  Include it BELOW the file's `#pragma clang fp contract(off)` and after bilinear.h, as bilinear.h itself asks:
// the selection compares values that must come out the same in both kernels, and so must whatever is added here later.
//
// Ownership.  A thread owns FOUR consecutive pixels of the flat stream (B * S * S, or H * W): its labels are one dword, its cover
// one dword, its conf one float4, its picture bytes three dwords - from dword-aligned addresses whatever the picture's width
// is (picture b of a batch starts at byte b * S * S, 25 for S = 5), as long as the buffer itself is aligned; the stream's last,
// partial group and a misaligned buffer are stored element by element.  Vector stores only, no atomics.
//
// Picture.  palette[label], or (photo * (256 - a8) + palette[label] * a8 + 128) >> 8 per byte over a photo of the output size:
// integer arithmetic, exact given the labels.
#pragma once

#define LP_THREADS 256                                      // threads per work-group
#define LP_QUAD 4                                           // pixels per thread
#define LP_PIX (LP_QUAD * LP_THREADS)                       // pixels per work-group
#define LP_MAX_C 255                                        // classes: a label is a byte, and 255 means none

// what both kernels write, and what the picture is made from
struct lp_out {
  uint8_t* labels; float* conf; uint8_t* cover;             // cover may be null (the label map has none)
  const uint8_t* palette; const uint8_t* photo; int a8; uint8_t* overlay;   // palette / overlay may be null, photo too
  float min_conf;
};

// the conditions of an entry point on its outputs (host side)
inline bool lp_out_ok(const lp_out& o) {
  if (!o.labels || !o.conf || ((uintptr_t)o.conf & 3)) return false;
  return !(o.overlay && !o.palette) && !(o.photo && !o.overlay) && o.a8 >= 0 && o.a8 <= 256;
}

// first pixel of this thread, and how many of its four lie inside a stream of npix pixels (call only with p0 < npix)
__device__ __forceinline__ long lp_first_pixel() { return ((long)blockIdx.x * LP_THREADS + threadIdx.x) * LP_QUAD; }
__device__ __forceinline__ int lp_live(long p0, long npix) { return npix - p0 < LP_QUAD ? (int)(npix - p0) : LP_QUAD; }

// The selection: class 0 seeds, a later class replaces the best only when strictly greater (an exact tie stays with the lower
// class), and the label is 255 when the best value is below min_conf.
struct lp_pick { float best; int arg; };
__device__ __forceinline__ lp_pick lp_seed(float u0) { return lp_pick{u0, 0}; }
__device__ __forceinline__ void lp_offer(lp_pick& p, int c, float u) {
  if (u > p.best) { p.best = u; p.arg = c; }
}
__device__ __forceinline__ unsigned lp_label(lp_pick p, float min_conf) { return p.best < min_conf ? 255u : (unsigned)p.arg; }

// the palette into LDS (pal: 256 * 3 bytes); the caller owns the barrier before lp_store_quad
__device__ __forceinline__ void lp_load_palette(unsigned char* pal, const lp_out& o) {
  if (o.overlay) {
#pragma unroll
    for (int i = 0; i < 3; ++i) pal[threadIdx.x + LP_THREADS * i] = o.palette[threadIdx.x + LP_THREADS * i];
  }
}

__device__ __forceinline__ void lp_store_bytes(uint8_t* base, long p0, int n_px, const unsigned v[4]) {
  uint8_t* dst = base + p0;
  if (n_px == 4 && !((uintptr_t)base & 3)) {
    *(unsigned*)dst = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n_px) dst[i] = (uint8_t)v[i];
  }
}

// the thread's n_px pixels from p0 on: labels, cover (when there is one), conf, and the picture (when there is one)
__device__ __forceinline__ void lp_store_quad(const lp_out& o, const unsigned char* pal, long p0, int n_px, const unsigned lab[4],
                                              const float cf[4], const unsigned cov[4]) {
  const bool whole = n_px == 4;
  lp_store_bytes(o.labels, p0, n_px, lab);
  if (o.cover) lp_store_bytes(o.cover, p0, n_px, cov);
  float* co = o.conf + p0;
  if (whole && !((uintptr_t)o.conf & 15)) {
    *(float4*)co = make_float4(cf[0], cf[1], cf[2], cf[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n_px) co[i] = cf[i];
  }
  if (!o.overlay) return;

  // the 12 picture bytes of the four pixels as three little-endian dwords
  unsigned w[3] = {0u, 0u, 0u};
  if (o.photo) {
    const uint8_t* ph = o.photo + 3 * p0;
    if (whole && !((uintptr_t)o.photo & 3)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = ((const unsigned*)ph)[k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * n_px) w[k >> 2] |= (unsigned)ph[k] << (8 * (k & 3));
    }
  }
  unsigned out[3] = {0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const unsigned col = pal[lab[k / 3] * 3 + k % 3];
    const unsigned src = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    const unsigned v = o.photo ? (src * (unsigned)(256 - o.a8) + col * (unsigned)o.a8 + 128u) >> 8 : col;
    out[k >> 2] |= v << (8 * (k & 3));
  }
  uint8_t* oo = o.overlay + 3 * p0;
  if (whole && !((uintptr_t)o.overlay & 3)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ((unsigned*)oo)[k] = out[k];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * n_px) oo[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
  }
}
