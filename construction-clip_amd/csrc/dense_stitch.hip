// Dense maps for whole photos: K small class maps probs [K][C][g][g], each the dense head's answer for one window (x0, y0, x1, y1)
// of an H x W picture, stitched into one label map, confidence map and picture at the picture's size - sliding windows, a
// multi-scale ensemble (squares of several sizes in one list) or one rectangle over a non-square picture.  fp32, one launch.
//
// Window k covers pixel (x, y) when x0 <= x < x1, y0 <= y < y1 and both sides lie in [1, CCLIP_OVERLAY_MAX_SIDE] (sides formed in
// 64 bits: any int32 box is safe); an empty, inverted or oversized box covers nothing and a box may hang over the picture's edge.
// A covering window's sample of class c is window-local align_corners=False bilinear sampling, each axis with its own side:
//     s_kc = ov_bil(probs[k][c], g, ov_coord_exact(y - y0, g, y1 - y0), ov_coord_exact(x - x0, g, x1 - x0))         (bilinear.h)
// where 0 <= x - x0 < side <= 16384, so every source index stays inside the g x g map whatever the box holds: no box value
// makes the kernel read outside probs.  With the n covering windows k1 < k2 < .. in ascending k
//     u_c = ((s_k1c + s_k2c) + ..) / (float)n       seeded with the first sample, fp32 adds left to right, ONE division (n = 1 too)
//     conf = max_c u_c, label = the lowest class reaching it (strictly greater replaces), 255 when conf < min_conf;
//     n = 0: label 255, conf 0;  cover = min(n, 255);  picture bytes: label_pixels.h's integer formula on the label.
// For K = 1, H = W = S and box (0, 0, S, S) this is dense_label_map's arithmetic, bit for bit (x / 1.0f == x): the selection
// rule, the ownership of the flat [H * W] stream (four consecutive pixels per thread) and every store are label_pixels.h's,
// shared with dense_classes.hip.
//
// A work-group's 1024 pixels lie in a band of rows ylo .. yhi (inside columns xlo .. xhi when the band is one row).  The group first
// scans the K boxes once, 256 at a time, and compacts IN ASCENDING k (wave ballot + a prefix over the four waves) the windows
// that meet the band into an LDS list of DS_LIST entries; a thread then walks that list, not all K.  When more than DS_LIST
// windows meet the band the group walks all K boxes from global memory instead (the same code, the same order, the same bytes).
// The list is only a filter: every walk applies the full coverage test.  Per pixel the axes of the first DS_FAST covering
// windows stay in registers, so their integer divisions are not repeated per class; windows past those are found and their
// axes formed again for every class (the recompute loop).  No atomics, nothing depends on the launch geometry: two calls give
// equal bytes.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)
#include "bilinear.h"
#include "label_pixels.h"

#define DS_LIST 512                                         // LDS list entries: 10 KB
#define DS_FAST 4                                           // covering windows per pixel whose axes stay in registers
#define DS_MAX_K 65535

struct ds_args {
  const float* probs; int K, C, g;
  const int* boxes; int H, W;
  lp_out out;
};

struct ds_box { int x0, y0, x1, y1; };
struct ds_win { int k; ov_axis ay, ax; };

__device__ __forceinline__ bool ds_valid(ds_box b) {
  const long sw = (long)b.x1 - (long)b.x0, sh = (long)b.y1 - (long)b.y0;
  return sw >= 1 && sw <= CCLIP_OVERLAY_MAX_SIDE && sh >= 1 && sh <= CCLIP_OVERLAY_MAX_SIDE;
}

__device__ __forceinline__ bool ds_covers(ds_box b, int x, int y) {
  return ds_valid(b) && b.x0 <= x && x < b.x1 && b.y0 <= y && y < b.y1;
}

__device__ __forceinline__ ds_box ds_load_box(const int* __restrict__ boxes, int k) {
  const int* p = boxes + 4 * (long)k;
  ds_box b;
  b.x0 = p[0]; b.y0 = p[1]; b.x1 = p[2]; b.y1 = p[3];
  return b;
}

__global__ __launch_bounds__(LP_THREADS) void dense_stitch_kernel(const ds_args a) {
  __shared__ unsigned char pal[256 * 3];
  __shared__ ds_box lbox[DS_LIST];
  __shared__ int lk[DS_LIST];
  __shared__ int wcnt[LP_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  lp_load_palette(pal, a.out);                              // (the scan's barriers come before any read of pal)

  const long npix = (long)a.H * a.W;
  const long g0 = (long)blockIdx.x * LP_PIX;                // first pixel of the group; < npix by the grid's size
  const long g1 = (g0 + LP_PIX < npix ? g0 + LP_PIX : npix) - 1;
  const int ylo = (int)(g0 / a.W), yhi = (int)(g1 / a.W);
  const bool one_row = ylo == yhi;
  const int xlo = one_row ? (int)(g0 - (long)ylo * a.W) : 0;
  const int xhi = one_row ? (int)(g1 - (long)yhi * a.W) : a.W - 1;

  // the windows that meet the band, in ascending k (all quantities block-uniform)
  int total = 0;
  for (int base = 0; base < a.K; base += LP_THREADS) {
    const int k = base + tid;
    bool hit = false;
    ds_box b = {0, 0, 0, 0};
    if (k < a.K) {
      b = ds_load_box(a.boxes, k);
      hit = ds_valid(b) && b.x0 <= xhi && b.x1 > xlo && b.y0 <= yhi && b.y1 > ylo;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int pos = total + __popcll(m & ((1ull << lane) - 1ull));
    int sum = 0;
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) {
      const int c = wcnt[w];
      if (w < wave) pos += c;
      sum += c;
    }
    if (hit && pos < DS_LIST) { lbox[pos] = b; lk[pos] = k; }
    total += sum;
    __syncthreads();                                        // wcnt is rewritten by the next round; the list is read below
  }
  const bool listed = total <= DS_LIST;                     // otherwise: walk all K boxes from global memory
  const int L = listed ? total : a.K;

  const long p0 = lp_first_pixel();                         // g0 + 4 tid
  if (p0 >= npix) return;
  const int n_px = lp_live(p0, npix);
  const long gg = (long)a.g * a.g, cgg = gg * a.C;

  unsigned lab[4], cov[4];
  float cf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lab[i] = 255u; cov[i] = 0u; cf[i] = 0.0f;
    if (i >= n_px) continue;
    const long p = p0 + i;
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);

    // one walk: count the covering windows, keep the first DS_FAST, remember where the rest begin
    ds_win f[DS_FAST];
#pragma unroll
    for (int q = 0; q < DS_FAST; ++q) { f[q].k = 0; f[q].ay = ov_axis{0, 0, 0.0f}; f[q].ax = ov_axis{0, 0, 0.0f}; }
    int n = 0, jrest = L;
    for (int j = 0; j < L; ++j) {
      const ds_box b = listed ? lbox[j] : ds_load_box(a.boxes, j);
      if (!ds_covers(b, x, y)) continue;
      if (n < DS_FAST) {
        ds_win w;
        w.k = listed ? lk[j] : j;
        w.ay = ov_coord_exact(y - b.y0, a.g, b.y1 - b.y0);
        w.ax = ov_coord_exact(x - b.x0, a.g, b.x1 - b.x0);
#pragma unroll
        for (int q = 0; q < DS_FAST; ++q)
          if (n == q) f[q] = w;                             // (selects, not a runtime-indexed array)
      } else if (n == DS_FAST) {
        jrest = j;
      }
      ++n;
    }
    if (n == 0) continue;

    const float fn = (float)n;
    lp_pick pk = lp_seed(0.0f);
    for (int c = 0; c < a.C; ++c) {
      const float* pc = a.probs + c * gg;
      float s = ov_bil(pc + f[0].k * cgg, a.g, f[0].ay, f[0].ax);
#pragma unroll
      for (int q = 1; q < DS_FAST; ++q)
        if (q < n) s = s + ov_bil(pc + f[q].k * cgg, a.g, f[q].ay, f[q].ax);
      if (n > DS_FAST) {
        for (int j = jrest; j < L; ++j) {                   // the recompute loop: windows past the register-resident ones
          const ds_box b = listed ? lbox[j] : ds_load_box(a.boxes, j);
          if (!ds_covers(b, x, y)) continue;
          const long k = listed ? lk[j] : j;
          s = s + ov_bil(pc + k * cgg, a.g, ov_coord_exact(y - b.y0, a.g, b.y1 - b.y0), ov_coord_exact(x - b.x0, a.g, b.x1 - b.x0));
        }
      }
      const float u = s / fn;
      if (c == 0) pk = lp_seed(u);                          // class 0 seeds whatever its value, as in dense_label_map; offering
      else lp_offer(pk, c, u);                              // it to a -inf start would part from that on a NaN or -inf sample
    }
    lab[i] = lp_label(pk, a.out.min_conf);
    cf[i] = pk.best;
    cov[i] = n < 255 ? (unsigned)n : 255u;
  }

  lp_store_quad(a.out, pal, p0, n_px, lab, cf, cov);
}

extern "C" int cclip_dense_stitch(const float* probs, int32_t K, int32_t C, int32_t g, const int32_t* boxes, int32_t H, int32_t W,
                                  float min_conf, uint8_t* labels, float* conf, uint8_t* cover, const uint8_t* palette,
                                  const uint8_t* photo, int32_t a8, uint8_t* overlay, hipStream_t stream) {
  if (!probs || !boxes || K < 1 || K > DS_MAX_K || C < 1 || C > LP_MAX_C || g < 1 || g > CCLIP_OVERLAY_MAX_SIDE || H < 1 ||
      H > CCLIP_OVERLAY_MAX_SIDE || W < 1 || W > CCLIP_OVERLAY_MAX_SIDE)
    return CCLIP_ERR_ARG;
  ds_args a;
  a.probs = probs; a.K = K; a.C = C; a.g = g; a.boxes = boxes; a.H = H; a.W = W;
  a.out = lp_out{labels, conf, cover, palette, photo, a8, overlay, min_conf};
  if (!lp_out_ok(a.out) || (((uintptr_t)probs | (uintptr_t)boxes) & 3)) return CCLIP_ERR_ARG;
  const int64_t npix = (int64_t)H * W;
  const int64_t blocks = (npix + LP_PIX - 1) / LP_PIX;
  if (blocks > 0x7fffffff) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(dense_stitch_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, a);
  return cclip_launch_status();
}
