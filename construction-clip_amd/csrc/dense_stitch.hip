// Dense maps for whole photos: K small class maps probs [K][C][g][g], each the dense head's answer for one window (x0, y0, x1, y1)
// of an H x W picture, stitched into one label map, confidence map and picture at the picture's size - sliding windows, a
// multi-scale ensemble (squares of several sizes in one list) or one rectangle over a non-square picture.  fp32, one launch.
// Two entry points on one core: cclip_dense_stitch keeps each pixel's best class, cclip_dense_stitch_maps every class's value.
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
// shared with dense_classes.hip.  cclip_dense_stitch_maps stores u_c [C][H][W] (0 where n = 0) from the same functions, so max_c
// of its maps IS conf, and its maps through dense_classes.hip's cclip_dense_maps_label are this file's labels, byte for byte.
//
// The core.  A work-group's 1024 pixels lie in a band of rows ylo .. yhi, inside columns xlo .. xhi when the band is one row
// (ds_band_of).  The group first scans the K boxes once, 256 at a time, and compacts IN ASCENDING k (wave ballot + a prefix over
// the four waves) the windows that meet the band into an LDS list of DS_LIST entries (ds_scan); a thread then walks that list,
// not all K.  When more than DS_LIST windows meet the band the group walks all K boxes from global memory instead (ds_list: the
// same code, the same order, the same bytes).  The list is only a filter: every walk applies the full coverage test.  Per pixel
// the axes of the first DS_FAST covering windows stay in registers (ds_walk), so their integer divisions are not repeated per
// class; windows past those are found and their axes formed again for every class (the recompute loop of ds_mean).  The two
// kernels differ in which pixels a thread owns and in what becomes of u_c, and in nothing else.  No atomics, nothing depends on
// the launch geometry: two calls give equal bytes.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)
#include "bilinear.h"
#include "label_pixels.h"

#define DS_LIST 512                                         // LDS list entries: 10 KB
#define DS_FAST 4                                           // covering windows per pixel whose axes stay in registers
#define DS_MAX_K 65535

struct ds_in { const float* probs; int K, C, g; const int* boxes; int H, W; };      // what both entry points read

// the conditions both entry points put on ds_in (host side)
static bool ds_in_ok(const ds_in& a) {
  if (!a.probs || !a.boxes || a.K < 1 || a.K > DS_MAX_K || a.C < 1 || a.C > LP_MAX_C || a.g < 1 || a.g > CCLIP_OVERLAY_MAX_SIDE)
    return false;
  if (a.H < 1 || a.H > CCLIP_OVERLAY_MAX_SIDE || a.W < 1 || a.W > CCLIP_OVERLAY_MAX_SIDE) return false;
  return !(((uintptr_t)a.probs | (uintptr_t)a.boxes) & 3);  // (H W / LP_PIX <= 2^18: the grid fits)
}

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

// the band of the group whose first pixel is g0 (< npix by the grid's size): pixels g0 .. g0 + LP_PIX - 1, clipped to the stream
struct ds_band { int ylo, yhi, xlo, xhi; };

__device__ __forceinline__ ds_band ds_band_of(long g0, long npix, int W) {
  const long g1 = (g0 + LP_PIX < npix ? g0 + LP_PIX : npix) - 1;
  ds_band bd;
  bd.ylo = (int)(g0 / W); bd.yhi = (int)(g1 / W);
  const bool one_row = bd.ylo == bd.yhi;
  bd.xlo = one_row ? (int)(g0 - (long)bd.ylo * W) : 0;
  bd.xhi = one_row ? (int)(g1 - (long)bd.yhi * W) : W - 1;
  return bd;
}

// The windows that meet the band, in ascending k, into lbox / lk [DS_LIST] (wcnt: one int per wave); returns how many meet it,
// of which the first DS_LIST are listed.  All quantities block-uniform; every round ends on a barrier, so the list may be read
// on return (K >= 1: there is a round).
__device__ __forceinline__ int ds_scan(const ds_in& a, ds_band bd, ds_box* lbox, int* lk, int* wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0;
  for (int base = 0; base < a.K; base += LP_THREADS) {
    const int k = base + tid;
    bool hit = false;
    ds_box b = {0, 0, 0, 0};
    if (k < a.K) {
      b = ds_load_box(a.boxes, k);
      hit = ds_valid(b) && b.x0 <= bd.xhi && b.x1 > bd.xlo && b.y0 <= bd.yhi && b.y1 > bd.ylo;
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
    __syncthreads();                                        // wcnt is rewritten by the next round; the list is read after the last
  }
  return total;
}

// What a walk reads: the first L entries of the LDS list, or (listed false, L = K) all K boxes from global memory.  The list's
// pointers carry the LDS address space: as plain pointers the two reads of an entry merge into one flat load of a selected address.
typedef const __attribute__((address_space(3))) int* ds_lds;
struct ds_list { ds_lds lbox, lk; const int* boxes; bool listed; int L; };

__device__ __forceinline__ ds_box ds_list_box(ds_lds lbox, int j) { return ds_box{lbox[4 * j], lbox[4 * j + 1], lbox[4 * j + 2], lbox[4 * j + 3]}; }
__device__ __forceinline__ ds_box ds_entry_box(const ds_list& li, int j) { return li.listed ? ds_list_box(li.lbox, j) : ds_load_box(li.boxes, j); }
__device__ __forceinline__ int ds_entry_k(const ds_list& li, int j) { return li.listed ? li.lk[j] : j; }

__device__ __forceinline__ ds_win ds_window(ds_box b, int k, int g, int x, int y) {
  ds_win w;
  w.k = k;
  w.ay = ov_coord_exact(y - b.y0, g, b.y1 - b.y0);
  w.ax = ov_coord_exact(x - b.x0, g, b.x1 - b.x0);
  return w;
}

// one walk for pixel (x, y): count the covering windows (n), keep the first DS_FAST in f, remember where the rest begin (jrest).
// The three stay the kernel's locals: returned in a struct, the selects below compiled to a compare tree with copies at every
// leaf, and the maps entry measured 0.6 % slower (profiles/dense_stitch_core_ab.txt).
__device__ __forceinline__ void ds_walk(const ds_list& li, int g, int x, int y, ds_win (&f)[DS_FAST], int& n, int& jrest) {
#pragma unroll
  for (int q = 0; q < DS_FAST; ++q) { f[q].k = 0; f[q].ay = ov_axis{0, 0, 0.0f}; f[q].ax = ov_axis{0, 0, 0.0f}; }
  n = 0; jrest = li.L;
  for (int j = 0; j < li.L; ++j) {
    const ds_box b = ds_entry_box(li, j);
    if (!ds_covers(b, x, y)) continue;
    if (n < DS_FAST) {
      const ds_win w = ds_window(b, ds_entry_k(li, j), g, x, y);
#pragma unroll
      for (int q = 0; q < DS_FAST; ++q)
        if (n == q) f[q] = w;                               // (selects, not a runtime-indexed array)
    } else if (n == DS_FAST) {
      jrest = j;
    }
    ++n;
  }
}

// u_c of a covered pixel (n >= 1) from its walk; pc = probs + c g g, cgg = C g g
__device__ __forceinline__ float ds_mean(const ds_list& li, const ds_win (&f)[DS_FAST], int n, int jrest, const float* pc, long cgg,
                                         int g, int x, int y) {
  float s = ov_bil(pc + f[0].k * cgg, g, f[0].ay, f[0].ax);
#pragma unroll
  for (int q = 1; q < DS_FAST; ++q)
    if (q < n) s = s + ov_bil(pc + f[q].k * cgg, g, f[q].ay, f[q].ax);
  if (n > DS_FAST) {
    for (int j = jrest; j < li.L; ++j) {                    // the recompute loop: windows past the register-resident ones
      const ds_box b = ds_entry_box(li, j);
      if (!ds_covers(b, x, y)) continue;
      const ds_win w = ds_window(b, ds_entry_k(li, j), g, x, y);
      s = s + ov_bil(pc + w.k * cgg, g, w.ay, w.ax);
    }
  }
  return s / (float)n;
}

// ---- labels, conf, cover, picture ---------------------------------------------------------------
struct ds_args { ds_in in; lp_out out; };

__global__ __launch_bounds__(LP_THREADS) void dense_stitch_kernel(const ds_args a) {
  __shared__ unsigned char pal[256 * 3];
  __shared__ ds_box lbox[DS_LIST];
  __shared__ int lk[DS_LIST];
  __shared__ int wcnt[LP_THREADS / 64];
  lp_load_palette(pal, a.out);                              // (the scan's barriers come before any read of pal)
  const ds_in& in = a.in;
  const long npix = (long)in.H * in.W;
  const int total = ds_scan(in, ds_band_of((long)blockIdx.x * LP_PIX, npix, in.W), lbox, lk, wcnt);
  const bool listed = total <= DS_LIST;                     // otherwise: walk all K boxes from global memory
  const ds_list li = {(ds_lds)lbox, (ds_lds)lk, in.boxes, listed, listed ? total : in.K};

  const long p0 = lp_first_pixel();                         // four consecutive pixels: lp_store_quad writes dwords
  if (p0 >= npix) return;
  const int n_px = lp_live(p0, npix);
  const long gg = (long)in.g * in.g, cgg = gg * in.C;

  unsigned lab[4], cov[4];
  float cf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lab[i] = 255u; cov[i] = 0u; cf[i] = 0.0f;
    if (i >= n_px) continue;
    const long p = p0 + i;
    const int y = (int)(p / in.W), x = (int)(p - (long)y * in.W);
    ds_win f[DS_FAST];
    int n, jrest;
    ds_walk(li, in.g, x, y, f, n, jrest);
    if (n == 0) continue;
    lp_pick pk = lp_seed(0.0f);
    for (int c = 0; c < in.C; ++c) {
      const float u = ds_mean(li, f, n, jrest, in.probs + c * gg, cgg, in.g, x, y);
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
  const ds_args a = {ds_in{probs, K, C, g, boxes, H, W}, lp_out{labels, conf, cover, palette, photo, a8, overlay, min_conf}};
  if (!ds_in_ok(a.in) || !lp_out_ok(a.out)) return CCLIP_ERR_ARG;
  const int64_t blocks = ((int64_t)H * W + LP_PIX - 1) / LP_PIX;
  hipLaunchKernelGGL(dense_stitch_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, a);
  return cclip_launch_status();
}

// ---- the averaged maps themselves ---------------------------------------------------------------
struct dm_args { ds_in in; float* maps; uint8_t* cover; };

__global__ __launch_bounds__(LP_THREADS) void dense_stitch_maps_kernel(const dm_args a) {
  __shared__ ds_box lbox[DS_LIST];
  __shared__ int lk[DS_LIST];
  __shared__ int wcnt[LP_THREADS / 64];
  const ds_in& in = a.in;
  const long npix = (long)in.H * in.W;
  const long g0 = (long)blockIdx.x * LP_PIX;
  const int total = ds_scan(in, ds_band_of(g0, npix, in.W), lbox, lk, wcnt);
  const bool listed = total <= DS_LIST;
  const ds_list li = {(ds_lds)lbox, (ds_lds)lk, in.boxes, listed, listed ? total : in.K};
  const long gg = (long)in.g * in.g, cgg = gg * in.C;

  for (int i = 0; i < LP_QUAD; ++i) {
    const long p = g0 + i * LP_THREADS + threadIdx.x;       // pixels g0 + t, g0 + 256 + t, ..: a class's stores are contiguous
    if (p >= npix) return;                                  // across the wave
    const int y = (int)(p / in.W), x = (int)(p - (long)y * in.W);
    ds_win f[DS_FAST];
    int n, jrest;
    ds_walk(li, in.g, x, y, f, n, jrest);
    if (a.cover) a.cover[p] = (uint8_t)(n < 255 ? n : 255);
    for (int c = 0; c < in.C; ++c)
      a.maps[c * npix + p] = n > 0 ? ds_mean(li, f, n, jrest, in.probs + c * gg, cgg, in.g, x, y) : 0.0f;
  }
}

extern "C" int cclip_dense_stitch_maps(const float* probs, int32_t K, int32_t C, int32_t g, const int32_t* boxes, int32_t H, int32_t W,
                                       float* maps, uint8_t* cover, hipStream_t stream) {
  const dm_args a = {ds_in{probs, K, C, g, boxes, H, W}, maps, cover};
  if (!ds_in_ok(a.in) || !maps || ((uintptr_t)maps & 3) || (int64_t)C * H * W > 0x7fffffffLL) return CCLIP_ERR_ARG;
  const int64_t blocks = ((int64_t)H * W + LP_PIX - 1) / LP_PIX;
  hipLaunchKernelGGL(dense_stitch_maps_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, a);
  return cclip_launch_status();
}
