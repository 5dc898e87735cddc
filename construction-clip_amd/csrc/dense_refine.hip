// Image-guided refinement of dense class maps (pixel-adaptive mask refinement, PAMR: Araslanov & Roth, "Single-Stage Semantic
// Segmentation from Image Labels", CVPR 2020), stated from the paper's formulas (include/cclip_hip.h holds the contract; no other
// implementation was compared).  fp32, two entry points (the maps come from dense_stitch.hip's cclip_dense_stitch_maps and are
// labelled by dense_classes.hip's cclip_dense_maps_label):
//
//   cclip_dense_refine_prepare  guide uint8 [B][H][W][3] -> key float4 per pixel: 1 / (1e-8 + 0.1 sigma_k), k = 0..2, and the
//                               log-normaliser L of the pixel's 8 D neighbour logits
//   cclip_dense_refine_step     one iteration maps_in -> maps_out: m'_c(p) = sum_n exp(a_n(p) - L(p)) m_c(q_n), ascending n
//
// Neighbour n = 8 j + e of pixel p is clamp(p + d_j o_e), o_e in the order (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1).
// The logit a_n = -(1/3) sum_k |x_k(p) - x_k(q_n)| f_k with x = byte / 255 is formed by ONE function (rf_logit) from the two
// packed pixels and the key's factors: the bytes' difference is an exact integer, so a_n = (sum_k |db_k| f_k) * (-1 / 765), and
// prepare's L and the step's weights see the same bits.
//
// Tiles.  prepare and step give a work-group a 32 x 32 tile, one pixel per thread (1024 threads), and stage the tile plus a
// halo of hal = max d (<= 24) in LDS: (32 + 2 hal)^2 <= 80 x 80 cells of 4 bytes, 25.6 KB a plane.  A halo cell holds the value
// at its CLAMPED coordinates, so cell (ly + oy d, lx + ox d) IS clamp(p + d o) and the inner loop has no bounds test.  Two planes:
// the step stages the packed guide in plane 1 and class 0 in plane 0, forms its 8 D weights into registers (the step kernel is
// instantiated per D, so the weights are named registers and not an indexed array), then streams the classes: class c + 1
// is fetched into registers before the 8 D FMAs of class c and written to the other plane after them - one barrier a class.
// A third table of 25.6 KB holds, per staged cell, where in a plane it comes from (76.8 KB of LDS in all, no scratch).
// Why 32 x 32 x 1: a thread that owned two pixels would hold 96 weights, past the 128-register budget of a 1024-thread group;
// a 16 x 16 tile would read (16 + 48)^2 / 256 = 16 cells per pixel from global memory where this one reads 6.25.
// No atomics, nothing depends on the launch geometry: two calls give equal bytes.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)
#include "bilinear.h"
#include "label_pixels.h"

#define RF_TILE 32
#define RF_THREADS (RF_TILE * RF_TILE)
#define RF_MAX_D CCLIP_REFINE_MAX_DILATIONS                 // 6
#define RF_MAX_DIL CCLIP_REFINE_MAX_DILATION                // 24
#define RF_SIDE (RF_TILE + 2 * RF_MAX_DIL)                  // 80
#define RF_CELLS (RF_SIDE * RF_SIDE)                        // 6400
#define RF_PER_THREAD ((RF_CELLS + RF_THREADS - 1) / RF_THREADS)   // 7 cells of a plane per thread

struct rf_geom {
  int B, H, W, D, hal, side;                                // hal = max d, side = 32 + 2 hal
  int tiles_x, tiles_y;
  int d[RF_MAX_D];
};

struct rf_tile { int b, y0, x0; };

__device__ __forceinline__ rf_tile rf_this_tile(const rf_geom& g) {
  const unsigned per = (unsigned)(g.tiles_x * g.tiles_y);   // <= 512 * 512
  rf_tile t;
  t.b = (int)(blockIdx.x / per);
  const int r = (int)(blockIdx.x - (unsigned)t.b * per);
  const int ty = r / g.tiles_x;
  t.y0 = ty * RF_TILE;
  t.x0 = (r - ty * g.tiles_x) * RF_TILE;
  return t;
}

__device__ __forceinline__ int rf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// offset (inside one H x W plane) of the clamped pixel behind cell i of the staged tile, -1 past the last cell
__device__ __forceinline__ int rf_cell_offset(const rf_geom& g, rf_tile t, int i) {
  if (i >= g.side * g.side) return -1;
  const int ly = i / g.side, lx = i - ly * g.side;
  return rf_clamp(t.y0 - g.hal + ly, g.H - 1) * g.W + rf_clamp(t.x0 - g.hal + lx, g.W - 1);
}

__device__ __forceinline__ unsigned rf_load_rgb(const uint8_t* __restrict__ guide, long pixel) {
  const uint8_t* p = guide + 3 * pixel;
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

__device__ __forceinline__ float rf_byte(unsigned v, int k) { return (float)((v >> (8 * k)) & 255u); }

// a_n of centre pc and neighbour qc (packed r, g, b) under the centre's three factors
__device__ __forceinline__ float rf_logit(unsigned pc, unsigned qc, float f0, float f1, float f2) {
  float s = fabsf(rf_byte(pc, 0) - rf_byte(qc, 0)) * f0;
  s = __builtin_fmaf(fabsf(rf_byte(pc, 1) - rf_byte(qc, 1)), f1, s);
  s = __builtin_fmaf(fabsf(rf_byte(pc, 2) - rf_byte(qc, 2)), f2, s);
  return s * (-1.0f / 765.0f);
}

// offset of neighbour e at dilation d from a cell of a staged plane whose rows are `side` cells apart (wave-uniform)
__device__ __forceinline__ int rf_tap(int e, int d, int side) {
  const int oy = e < 3 ? -1 : (e < 5 ? 0 : 1);
  const int ox = (e == 0 || e == 3 || e == 5) ? -1 : ((e == 1 || e == 6) ? 0 : 1);
  return (oy * side + ox) * d;
}

// ---- prepare ------------------------------------------------------------------------------------
struct rf_prepare_args { const uint8_t* guide; float4* key; rf_geom g; };

__global__ __launch_bounds__(RF_THREADS) void dense_refine_prepare_kernel(const rf_prepare_args a) {
  __shared__ unsigned gl[RF_CELLS];
  const rf_geom& g = a.g;
  const rf_tile t = rf_this_tile(g);
  const int tid = threadIdx.x;
  const long plane = (long)g.H * g.W;
  for (int i = tid; i < g.side * g.side; i += RF_THREADS) gl[i] = rf_load_rgb(a.guide, t.b * plane + rf_cell_offset(g, t, i));
  __syncthreads();
  const int tx = tid & (RF_TILE - 1), ty = tid >> 5;
  const int y = t.y0 + ty, x = t.x0 + tx;
  if (y >= g.H || x >= g.W) return;
  const int base = (ty + g.hal) * g.side + tx + g.hal;
  const unsigned pc = gl[base];

  // sigma from integer sums of the bytes over the 9 D taps (the centre once per dilation): n sum(b^2) - sum(b)^2 is exact
  int s1[3], s2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = (int)((pc >> (8 * k)) & 255u);
    s1[k] = g.D * v; s2[k] = g.D * v * v;
  }
  for (int j = 0; j < g.D; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned q = gl[base + rf_tap(e, g.d[j], g.side)];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int v = (int)((q >> (8 * k)) & 255u);
        s1[k] += v; s2[k] += v * v;
      }
    }
  }
  const int n = 9 * g.D;                                    // n s2 <= 54 * 54 * 65025 < 2^31
  float f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float var = (float)(n * s2[k] - s1[k] * s1[k]) / (float)(n * (n - 1));   // of the bytes
    const float sigma = sqrtf(var) / 255.0f;
    f[k] = 1.0f / (1e-8f + 0.1f * sigma);
  }

  // L = max a + log sum exp(a - max), the logits formed twice rather than kept
  float mx = -INFINITY;
  for (int j = 0; j < g.D; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, rf_logit(pc, gl[base + rf_tap(e, g.d[j], g.side)], f[0], f[1], f[2]));
  }
  float sum = 0.0f;
  for (int j = 0; j < g.D; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sum = sum + expf(rf_logit(pc, gl[base + rf_tap(e, g.d[j], g.side)], f[0], f[1], f[2]) - mx);
  }
  a.key[t.b * plane + (long)y * g.W + x] = make_float4(f[0], f[1], f[2], mx + logf(sum));
}

// ---- step ---------------------------------------------------------------------------------------
struct rf_step_args { const float* in; float* out; const uint8_t* guide; const float4* key; int C; rf_geom g; };

template <int D>
__global__ __launch_bounds__(RF_THREADS) void dense_refine_step_kernel(const rf_step_args a) {
  __shared__ float buf[2 * RF_CELLS];                       // two planes
  const rf_geom& g = a.g;
  const rf_tile t = rf_this_tile(g);
  const int tid = threadIdx.x;
  const long plane = (long)g.H * g.W;

  // where this thread's cells of every staged plane come from; kept in LDS (each thread reads back its own entries only):
  // seven more registers, and the 64-bit addresses made from them, would not fit beside 48 weights
  __shared__ int offs[RF_CELLS];
#pragma unroll
  for (int r = 0; r < RF_PER_THREAD; ++r)
    if (tid + r * RF_THREADS < RF_CELLS) offs[tid + r * RF_THREADS] = rf_cell_offset(g, t, tid + r * RF_THREADS);
#define RF_OFF(r) (tid + (r) * RF_THREADS < RF_CELLS ? offs[tid + (r) * RF_THREADS] : -1)

  unsigned* gl = (unsigned*)(buf + RF_CELLS);
  const float* in = a.in + (long)t.b * a.C * plane;
#pragma unroll
  for (int r = 0; r < RF_PER_THREAD; ++r) {
    if (RF_OFF(r) >= 0) {
      gl[tid + r * RF_THREADS] = rf_load_rgb(a.guide, t.b * plane + RF_OFF(r));
      buf[tid + r * RF_THREADS] = in[RF_OFF(r)];
    }
  }
  __syncthreads();

  const int tx = tid & (RF_TILE - 1), ty = tid >> 5;
  const int y = t.y0 + ty, x = t.x0 + tx;
  const bool live = y < g.H && x < g.W;
  const int base = (ty + g.hal) * g.side + tx + g.hal;
  int tap[8 * D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) tap[8 * j + e] = rf_tap(e, g.d[j], g.side);
  }
  float w[8 * D];
  {
    const float4 key = live ? a.key[t.b * plane + (long)y * g.W + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const unsigned pc = gl[base];
#pragma unroll
    for (int n = 0; n < 8 * D; ++n) w[n] = expf(rf_logit(pc, gl[base + tap[n]], key.x, key.y, key.z) - key.w);
  }
  __syncthreads();                                          // the guide's plane is free: class 1 lands there

  float* out = a.out + (long)t.b * a.C * plane + (long)y * g.W + x;
  for (int c = 0; c < a.C; ++c) {
    const float* cur = buf + (c & 1) * RF_CELLS + base;     // this pixel in plane c
    float* nxt = buf + ((c + 1) & 1) * RF_CELLS;
    const bool more = c + 1 < a.C;
    float pre[RF_PER_THREAD];
#pragma unroll
    for (int r = 0; r < RF_PER_THREAD; ++r) pre[r] = (more && RF_OFF(r) >= 0) ? in[(c + 1) * plane + RF_OFF(r)] : 0.0f;

    float acc = w[0] * cur[tap[0]];
#pragma unroll
    for (int n = 1; n < 8 * D; ++n) acc = __builtin_fmaf(w[n], cur[tap[n]], acc);
    if (live) out[c * plane] = acc;

    if (more) {
#pragma unroll
      for (int r = 0; r < RF_PER_THREAD; ++r)
        if (RF_OFF(r) >= 0) nxt[tid + r * RF_THREADS] = pre[r];
    }
    __syncthreads();                                        // plane c + 1 is written; plane c may be overwritten next round
  }
}

// ---- host side of prepare / step ----------------------------------------------------------------
static bool rf_geom_ok(rf_geom& g, int32_t B, int32_t H, int32_t W, const int32_t* dilations, int32_t D, int64_t per_pixel) {
  if (!dilations || D < 1 || D > RF_MAX_D || B < 1 || H < 1 || H > CCLIP_OVERLAY_MAX_SIDE || W < 1 || W > CCLIP_OVERLAY_MAX_SIDE) return false;
  if ((int64_t)B * H * W * per_pixel > 0x7fffffffLL) return false;
  g.B = B; g.H = H; g.W = W; g.D = D; g.hal = 0;
  for (int j = 0; j < RF_MAX_D; ++j) {
    g.d[j] = j < D ? dilations[j] : 0;
    if (j < D && (g.d[j] < 1 || g.d[j] > RF_MAX_DIL)) return false;
    if (g.d[j] > g.hal) g.hal = g.d[j];
  }
  g.side = RF_TILE + 2 * g.hal;
  g.tiles_x = (W + RF_TILE - 1) / RF_TILE;
  g.tiles_y = (H + RF_TILE - 1) / RF_TILE;
  return true;                                              // B tiles_x tiles_y <= B H W <= 2^31 - 1: the grid fits
}

extern "C" int cclip_dense_refine_prepare(const uint8_t* guide, int32_t B, int32_t H, int32_t W, const int32_t* dilations,
                                          int32_t D, float* key, hipStream_t stream) {
  rf_prepare_args a;
  if (!guide || !key || ((uintptr_t)key & 15) || !rf_geom_ok(a.g, B, H, W, dilations, D, 1)) return CCLIP_ERR_ARG;
  a.guide = guide; a.key = (float4*)key;
  const unsigned blocks = (unsigned)B * (unsigned)(a.g.tiles_x * a.g.tiles_y);
  hipLaunchKernelGGL(dense_refine_prepare_kernel, dim3(blocks), dim3(RF_THREADS), 0, stream, a);
  return cclip_launch_status();
}

extern "C" int cclip_dense_refine_step(const float* maps_in, float* maps_out, const uint8_t* guide, const float* key, int32_t B,
                                       int32_t C, int32_t H, int32_t W, const int32_t* dilations, int32_t D, hipStream_t stream) {
  rf_step_args a;
  if (!maps_in || !maps_out || !guide || !key || C < 1 || C > LP_MAX_C || !rf_geom_ok(a.g, B, H, W, dilations, D, C)) return CCLIP_ERR_ARG;
  if ((((uintptr_t)maps_in | (uintptr_t)maps_out) & 3) || ((uintptr_t)key & 15)) return CCLIP_ERR_ARG;
  const uintptr_t bytes = (uintptr_t)B * C * H * W * 4, pi = (uintptr_t)maps_in, po = (uintptr_t)maps_out;
  if (pi < po + bytes && po < pi + bytes) return CCLIP_ERR_ARG;                  // in place, or overlapping
  a.in = maps_in; a.out = maps_out; a.guide = guide; a.key = (const float4*)key; a.C = C;
  const dim3 grid((unsigned)B * (unsigned)(a.g.tiles_x * a.g.tiles_y)), block(RF_THREADS);
  switch (D) {
    case 1: hipLaunchKernelGGL(dense_refine_step_kernel<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(dense_refine_step_kernel<2>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(dense_refine_step_kernel<3>, grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(dense_refine_step_kernel<4>, grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL(dense_refine_step_kernel<5>, grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL(dense_refine_step_kernel<6>, grid, block, 0, stream, a); break;
  }
  return cclip_launch_status();
}
