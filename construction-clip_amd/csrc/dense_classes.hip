// Dense zero-shot maps (training-free dense CLIP: MaskCLIP, Zhou et al. 2022; SCLIP / ClearCLIP-style q.q^T, k.k^T variants):
// the head that turns per-patch features and C class embeddings into per-patch class probabilities, and those into a label
// map and picture at display size.  Three kernels, all fp32.
//
// cclip_dense_class_probs.  feat [M = B * P][E] (row stride ldf), text [C][E], neither normalised:
//     cos[m][c]      = <feat_m, text_c> * inv(|feat_m|) * inv(|text_c|),  inv(n) = 1 / n, and 0 when n == 0 (no epsilon is added
//                      to a norm, as in cclip_l2norm_fwd; a zero row scores cos = 0 against every class: the uniform distribution)
//     probs[b][c][p] = softmax_c(scale * cos[b * P + p][c])               class-major: probs[b][c] is a g x g map
// One wave per feature row, 16 rows per work-group.  A lane keeps its part of the row in registers (float4 lane, lane + 64, ..:
// E <= 1024 is four of them).  The text passes through LDS in tiles of 16 classes (8 above E = 512: 32 KB), staged once for the
// 16 rows; wave w forms the inverse norm of the tile's class w from the LDS copy.  A dot product is the lane's float4s in
// ascending order, then the fixed xor butterfly of wave_sum; lane c % 64 keeps logit c in register c / 64 (C <= 255 is four);
// the softmax is a wave maximum and a wave sum.  No atomics, nothing depends on M or on the row's position in the launch: two
// calls give equal bytes.
//
// cclip_dense_label_map.  probs [B][C][g][g] -> per output pixel of the S x S picture the bilinear sample u_c of every class map
// (bilinear.h: F.interpolate(mode="bilinear", align_corners=False), the source coordinate formed in integers - conf is held to
// 1e-6 of float64, which the fp32 coordinate product misses at grid 24), conf = max_c u_c, label = the FIRST class that reaches
// it (a later class replaces the best only when strictly greater), 255 when conf < min_conf; and optionally the picture, the
// label's palette colour alone or blended in integers over a photo of the output size.  The selection rule, the ownership of
// the flat [B * S * S] stream (four consecutive pixels per thread), every store and the picture's formula are label_pixels.h's,
// shared with dense_stitch.hip: the kernel here is the per-pixel class loop and one call.
//
// cclip_dense_maps_label.  maps [B][C][H][W] already at the output size (dense_stitch.hip's averaged maps, refined or not by
// dense_refine.hip) -> labels, conf and the picture by the same selection and the same writer; a pixel whose cover byte is 0
// gets label 255 and conf 0, the stitch's n = 0 rule.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#define DC_THREADS 1024
#define DC_ROWS (DC_THREADS / 64)                           // feature rows per work-group: one per wave
#define DC_TILE 16                                          // classes per LDS tile at E <= 512
#define DC_TILE_FLOATS 8192                                 // 32 KB
#define DC_MAX_C 255                                        // label_pixels.h's cap (asserted below), inside the 4 * 64 logit slots
#define DC_MAX_E 1024

__device__ __forceinline__ float dc_dot4(float4 a, float4 b, float acc) {
  acc = __builtin_fmaf(a.x, b.x, acc);
  acc = __builtin_fmaf(a.y, b.y, acc);
  acc = __builtin_fmaf(a.z, b.z, acc);
  return __builtin_fmaf(a.w, b.w, acc);
}

__device__ __forceinline__ float dc_inv_norm(float ss) { return ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f; }

__global__ __launch_bounds__(DC_THREADS) void dense_class_probs_kernel(const float* __restrict__ feat, long ldf, int M, int P,
                                                                       const float* __restrict__ text, int C, int E, float scale,
                                                                       float* __restrict__ probs, float* __restrict__ logits_out) {
  __shared__ __attribute__((aligned(16))) float tile[DC_TILE_FLOATS];
  __shared__ float tinv[DC_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E4 = E >> 2;
  const int tcap = E <= DC_TILE_FLOATS / DC_TILE ? DC_TILE : DC_TILE / 2;      // 16 * 512 = 8 * 1024 = DC_TILE_FLOATS
  const long row = (long)blockIdx.x * DC_ROWS + wave;
  const bool live = row < M;                                // (a dead wave still stages and meets the barriers)

  float4 f[4];
  float ss = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k;
    f[k] = (live && i < E4) ? ((const float4*)(feat + row * ldf))[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    ss = dc_dot4(f[k], f[k], ss);
  }
  const float finv = dc_inv_norm(wave_sum(ss));

  float lg[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // logit of class 64 s + lane
  const float4* tile4 = (const float4*)tile;
  for (int c0 = 0; c0 < C; c0 += tcap) {                    // (c0 is a multiple of 8: a tile lies inside one 64-class slot)
    const int tc = min(tcap, C - c0);
    __syncthreads();                                        // the previous tile has been read
    const float4* src = (const float4*)(text + (long)c0 * E);
    for (int i = tid; i < tc * E4; i += DC_THREADS) ((float4*)tile)[i] = src[i];
    __syncthreads();
    if (wave < tc) {                                        // (wave-uniform)
      float ts = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        if (i < E4) { const float4 t = tile4[wave * E4 + i]; ts = dc_dot4(t, t, ts); }
      }
      ts = wave_sum(ts);
      if (lane == 0) tinv[wave] = dc_inv_norm(ts);
    }
    __syncthreads();
    float acc[DC_TILE];
#pragma unroll
    for (int j = 0; j < DC_TILE; ++j) {
      acc[j] = 0.0f;
      if (j < tc) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = lane + 64 * k;
          if (i < E4) acc[j] = dc_dot4(f[k], tile4[j * E4 + i], acc[j]);
        }
      }
    }
    const int slot = c0 >> 6;
#pragma unroll
    for (int j = 0; j < DC_TILE; ++j) {
      if (j < tc) {                                         // (wave-uniform)
        const float v = scale * (wave_sum(acc[j]) * finv * tinv[j]);
        if (lane == ((c0 + j) & 63)) {
#pragma unroll
          for (int s = 0; s < 4; ++s) lg[s] = s == slot ? v : lg[s];
        }
      }
    }
  }

  const float m = wave_max(fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3])));
  float e[4], sum = 0.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    e[s] = 64 * s + lane < C ? expf(lg[s] - m) : 0.0f;
    sum += e[s];
  }
  sum = wave_sum(sum);
  if (!live) return;
  const long b = row / P, p = row - b * P;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = 64 * s + lane;
    if (c < C) {
      const long o = (b * C + c) * P + p;
      probs[o] = e[s] / sum;
      if (logits_out) logits_out[o] = lg[s];
    }
  }
}

extern "C" int cclip_dense_class_probs(const float* feat, int64_t ldf, int64_t M, int32_t P, const float* text, int32_t C, int32_t E,
                                       float scale, float* probs, float* logits_out, hipStream_t stream) {
  if (!feat || !text || !probs || M < 1 || M > 0x7fffffff || P < 1 || M % P != 0) return CCLIP_ERR_ARG;
  if (C < 1 || C > DC_MAX_C || E < 4 || (E & 3) || E > DC_MAX_E || ldf < E || (ldf & 3)) return CCLIP_ERR_ARG;
  if ((((uintptr_t)feat | (uintptr_t)text) & 15) || (((uintptr_t)probs | (uintptr_t)logits_out) & 3)) return CCLIP_ERR_ARG;
  const int64_t blocks = (M + DC_ROWS - 1) / DC_ROWS;
  hipLaunchKernelGGL(dense_class_probs_kernel, dim3((unsigned)blocks), dim3(DC_THREADS), 0, stream, feat, (long)ldf, (int)M, P, text, C, E,
                     scale, probs, logits_out);
  return cclip_launch_status();
}

// ---- label map ---------------------------------------------------------------------------------
#pragma clang fp contract(off)
#include "bilinear.h"
#include "label_pixels.h"

static_assert(DC_MAX_C == LP_MAX_C, "dense_class_probs must not make more classes than a label can name");

struct dl_args {
  const float* probs; int B, C, g, S;
  lp_out out;
};

__global__ __launch_bounds__(LP_THREADS) void dense_label_map_kernel(const dl_args a) {
  __shared__ unsigned char pal[256 * 3];
  lp_load_palette(pal, a.out);
  __syncthreads();
  const long plane = (long)a.S * a.S, npix = plane * a.B;
  const long p0 = lp_first_pixel();
  if (p0 >= npix) return;
  const int n = lp_live(p0, npix);
  const long gg = (long)a.g * a.g;

  unsigned lab[4];
  const unsigned nocov[4] = {0u, 0u, 0u, 0u};               // (a.out.cover is null: never stored)
  float cf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lab[i] = 0u; cf[i] = 0.0f;
    if (i < n) {
      const long p = p0 + i, b = p / plane, r = p - b * plane;
      const int y = (int)(r / a.S), x = (int)(r - (long)y * a.S);
      const ov_axis ay = ov_coord_exact(y, a.g, a.S), ax = ov_coord_exact(x, a.g, a.S);
      const float* src = a.probs + b * a.C * gg;
      lp_pick pk = lp_seed(ov_bil(src, a.g, ay, ax));
      for (int c = 1; c < a.C; ++c) lp_offer(pk, c, ov_bil(src + c * gg, a.g, ay, ax));
      lab[i] = lp_label(pk, a.out.min_conf);
      cf[i] = pk.best;
    }
  }
  lp_store_quad(a.out, pal, p0, n, lab, cf, nocov);
}

extern "C" int cclip_dense_label_map(const float* probs, int32_t B, int32_t C, int32_t g, int32_t S, float min_conf, uint8_t* labels,
                                     float* conf, const uint8_t* palette, const uint8_t* photo, int32_t a8, uint8_t* overlay,
                                     hipStream_t stream) {
  if (!probs || B < 1 || C < 1 || C > LP_MAX_C || g < 1 || g > CCLIP_OVERLAY_MAX_SIDE || S < 1 || S > CCLIP_OVERLAY_MAX_SIDE)
    return CCLIP_ERR_ARG;
  dl_args a;
  a.probs = probs; a.B = B; a.C = C; a.g = g; a.S = S;
  a.out = lp_out{labels, conf, nullptr, palette, photo, a8, overlay, min_conf};
  if (!lp_out_ok(a.out) || ((uintptr_t)probs & 3)) return CCLIP_ERR_ARG;
  const int64_t npix = (int64_t)B * S * S;
  const int64_t blocks = (npix + LP_PIX - 1) / LP_PIX;
  if (blocks > 0x7fffffff) return CCLIP_ERR_ARG;
  hipLaunchKernelGGL(dense_label_map_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, a);
  return cclip_launch_status();
}

// ---- class maps at the output size -> labels, conf, picture -------------------------------------
struct ml_args { const float* maps; const uint8_t* cover; int B, C; long plane; lp_out out; };

__global__ __launch_bounds__(LP_THREADS) void dense_maps_label_kernel(const ml_args a) {
  __shared__ unsigned char pal[256 * 3];
  lp_load_palette(pal, a.out);
  __syncthreads();
  const long npix = a.B * a.plane;
  const long p0 = lp_first_pixel();
  if (p0 >= npix) return;
  const int n_px = lp_live(p0, npix);
  unsigned lab[4], cov[4];
  float cf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lab[i] = 255u; cov[i] = 0u; cf[i] = 0.0f;
    if (i >= n_px) continue;
    const long p = p0 + i;
    if (a.cover && a.cover[p] == 0) continue;               // the stitch's n = 0 rule
    const long b = p / a.plane;
    const float* m = a.maps + b * a.C * a.plane + (p - b * a.plane);
    lp_pick pk = lp_seed(m[0]);
    for (int c = 1; c < a.C; ++c) lp_offer(pk, c, m[c * a.plane]);
    lab[i] = lp_label(pk, a.out.min_conf);
    cf[i] = pk.best;
  }
  lp_store_quad(a.out, pal, p0, n_px, lab, cf, cov);
}

extern "C" int cclip_dense_maps_label(const float* maps, int32_t B, int32_t C, int32_t H, int32_t W, const uint8_t* cover,
                                      float min_conf, uint8_t* labels, float* conf, const uint8_t* palette, const uint8_t* photo,
                                      int32_t a8, uint8_t* overlay, hipStream_t stream) {
  if (!maps || B < 1 || C < 1 || C > LP_MAX_C || H < 1 || H > CCLIP_OVERLAY_MAX_SIDE || W < 1 || W > CCLIP_OVERLAY_MAX_SIDE) return CCLIP_ERR_ARG;
  if ((int64_t)B * C * H * W > 0x7fffffffLL || ((uintptr_t)maps & 3)) return CCLIP_ERR_ARG;
  ml_args a;
  a.maps = maps; a.cover = cover; a.B = B; a.C = C; a.plane = (long)H * W;
  a.out = lp_out{labels, conf, nullptr, palette, photo, a8, overlay, min_conf};
  if (!lp_out_ok(a.out)) return CCLIP_ERR_ARG;
  const int64_t blocks = ((int64_t)B * a.plane + LP_PIX - 1) / LP_PIX;
  hipLaunchKernelGGL(dense_maps_label_kernel, dim3((unsigned)blocks), dim3(LP_THREADS), 0, stream, a);
  return cclip_launch_status();
}
