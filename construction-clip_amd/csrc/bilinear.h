// F.interpolate(mode="bilinear", align_corners=False) of one fp32 plane, as the pixel kernels take it (relevance_overlay.hip,
// dense_classes.hip, dense_stitch.hip): s = max((i + 0.5) * L / S - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, L - 1), weight
// s - i0; separable in y and x; the identity when L == S.  Include it BELOW the file's `#pragma clang fp contract(off)`: every
// kernel needs a sample to come out the same wherever the expression is inlined.  (What the two dense kernels do with their
// samples - pick a label, store it, paint it - is label_pixels.h.)
#pragma once

struct ov_axis { int i0, i1; float w; };

// source samples and weight of output index i on an axis of L source samples (scale = L / S)
__device__ __forceinline__ ov_axis ov_coord(int i, float scale, int L) {
  float s = __builtin_fmaf(scale, (float)i + 0.5f, -0.5f);
  s = s > 0.0f ? s : 0.0f;
  ov_axis a;
  a.i0 = (int)s;
  if (a.i0 > L - 1) a.i0 = L - 1;                           // s < L - 0.5 in exact arithmetic; never leave the source
  a.i1 = a.i0 + 1 < L ? a.i0 + 1 : L - 1;
  a.w = s - (float)a.i0;
  return a;
}

// The same axis with the source coordinate formed in integers: s = ((2 i + 1) L - S) / (2 S) exactly, so i0 is exact and the
// weight is one rounding of remainder / (2 S).  ov_coord's fp32 product carries the rounding of s itself, half an ulp of L
// (1e-6 at L = 24), into the weight; a result that is held to 1e-6 of float64 needs this form.  L, S <= 16384: (2 i + 1) L < 2^30.
__device__ __forceinline__ ov_axis ov_coord_exact(int i, int L, int S) {
  const int num = (2 * i + 1) * L - S, den = 2 * S;
  ov_axis a;
  if (num <= 0) { a.i0 = 0; a.w = 0.0f; }
  else { a.i0 = num / den; a.w = (float)(num - a.i0 * den) / (float)den; }
  a.i1 = a.i0 + 1 < L ? a.i0 + 1 : L - 1;
  return a;
}

__device__ __forceinline__ float ov_bil(const float* __restrict__ src, int ld, ov_axis ay, ov_axis ax) {
  const float* r0 = src + (long)ay.i0 * ld;
  const float* r1 = src + (long)ay.i1 * ld;
  const float p00 = r0[ax.i0], p01 = r0[ax.i1], p10 = r1[ax.i0], p11 = r1[ax.i1];
  const float w1 = ax.w, w0 = 1.0f - w1, h1 = ay.w, h0 = 1.0f - h1;
  return h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11);
}
