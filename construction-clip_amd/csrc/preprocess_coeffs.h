// PIL's BICUBIC resampling windows and 8-bit integer coefficients (libImaging/Resample.c: precompute_coeffs +
// normalize_coeffs_8bpc, restated from the published algorithm; bicubic a = -0.5, 22 fraction bits), one output sample at a
// time, for the host and for the device.  clip/preprocess_device.py:resample_coeffs is the Python statement of the same
// arithmetic and tests compare the two number by number, so everything here is double precision in PIL's operation order:
//   * no expression may be contracted into a fused multiply-add (one fma changes a rounded coefficient): every function body
//     below starts with CCLIP_NO_FMA, and a host-only build adds -ffp-contract=off for compilers without the pragma;
//   * double -> int conversions truncate (C casts);
//   * the weights of a window are summed one after the other and each is divided by that sum;
//   * rounding is (int)(+-0.5 + w * 2^22).
// Plain C++ with no HIP dependency: a host compiler can build it alone (tests/test_preprocess_rois_cpu.py does).
#ifndef CCLIP_PREPROCESS_COEFFS_H
#define CCLIP_PREPROCESS_COEFFS_H
#include <math.h>

// contraction off for the one function body the macro opens (a file-scope pragma would reach into every includer)
#if defined(__clang__)
#define CCLIP_NO_FMA _Pragma("clang fp contract(off)")
#else
#define CCLIP_NO_FMA
#endif

#if defined(__HIPCC__)
#define CCLIP_HD __host__ __device__ static inline
#else
#define CCLIP_HD static inline
#endif

#define CCLIP_PRE_BITS 22
#define CCLIP_ROI_MAX_KSIZE 257       // taps of a window at a downscale factor of 64, the largest the ROI kernels accept

CCLIP_HD double cclip_bicubic(double x) {
  CCLIP_NO_FMA
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// row length of the coefficient table of an in_size -> out_size resize (PIL's ksize)
CCLIP_HD int cclip_window_ksize(int in_size, int out_size) {
  CCLIP_NO_FMA
  double filterscale = (double)in_size / (double)out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale;
  return (int)ceil(support) * 2 + 1;
}

// window [*first, *first + count) of output sample xx; returns count
CCLIP_HD int cclip_window_bounds(int in_size, int out_size, int xx, int* first) {
  CCLIP_NO_FMA
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *first = xmin;
  return xmax - xmin;
}

// window and coefficients of output sample xx: writes min(count, cap) integers to k, returns count.  The weights are
// evaluated twice (once for the sum, once for the quotient) instead of being kept: the same expression gives the same bits.
CCLIP_HD int cclip_window_coeffs(int in_size, int out_size, int xx, int* first, int* k, int cap) {
  CCLIP_NO_FMA
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double ss = 1.0 / filterscale;
  const double center = (xx + 0.5) * scale;
  int xmin;
  const int count = cclip_window_bounds(in_size, out_size, xx, &xmin);
  double ww = 0.0;
  for (int x = 0; x < count; ++x) ww += cclip_bicubic(((double)(x + xmin) - center + 0.5) * ss);
  const int m = count < cap ? count : cap;
  for (int x = 0; x < m; ++x) {
    double w = cclip_bicubic(((double)(x + xmin) - center + 0.5) * ss);
    if (ww != 0.0) w = w / ww;
    k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << CCLIP_PRE_BITS)) : (int)(0.5 + w * (double)(1 << CCLIP_PRE_BITS));
  }
  *first = xmin;
  return count;
}

#endif
