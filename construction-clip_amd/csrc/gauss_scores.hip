// Gaussian class scores of 16-bit rows for gfx950: a fp32 transform T [R, D] of every row x [Q, D], then squared distances to
// C centres in the transformed space.  One kernel serves the shared-covariance classifier (T a whitening, centres the whitened
// class means, offset the log priors), the Mahalanobis outlier score (dmin) and the PCA transform (no centres: z alone).
//
// The arithmetic of hi + lo.  T enters the MFMA as the 16-bit pair hi = round16(T), lo = round16(T - hi), by
// score_pair.h's pair_image_kernel (into the workspace: a tile of 32 image rows holds hi and lo of 16 transform rows; padding
// rows are zero):
//     z[q, r]     = acc - t0[r],  acc ONE fp32 accumulator chain on v_mfma_f32_16x16x32 that takes x * hi then x * lo of
//                   every k-step d = 0, 32, 64 .. in ascending order
//     d2[q, c]    = sum_r (z[q, r] - centres[c, r])^2        fp32, r ascending, subtract - multiply - add, never expanded:
//                   |z|^2 - 2 z.m + |m|^2 cancels once the covariance is ill-conditioned, and for few-shot CLIP features it is
//     score[q, c] = -0.5 d2[q, c] + offset[c]
//     pred = argmax_c score (ties to the LOWER class, NaN lowest: score_key.h)     lse = log sum_c exp score (running maximum)
//     nearest = argmax_c (-d2) under the same rule     dmin = d2[q, nearest]
//
// Geometry.  A work-group owns 32 rows of x (16 above D = 512, where the A fragments of 32 rows would not fit the register
// file) and keeps their z on chip: fp32 [rows][Rp + 1] in LDS (Rp = 16 ceil(R / 16); at most 128.1 KB).  Stage 1: every wave
// holds the work-group's rows as A fragments and takes the transform tiles t = wave, wave + 4, ..; a tile belongs to one wave
// alone, so nothing would be shared through LDS and score_tiles.h's mover does not fit: the B fragments are read from the
// image (L2-resident, re-streamed per row block) in 16-byte loads.  That is an expectation, not a measurement; the variant
// with 64 rows and shared tiles needs 256 KB of z at R = 1024.  Stage 2, behind one barrier: 256 / rows threads per row take the
// classes c = sub, sub + tpr, .. in ascending order with a running (max, sum), best keys and the fixed xor butterfly of the
// probe's forward over the row's lanes.  A row's outputs depend on neither Q nor its position; no atomics, no fused
// multiply-add; two calls are bitwise equal.  A NaN in a row makes that row's z, d2, lse and dmin NaN (pred = nearest = 0) and
// touches no other row: a row lives on one accumulator row of every product.
#include "score_pair.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)

#define GAUSS_MAX_R 1024
#define GAUSS_MAX_C 256
#define GAUSS_NONE (-3.0e38f)                     // running maximum before the first class

namespace CCLIP_NS {

struct GaussArgs {
  const bf16* x; const bf16* img;
  long ldx;
  int Q, D, R, C;                                 // C = 0: no centres, z alone
  const float* t0; const float* centres; const float* offset;     // t0, offset may be null
  int* pred; float* lse; int* nearest; float* dmin;
  float* d2; float* z;                            // may be null
};

template <int KSMAX, int MT>
__global__ __launch_bounds__(256) void gauss_scores_kernel(const GaussArgs a) {
  constexpr int ROWS = 16 * MT, TPR = 256 / ROWS;                 // rows per work-group; threads per row in stage 2
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* zs = (float*)lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int D = a.D, R = a.R, C = a.C;
  const int nks = D >> 5;
  const int ntiles = (R + 15) >> 4;
  const int zst = 16 * ntiles + 1;                // odd: the rows of a wave's stage-2 lanes fall on different banks

  const long row0 = (long)blockIdx.x * ROWS;      // (row0 < Q: the grid has no empty block)
  const int last = (int)min((long)a.Q - 1 - row0, (long)(ROWS - 1));

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, a.x + row0 * a.ldx, a.ldx, 0, last, nks, lane);

  for (int t = wave; t < ntiles; t += 4) {        // (wave-uniform)
    const bf16* hi = a.img + ((long)t * 32 + li) * D + 8 * g;
    const bf16* lo = hi + (long)16 * D;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KSMAX; ++ks) {
      if (ks >= nks) continue;
      const bf16x8 bh = *(const bf16x8*)(hi + 32 * ks), bl = *(const bf16x8*)(lo + 32 * ks);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[mt] = CCLIP_MFMA_16x16x32(af[mt][ks], bh, acc[mt]);
        acc[mt] = CCLIP_MFMA_16x16x32(af[mt][ks], bl, acc[mt]);
      }
    }
    // lane (li, g) holds rows 16 mt + 4 g + r of transform row 16 t + li
    const int rc = 16 * t + li;
    const float sub = (a.t0 && rc < R) ? a.t0[rc] : 0.0f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rel = 16 * mt + 4 * g + r;
        const float v = acc[mt][r] - sub;
        zs[rel * zst + rc] = v;
        if (a.z && rc < R && rel <= last) a.z[(row0 + rel) * R + rc] = v;
      }
  }
  if (C == 0) return;                             // (uniform)
  __syncthreads();                                // z of the work-group's rows is whole

  const int rel = tid / TPR, sub = tid % TPR;     // the TPR lanes of a row are consecutive lanes of one wave
  const float* zr = zs + rel * zst;
  float m = GAUSS_NONE, s = 0.0f;
  u64 kbest = 0ull, knear = 0ull;
  for (int c = sub; c < C; c += TPR) {
    const float* mc = a.centres + (long)c * R;
    float d2 = 0.0f;
    for (int r = 0; r < R; ++r) {
      const float dz = zr[r] - mc[r];
      d2 += dz * dz;
    }
    const float sc = -0.5f * d2 + (a.offset ? a.offset[c] : 0.0f);
    if (a.d2 && rel <= last) a.d2[(row0 + rel) * C + c] = d2;
    const float mo = m, mn = fmaxf(mo, sc);       // a NaN score leaves the maximum and turns the sum NaN
    s = s * expf(mo - mn) + expf(sc - mn);
    m = mn;
    const unsigned low = ~(unsigned)c;
    const u64 cb = ((u64)score_key(sc) << 32) | low, cn = ((u64)score_key(-d2) << 32) | low;
    kbest = cb > kbest ? cb : kbest;
    knear = cn > knear ? cn : knear;
  }
  // the lanes of a row hold disjoint classes: a fixed xor butterfly, both partners compute the same bits.  A lane without a
  // class (C < TPR) carries (GAUSS_NONE, 0) and key 0: it changes neither the sum nor the keys.
#pragma unroll
  for (int o = 1; o < TPR; o <<= 1) {
    const float pm = __shfl_xor(m, o, 64), ps = __shfl_xor(s, o, 64);
    const u64 pb = shfl_xor64(kbest, o), pn = shfl_xor64(knear, o);
    const float mn = fmaxf(m, pm);
    const float ta = s * expf(m - mn), tb = ps * expf(pm - mn);
    s = ta + tb;
    m = mn;
    kbest = kbest > pb ? kbest : pb;
    knear = knear > pn ? knear : pn;
  }
  if (sub == 0 && rel <= last) {
    const long row = row0 + rel;
    const int nr = (int)~(unsigned)knear;
    a.pred[row] = (int)~(unsigned)kbest;
    a.lse[row] = m + logf(s);
    a.nearest[row] = nr;
    a.dmin[row] = 0.0f - key_score((unsigned)(knear >> 32));      // the key holds -d2 (its -0 as +0); NaN stays NaN
  }
}

static inline bool gauss_sizes_ok(int64_t R, int32_t D) {
  return !(R < 1 || R > GAUSS_MAX_R || !score_dim_ok(D));
}

template <int KSMAX, int MT>
static int gauss_launch(const GaussArgs& a, hipStream_t stream) {
  const int rows = 16 * MT;
  const int64_t blocks = ((int64_t)a.Q + rows - 1) / rows;
  const size_t lds = (size_t)rows * (16 * ((a.R + 15) / 16) + 1) * 4;
  return score_launch(gauss_scores_kernel<KSMAX, MT>, (unsigned)blocks, lds, a, stream);
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_gauss_scores_workspace(int64_t R, int32_t D) {
  return gauss_sizes_ok(R, D) ? (int64_t)4 * pair_image_rows((int)R) * D : 0;
}
#endif

extern "C" int CCLIP_FN(cclip_gauss_scores)(const void* x, int64_t ldx, int64_t Q, int32_t D, const float* T, const float* t0,
                                             int32_t R, const float* centres, const float* offset, int32_t C, int32_t* pred,
                                             float* lse, int32_t* nearest, float* dmin, float* d2, float* z, void* workspace,
                                             int64_t workspace_bytes, hipStream_t stream) {
  if (!x || !T || !workspace) return CCLIP_ERR_ARG;
  if (!score_rows_ok(Q) || !gauss_sizes_ok(R, D)) return CCLIP_ERR_ARG;
  if (centres) {
    if (C < 1 || C > GAUSS_MAX_C || !pred || !lse || !nearest || !dmin) return CCLIP_ERR_ARG;
  } else if (!z || offset || d2 || C != 0) return CCLIP_ERR_ARG;
  if (!score_operand_ok(x, ldx, D) || ((uintptr_t)workspace & 15)) return CCLIP_ERR_ARG;
  if (((uintptr_t)T | (uintptr_t)t0 | (uintptr_t)centres | (uintptr_t)offset | (uintptr_t)pred | (uintptr_t)lse | (uintptr_t)nearest |
       (uintptr_t)dmin | (uintptr_t)d2 | (uintptr_t)z) & 3)
    return CCLIP_ERR_ARG;
  if (workspace_bytes < (int64_t)4 * pair_image_rows(R) * D) return CCLIP_ERR_ARG;
  pair_image_launch(T, R, D, workspace, stream);
  GaussArgs a;
  a.x = (const bf16*)x; a.img = (const bf16*)workspace; a.ldx = ldx;
  a.Q = (int)Q; a.D = D; a.R = R; a.C = centres ? C : 0;
  a.t0 = t0; a.centres = centres; a.offset = offset;
  a.pred = pred; a.lse = lse; a.nearest = nearest; a.dmin = dmin; a.d2 = d2; a.z = z;
  int st;
  if (D <= 128) st = gauss_launch<4, 2>(a, stream);
  else if (D <= 512) st = gauss_launch<16, 2>(a, stream);
  else st = gauss_launch<32, 1>(a, stream);
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}
