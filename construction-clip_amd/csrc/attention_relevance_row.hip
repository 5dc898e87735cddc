// One row of the attention relevance (Chefer et al.) of one layer for gfx950, any T <= 8192, head_dim 64: the per-layer step of
// the reference's `interpret()` (attention.py:14-69) for the only rows its callers read - the class-token row of R_image and
// the EOT row of R_text.  The backward visits the layers top-down and right-multiplies (R <- R + R C_l), so one row of the final
// R obeys the same recurrence on a row vector; for every sequence b (length T_b):
//     P_h  = exp(scale Q_h K_h^T - lse_h)            (causal: 0 above the diagonal)
//     dP_h = dA_h V_h^T                              (dA: gradient at the attention output, from the dgrad chain)
//     r_out[j] = r_in[j] + 1 / (H grad_scale) * sum_{i < T_b} r_in[i] * sum_h max(P_h[i, j] dP_h[i, j], 0)     (j < T_b)
//     r_out[j] = r_in[j]                                                                                      (T_b <= j < T)
// A flash-style streaming reduction over the query rows: no T x T object exists, neither in LDS nor in HBM (attention_relevance.hip
// keeps the whole C in LDS, which ends at T = 128).
//
// One workgroup (4 waves) per sequence and per block of 64 keys.  Heads are looped; K_h and V_h of the key block are staged in LDS
// with blk_load / blk_store (attention_tiles.h), the next head's loads in flight under this head's MFMAs.  Each wave walks the
// query tiles wave, wave + 4, ...: rel_tile of attention_relevance_core.h (shared with the matrix kernel) forms max(p dp, 0), and
// max(p dp, 0) r_in[i] accumulates in 4 key tiles x 4 registers per lane across all heads and query tiles.  A query tile whose 16
// r_in values are all zero is skipped (wave-uniform; it would add exactly zero), so a one-hot r - the default start_layer = -1 -
// touches one query tile per sequence.  The end is a fixed-order reduction: the 4 accumulator rows, the 4 lane groups (cross-lane
// moves), the 4 waves (LDS).  No atomics: two launches agree bit for bit.  No predicated global loads: rows are clamped.
//
// Correctness and determinism at every T are the goal here, not speed: the grid is B x ceil(T / 64), so one ViT-L/14@336px image
// (T = 577) is 10 workgroups, and every workgroup re-reads all of Q and dA of its sequence.  That is accepted - the step runs once
// per layer of a single explanation pass, next to a dgrad chain that costs far more.
#include "attention_relevance_core.h"

namespace CCLIP_NS {

struct RelRowArgs : RelCommon {
  const float* r_in;                              // [B, T]
  float* r_out;                                   // [B, T], not r_in
  int nkb;                                        // ceil(T / 64) key blocks per sequence
};

// dynamic LDS: K image (8 KiB) | V image (8 KiB) | r_in of the sequence, zero-padded to whole query tiles (16 ceil(T / 16) floats)
// Held at three waves per SIMD, as the kernel ran before the tile moved to the shared header (the allocation alone, 124 registers,
// allows four): at T = 577 the 640 workgroups are 2.5 per CU, and with room for a fourth they pack unevenly - 346 us against 328 us.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_relevance_row_kernel(const RelRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + 64 * 128;
  float* red = (float*)smem;                      // after the head loop: [4 waves][64 keys]
  float* rs = (float*)(smem + 2 * 64 * 128);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.nkb, k0 = 64 * (blockIdx.x - b * a.nkb);
  long row0;
  const int T = rel_seq(a, b, row0);
  const float* rin = a.r_in + (long)b * a.T;
  float* rout = a.r_out + (long)b * a.T;
  if (k0 >= T) {                                  // (workgroup-uniform) no live key in this block: the row passes through
    if (tid < 64 && k0 + tid < a.T) rout[k0 + tid] = rin[k0 + tid];
    return;
  }
  const int nqt = (T + 15) >> 4;
  for (int i = tid; i < 16 * nqt; i += 256) rs[i] = i < T ? rin[i] : 0.f;

  f32x4 c[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) c[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (T - k0 + 15) >> 4;             // live key tiles of this block (>= 1)
  const int qt0 = a.causal ? k0 >> 4 : 0;         // causal: every query before the block's first key sees none of its keys

  uint4 rk[2], rv[2];
  auto kv_load = [&](int h) {
    blk_load(a.k + h * 64, a.ldk, row0, k0, T, rk, tid);
    blk_load(a.v + h * 64, a.ldv, row0, k0, T, rv, tid);
  };
  kv_load(0);
  for (int h = 0; h < a.H; ++h) {
    __syncthreads();                              // everyone is done with the previous head's K / V (first pass: rs is written)
    blk_store(Ks, k0, T, rk, tid);
    blk_store(Vs, k0, T, rv, tid);
    if (h + 1 < a.H) kv_load(h + 1);              // in flight under this head's MFMAs
    __syncthreads();
    for (int qt = qt0 + wave; qt < nqt; qt += 4) {
      float rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rq[r] = rs[16 * qt + 4 * g + r];
      if (!__ballot(rq[0] != 0.f || rq[1] != 0.f || rq[2] != 0.f || rq[3] != 0.f)) continue;   // (wave-uniform) adds exactly zero
      const RelQTile q = rel_qtile(a, row0, b, h, qt, T, lane);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        if (kt >= nkt || (a.causal && k0 + 16 * kt > 16 * qt + 15)) continue;
        const f32x4 t = rel_tile(a, q, Ks, Vs, qt, kt, k0, T, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r)               // a masked entry adds an exact zero whatever r_in holds (no 0 * inf)
          c[kt][r] += rel_sees(a, T, 16 * qt + 4 * g + r, k0 + 16 * kt + li) ? t[r] * rq[r] : 0.f;
      }
    }
  }
  __syncthreads();                                // K / V images are dead: the waves' partial rows take their place
  // fixed order: the 4 accumulator rows, then the 4 lane groups, then (below) the 4 waves
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    float s = (c[kt][0] + c[kt][1]) + (c[kt][2] + c[kt][3]);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (g == 0) red[wave * 64 + 16 * kt + li] = s;
  }
  __syncthreads();
  if (tid < 64 && k0 + tid < a.T) {
    const int j = k0 + tid;
    const float s = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
    rout[j] = j < T ? rin[j] + s * a.cscale : rin[j];
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_attention_relevance_row)(const cclip_attn_desc* d, float grad_scale, const float* r_in, float* r_out,
                                                       hipStream_t stream) {
  RelRowArgs a;
  if (rel_common_from_desc(d, grad_scale, 8192, a) != CCLIP_OK) return CCLIP_ERR_ARG;
  if (!r_in || !r_out || r_in == r_out || (((uintptr_t)r_in | (uintptr_t)r_out) & 3)) return CCLIP_ERR_ARG;
  a.r_in = r_in; a.r_out = r_out; a.nkb = (d->T + 63) / 64;
  if ((long)a.B * a.nkb > 0x7fffffffL) return CCLIP_ERR_ARG;
  const size_t lds = 2 * 64 * 128 + sizeof(float) * 16 * ((d->T + 15) / 16);     // <= 48 KiB at T = 8192
  hipLaunchKernelGGL(attn_relevance_row_kernel, dim3(a.B * a.nkb), dim3(256), lds, stream, a);
  return cclip_launch_status();
}
