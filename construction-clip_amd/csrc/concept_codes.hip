// Concept decomposition for gfx950: every row of x [N, D] (unit 16-bit rows) as a sparse, non-negative combination of the rows
// of a dictionary c [V, D] (unit 16-bit rows).  Per row, independently,
//     minimise over w >= 0:   1/2 |x - sum_v w_v c_v|^2  +  l1 sum_v w_v
// by FISTA with the non-negative soft threshold, a FIXED iteration count and beta_k = k / (k + 3):
//     y_k     = w_k + beta_k (w_k - w_{k-1})                    (w_0 = w_{-1} = 0)
//     g_v     = <c_v, x - sum_u y_{k,u} c_u>
//     w_{k+1} = max(0, y_k + eta (g - l1))
// All `iters` iterations and the closing read-out run inside ONE launch: rows never interact, so a work-group owns 16 MT rows
// from the first iteration to the last and re-streams the dictionary (from L2 / HBM) once per iteration.  No grid-wide
// synchronisation, no host read.
//
// One iteration = one sweep.  The only state carried between sweeps besides w is the residual at the NEXT point the gradient is
// taken at, r(y_{k+1}) = x - sum_v y_{k+1,v} c_v: when a tile's w_{k+1} is known, so is y_{k+1} (w_k was just read for y_k), and
// it is y_{k+1} that is multiplied back.  The last iteration multiplies w_T back instead, so that the closing sweep takes its
// gradient at w_T itself.  Per tile of 32 concepts (score_tiles.h's image, two LDS buffers):
//   1. g^T[v, row] partial = tile x r over this wave's columns                        (MFMA, A from LDS, B = r as hi + lo)
//   2. the four waves' partials meet in LDS and are added ((p0 + p1) + p2) + p3; every wave applies the prox to the whole
//      16 MT x 32 block (redundantly: each needs all of it as an operand), one wave per row tile stores w_{k+1}
//   3. acc[d, row] += c^T[d, v] (-y_{k+1})[v, row] over the wave's columns            (MFMA, A from the SAME LDS tile through
//      ds_read_b64_tr_b16 - score_pair.h's tile_frag_tr -, B = -y_{k+1} as hi + lo) - acc started the sweep as x
// The columns are split over the four waves in runs of ceil(D / 128) k-steps of 32 (a wave beyond D only helps to load), the
// rows are not: a wave holds all 16 MT rows of its columns, as fp32 accumulators AND as the 16-bit pair the next sweep's first
// product reads.  That is 2 x MT x KSW x 8 registers: 128 at <KSW, MT> = <4, 2> (D <= 512, 32 rows) and <8, 1> (D <= 1024, 16 rows).
// Twice the rows (256 registers of state) were built first and spilled 560 - 656 bytes a lane: the tile staging, the weights
// held across the second barrier and the four partials of every row tile live beside the state.  As chosen no variant
// spills (409 / 481 registers at D <= 512 / D <= 1024: one work-group of four waves on a CU).  The first product's k
// index inside a k-step is permuted (k = 4 h + r  <->  d = 32 ks + 16 h + 4 g + r) so that a lane's accumulators ARE its B
// operand: no shuffle, no LDS round trip between the sweeps.
//
// Operand form.  r and -y enter the MFMA as hi = round16(v), lo = round16(v - hi) (split16); one accumulator chain takes hi then lo of
// every k-step in ascending order.  w is fp32; w_{k+1} is written over w_{k-1} (two buffers, [N, V] each: the caller's w and the
// workspace; the last iteration writes the caller's).  Padding concepts (V up to the tile) are loaded as copies of the last
// row, their operand is a selected 0, their weights are never written and never counted.
// Read-outs (closing sweep, at w_T): resid2 = |r(w_T)|^2 from the fp32 accumulators, l1norm = sum w, nnz = #{w > 0},
// delta = max |w_T - w_{T-1}|, kkt = max (w > 0 ? |g - l1| : max(0, g - l1)).  Maxima propagate NaN: a NaN in a row of x makes
// every float read-out of that row NaN (nnz counts w > 0, so 0) and touches no other row - a row lives on one lane column of
// every product.  A row's outputs are a function of (the row, c, l1, eta, iters) alone; no atomics, no fused multiply-add, one
// summation order: two calls are bitwise equal.
#include "score_pair.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them
#pragma clang fp contract(off)

#define CONCEPT_GT 32                             // concepts per tile: one k-step of the second product
#define CONCEPT_MAX_V (1 << 24)

namespace CCLIP_NS {

struct ConceptArgs {
  const bf16* x; const bf16* c;
  long ldx, ldc;
  int N, V, D, iters;
  float l1, eta;
  float* w; long ldw;                             // the caller's [N, V]: w_T at the end
  float* w2; long ldw2;                           // the workspace's [N, V]
  float* resid2; float* l1norm; int* nnz; float* delta; float* kkt;
};

// max that keeps a NaN once it has met one
__device__ __forceinline__ float concept_nanmax(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

// four weights v0 .. v0 + 3 of a row: one 16-byte access where all four exist, else element by element below V
__device__ __forceinline__ f32x4 concept_load4(const float* row, int v0, int V) {
  if (v0 + 3 < V) return *(const f32x4*)(row + v0);
  f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (v0 + r < V) o[r] = row[v0 + r];
  return o;
}
__device__ __forceinline__ void concept_store4(float* row, int v0, int V, f32x4 v) {
  if (v0 + 3 < V) { *(f32x4*)(row + v0) = v; return; }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (v0 + r < V) row[v0 + r] = v[r];
}

// <KSMAX, KSW, MT>: k-steps of 32 a tile row has at most (D <= 32 KSMAX); k-steps a wave owns at most (D <= 128 KSW); row tiles
// of 16 per work-group
template <int KSMAX, int KSW, int MT>
__global__ __launch_bounds__(256) void concept_codes_kernel(const ConceptArgs a) {
  constexpr int GT = CONCEPT_GT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int V = a.V, D = a.D, T = a.iters;
  const TileGeom geo(D);
  const int tilebytes = GT * geo.rowbytes;
  f32x4* part = (f32x4*)(lds + 2 * tilebytes);    // [wave][mt][st][lane]: the waves' partial gradients of a tile
  const int ntiles = (V + GT - 1) / GT;

  const int ksw = (geo.nks + 3) >> 2;             // k-steps per wave; this wave's are ks0 .. ks0 + nown - 1
  const int ks0 = wave * ksw;
  const int nown = max(0, min(ksw, geo.nks - ks0));               // (wave-uniform)

  const long row0 = (long)blockIdx.x * (16 * MT);                 // (row0 < N: the grid has no empty block)
  const int last = (int)min((long)a.N - 1 - row0, (long)(16 * MT - 1));
  // this lane's row of row tile mt is 16 mt + li; a row beyond the last is computed on a copy of the last and never stored
  long xr[MT];
  bool live[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    live[mt] = 16 * mt + li <= last;
    xr[mt] = row0 + min(16 * mt + li, last);
  }

  f32x4 acc[MT][2 * KSW];                         // [mt][2 i + h]: row 16 mt + li, columns 32 (ks0 + i) + 16 h + 4 g .. + 3
  bf16x8 rhi[MT][KSW], rlo[MT][KSW];              // the same values as the first product's B operand
  auto load_x = [&]() CCLIP_SWEEP_INLINE {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < KSW; ++i) {
        if (i >= nown) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bf16x4 v = *(const bf16x4*)(a.x + xr[mt] * a.ldx + 32 * (ks0 + i) + 16 * h + 4 * g);
          acc[mt][2 * i + h] = (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        }
      }
  };
  auto split = [&]() CCLIP_SWEEP_INLINE {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < KSW; ++i) {
        if (i >= nown) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) split16(acc[mt][2 * i + (j >> 2)][j & 3], rhi[mt][i], rlo[mt][i], j);
      }
  };

  // read-outs of the closing sweep, per row tile: this lane's share of its row
  float so_l1[MT], so_delta[MT], so_kkt[MT];
  int so_nnz[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) { so_l1[mt] = 0.0f; so_delta[mt] = 0.0f; so_kkt[mt] = 0.0f; so_nnz[mt] = 0; }

  TileMover<KSMAX, GT> mover(geo, tid);
  load_x();
  int buf = 0;                                    // alternates over ALL tiles of all sweeps: a sweep of one tile never meets its own buffer
  for (int k = 0; k <= T; ++k) {
    const bool closing = k == T;                  // (uniform)
    split();
    if (!closing) load_x();
    // w_k is read from cur, w_{k-1} from prev, w_{k+1} written over w_{k-1}; iteration k writes the caller's buffer iff T - 1 - k is even
    const bool to_w = ((T - 1 - k) & 1) == 0;
    float* const nxt = closing ? a.w : (to_w ? a.w : a.w2);
    const long ldn = closing ? a.ldw : (to_w ? a.ldw : a.ldw2);
    const float* const cur = closing ? a.w : (to_w ? a.w2 : a.w);
    const long ldc_ = closing ? a.ldw : (to_w ? a.ldw2 : a.ldw);
    const float* const prv = closing ? a.w2 : nxt;
    const long ldp = closing ? a.ldw2 : ldn;
    const bool have_cur = k >= 1, have_prv = k >= 2;              // before that the weights are zero and nothing is read
    const float beta = (float)k / (float)(k + 3);
    const bool last_it = k + 1 == T;
    const float betan = (float)(k + 1) / (float)(k + 4);

    mover.fetch(a.c, a.ldc, 0, min(V - 1, GT - 1));
    for (int t = 0; t < ntiles; ++t, buf ^= 1) {
      char* tile = lds + buf * tilebytes;
      mover.store(tile);
      __syncthreads();                            // tile t is whole; every wave has left the tile before last and the partials of the last
      if (t + 1 < ntiles) mover.fetch(a.c + (long)(t + 1) * GT * a.ldc, a.ldc, 0, min(V - 1 - (t + 1) * GT, GT - 1));

      // this lane's weights: row 16 mt + li, concepts 32 t + 16 st + 4 g .. + 3.  Read BEFORE the second barrier: behind it
      // another wave writes w_{k+1} over w_{k-1}.
      const int v0 = GT * t + 4 * g;
      f32x4 wc[MT][2], wp[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          wc[mt][st] = have_cur ? concept_load4(cur + xr[mt] * ldc_, v0 + 16 * st, V) : (f32x4){0.f, 0.f, 0.f, 0.f};
          wp[mt][st] = have_prv ? concept_load4(prv + xr[mt] * ldp, v0 + 16 * st, V) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }

      // g^T partial over this wave's columns: concept on the accumulator row, row of x on the lane
      f32x4 gp[MT][2];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) gp[mt][0] = gp[mt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < KSW; ++i) {
        if (i >= nown) continue;
        const int ch = 4 * (ks0 + i) + (g >> 1), sub = 8 * (g & 1);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const bf16x4 c0 = *(const bf16x4*)(tile + geo.off(16 * st + li, ch) + sub);
          const bf16x4 c1 = *(const bf16x4*)(tile + geo.off(16 * st + li, ch + 2) + sub);
          const bf16x8 cf = __builtin_shufflevector(c0, c1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            gp[mt][st] = CCLIP_MFMA_16x16x32(cf, rhi[mt][i], gp[mt][st]);
            gp[mt][st] = CCLIP_MFMA_16x16x32(cf, rlo[mt][i], gp[mt][st]);
          }
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int st = 0; st < 2; ++st) part[((wave * MT + mt) * 2 + st) * 64 + lane] = gp[mt][st];
      __syncthreads();                            // the four partials are whole; every wave holds its w_k and w_{k-1} of the tile

      bf16x8 nyhi[MT], nylo[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const f32x4 p0 = part[((0 * MT + mt) * 2 + st) * 64 + lane], p1 = part[((1 * MT + mt) * 2 + st) * 64 + lane];
          const f32x4 p2 = part[((2 * MT + mt) * 2 + st) * 64 + lane], p3 = part[((3 * MT + mt) * 2 + st) * 64 + lane];
          f32x4 wn;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gg = ((p0[r] + p1[r]) + p2[r]) + p3[r];
            const bool okv = v0 + 16 * st + r < V;
            const float wk = wc[mt][st][r], wo = wp[mt][st][r];
            if (closing) {
              if (okv) {                          // (no cross-lane operation inside)
                const float over = gg - a.l1;
                const float viol = wk > 0.0f ? fabsf(over) : (over <= 0.0f ? 0.0f : over);         // a NaN stays
                so_l1[mt] += wk;
                so_nnz[mt] += wk > 0.0f ? 1 : 0;
                so_delta[mt] = concept_nanmax(so_delta[mt], fabsf(wk - wo));
                so_kkt[mt] = concept_nanmax(so_kkt[mt], viol);
              }
              wn[r] = wk;
            } else {
              const float y = wk + beta * (wk - wo);
              const float tt = y + a.eta * (gg - a.l1);
              const float w1 = tt <= 0.0f ? 0.0f : tt;            // a NaN stays, -0 becomes +0
              wn[r] = w1;
              const float yn = last_it ? w1 : w1 + betan * (w1 - wk);
              const float ny = okv ? -yn : 0.0f;                  // selected: a padding concept adds nothing
              split16(ny, nyhi[mt], nylo[mt], 4 * st + r);
            }
          }
          // T == 0 leaves w = 0 to the closing sweep; otherwise the closing sweep writes nothing
          if (live[mt] && wave == (mt & 3) && (!closing || T == 0)) concept_store4(nxt + xr[mt] * ldn, v0 + 16 * st, V, wn);
        }
      }
      if (closing) continue;                      // (uniform)

      // acc[d, row] += c^T[d, v] (-y)[v, row] over the 32 concepts of the tile: k index = (st, g, r) on both operands
#pragma unroll
      for (int i = 0; i < KSW; ++i) {
        if (i >= nown) continue;                  // (wave-uniform)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bf16x8 ct = tile_frag_tr(tile, geo, 4 * g, 16 + 4 * g, 2 * (ks0 + i) + h, lane);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[mt][2 * i + h] = CCLIP_MFMA_16x16x32(ct, nyhi[mt], acc[mt][2 * i + h]);
            acc[mt][2 * i + h] = CCLIP_MFMA_16x16x32(ct, nylo[mt], acc[mt][2 * i + h]);
          }
        }
      }
    }
  }

  // |r(w_T)|^2: this wave's columns in ascending order, the four lane groups by a fixed butterfly, the waves in ascending order
  float* red = (float*)part;                      // [wave][mt][16]
  __syncthreads();                                // every wave has read the last tile's partials
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < KSW; ++i) {
      if (i >= nown) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc[mt][2 * i + h][r] * acc[mt][2 * i + h][r];
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (g == 0) red[(wave * MT + mt) * 16 + li] = s;
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float sl = so_l1[mt], sd = so_delta[mt], sk = so_kkt[mt];
    int sn = so_nnz[mt];
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {           // the four lane groups hold disjoint concepts: both partners compute the same bits
      sl += __shfl_xor(sl, o, 64);
      sn += __shfl_xor(sn, o, 64);
      sd = concept_nanmax(sd, __shfl_xor(sd, o, 64));
      sk = concept_nanmax(sk, __shfl_xor(sk, o, 64));
    }
    if (wave == (mt & 3) && g == 0 && live[mt]) {
      const long row = xr[mt];
      a.resid2[row] = ((red[(0 * MT + mt) * 16 + li] + red[(1 * MT + mt) * 16 + li]) + red[(2 * MT + mt) * 16 + li]) +
                      red[(3 * MT + mt) * 16 + li];
      a.l1norm[row] = sl;
      a.nnz[row] = sn;
      a.delta[row] = sd;
      a.kkt[row] = sk;
    }
  }
}

struct ConceptGeom {
  int mt;                                         // row tiles of 16 per work-group
  int64_t blocks, ldw2, total;
};

// of (N, V, D) alone
static inline bool concept_geom(int64_t N, int64_t V, int32_t D, ConceptGeom& g) {
  if (!score_rows_ok(N) || V < 1 || V > CONCEPT_MAX_V || !score_dim_ok(D)) return false;
  g.mt = D <= 512 ? 2 : 1;
  g.blocks = (N + 16 * g.mt - 1) / (16 * g.mt);
  g.ldw2 = (V + 3) / 4 * 4;
  g.total = N * g.ldw2 * 4;
  return true;
}

template <int KSMAX, int KSW, int MT>
static int concept_launch(const ConceptArgs& a, const ConceptGeom& g, hipStream_t stream) {
  const size_t lds = (size_t)2 * CONCEPT_GT * a.D * 2 + (size_t)4 * MT * 2 * 64 * 16;
  return score_launch(concept_codes_kernel<KSMAX, KSW, MT>, (unsigned)g.blocks, lds, a, stream);
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_concept_codes_workspace(int64_t N, int64_t V, int32_t D) {
  ConceptGeom g;
  return concept_geom(N, V, D, g) ? g.total : 0;
}
#endif

extern "C" int CCLIP_FN(cclip_concept_codes)(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t V, int32_t D,
                                              float l1, float eta, int32_t iters, float* w, int64_t ldw, float* resid2,
                                              float* l1norm, int32_t* nnz, float* delta, float* kkt, void* workspace,
                                              int64_t workspace_bytes, hipStream_t stream) {
  ConceptGeom g;
  if (!x || !c || !w || !resid2 || !l1norm || !nnz || !delta || !kkt || !workspace) return CCLIP_ERR_ARG;
  if (!concept_geom(N, V, D, g) || !score_operands_ok(x, ldx, c, ldc, D)) return CCLIP_ERR_ARG;
  if (ldw < V || (ldw & 3) || (((uintptr_t)w | (uintptr_t)workspace) & 15)) return CCLIP_ERR_ARG;
  if (((uintptr_t)resid2 | (uintptr_t)l1norm | (uintptr_t)nnz | (uintptr_t)delta | (uintptr_t)kkt) & 3) return CCLIP_ERR_ARG;
  if (!score_finite(l1) || !score_finite(eta) || l1 < 0.0f || eta < 0.0f || iters < 0) return CCLIP_ERR_ARG;
  if (workspace_bytes < g.total) return CCLIP_ERR_ARG;
  ConceptArgs a;
  a.x = (const bf16*)x; a.c = (const bf16*)c; a.ldx = ldx; a.ldc = ldc;
  a.N = (int)N; a.V = (int)V; a.D = D; a.iters = iters; a.l1 = l1; a.eta = eta;
  a.w = w; a.ldw = ldw; a.w2 = (float*)workspace; a.ldw2 = g.ldw2;
  a.resid2 = resid2; a.l1norm = l1norm; a.nnz = nnz; a.delta = delta; a.kkt = kkt;
  int st;
  if (D <= 128) st = concept_launch<4, 1, 2>(a, g, stream);
  else if (D <= 512) st = concept_launch<16, 4, 2>(a, g, stream);
  else st = concept_launch<32, 8, 1>(a, g, stream);
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}
