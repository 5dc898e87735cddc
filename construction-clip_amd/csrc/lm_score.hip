// lm_head scoring for gfx950: for hidden rows X [R, D] and the tied vocabulary matrix W [V, D] (16-bit rows), per row r of
//     z[r, j] = sum_d X[r, d] W[j, d]             (fp32 accumulation on v_mfma_f32_16x16x32)
// the log-sum-exp over j, the log-probability of labels[r], the argmax column and its logit.  The R x V logits are never
// written: what reaches memory is one 24-byte partial per (row, vocabulary split), then four numbers per row.
//
// Logit independent of position.  Every logit is ONE accumulator chain over d = 0, 32, 64 .. in that order (the tile multiply
// of score_tiles.h), whichever tile, split, lane or kernel variant its column and row land on.
// Reduction independent of R.  The vocabulary is cut into splits of LM_SPLIT_COLS columns: a function of V alone.  Inside a
// split, lane li of a 16-lane group meets the columns n0 + li, n0 + li + 16, .. in ascending order and keeps, per row, an online
// (max, sum of exp relative to it), the best column and the target logit; the 16 lanes are then combined by a fixed xor
// butterfly and phase 2 combines the splits in ascending order.  None of this depends on how many rows are scored, on which
// accumulator row a hidden row sits, or on the variant (rows per wave, tile height) the launcher picks from R: a row's four
// outputs are bit-identical scored alone or inside any batch.  No atomics: two launches are bitwise equal.
//
// Order of the argmax: score_key (score_key.h: the logit's bits made monotone, NaN -> 0, -0 -> +0) as the high word with
// ~column as the low word.  The largest key wins: equal fp32 logits go to the LOWER column, NaN ranks below every number.
//
// Phase 1 (lm_partial_kernel): grid = row blocks x splits.  A work-group (4 waves) owns 64 * MT rows, wave w the rows
// 16 MT w ..; their A fragments stay in registers.  W streams through two LDS buffers in tiles of GT vocabulary rows (the
// swizzled [row][D] image, the tile mover and the multiply of score_tiles.h); tile t + 1 is fetched into
// registers while tile t is multiplied and lands in the other buffer, so a tile costs one barrier.  Rows beyond R and
// columns beyond V are loaded clamped (never out of bounds) and masked: they contribute nothing.
// Phase 2 (lm_merge_kernel): one thread per row folds its partials in split order.
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

// the reductions below are written out operation by operation: no fused multiply-add may be formed from them, so that every
// instantiation of the kernel rounds alike
#pragma clang fp contract(off)

#define LM_SPLIT_COLS 1024                        // vocabulary columns per split (a multiple of every GT)

namespace CCLIP_NS {

struct LmPartial {                                // what one split knows about one row
  u64 key;                                        // best (monotone logit bits, ~column); 0 = none
  float m, s;                                     // running max; sum_j exp(z_j - m)   (m = -inf, s = 0: no column)
  float tz;                                       // z[label] when the label's column lies in this split
  float pad;
};

struct LmArgs {
  const bf16* x; const bf16* w;
  long ldx, ldw;
  int R, V, D;
  int splits;
  const int* labels;
  LmPartial* ws;
};

// weight of a partial whose max is m inside a combination whose max is M (an empty partial, m = -inf, weighs nothing)
__device__ __forceinline__ float lm_weight(float m, float M) { return m == -__builtin_huge_valf() ? 0.0f : __expf(m - M); }

// <KSMAX, MT, GT> as in score_tiles.h: MT row tiles of 16 per wave, GT vocabulary rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void lm_partial_kernel(const LmArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 vocabulary rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int R = a.R, V = a.V;
  const TileGeom geo(a.D);
  const int tilebytes = GT * geo.rowbytes;

  const int split = blockIdx.x % a.splits, rb = blockIdx.x / a.splits;
  const int n0 = split * LM_SPLIT_COLS;
  const int n1 = min(V, n0 + LM_SPLIT_COLS);      // (n0 < V: the launcher leaves no split empty)
  const int q0 = (rb * 4 + wave) * (16 * MT);
  const bool active = q0 < R;                     // (wave-uniform) a wave without rows only helps to load

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, a.x, a.ldx, q0, R - 1, geo.nks, lane);
  // per-row state of this lane: rows q0 + 16 mt + 4 g + r against the columns n0 + li + 16 i
  float rm[MT][4], rs[MT][4], rt[MT][4];
  unsigned bhi[MT][4];
  int bi[MT][4], lab[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = q0 + 16 * mt + 4 * g + r;
      rm[mt][r] = -__builtin_huge_valf(); rs[mt][r] = 0.0f; rt[mt][r] = 0.0f;
      bhi[mt][r] = 0u; bi[mt][r] = n0 + li;
      lab[mt][r] = row < R ? a.labels[row] : -1;  // a label outside the split's columns simply never matches
    }

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.w, a.ldw, n0, V - 1);             // rows >= V are clamped (masked below)
  int buf = 0;
  for (int base = n0; base < n1; base += GT, buf ^= 1) {
    char* Ws = lds + buf * tilebytes;
    mover.store(Ws);
    __syncthreads();                              // tile `base` is whole; every wave has left the tile before last (this buffer's next content)
    if (base + GT < n1) mover.fetch(a.w, a.ldw, base + GT, V - 1);
    if (!active) continue;

    f32x4 acc[MT][NST];
    tile_multiply<KSMAX, MT, GT>(acc, af, Ws, geo, lane);

#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int nb = base + 16 * st;
      if (nb >= n1) continue;                     // (wave-uniform)
      const int col = nb + li;
      if (col >= n1) continue;                    // a masked column contributes nothing
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = acc[mt][st][r];
          const float m = rm[mt][r];
          const float e = __expf(-fabsf(z - m));  // exp(min - max); the first column meets m = -inf: e = 0, s = 1
          rs[mt][r] = z > m ? rs[mt][r] * e + 1.0f : rs[mt][r] + e;   // NaN z: s = NaN, m unchanged
          rm[mt][r] = fmaxf(m, z);
          const unsigned hi = score_key(z);
          if (hi > bhi[mt][r]) { bhi[mt][r] = hi; bi[mt][r] = col; }  // ascending columns: ties keep the lower one
          if (col == lab[mt][r]) rt[mt][r] = z;
        }
    }
  }

  if (!active) return;
  // the 16 lanes of a group -> one partial per row (xor butterfly: both partners compute the same bits)
  const bool has = n0 + li < n1;                  // this lane met at least one column
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = rm[mt][r], s = rs[mt][r], t = rt[mt][r];
      unsigned khi = has ? bhi[mt][r] : 0u, klo = has ? ~(unsigned)bi[mt][r] : 0u;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64), t2 = __shfl_xor(t, o, 64);
        const unsigned khi2 = __shfl_xor(khi, o, 64), klo2 = __shfl_xor(klo, o, 64);
        const float M = fmaxf(m, m2);
        s = s * lm_weight(m, M) + s2 * lm_weight(m2, M);
        m = M;
        t += t2;                                  // at most one lane holds the target logit, the others hold +0
        const bool take = khi2 > khi || (khi2 == khi && klo2 > klo);
        khi = take ? khi2 : khi; klo = take ? klo2 : klo;
      }
      const int row = q0 + 16 * mt + 4 * g + r;
      if (li == 0 && row < R) {
        LmPartial p;
        p.key = ((u64)khi << 32) | klo; p.m = m; p.s = s; p.tz = t; p.pad = 0.0f;
        a.ws[(long)row * a.splits + split] = p;
      }
    }
}

// One thread per row: its partials in ascending split order.
__global__ __launch_bounds__(256) void lm_merge_kernel(const LmPartial* __restrict__ ws, int R, int V, int splits,
                                                       const int* __restrict__ labels, int ignore_index, float* __restrict__ logp,
                                                       float* __restrict__ lse, int* __restrict__ pred, float* __restrict__ pred_logit) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= R) return;
  const LmPartial* p = ws + row * splits;
  float M = -__builtin_huge_valf(), S = 0.0f;
  u64 key = 0ull;
  for (int i = 0; i < splits; ++i) {
    const float m = p[i].m, s = p[i].s;
    const float Mn = fmaxf(M, m);
    const float wa = M == -__builtin_huge_valf() ? 0.0f : expf(M - Mn), wb = m == -__builtin_huge_valf() ? 0.0f : expf(m - Mn);
    S = S * wa + s * wb;
    M = Mn;
    key = p[i].key > key ? p[i].key : key;
  }
  const float l = M + logf(S);
  const int lab = labels[row];
  float lp;
  if (lab == ignore_index) lp = 0.0f;
  else if (lab < 0 || lab >= V) lp = __uint_as_float(0x7fc00000u);
  else lp = p[lab / LM_SPLIT_COLS].tz - l;
  logp[row] = lp;
  if (lse) lse[row] = l;
  if (pred) pred[row] = (int)~(unsigned)key;
  if (pred_logit) pred_logit[row] = key_score((unsigned)(key >> 32));
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_lm_head_score_workspace(int32_t R, int32_t V) {
  if (R <= 0 || V <= 0) return 0;
  return (int64_t)R * ((V + LM_SPLIT_COLS - 1) / LM_SPLIT_COLS) * (int64_t)sizeof(LmPartial);
}
#endif

extern "C" int CCLIP_FN(cclip_lm_head_score)(const void* x, int64_t ldx, int32_t R, int32_t D, const void* w, int64_t ldw, int32_t V,
                                              const int32_t* labels, int32_t ignore_index, float* logp, float* lse, int32_t* pred,
                                              float* pred_logit, void* workspace, hipStream_t stream) {
  if (!x || !w || !labels || !logp || !workspace) return CCLIP_ERR_ARG;
  if (R <= 0 || V <= 0) return CCLIP_ERR_ARG;
  if (!score_operands_ok(x, ldx, w, ldw, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)logp & 3) || ((uintptr_t)lse & 3) || ((uintptr_t)pred & 3) ||
      ((uintptr_t)pred_logit & 3) || ((uintptr_t)labels & 3))
    return CCLIP_ERR_ARG;
  LmArgs a;
  a.x = (const bf16*)x; a.w = (const bf16*)w; a.ldx = ldx; a.ldw = ldw;
  a.R = R; a.V = V; a.D = D;
  a.splits = (V + LM_SPLIT_COLS - 1) / LM_SPLIT_COLS;
  a.labels = labels;
  a.ws = (LmPartial*)workspace;
  const int st = score_dispatch<true>(D, R > 64, [&](auto s) {
    using S = decltype(s);
    static_assert(LM_SPLIT_COLS % S::GT == 0, "a split is a whole number of tiles");
    return sweep_launch(lm_partial_kernel<S::KSMAX, S::MT, S::GT>, a, R, S::MT, S::GT, D, a.splits, 2, 0, stream);
  });
  if (st != CCLIP_OK) return st;
  hipLaunchKernelGGL(lm_merge_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, (const LmPartial*)a.ws, R, V, a.splits,
                     labels, ignore_index, logp, lse, pred, pred_logit);
  return cclip_launch_status();
}
