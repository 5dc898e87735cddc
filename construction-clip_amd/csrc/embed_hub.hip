// Hubness of stored embeddings for gfx950: how strongly a bank of typical queries points at every gallery row.  For the
// gallery g [N, D] and the bank [B, D] (16-bit rows) and a float beta
//     lse[j] = log sum_{b < B} exp(t[b, j]),   t[b, j] = beta * s[b, j] (one fp32 multiply),   s[b, j] = sum_d bank[b, d] g[j, d]
// with s in fp32 on v_mfma_f32_16x16x32.  -lse is the per-row bias of the inverted softmax (clip/hubness.py); the B x N matrix
// is never written.
//
// Score.  Every s is ONE accumulator chain over d = 0, 32, 64 .. in that order, whichever tile, split or lane the pair lands on:
// the bits cclip_similarity_topk returns for the pair.
//
// Partial (bank_lse_partial_kernel): the sweep of score_sweep.h (two tile buffers) over blocks of 64 * MT gallery rows as A
// fragments in registers, the bank streamed through LDS, cut into splits by gallery_splits.  Lane (li, g) meets the bank rows
// 16 st + li of every tile and keeps per gallery row it owns a running pair (m, s): m the largest t met, s the sum of
// exp(t - m).  A tile's sub-tiles enter together: the new maximum first, then one rescale of s and one exp per score, added in
// ascending sub-tile order.  The 16 lanes of a group are combined by the fixed xor butterfly 1, 2, 4, 8 with the merge
//     M = max(m1, m2),   S = s1 exp(m1 - M) + s2 exp(m2 - M)      (exp(m - M) is exactly 1 where m == M, -inf included)
// written without a fused multiply-add, so that both partners compute the same bits.  Lane 0 writes (M, S) to the workspace
// [N][splits].  Merge (bank_lse_merge_kernel): one thread per gallery row folds its pairs in ascending split order with the
// same merge and writes M + log S.  No atomics: two launches are bitwise equal.
//
// Not finite.  A NaN score never becomes a maximum (fmaxf drops it) and turns the sum, hence lse, into NaN: a NaN in gallery
// row j makes lse[j] NaN and touches no other entry.  A non-finite bank row meets every gallery row and reaches every entry.
// t = +inf gives +inf, a row whose every t is -inf gives -inf.  Large beta is safe: nothing above exp(0) is ever formed.
// Gallery rows beyond N and bank rows beyond B are loaded clamped (never out of bounds), never summed and never stored.
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

// the merge is written out operation by operation: a fused multiply-add would round the two partners' sums differently
#pragma clang fp contract(off)

namespace CCLIP_NS {

struct BankLseArgs {
  const bf16* g; const bf16* bank;
  long ldg, ldb;
  int N, B, D;
  int splits, rows_per_split;                     // of the bank; rows_per_split is a multiple of 64
  float beta;
  f32x2* ws;                                      // [N][splits] pairs (m, s)
};

// exp(m - M) for m <= M, exactly 1 where the two are equal (so that -inf against -inf is 1, not NaN); NaN for a NaN m
__device__ __forceinline__ float lse_weight(float m, float M) { return m == M ? 1.0f : __expf(m - M); }

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = s * lse_weight(m, M) + s2 * lse_weight(m2, M);
  m = M;
}

// <KSMAX, MT, GT> as in score_tiles.h: MT tiles of 16 gallery rows per wave, GT bank rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void bank_lse_partial_kernel(const BankLseArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 bank rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const SweepCtx<MT> ctx(a.D, a.N, a.B, a.splits, a.rows_per_split);
  const int li = ctx.li;
  const float beta = a.beta;

  bf16x8 af[MT][KSMAX];
  ctx.load_a(af, a.g, a.ldg);
  // per-row state of this lane: the largest t met and the sum of exp(t - m); (-inf, 0) = nothing met yet
  float m[MT][4], s[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[mt][r] = -__builtin_huge_valf(); s[mt][r] = 0.f; }

  // rows >= B are clamped (never summed below)
  stream_tiles<KSMAX, MT, GT>(ctx, af, a.bank, a.ldb, ctx.n0, ctx.n1, (long)a.B - 1, lds,
                              [&](long base, f32x4 (&acc)[MT][NST]) CCLIP_SWEEP_INLINE {
    bool live[NST];                               // this lane's bank row of sub-tile st lies inside the split
#pragma unroll
    for (int st = 0; st < NST; ++st) live[st] = base + 16 * st + li < ctx.n1;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t[NST];
        float M = m[mt][r];
#pragma unroll
        for (int st = 0; st < NST; ++st) {
          t[st] = beta * acc[mt][st][r];
          M = live[st] ? fmaxf(M, t[st]) : M;     // selected, not multiplied
        }
        float sum = s[mt][r] * lse_weight(m[mt][r], M);
#pragma unroll
        for (int st = 0; st < NST; ++st) sum += live[st] ? lse_weight(t[st], M) : 0.f;
        m[mt][r] = M; s[mt][r] = sum;
      }
  });
  if (!ctx.active) return;

  // the 16 lanes of a group hold disjoint bank rows: the butterfly of score_key.h's group_sum with the pair merge; lane 0 writes
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float M = m[mt][r], S = s[mt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float pm = __shfl_xor(M, o, 64), ps = __shfl_xor(S, o, 64);
        lse_merge(M, S, pm, ps);
      }
      if (li == 0 && ctx.row_live(mt, r)) a.ws[ctx.row(mt, r) * a.splits + ctx.split] = (f32x2){M, S};
    }
}

// one thread per gallery row: its pairs in ascending split order
__global__ __launch_bounds__(256) void bank_lse_merge_kernel(const f32x2* __restrict__ ws, long N, int splits, float* __restrict__ lse) {
  const long row = blockIdx.x * 256L + threadIdx.x;
  if (row >= N) return;
  const f32x2* p = ws + row * splits;
  float M = p[0][0], S = p[0][1];
  for (int sp = 1; sp < splits; ++sp) lse_merge(M, S, p[sp][0], p[sp][1]);
  lse[row] = M + logf(S);
}

// bank splits from (N, B) alone, so that the size queries need no D: about 512 work-groups while a split keeps at least 256
// bank rows, with the gallery counted in blocks of 64 rows.  The MT = 2 variants (N > 64, D <= 768) run blocks of 128 rows,
// half as many, so the grid is then about one work-group per CU, not two; the result does not depend on the count.
static inline void bank_lse_splits(int64_t N, int64_t B, int* splits, int* rows_per_split) {
  gallery_splits(B, (N + 63) / 64, 512, 256, splits, rows_per_split);
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int32_t cclip_bank_lse_splits(int64_t N, int64_t B) {
  if (!score_rows_ok(N) || !score_rows_ok(B)) return 0;
  int splits, rows;
  bank_lse_splits(N, B, &splits, &rows);
  return splits;
}

extern "C" int64_t cclip_bank_lse_workspace(int64_t N, int64_t B) { return (int64_t)N * cclip_bank_lse_splits(N, B) * 8; }
#endif

extern "C" int CCLIP_FN(cclip_bank_lse)(const void* g, int64_t ldg, int64_t N, const void* bank, int64_t ldb, int64_t B, int32_t D,
                                         float beta, float* lse, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!g || !bank || !lse || !workspace) return CCLIP_ERR_ARG;
  if (!score_rows_ok(N) || !score_rows_ok(B)) return CCLIP_ERR_ARG;
  if (!score_operands_ok(g, ldg, bank, ldb, D)) return CCLIP_ERR_ARG;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)lse & 3)) return CCLIP_ERR_ARG;
  BankLseArgs a;
  a.g = (const bf16*)g; a.bank = (const bf16*)bank; a.ldg = ldg; a.ldb = ldb;
  a.N = (int)N; a.B = (int)B; a.D = D; a.beta = beta;
  bank_lse_splits(N, B, &a.splits, &a.rows_per_split);
  a.ws = (f32x2*)workspace;
  if (workspace_bytes < (int64_t)N * a.splits * 8) return CCLIP_ERR_ARG;
  const int st = score_dispatch<true>(D, N > 64, [&](auto s) {
    using S = decltype(s);
    return sweep_launch(bank_lse_partial_kernel<S::KSMAX, S::MT, S::GT>, a, N, S::MT, S::GT, D, a.splits, 2, 0, stream);
  });
  if (st != CCLIP_OK) return st;
  hipLaunchKernelGGL(bank_lse_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const f32x2*)a.ws, (long)N,
                     a.splits, lse);
  return cclip_launch_status();
}
