// k-centre greedy selection (farthest-point sampling, the coreset of Sener & Savarese 2018) over stored embeddings for gfx950:
// one launch per pick.  State on the device, for unit 16-bit rows x [N, D]:
//     mind  fp32 [N]   the row's cosine distance 1 - <x_i, x_c> to its nearest centre so far, +inf = none yet
//     owner int32 [N]  that centre's row, -1 = none; owner[i] == i marks a row that is itself a centre
//     partial[2][P]    64-bit keys, P = cclip_coreset_blocks(N): the best eligible row of every work-group
// A key is score_key(weight * mind) in the high word and ~row in the low one (the order of score_key.h / embed_topk.hip: larger
// = better, equal values to the LOWER row, NaN below every number); key 0 = no eligible row.
//
// coreset_step_kernel, grid = P work-groups of 256 threads, three modes (block-uniform, held in scalar registers):
//   from partials  every work-group takes the maximum of the P keys of partial_in.  The keys are distinct, so the maximum does not
//                  depend on the order they are met in: the work-groups agree without talking - no atomics, no tickets, no
//                  spin-wait, no cross-work-group barrier.  The winner's low word gives the centre c, clamped into [0, N - 1]
//                  before use.  Key 0: pick -1, radius NaN, nothing updated (the scan below still runs and writes partial_out).
//   given centre   c comes from the caller (the first pick without seeds).
//   scan only      no centre, no update: only the keys (after seeding).
// Then ONE pass over the work-group's rows, dealt by a grid stride: trip t of work-group b holds the rows (t P + b) RPT ..
// + RPT - 1, RPT = 256 / T rows a trip.  A row belongs to a team of T lanes, T = the power of two >= D / 8 capped at 64 (a
// function of D alone); lane l of the team holds the 8 elements 8 l .. 8 l + 7 (one 16-byte load) and, for D > 512, the 8
// elements 512 + 8 l .. of a second pass; lanes past the row's end hold zeros.  The centre row sits in registers the same way.
//   update   s = the fp32 dot in ONE fixed order: per lane the 8 products (exact in fp32) added in ascending element order from the
//            first, the second pass likewise and added to the first, then the team's xor butterfly over lane distances 1, 2, ..
//            T / 2 (both partners add the same two numbers, so every lane holds the same bits).  No fused multiply-add.
//            d = 1 - s;  a row that is not a centre with d < mind[i] takes mind[i] = d, owner[i] = c - strictly smaller, an equal
//            distance keeps the earlier centre; a NaN d changes nothing; a row that is a centre (owner[i] == i) keeps its 0.
//            Row c itself: its team first writes pick_out[0] = c and radius_out[0] = mind[c], the value BEFORE the update (the
//            covering radius of everything chosen before this pick), then mind[c] = 0, owner[c] = c.
//   scan     a row is eligible if owner[i] != i and its weight, where given, is > 0 (a NaN weight is not); its value is
//            weight[i] * mind[i] (mind[i] itself without weights; +inf allowed).  The work-group's best key - a running maximum
//            per lane, the wave's xor butterfly, the four waves through LDS - goes to partial_out[blockIdx].
// A row's new mind and owner are a function of (x_i, x_c, old mind, old owner) alone: not of N, of where the row sits or of the
// grid.  mind[i] / owner[i] are read and written by the row's own team only, x is never written, and partial_in != partial_out (a
// late work-group still reads the old keys while an early one writes the new ones): two launches are bitwise equal.
// Rows past N are loaded clamped to row N - 1 (never out of bounds), never written and never selected; c is the only index taken
// from memory and it is clamped.
//
// cclip_coreset_greedy enqueues the m launches of a whole selection from one C loop (the pattern of decode_driver.hip),
// alternating the two partial buffers: the host cost of a pick is a launch, not a ctypes round trip, and nothing is read back.
#include "score_tiles.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them
#pragma clang fp contract(off)

#define CS_MAX_BLOCKS 1024
#define CS_ROWS_PER_BLOCK 64                      // the rows of a trip at the smallest team (D = 32): sizes the grid
#define CS_UNROLL 4                               // trips in flight per work-group

namespace CCLIP_NS {

struct CoresetArgs {
  const bf16* x; long ldx;
  int N, D;
  const float* weight;                            // may be null
  float* mind; int* owner;
  const u64* pin; u64* pout; int P;
  int centre;                                     // >= 0 given, CCLIP_CORESET_FROM_PARTIALS, CCLIP_CORESET_SCAN_ONLY
  int* pick; float* radius;
};

__device__ __forceinline__ u64 cs_max(u64 a, u64 b) { return a > b ? a : b; }

// the maximum of one key per thread over the work-group, in every thread (red: 4 entries of LDS, free again on return)
__device__ __forceinline__ u64 cs_block_max(u64 v, u64* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = cs_max(v, shfl_xor64(v, o));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = cs_max(cs_max(red[0], red[1]), cs_max(red[2], red[3]));
  __syncthreads();
  return v;
}

// the 8 products of a lane added in ascending element order from the first
__device__ __forceinline__ float cs_dot8(const bf16x8 v, const float* c) {
  float acc = (float)v[0] * c[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) acc += (float)v[j] * c[j];
  return acc;
}

template <int T, bool TWO>
__global__ __launch_bounds__(256) void coreset_step_kernel(const CoresetArgs a) {
  __shared__ u64 red[4];
  constexpr int RPT = 256 / T;
  const int tid = threadIdx.x;
  const int team = tid / T, lt = tid & (T - 1);
  const int N = a.N, D = a.D;

  int c = a.centre;
  bool update = c >= 0;
  if (a.centre == CCLIP_CORESET_FROM_PARTIALS) {
    u64 top = 0ull;
    for (int p = tid; p < a.P; p += 256) top = cs_max(top, a.pin[p]);
    top = cs_block_max(top, red, tid);
    update = top != 0ull;
    const unsigned cu = ~(unsigned)top;
    c = cu > (unsigned)(N - 1) ? N - 1 : (int)cu;                 // the one index taken from memory: clamped before use
    if (!update && blockIdx.x == 0 && tid == 0) {
      a.pick[0] = -1;
      a.radius[0] = __uint_as_float(0x7fc00000u);
    }
  }
  c = __builtin_amdgcn_readfirstlane(c);                          // (every lane holds the same value: keep the mode scalar)
  update = __builtin_amdgcn_readfirstlane((int)update) != 0;

  const bool on = lt * 8 < D;                                     // lanes past the row's end idle (D / 8 is no power of two)
  const bool on2 = TWO && 512 + lt * 8 < D;
  float c0[8], c1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { c0[j] = 0.0f; c1[j] = 0.0f; }
  if (update) {
    const bf16* cr = a.x + (long)c * a.ldx + lt * 8;
    if (on) {
      const bf16x8 v = *(const bf16x8*)cr;
#pragma unroll
      for (int j = 0; j < 8; ++j) c0[j] = (float)v[j];
    }
    if (on2) {
      const bf16x8 v = *(const bf16x8*)(cr + 512);
#pragma unroll
      for (int j = 0; j < 8; ++j) c1[j] = (float)v[j];
    }
  }

  u64 best = 0ull;
  const long stride = (long)gridDim.x * RPT;
  for (long b0 = (long)blockIdx.x * RPT; b0 < N; b0 += CS_UNROLL * stride) {          // (block-uniform)
    bf16x8 v0[CS_UNROLL], v1[CS_UNROLL];
    float md[CS_UNROLL], wt[CS_UNROLL];
    int ow[CS_UNROLL], rw[CS_UNROLL];
    bool ok[CS_UNROLL];
#pragma unroll
    for (int u = 0; u < CS_UNROLL; ++u) {
      const long r = b0 + u * stride + team;
      ok[u] = r < N;
      rw[u] = ok[u] ? (int)r : N - 1;             // (a clamped row is loaded, never written, never selected)
#pragma unroll
      for (int j = 0; j < 8; ++j) { v0[u][j] = (bf16)0.0f; v1[u][j] = (bf16)0.0f; }
      if (update) {
        const bf16* src = a.x + (long)rw[u] * a.ldx + lt * 8;
        if (on) v0[u] = *(const bf16x8*)src;
        if (on2) v1[u] = *(const bf16x8*)(src + 512);
      }
      md[u] = a.mind[rw[u]];
      ow[u] = a.owner[rw[u]];
      wt[u] = a.weight ? a.weight[rw[u]] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < CS_UNROLL; ++u) {
      const int r = rw[u];
      float m = md[u];
      int o = ow[u];
      if (update) {
        float s = cs_dot8(v0[u], c0);
        if (TWO) s = s + cs_dot8(v1[u], c1);
#pragma unroll
        for (int d = 1; d < T; d <<= 1) s += __shfl_xor(s, d, 64);
        const float dist = 1.0f - s;
        bool changed = false;
        if (r == c) {
          if (ok[u] && lt == 0) { a.pick[0] = c; a.radius[0] = m; }       // mind[c] BEFORE the update
          m = 0.0f; o = c; changed = true;
        } else if (o != r && dist < m) {
          m = dist; o = c; changed = true;
        }
        if (changed && ok[u] && lt == 0) { a.mind[r] = m; a.owner[r] = o; }
      }
      const bool eligible = ok[u] && o != r && wt[u] > 0.0f;      // (a NaN weight fails the comparison)
      const float val = a.weight ? wt[u] * m : m;
      const u64 key = ((u64)score_key(val) << 32) | (unsigned)~(unsigned)r;
      best = cs_max(best, eligible ? key : 0ull);                 // selected, not multiplied
    }
  }
  best = cs_block_max(best, red, tid);
  if (tid == 0) a.pout[blockIdx.x] = best;
}

static inline int64_t coreset_blocks(int64_t N) {
  const int64_t b = (N + CS_ROWS_PER_BLOCK - 1) / CS_ROWS_PER_BLOCK;
  return b > CS_MAX_BLOCKS ? CS_MAX_BLOCKS : b;
}

template <int T, bool TWO>
static void coreset_launch(const CoresetArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((coreset_step_kernel<T, TWO>), dim3((unsigned)a.P), dim3(256), 0, stream, a);
}

static void coreset_dispatch(const CoresetArgs& a, hipStream_t stream) {
  const int chunks = a.D >> 3;                    // 16-byte chunks a row: 4 .. 128
  if (chunks <= 4) coreset_launch<4, false>(a, stream);
  else if (chunks <= 8) coreset_launch<8, false>(a, stream);
  else if (chunks <= 16) coreset_launch<16, false>(a, stream);
  else if (chunks <= 32) coreset_launch<32, false>(a, stream);
  else if (chunks <= 64) coreset_launch<64, false>(a, stream);
  else coreset_launch<64, true>(a, stream);
}

// the checks the two entries share; fills everything of `a` but the mode, the partial buffers and the outputs
static bool coreset_state_ok(CoresetArgs& a, const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind,
                             int32_t* owner) {
  if (!x || !mind || !owner) return false;
  if (N <= 0 || N > 0x7fffffffLL) return false;
  if (!score_dim_ok(D) || !score_operand_ok(x, ldx, D)) return false;
  if (((uintptr_t)weight & 3) || ((uintptr_t)mind & 3) || ((uintptr_t)owner & 3)) return false;
  a.x = (const bf16*)x; a.ldx = ldx; a.N = (int)N; a.D = D;
  a.weight = weight; a.mind = mind; a.owner = owner;
  a.P = (int)coreset_blocks(N);
  return true;
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int32_t cclip_coreset_blocks(int64_t N) {
  if (N <= 0 || N > 0x7fffffffLL) return 0;
  return (int32_t)coreset_blocks(N);
}

extern "C" int64_t cclip_coreset_workspace(int64_t N) {
  if (N <= 0 || N > 0x7fffffffLL) return 0;
  return 2 * coreset_blocks(N) * 8;
}
#endif

extern "C" int CCLIP_FN(cclip_coreset_step)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind,
                                             int32_t* owner, int32_t centre, const void* partial_in, void* partial_out,
                                             int32_t* pick_out, float* radius_out, hipStream_t stream) {
  CoresetArgs a;
  if (!coreset_state_ok(a, x, ldx, N, D, weight, mind, owner)) return CCLIP_ERR_ARG;
  if (centre < CCLIP_CORESET_SCAN_ONLY || centre >= N) return CCLIP_ERR_ARG;
  if (!partial_out || ((uintptr_t)partial_out & 7) || ((uintptr_t)partial_in & 7) || partial_in == partial_out) return CCLIP_ERR_ARG;
  if (centre == CCLIP_CORESET_FROM_PARTIALS && !partial_in) return CCLIP_ERR_ARG;
  if (centre != CCLIP_CORESET_SCAN_ONLY && (!pick_out || !radius_out)) return CCLIP_ERR_ARG;
  if (((uintptr_t)pick_out & 3) || ((uintptr_t)radius_out & 3)) return CCLIP_ERR_ARG;
  a.centre = centre; a.pin = (const u64*)partial_in; a.pout = (u64*)partial_out;
  a.pick = pick_out; a.radius = radius_out;
  coreset_dispatch(a, stream);
  return cclip_launch_status();
}

extern "C" int CCLIP_FN(cclip_coreset_greedy)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind,
                                               int32_t* owner, int32_t first, int64_t m, int32_t* picks, float* radius,
                                               void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  CoresetArgs a;
  if (!coreset_state_ok(a, x, ldx, N, D, weight, mind, owner)) return CCLIP_ERR_ARG;
  if (m < 0 || m > N) return CCLIP_ERR_ARG;
  if (first < CCLIP_CORESET_FROM_PARTIALS || first >= N) return CCLIP_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < 2 * (int64_t)a.P * 8) return CCLIP_ERR_ARG;
  if (m > 0 && (!picks || !radius)) return CCLIP_ERR_ARG;
  if (((uintptr_t)picks & 3) || ((uintptr_t)radius & 3)) return CCLIP_ERR_ARG;
  u64* part[2] = {(u64*)workspace, (u64*)workspace + a.P};
  for (int64_t t = 0; t < m; ++t) {               // pick t reads partial[t & 1] and writes the other
    a.centre = (t == 0 && first >= 0) ? first : CCLIP_CORESET_FROM_PARTIALS;
    a.pin = part[t & 1]; a.pout = part[(t + 1) & 1];
    a.pick = picks + t; a.radius = radius + t;
    coreset_dispatch(a, stream);
    if ((t & 63) == 63 && hipGetLastError() != hipSuccess) return CCLIP_ERR_LAUNCH;
  }
  return cclip_launch_status();
}
