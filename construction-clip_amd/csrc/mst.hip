// The maximum spanning tree of the complete graph on stored embeddings under mutual-reachability similarity, for gfx950: the
// hot path of HDBSCAN (Campello, Moulavi & Sander 2013).  For unit 16-bit rows x [N, D], core fp32 [N]:
//     s[i, j] = sum_d x[i, d] x[j, d]             (fp32 accumulation on v_mfma_f32_16x16x32, ONE chain over d = 0, 32, 64 ..:
//                                                  the bits cclip_similarity_topk returns for the pair)
//     m[i, j] = min(s[i, j], core[i], core[j])    taken on score_key images: -0 == +0, a NaN operand makes m NaN, the lowest
// Larger = closer, so the tree is a MAXIMUM spanning tree; the N x N matrix is never written.
//
// Strict total order on edges: {i, j} ranks before {k, l} if its m is larger (score_key order); on equal m the smaller
// min(i, j) wins, then the smaller max(i, j).  min() makes exact ties the rule, not the exception - every edge into a sparse
// row carries that row's core - and Boruvka is only correct (no cycles but the two-cycles it expects) when all components
// choose under ONE strict order.  The tree under this order is unique: a pure function of the score bits and core.
// For a fixed row i the order reads "larger m, equal m to the lower j", which is the usual key score_key(m) << 32 | ~j.
//
// mreach_nearest_kernel (the N^2 kernel), grid = blocks of 64 * MT rows x gallery splits: per row i the best key over the rows
// j with comp[j] != comp[i] (so j != i), 0 = no such row.  The sweep of score_sweep.h with two tile buffers: the split's rows
// of the SAME matrix are the streamed ones, with comp / core of the next tile's rows in flight beside them (the fetch hook).
// A lane keeps a running maximum per row it owns; the 16 lanes of a group combine by group_max_key.  One split: lane 0 stores.  Several: the output is zeroed
// first and lane 0 takes atomicMax on the 64-bit key - an integer maximum of distinct keys has no order, so the output is the
// same bits for any split and any launch order.  comp is only compared, never used as an index.
//
// cclip_mst_boruvka enqueues ceil(log2 N) rounds from one C loop (the pattern of coreset.hip / decode_driver.hip) and reads
// nothing on the host.  A component is named by one of its rows, comp[name] == name.  Round r, flags[r] != 0 ("more than one
// component is left"; every kernel of a round returns at once otherwise), reads comp_in = comp[r & 1]:
//   nearest   rowkey[i]                                                                         (the N^2 kernel)
//   best1     ck1[c] = max over the rows i of c of score_key(m) << 32 | ~min(i, j)              (atomicMax, 64-bit)
//   best2     ck2[c] = min of max(i, j) over the rows of c that reach ck1[c]                     (atomicMin, 32-bit)
//             (ck1, ck2) IS the component's best outgoing edge under the total order: its m, its smaller and larger row
//   hook      one thread per name c: the endpoint inside c is i, the other j, the target t = comp_in[j].  If t chose the same
//             edge, the lower name stays a root; every other component hangs under its target, parent[c] = t, and records
//             (i, j, m) in slot c of u, v, m.  A name that was hung is never a name again, so exactly one slot, the final
//             root's, stays empty (u = v = -1, m = NaN) and the arrays hold N - 1 edges.  No counters.
//   relabel   comp_out[i] = the root above comp_in[i], by chasing parent (bounded by N steps); flags[r + 1] = 1 if the row's
//             root differs from row 0's; ck1 / ck2 of slot i and rowkey[i] are reset for the next round (the driver
//             queues no memset: a round that is not live touches nothing).
// comp_in != comp_out: a late work-group of relabel still reads the labels an early one would otherwise have rewritten (the
// partial_in != partial_out rule of coreset.hip).  Every index taken from memory is clamped into [0, N - 1] before use.
// Integer atomics only, no float atomics: two calls are bitwise equal.
#include "score_sweep.h"
#include "../../include/cclip_hip.h"

#define MST_FLAGS 64                              // int32 flags in the workspace: rounds + 1 <= 32 used

namespace CCLIP_NS {

struct NearestArgs {
  const bf16* x; long ldx;
  int N, D;
  const float* core; const int* comp;
  u64* out;
  const int* live;                                // device flag, may be null: 0 = return at once
  int splits, rows_per_split;                     // rows_per_split is a multiple of 64
};

// <KSMAX, MT, GT> as in score_tiles.h: MT tiles of 16 operand rows per wave, GT streamed rows per tile
template <int KSMAX, int MT, int GT>
__global__ __launch_bounds__(256) void mreach_nearest_kernel(const NearestArgs a) {
  constexpr int NST = GT / 16;                    // sub-tiles of 16 streamed rows
  extern __shared__ __attribute__((aligned(16))) char lds[];
  if (a.live && *a.live == 0) return;             // (grid-uniform, before any barrier)
  const SweepCtx<MT> ctx(a.D, a.N, a.N, a.splits, a.rows_per_split);
  const int li = ctx.li;
  const long N = a.N;

  bf16x8 af[MT][KSMAX];
  ctx.load_a(af, a.x, a.ldx);
  // per-row state of this lane: the row's component, its core key, the best key so far
  int ci[MT][4];
  unsigned kci[MT][4];
  u64 b1[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = ctx.row_clamped(mt, r);    // (a clamped row is loaded, never written)
      ci[mt][r] = a.comp[row];
      kci[mt][r] = score_key(a.core[row]);
      b1[mt][r] = 0ull;
    }

  // comp and the core key of the streamed rows this lane meets in a tile: rows base + 16 st + li, clamped to N - 1
  int cj[NST], cjn[NST];
  unsigned kcj[NST], kcjn[NST];
  auto side = [&](long base, int (&c)[NST], unsigned (&k)[NST]) CCLIP_SWEEP_INLINE {
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const long j = min(base + 16 * st + li, N - 1);
      c[st] = a.comp[j];
      k[st] = score_key(a.core[j]);
    }
  };
  side(ctx.n0, cj, kcj);

  // rows >= N are clamped (never selected below)
  stream_tiles<KSMAX, MT, GT>(
      ctx, af, a.x, a.ldx, ctx.n0, ctx.n1, N - 1, lds,
      [&](long base, f32x4 (&acc)[MT][NST]) CCLIP_SWEEP_INLINE {
        for_subtiles<GT>(ctx, base, ctx.n1, [&](int st, long nb, bool okc) CCLIP_SWEEP_INLINE {
          const unsigned low = ~(unsigned)(nb + li);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const unsigned k = min(min(score_key(acc[mt][st][r]), kci[mt][r]), kcj[st]);
              const bool valid = okc && cj[st] != ci[mt][r];
              const u64 cand = valid ? (((u64)k << 32) | low) : 0ull;                 // selected, not multiplied
              b1[mt][r] = cand > b1[mt][r] ? cand : b1[mt][r];
            }
        });
#pragma unroll
        for (int st = 0; st < NST; ++st) { cj[st] = cjn[st]; kcj[st] = kcjn[st]; }    // the next tile's, fetched beside it
      },
      [&](long next) CCLIP_SWEEP_INLINE { side(next, cjn, kcjn); });
  if (!ctx.active) return;

  // the 16 lanes of a group hold disjoint rows j; lane 0 writes
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u64 m1 = group_max_key(b1[mt][r]);
      if (li == 0 && ctx.row_live(mt, r)) {
        if (a.splits == 1) a.out[ctx.row(mt, r)] = m1;
        else if (m1 != 0ull) atomicMax(a.out + ctx.row(mt, r), m1);   // (the launcher zeroed out; distinct keys: no order)
      }
    }
}

// gallery splits from N alone: about 1024 work-groups of 128 rows while a split keeps at least 1024 rows
static inline void nearest_splits(int64_t N, int* splits, int* rows_per_split) {
  gallery_splits(N, (N + 127) / 128, 1024, 1024, splits, rows_per_split);
}

// a.x .. a.live set by the caller, whose arguments have been checked.  zero: a.out is not known to hold zeros (more than one
// split meets in atomicMax)
static int nearest_dispatch(NearestArgs& a, bool zero, hipStream_t stream) {
  nearest_splits(a.N, &a.splits, &a.rows_per_split);
  if (zero && a.splits > 1 && hipMemsetAsync(a.out, 0, (size_t)a.N * 8, stream) != hipSuccess) return CCLIP_ERR_LAUNCH;
  return score_dispatch<true>(a.D, a.N > 64, [&](auto s) {
    using S = decltype(s);
    return sweep_launch(mreach_nearest_kernel<S::KSMAX, S::MT, S::GT>, a, a.N, S::MT, S::GT, a.D, a.splits, 2, 0, stream);
  });
}

static bool nearest_operands_ok(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core) {
  if (!x || !core) return false;
  if (!score_rows_ok(N) || !score_operands_ok(x, ldx, x, ldx, D)) return false;
  return !((uintptr_t)core & 3);
}

// ------------------------------------------------------------------------------------------------------------------------
struct MstArgs {
  int N;
  u64* rowkey; u64* ck1; unsigned* ck2; int* parent;
  const int* cin; int* cout;
  int* u; int* v; float* m;
  int* flags; int round;                          // flags[round]: this round is live; flags[round + 1]: the next one is
};

__global__ __launch_bounds__(256) void mst_init_kernel(const MstArgs a, int* comp0) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i < MST_FLAGS) a.flags[i] = (i == 0 && a.N > 1) ? 1 : 0;
  if (i >= a.N) return;
  comp0[i] = (int)i; a.parent[i] = (int)i;
  a.ck1[i] = 0ull; a.ck2[i] = 0xffffffffu; a.rowkey[i] = 0ull;
  a.u[i] = -1; a.v[i] = -1; a.m[i] = __uint_as_float(0x7fc00000u);
}

// the row's candidate for its component: (key of m, ~min(i, j)) and max(i, j); false = the row has no outgoing edge
__device__ __forceinline__ bool mst_row_edge(const MstArgs& a, int i, int& c, u64& k1, unsigned& hi) {
  const u64 key = a.rowkey[i];
  if (key == 0ull) return false;
  const int j = clamp_index((int)~(unsigned)key, 0, a.N - 1);
  c = clamp_index(a.cin[i], 0, a.N - 1);                   // (a name is a row: it indexes ck1 / ck2)
  k1 = (key & 0xffffffff00000000ull) | (unsigned)~(unsigned)min(i, j);
  hi = (unsigned)max(i, j);
  return true;
}

__global__ __launch_bounds__(256) void mst_best1_kernel(const MstArgs a) {
  if (a.flags[a.round] == 0) return;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= a.N) return;
  int c; u64 k1; unsigned hi;
  if (mst_row_edge(a, (int)i, c, k1, hi)) atomicMax(a.ck1 + c, k1);
}

__global__ __launch_bounds__(256) void mst_best2_kernel(const MstArgs a) {
  if (a.flags[a.round] == 0) return;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= a.N) return;
  int c; u64 k1; unsigned hi;
  if (mst_row_edge(a, (int)i, c, k1, hi) && k1 == a.ck1[c]) atomicMin(a.ck2 + c, hi);
}

__global__ __launch_bounds__(256) void mst_hook_kernel(const MstArgs a) {
  if (a.flags[a.round] == 0) return;
  const long il = blockIdx.x * 256L + threadIdx.x;
  if (il >= a.N) return;
  const int c = (int)il, N = a.N;
  if (a.cin[c] != c) return;                      // one thread per name
  const u64 k1 = a.ck1[c];
  const unsigned k2 = a.ck2[c];
  int par = c;
  if (k1 != 0ull) {
    const int lo = clamp_index((int)~(unsigned)k1, 0, N - 1), hi = clamp_index((int)k2, 0, N - 1);
    const bool lo_in = clamp_index(a.cin[lo], 0, N - 1) == c;              // exactly one endpoint of an outgoing edge lies in c
    const int i = lo_in ? lo : hi, j = lo_in ? hi : lo;
    const int t = clamp_index(a.cin[j], 0, N - 1);
    const bool same = a.ck1[t] == k1 && a.ck2[t] == k2;           // t chose this very edge
    if (t != c && !(same && c < t)) {
      par = t;
      a.u[c] = i; a.v[c] = j; a.m[c] = key_score((unsigned)(k1 >> 32));
    }
  }
  a.parent[c] = par;
}

__device__ __forceinline__ int mst_root(const int* parent, int c, int N) {
  int r = c;
  for (int step = 0; step < N; ++step) {          // (the hooks form a forest; the bound only guards garbage)
    const int p = clamp_index(parent[r], 0, N - 1);
    if (p == r) break;
    r = p;
  }
  return r;
}

__global__ __launch_bounds__(256) void mst_relabel_kernel(const MstArgs a) {
  if (a.flags[a.round] == 0) return;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= a.N) return;
  const int r = mst_root(a.parent, clamp_index(a.cin[i], 0, a.N - 1), a.N);
  const int r0 = mst_root(a.parent, clamp_index(a.cin[0], 0, a.N - 1), a.N);
  a.cout[i] = r;
  if (r != r0) a.flags[a.round + 1] = 1;          // (every writer stores the same value)
  a.ck1[i] = 0ull; a.ck2[i] = 0xffffffffu;        // (not read in this kernel)
  a.rowkey[i] = 0ull;                             // the next round's splits meet in atomicMax on zeros
}

static inline int64_t mst_workspace(int64_t N) { return N * 32 + MST_FLAGS * 4; }

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_mst_workspace(int64_t N) {
  if (!score_rows_ok(N)) return 0;
  return mst_workspace(N);
}

extern "C" int32_t cclip_mreach_nearest_splits(int64_t N) {
  if (!score_rows_ok(N)) return 0;
  int splits, rows;
  nearest_splits(N, &splits, &rows);
  return splits;
}
#endif

extern "C" int CCLIP_FN(cclip_mreach_nearest)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core,
                                               const int32_t* comp, void* keys, hipStream_t stream) {
  if (!nearest_operands_ok(x, ldx, N, D, core)) return CCLIP_ERR_ARG;
  if (!comp || !keys || ((uintptr_t)comp & 3) || ((uintptr_t)keys & 7)) return CCLIP_ERR_ARG;
  NearestArgs a;
  a.x = (const bf16*)x; a.ldx = ldx; a.N = (int)N; a.D = D;
  a.core = core; a.comp = comp; a.out = (u64*)keys; a.live = nullptr;
  const int st = nearest_dispatch(a, true, stream);
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}

extern "C" int CCLIP_FN(cclip_mst_boruvka)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core, int32_t* u,
                                            int32_t* v, float* m, void* workspace, int64_t workspace_bytes,
                                            hipStream_t stream) {
  if (!nearest_operands_ok(x, ldx, N, D, core)) return CCLIP_ERR_ARG;
  if (!u || !v || !m || ((uintptr_t)u & 3) || ((uintptr_t)v & 3) || ((uintptr_t)m & 3)) return CCLIP_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < mst_workspace(N)) return CCLIP_ERR_ARG;
  char* w = (char*)workspace;                     // rowkey, ck1: u64 [N]; ck2, parent, comp[2]: 32-bit [N]; the flags
  u64* rowkey = (u64*)w;
  MstArgs b;
  b.N = (int)N; b.rowkey = rowkey; b.ck1 = rowkey + N;
  b.ck2 = (unsigned*)(w + 16 * N); b.parent = (int*)(w + 20 * N);
  int* comp[2] = {(int*)(w + 24 * N), (int*)(w + 28 * N)};
  b.flags = (int*)(w + 32 * N); b.u = u; b.v = v; b.m = m;
  b.cin = comp[0]; b.cout = comp[1]; b.round = 0;
  const unsigned grid = (unsigned)((N + 255) / 256);              // (>= 1 block: covers the MST_FLAGS flags too)
  hipLaunchKernelGGL(mst_init_kernel, dim3(grid), dim3(256), 0, stream, b, comp[0]);
  if (hipGetLastError() != hipSuccess) return CCLIP_ERR_LAUNCH;
  int rounds = 0;
  while (((int64_t)1 << rounds) < N) ++rounds;    // ceil(log2 N): every round at least halves the components
  NearestArgs a;
  a.x = (const bf16*)x; a.ldx = ldx; a.N = (int)N; a.D = D; a.core = core; a.out = rowkey;
  for (int r = 0; r < rounds; ++r) {              // round r reads comp[r & 1] and writes the other
    b.round = r; b.cin = comp[r & 1]; b.cout = comp[(r + 1) & 1];
    a.comp = b.cin; a.live = b.flags + r;
    const int st = nearest_dispatch(a, false, stream);        // (rowkey holds zeros: init, then every live relabel)
    if (st != CCLIP_OK) return st;
    hipLaunchKernelGGL(mst_best1_kernel, dim3(grid), dim3(256), 0, stream, b);
    hipLaunchKernelGGL(mst_best2_kernel, dim3(grid), dim3(256), 0, stream, b);
    hipLaunchKernelGGL(mst_hook_kernel, dim3(grid), dim3(256), 0, stream, b);
    hipLaunchKernelGGL(mst_relabel_kernel, dim3(grid), dim3(256), 0, stream, b);
    if (hipGetLastError() != hipSuccess) return CCLIP_ERR_LAUNCH;
  }
  return cclip_launch_status();
}
