// Linear probe over stored embeddings for gfx950: multinomial logistic regression on 16-bit rows x [N, D] with fp32 weights
// W [C, D] and bias [C].  One evaluation of the objective and its gradient, without the N x C logits in memory.
//
// The objective of hi + lo.  W enters the MFMA as a 16-bit pair hi = round16(W), lo = round16(W - hi) (score_pair.h's
// pair_image_kernel, into the workspace), and everything below is a function of that pair:
//     z[n, c]   = (bias[c] + H[n, c]) + L[n, c],  H = sum_d x[n, d] hi[c, d],  L = sum_d x[n, d] lo[c, d]
//                 H and L are each ONE fp32 accumulator chain over d = 0, 32, 64 .. on v_mfma_f32_16x16x32; the two adds in
//                 the order written.
//     lse[n]    = log sum_c exp z[n, c]          loss[n] = rw[n] (lse[n] - z[n, y_n])          pred[n] = argmax_c z[n, c]
//     g[n, c]   = rw[n] (exp(z[n, c] - lse[n]) - [c == y_n])
//     dW[c, :]  = scale sum_n g[n, c] x[n, :] + l2 W[c, :]        db[c] = scale sum_n g[n, c]
//     objective = scale sum_n loss[n] + l2 / 2 sum W^2
// rw = row_weight clamped into [0, 1] (NaN -> 0; 1 without the array).  A row whose label lies outside [0, C) or whose rw is 0
// is ignored: its loss is +0.0f and its g is 0, both SELECTED, never multiplied - a NaN row of x that is ignored leaves no
// trace.  dW is the gradient of the objective as a function of the pair (d z / d W taken as x: W - (hi + lo) is below 2^-16 |W|
// for bf16, 2^-22 |W| for fp16); loss and gradient therefore belong to the same function, which is what a line search needs.
//
// The image.  Classes are padded to Cp = 16 ceil(C / 16); a tile of 32 image rows holds hi and lo of 16 classes, the two chains
// (the layout is pair_image_kernel's).
//
// Forward (probe_fwd_kernel): the geometry of kmeans_assign_kernel.  Grid = blocks of 64 * MT rows of x, a work-group keeps its
// rows as A fragments and streams all class tiles through two LDS buffers (one barrier per tile; its own loop, see
// score_sweep.h).  Lane (li, g) meets class
// 16 t + li of every tile and keeps per row a running (max, sum) pair, the label's logit and the best (score_key, ~class) key;
// the 16 lanes of a group are combined by a fixed xor butterfly whose two partners compute the same bits.  So a row's outputs
// depend on neither N nor the row's position nor MT.  Ties in pred go to the LOWER class, NaN ranks lowest (score_key.h).
//
// Backward (probe_bwd_kernel): the two products of embed_cache_bwd.hip (the inner step both share is score_pair.h's) with the
// roles of its stored rows taken by the classes.
// A wave keeps hi and lo of 16 classes as B fragments in registers, the rows of x stream through two LDS buffers in tiles of
// 32 (an ignored row's content replaced by zeros: 0 * NaN would be NaN in the second product), z^T comes with the row on the accumulator row and the class on the lane, g is split into a 16-bit hi + lo pair (|g| <= 1:
// no scale) and dW^T[d, c] += x^T[d, n] g[n, c] takes its A operand from the SAME LDS image through ds_read_b64_tr_b16.
// Unlike there, the ROWS are split over the grid: work-group (column part, class block, row part) owns `tpp` consecutive row
// tiles.  Its four waves are cbw class blocks x rs row streams (cbw = 4, 2, 1 for Cp >= 48, Cp == 32, Cp == 16: few classes
// leave no wave idle); stream s takes the tiles s, s + rs, .. of the part in ascending order into its register accumulator
// and writes ONE fp32 partial to workspace slot part * rs + s.  db's partial is the fp32 g summed in the same order, then over
// the four lane groups by a fixed butterfly.  Above D = 512 the columns are cut in four parts over the grid so that no variant
// spills.  probe_merge_kernel adds the slots in ascending order, applies scale and l2 (the bias is not regularised), and its
// further blocks reduce loss[] and W^2 by a fixed tree; probe_objective_kernel finishes the scalar.
// Slots, tiles per part and every other choice are functions of (N, C, D) alone (probe_geom); no atomics, no fused
// multiply-add: two calls are bitwise equal.  The row parts are score_sweep.h's row_parts.  Every index taken from labels is compared, never used as an address.
#include "score_pair.h"
#include "../../include/cclip_hip.h"

// the sums below are written out operation by operation: no fused multiply-add may be formed from them
#pragma clang fp contract(off)

#define PROBE_MAX_C 256
#define PROBE_RT 32                               // rows of x per backward tile: one k-step of the second product
#define PROBE_LOSS_BLOCKS 256
#define PROBE_NONE (-3.0e38f)                     // running maximum before the first class

namespace CCLIP_NS {

struct ProbeGeom {
  int cpad, rs, cbw, ncb, ds, tpp, parts, slots, ntiles, wblocks;
  int64_t off_part, off_db, off_red, total;
};

static inline bool probe_geom(int64_t N, int64_t C, int32_t D, ProbeGeom& g) {
  if (!score_rows_ok(N) || C < 2 || C > PROBE_MAX_C || !score_dim_ok(D)) return false;
  g.cpad = (int)((C + 15) / 16 * 16);
  const int nb = g.cpad / 16;
  g.cbw = nb >= 3 ? 4 : nb;                       // class blocks of 16 per work-group
  g.rs = 4 / g.cbw;                               // row streams per work-group
  g.ncb = (nb + g.cbw - 1) / g.cbw;
  g.ds = D > 512 ? 4 : 1;
  row_parts(N, (int64_t)g.rs * g.cpad * D * 4, &g.ntiles, &g.tpp, &g.parts);      // a part holds rs slots of [cpad][D] fp32
  g.slots = g.parts * g.rs;
  g.wblocks = (int)((C * D + 255) / 256);
  g.off_part = (int64_t)4 * g.cpad * D;                           // behind the image: 2 Cp rows of D 16-bit elements
  g.off_db = g.off_part + (int64_t)4 * g.slots * g.cpad * D;
  g.off_red = g.off_db + (int64_t)4 * g.slots * g.cpad;
  g.total = g.off_red + (int64_t)4 * (g.wblocks + PROBE_LOSS_BLOCKS);
  return true;
}

// row_weight into [0, 1]; NaN fails the comparison and becomes 0
__device__ __forceinline__ float probe_weight(const float* __restrict__ rw, long row) {
  if (!rw) return 1.0f;
  const float v = rw[row];
  return v > 0.0f ? fminf(v, 1.0f) : 0.0f;
}

struct ProbeFwdArgs {
  const bf16* x; const bf16* img;
  long ldx;
  int N, C, D;
  const float* bias; const int* labels; const float* rw;          // each may be null
  float* lse; float* loss; int* pred; float* logits;              // logits may be null
};

template <int KSMAX, int MT>
__global__ __launch_bounds__(256) void probe_fwd_kernel(const ProbeFwdArgs a) {
  constexpr int GT = 32;                          // image rows per tile: hi and lo of 16 classes
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int C = a.C, D = a.D;
  const TileGeom geo(D);
  const int tilebytes = GT * geo.rowbytes;
  const int ntiles = (C + 15) >> 4;

  const long row0 = (long)blockIdx.x * (64 * MT);                 // (row0 < N: the grid has no empty block)
  const int last = (int)min((long)a.N - 1 - row0, (long)(64 * MT - 1));
  const bf16* xb = a.x + row0 * a.ldx;
  const int q0 = wave * (16 * MT);
  const bool active = q0 <= last;                 // (wave-uniform) a wave without rows only helps to load

  bf16x8 af[MT][KSMAX];
  load_a_frags<KSMAX, MT>(af, xb, a.ldx, q0, last, geo.nks, lane);
  // per-row state of this lane, rows q0 + 16 mt + 4 g + r
  float m[MT][4], s[MT][4], zy[MT][4];
  u64 b1[MT][4];
  int y[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[mt][r] = PROBE_NONE; s[mt][r] = 0.0f; zy[mt][r] = 0.0f; b1[mt][r] = 0ull;
      y[mt][r] = a.labels ? a.labels[row0 + min(q0 + 16 * mt + 4 * g + r, last)] : -1;
    }

  TileMover<KSMAX, GT> mover(geo, tid);
  mover.fetch(a.img, D, 0, GT - 1);               // the image is padded to whole tiles
  int buf = 0;
  for (int t = 0; t < ntiles; ++t, buf ^= 1) {
    char* Cs = lds + buf * tilebytes;
    mover.store(Cs);
    __syncthreads();                              // tile t is whole; every wave has left the tile before last (this buffer's next content)
    if (t + 1 < ntiles) mover.fetch(a.img + (long)(t + 1) * GT * D, D, 0, GT - 1);
    if (!active) continue;

    f32x4 acc[MT][2];                             // [0]: the hi chain, [1]: the lo chain
    tile_multiply<KSMAX, MT, GT>(acc, af, Cs, geo, lane);

    const int cls = 16 * t + li;
    const bool okc = cls < C;
    const float b = a.bias ? a.bias[min(cls, C - 1)] : 0.0f;
    const unsigned low = ~(unsigned)cls;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = (b + acc[mt][0][r]) + acc[mt][1][r];
        if (okc) {                                // (no cross-lane operation inside)
          const float mo = m[mt][r], mn = fmaxf(mo, z);           // a NaN logit leaves the maximum and turns the sum NaN
          s[mt][r] = s[mt][r] * expf(mo - mn) + expf(z - mn);
          m[mt][r] = mn;
          const u64 cand = ((u64)score_key(z) << 32) | low;
          b1[mt][r] = cand > b1[mt][r] ? cand : b1[mt][r];
          zy[mt][r] = cls == y[mt][r] ? z : zy[mt][r];
          const int rel = q0 + 16 * mt + 4 * g + r;
          if (a.logits && rel <= last) a.logits[(row0 + rel) * C + cls] = z;
        }
      }
  }
  if (!active) return;

  // the 16 lanes of a group hold disjoint classes: a fixed xor butterfly, both partners compute the same bits
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mm = m[mt][r], ss = s[mt][r], zz = zy[mt][r];
      u64 k1 = b1[mt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float pm = __shfl_xor(mm, o, 64), ps = __shfl_xor(ss, o, 64), pz = __shfl_xor(zz, o, 64);
        const u64 pk = shfl_xor64(k1, o);
        const float mn = fmaxf(mm, pm);
        const float ta = ss * expf(mm - mn), tb = ps * expf(pm - mn);
        ss = ta + tb;                             // commutative: the partner adds the same two numbers
        mm = mn;
        zz = zz + pz;                             // one lane holds the label's logit, the others 0
        k1 = k1 > pk ? k1 : pk;
      }
      const int rel = q0 + 16 * mt + 4 * g + r;
      if (li == 0 && rel <= last) {
        const long row = row0 + rel;
        const float lse = mm + logf(ss);
        const float w = probe_weight(a.rw, row);
        const bool live = y[mt][r] >= 0 && y[mt][r] < C && w > 0.0f;
        a.lse[row] = lse;
        a.loss[row] = live ? w * (lse - zz) : 0.0f;               // selected, not multiplied
        a.pred[row] = (int)~(unsigned)k1;
      }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
struct ProbeBwdArgs {
  const bf16* x; const bf16* img;
  long ldx;
  int N, C, D, cpad;
  const float* bias; const int* labels; const float* rw; const float* lse;
  int tpp, ntiles, rs, cbw;
  float* part; float* dbpart;                     // [slots][cpad][D], [slots][cpad]
};

// <KSMAX, DS, PRE>: k-steps of 32 the class fragments are sized for (D <= 32 KSMAX); DS column parts over the grid; PRE: the next
// tile's loads are in flight under the current tile's products (above D = 512 their 64 staging registers would spill: the tile
// is loaded at the top of its own step instead)
template <int KSMAX, int DS, bool PRE>
__global__ __launch_bounds__(256) void probe_bwd_kernel(const ProbeBwdArgs a) {
  constexpr int GT = PROBE_RT;
  constexpr int NDT = 2 * KSMAX / DS;             // column tiles of 16 this work-group accumulates
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int N = a.N, C = a.C, D = a.D;
  const TileGeom geo(D);
  const int tilebytes = GT * geo.rowbytes;

  const int dt0 = (int)blockIdx.x * NDT;          // first column tile of this part
  const int part = blockIdx.z;
  const int blk16 = (int)blockIdx.y * a.cbw + wave % a.cbw;       // this wave's block of 16 classes
  const int stream = wave / a.cbw;
  const int t0 = part * a.tpp, t1 = min(t0 + a.tpp, a.ntiles);    // (t0 < ntiles: the grid has no empty part)
  const int c0 = 16 * blk16;
  const bool active = c0 < C && 16 * dt0 < D;     // (wave-uniform) a wave without classes or columns only helps to load
  const int cls = c0 + li;
  const bool okc = cls < C;
  const float b = a.bias ? a.bias[min(cls, C - 1)] : 0.0f;

  bf16x8 wf[2][KSMAX];                            // [0]: hi, [1]: lo of the 16 classes (image rows 32 blk + 16 h + li)
  load_a_frags<KSMAX, 2>(wf, a.img + (long)min(blk16, a.cpad / 16 - 1) * 32 * D, D, 0, 31, geo.nks, lane);

  f32x4 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.0f;

  TileMover<KSMAX, GT> mover(geo, tid);
  // An ignored row (and a row beyond N) has g = 0, but 0 * NaN is NaN inside the second product: its content is replaced by
  // zeros on the way into LDS.  Bit `it` of the mask: the it-th chunk this thread moves belongs to such a row.
  auto dead_rows = [&](int tb) -> unsigned {
    unsigned mk = 0u;
#pragma unroll
    for (int it = 0; it < TileMover<KSMAX, GT>::IT; ++it) {
      const long row = (long)tb + (mover.where[it] >> 8);
      const long rc = min(row, (long)N - 1);
      const int yy = a.labels ? a.labels[rc] : -1;
      const bool dead = row >= N || yy < 0 || yy >= C || !(probe_weight(a.rw, rc) > 0.0f);
      mk |= dead ? (1u << it) : 0u;
    }
    return mk;
  };
  unsigned deadmask = 0u;
  if (PRE) { mover.fetch(a.x + (long)t0 * GT * a.ldx, a.ldx, 0, N - 1 - t0 * GT); deadmask = dead_rows(t0 * GT); }   // rows >= N are clamped
  int buf = 0;
  for (int t = t0; t < t1; ++t, buf ^= 1) {
    const int base = t * GT;                      // < 2^31: base <= N - 1
    char* Xs = lds + buf * tilebytes;
    if (!PRE) { mover.fetch(a.x + (long)base * a.ldx, a.ldx, 0, N - 1 - base); deadmask = dead_rows(base); }
#pragma unroll
    for (int it = 0; it < TileMover<KSMAX, GT>::IT; ++it)
      if ((deadmask >> it) & 1u) mover.stage[it] = (u32x4){0u, 0u, 0u, 0u};
    mover.store(Xs);
    __syncthreads();                              // tile t is whole; every wave has left the tile before last (this buffer's next content)
    if (PRE && t + 1 < t1) { mover.fetch(a.x + ((long)base + GT) * a.ldx, a.ldx, 0, N - 1 - (base + GT)); deadmask = dead_rows(base + GT); }
    if (!active || (t - t0) % a.rs != stream) continue;           // (wave-uniform)
    const int lane_t = opaque_lane(lane);         // the tile's LDS addresses are formed per tile (score_pair.h)

    // this lane's rows base + 16 st + 4 g + r
    float lse[2][4], w[2][4];
    int y[2][4];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long qi = min((long)base + 16 * st + 4 * g + r, (long)N - 1);
        lse[st][r] = a.lse[qi];
        w[st][r] = probe_weight(a.rw, qi);
        y[st][r] = a.labels ? a.labels[qi] : -1;
      }

    // z^T: row of x on the accumulator row, class on the lane; s[0] the hi chain, s[1] the lo chain
    f32x4 s[2][2];
    tile_scores_t<KSMAX, 2>(s, wf, Xs, geo, lane_t);

    bf16x8 ghi, glo;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long qi = (long)base + 16 * st + 4 * g + r;
        const float z = (b + s[0][st][r]) + s[1][st][r];
        const float p = expf(z - lse[st][r]);
        const int yy = y[st][r];
        const bool take = okc && qi < N && yy >= 0 && yy < C && w[st][r] > 0.0f;
        const float gg = take ? w[st][r] * (p - (cls == yy ? 1.0f : 0.0f)) : 0.0f;   // selected, not multiplied
        dbacc += gg;
        split16(gg, ghi, glo, 4 * st + r);
      }

    // dW^T[d, c] += x^T[d, n] g[n, c] over the 32 rows of the tile: k index = (st, g, r) on both operands
    tr_accumulate<NDT>(acc, Xs, geo, dt0, D, ghi, glo, lane_t);
  }
  if (!active) return;

  // lane (li, g) holds the slot's [cls][16 dt + 4 g .. + 3]; cls < cpad.  A stream without a tile writes zeros.
  const long slot = (long)part * a.rs + stream;
  store_dt_columns<NDT>(a.part + (slot * a.cpad + cls) * D + 4 * g, dt0, D, [&](int dt) CCLIP_SWEEP_INLINE { return acc[dt]; });
  dbacc += __shfl_xor(dbacc, 16, 64);             // the four lane groups (rows 4 g + r), a fixed butterfly
  dbacc += __shfl_xor(dbacc, 32, 64);
  if (blockIdx.x == 0 && g == 0) a.dbpart[slot * a.cpad + cls] = dbacc;
}

struct ProbeMergeArgs {
  const float* W; const float* part; const float* dbpart; const float* loss;    // loss may be null
  int N, C, D, cpad, slots, wblocks;
  float scale, l2;
  float* dW; float* db; float* red;               // red: [wblocks] sums of W^2, then [PROBE_LOSS_BLOCKS] sums of loss
};

__global__ __launch_bounds__(256) void probe_merge_kernel(const ProbeMergeArgs a) {
  __shared__ float red[4];
  const int tid = threadIdx.x, blk = blockIdx.x;
  float v = 0.0f;
  if (blk < a.wblocks) {
    const long idx = (long)blk * 256 + tid;
    if (idx < (long)a.C * a.D) {
      const int c = (int)(idx / a.D), d = (int)(idx - (long)c * a.D);
      const long stride = (long)a.cpad * a.D;
      const float* p = a.part + (long)c * a.D + d;
      float sum = p[0];
      for (int s = 1; s < a.slots; ++s) sum += p[s * stride];     // ascending slots
      const float w = a.W[idx];
      a.dW[idx] = sum * a.scale + a.l2 * w;
      v = w * w;
      if (d == 0) {
        float sb = a.dbpart[c];
        for (int s = 1; s < a.slots; ++s) sb += a.dbpart[(long)s * a.cpad + c];
        a.db[c] = sb * a.scale;
      }
    }
  } else if (a.loss) {
    for (long i = (long)(blk - a.wblocks) * 256 + tid; i < a.N; i += (long)PROBE_LOSS_BLOCKS * 256) v += a.loss[i];
  }
  v = block_sum4(v, red);
  if (tid == 0) a.red[blk] = v;
}

__global__ __launch_bounds__(256) void probe_objective_kernel(const float* __restrict__ part, int wblocks, float scale, float l2,
                                                              float* __restrict__ objective) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float sw = 0.0f, sl = 0.0f;
  for (int i = tid; i < wblocks; i += 256) sw += part[i];
  sl = part[wblocks + tid];
  sw = block_sum4(sw, red);
  __syncthreads();
  sl = block_sum4(sl, red);
  if (tid == 0) objective[0] = scale * sl + (0.5f * l2) * sw;
}

template <int KSMAX, int DS, bool PRE>
static int probe_bwd_launch(const ProbeBwdArgs& a, const ProbeGeom& g, hipStream_t stream) {
  return score_launch(probe_bwd_kernel<KSMAX, DS, PRE>, dim3(DS, g.ncb, g.parts), (size_t)2 * PROBE_RT * a.D * 2, a, stream);
}

// the checks the two entries share
static bool probe_args_ok(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias, int32_t C,
                          const int32_t* labels, const float* rw, const void* ws, int64_t ws_bytes, ProbeGeom& g) {
  if (!x || !W || !ws) return false;
  if (!probe_geom(N, C, D, g)) return false;
  if (!score_operand_ok(x, ldx, D) || ((uintptr_t)ws & 15)) return false;
  if (((uintptr_t)W & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)rw & 3)) return false;
  return ws_bytes >= g.total;
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

#ifndef CCLIP_F16
extern "C" int64_t cclip_probe_workspace(int64_t N, int32_t C, int32_t D) {
  ProbeGeom g;
  return probe_geom(N, C, D, g) ? g.total : 0;
}

extern "C" int32_t cclip_probe_parts(int64_t N, int32_t C, int32_t D) {
  ProbeGeom g;
  return probe_geom(N, C, D, g) ? g.slots : 0;
}
#endif

extern "C" int CCLIP_FN(cclip_probe_forward)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias,
                                              int32_t C, const int32_t* labels, const float* row_weight, float* lse, float* loss,
                                              int32_t* pred, float* logits, void* workspace, int64_t workspace_bytes,
                                              hipStream_t stream) {
  ProbeGeom g;
  if (!lse || !loss || !pred) return CCLIP_ERR_ARG;
  if (!probe_args_ok(x, ldx, N, D, W, bias, C, labels, row_weight, workspace, workspace_bytes, g)) return CCLIP_ERR_ARG;
  if (((uintptr_t)lse & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)logits & 3)) return CCLIP_ERR_ARG;
  pair_image_launch(W, C, D, workspace, stream);
  ProbeFwdArgs a;
  a.x = (const bf16*)x; a.img = (const bf16*)workspace; a.ldx = ldx;
  a.N = (int)N; a.C = C; a.D = D;
  a.bias = bias; a.labels = labels; a.rw = row_weight;
  a.lse = lse; a.loss = loss; a.pred = pred; a.logits = logits;
  const int st = score_dispatch<false>(D, N > 64, [&](auto s) {                  // (tiles of 32 image rows on every rung)
    using S = decltype(s);
    return sweep_launch(probe_fwd_kernel<S::KSMAX, S::MT>, a, N, S::MT, 32, D, 1, 2, 0, stream);
  });
  if (st != CCLIP_OK) return st;
  return cclip_launch_status();
}

extern "C" int CCLIP_FN(cclip_probe_backward)(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias,
                                               int32_t C, const int32_t* labels, const float* row_weight, const float* lse,
                                               const float* loss, float scale, float l2, float* dW, float* db, float* objective,
                                               void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  ProbeGeom g;
  if (!lse || !dW || !db || (loss == nullptr) != (objective == nullptr)) return CCLIP_ERR_ARG;
  if (!score_finite(scale) || !score_finite(l2) || scale < 0.0f || l2 < 0.0f) return CCLIP_ERR_ARG;
  if (!probe_args_ok(x, ldx, N, D, W, bias, C, labels, row_weight, workspace, workspace_bytes, g)) return CCLIP_ERR_ARG;
  if (((uintptr_t)lse & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)dW & 3) || ((uintptr_t)db & 3) || ((uintptr_t)objective & 3))
    return CCLIP_ERR_ARG;
  char* ws = (char*)workspace;
  pair_image_launch(W, C, D, workspace, stream);
  ProbeBwdArgs a;
  a.x = (const bf16*)x; a.img = (const bf16*)workspace; a.ldx = ldx;
  a.N = (int)N; a.C = C; a.D = D; a.cpad = g.cpad;
  a.bias = bias; a.labels = labels; a.rw = row_weight; a.lse = lse;
  a.tpp = g.tpp; a.ntiles = g.ntiles; a.rs = g.rs; a.cbw = g.cbw;
  a.part = (float*)(ws + g.off_part); a.dbpart = (float*)(ws + g.off_db);
  int st;
  if (D <= 128) st = probe_bwd_launch<4, 1, true>(a, g, stream);
  else if (D <= 512) st = probe_bwd_launch<16, 1, true>(a, g, stream);
  else st = probe_bwd_launch<32, 4, false>(a, g, stream);
  if (st != CCLIP_OK) return st;
  ProbeMergeArgs m;
  m.W = W; m.part = a.part; m.dbpart = a.dbpart; m.loss = loss;
  m.N = (int)N; m.C = C; m.D = D; m.cpad = g.cpad; m.slots = g.slots; m.wblocks = g.wblocks;
  m.scale = scale; m.l2 = l2; m.dW = dW; m.db = db; m.red = (float*)(ws + g.off_red);
  hipLaunchKernelGGL(probe_merge_kernel, dim3((unsigned)(g.wblocks + (loss ? PROBE_LOSS_BLOCKS : 0))), dim3(256), 0, stream, m);
  if (objective)
    hipLaunchKernelGGL(probe_objective_kernel, dim3(1), dim3(256), 0, stream, (const float*)m.red, g.wblocks, scale, l2, objective);
  return cclip_launch_status();
}
