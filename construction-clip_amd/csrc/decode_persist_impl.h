// What the two persistent KV-cached beam-search kernels share: decode_persist.hip (one caption, GEMV projections) and
// decode_persist_batch.hip (up to 64 rows, MFMA projections).  The phase hand-over, the decode attention task, the per-slice
// selection partials, the selection proper and the host side's descriptor checks, grid choice and launch live here once; each
// .hip keeps its argument struct, its projection engine, its lm_head phase, its kernel and its entry point.
#pragma once
#include "gemm_skinny_impl.h"

namespace CCLIP_NS {

constexpr int DECODE_MAXL = 24;    // layers
constexpr int DECODE_PS = 20;      // floats per (caption, workgroup, beam) selection partial: max, sum, 8 x (value, index) + pad
constexpr int DECODE_MAXR = 256;   // vocabulary rows per workgroup slice (4 per lane in the local top-k)

// ---- phase hand-over --------------------------------------------------------------------------------------------------
// One monotonic counter.  A phase's PRODUCERS (the workgroups that had a column block / task / slice in it) add 1 when their
// part is written; every workgroup keeps the same running total of producers (`target`), and a workgroup waits for that total
// only when it is about to work in the next phase.  Idle workgroups neither add nor poll: with 24-96 of 256 workgroups active
// in a projection phase, a full barrier's 256 serialized atomics and 256 pollers were most of its 2-5 us.
// (The phase's hand-over buffers are written with write-through sc1 stores and read with sc1 loads - st_coh / ld_coh - so no
// cache-wide write-back / invalidate is needed: a release + acquire fence pair per workgroup per phase cost ~30 us per phase.)
struct PhaseSync {
  int* counter; int* err; int target; bool dead;
  // end of a phase that `nprod` workgroups worked in; `worked`: this workgroup was one of them
  __device__ __forceinline__ void arrive(int nprod, bool worked) {
    __syncthreads();                                               // every wave's stores of the phase are out (vmcnt(0) + barrier)
    target += nprod;
    if (worked && !dead && threadIdx.x == 0) __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // before reading what the phases so far produced
  __device__ __forceinline__ void wait() {
    if (!dead && threadIdx.x == 0) {
      int spins = 0;
      while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 23) || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
          __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
    __syncthreads();
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) dead = true;   // uniform per workgroup: read after the barrier
  }
};

// the fields of one caption that the selection reads and writes: rows of x / tokens / scores / seq_len / stopped are the
// caption's beams, slot_of its [max_len][8] slot table, part its [G][8][DECODE_PS] partials, state its bookkeeping words
// ([2] stopped, [3] selections made by then, [4] token columns)
struct CapView {
  int nb, V, D, pos0, max_len, ld_tokens, stop_token;
  const float* wte32; const float* wpe32;
  float* x; int* slot_of; int* tokens; float* scores; float* seq_len; int* stopped; int* state; float* part;
};

// ---- decode attention for one (row, head) by one wave; p_l: S floats, ro_l: S row offsets, q_l: 64 floats of this wave -----
// `row`: the row of q / out; `slot`: its caption's slot table, `b` its beam in it; `sbase`: the caption's first cache slot.
// Memory round trips are what this phase costs, so they are kept to two: the slot table of every key (one batch), then ALL key
// rows and value rows of a 128-key chunk in flight together (S <= 128 is one chunk - the caption lengths of this path).
__device__ __forceinline__ void attn_task(const int* slot, int sbase, int nb, long ld_seq, int D, const bf16* q, long ldq, const bf16* kc,
                                          const bf16* vc, bf16* out, long ldo, int row, int b, int h, int S, bool valid, float* p_l,
                                          int* ro_l, float* q_l) {
  const int lane = threadIdx.x & 63;
  for (int k0 = 0; k0 < S; k0 += 256) {                           // row offsets: cache slot of (position, beam) from the slot table
    int sl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int key = k0 + lane + 64 * u; sl[u] = ld_coh<true>(slot + (long)(key < S ? key : S - 1) * 8 + b); }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = k0 + lane + 64 * u;
      const int v = sl[u] < 0 ? 0 : (sl[u] >= nb ? nb - 1 : sl[u]);
      if (key < S) ro_l[key] = (int)((long)(sbase + v) * ld_seq + (long)key * D + h * 64);
    }
  }
  q_l[lane] = (float)ld_coh<true>(q + (long)row * ldq + h * 64 + lane);
  __syncthreads();
  const int c = lane & 7, kg = lane >> 3;
  float m = -__builtin_inff(), l = 0.f;
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;
  for (int c0 = 0; c0 < S; c0 += 128) {                           // online softmax over 128-key chunks
    bf16x8 kv[2][8], vv[4][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = c0 + lane + 64 * t;
      const bf16* kr = kc + ro_l[key < S ? key : S - 1];
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) kv[t][cc] = ld_coh<true>((const bf16x8*)(kr + 8 * cc));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int key = c0 + 32 * t + 8 * u + kg;
        vv[t][u] = ld_coh<true>((const bf16x8*)(vc + ro_l[key < S ? key : S - 1] + 8 * c));
      }
    float sc[2], cm = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = c0 + lane + 64 * t;
      float acc = 0.f;
#pragma unroll
      for (int cc = 0; cc < 8; ++cc)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += q_l[8 * cc + j] * (float)kv[t][cc][j];
      sc[t] = key < S ? acc * 0.125f : -__builtin_inff();
      cm = fmaxf(cm, sc[t]);
    }
    cm = wave_max(cm);
    const float mn = fmaxf(m, cm);
    const float resc = __expf(m - mn);                              // (first chunk: exp(-inf) = 0 on l = 0, o = 0)
    float cl = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = c0 + lane + 64 * t;
      const float e = key < S ? __expf(sc[t] - mn) : 0.f;
      p_l[lane + 64 * t] = e;
      cl += e;
    }
    l = l * resc + wave_sum(cl);
    m = mn;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= resc;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float w = p_l[32 * t + 8 * u + kg];                   // 0 for keys past S
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += w * (float)vv[t][u][j];
      }
    __syncthreads();
  }
  const float inv = 1.0f / l;
  bf16x8 ov;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float t = o[j];
    t += __shfl_xor(t, 8, 64);
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    ov[j] = (bf16)(t * inv);
  }
  if (valid && kg == 0) st_coh<true>((bf16x8*)(out + (long)row * ldo + h * 64 + 8 * c), ov);
  __syncthreads();
}

// ---- per-row partials of one vocabulary slice (sl: [n_in][DECODE_MAXR] logits of rows r0..r0+nr) --------------------------------
// wave w handles rows w, w+4, ..: slice max and sum-exp of z = logit / T, and the slice's top-k by z (k = nb).  Row m is caption
// m / nb, beam m % nb, or, in the first selection (one row per caption), caption m, beam 0; part: [n_cap][G][8][DECODE_PS]
__device__ __forceinline__ void select_partials(float* part, int nb, const float* sl, int n_in, bool first, int r0, int nr, float T, int G) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = wave; m < n_in; m += 4) {
    float z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = lane + 64 * i;
      z[i] = j < nr ? sl[m * DECODE_MAXR + j] / T : -__builtin_inff();
    }
    float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += (lane + 64 * i < nr) ? expf(z[i] - mx) : 0.f;
    s = wave_sum(s);
    const int c = first ? m : m / nb, b = first ? 0 : m % nb;
    float* pp = part + (((long)c * G + blockIdx.x) * 8 + b) * DECODE_PS;
    if (lane == 0) { st_coh<true>(pp, nr > 0 ? mx : -__builtin_inff()); st_coh<true>(pp + 1, nr > 0 ? s : 0.f); }
    for (int r = 0; r < nb; ++r) {                                  // k rounds of wave arg-max (ties: the lower row first)
      float bv = z[0]; int bi = lane;
#pragma unroll
      for (int i = 1; i < 4; ++i) if (z[i] > bv) { bv = z[i]; bi = lane + 64 * i; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { st_coh<true>(pp + 2 + 2 * r, bv); st_coh<true>((int*)pp + 3 + 2 * r, r0 + bi); }
#pragma unroll
      for (int i = 0; i < 4; ++i) if (lane + 64 * i == bi) z[i] = -__builtin_inff();
    }
  }
}

// ---- the selection proper of one caption, by one workgroup (256 threads); lds: 64 + 512 + 4096 + 2 * n_in*G*k floats ----------
// The arithmetic of the reference's generate_beam loop body, restated: temperature / log-softmax / stopped-beam rule /
// length-normalised top-k, token append, beam reorder (a permutation of the slot table), next input embedding.
template <int MCAP>
__device__ __forceinline__ void select_merge(const CapView& a, int n_in, bool first, int it, int cur_pos, int G, int ntok, float* lds) {
  const int tid = threadIdx.x;
  const int nb = a.nb, k = a.nb;
  float* bM = lds;            // [8] global max per beam
  float* bS = lds + 8;        // [8] global sum per beam
  float* o_sc = lds + 16;     // [8] scores, [8] current lengths, [8] stopped (old beams)
  float* o_len = lds + 24;
  int* o_st = (int*)(lds + 32);
  float* w_avg = lds + 40;    // [8] winners
  int* w_flat = (int*)(lds + 48);
  float* red_v = lds + 64;    // [256] reduction scratch
  int* red_i = (int*)(lds + 64 + 256);
  float* stat = lds + 64 + 512;          // [8][256 max | 256 sum] slice statistics
  float* cav = stat + 4096;              // candidate averages [n_in * G * k]
  int* cfl = (int*)(cav + n_in * G * k); // candidate flat indices
  // per-beam softmax statistics from the workgroups' slice partials: thread g fetches slice g's (max, sum) of every beam (all
  // loads in flight), the reduction runs out of LDS in slice order (deterministic).  A serial loop over the slices is one
  // memory round trip per slice: 2 x 256 of them were 0.8 ms of a 1.4 ms step.
  {
    float pm[8], ps[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float* pp = a.part + ((long)(tid < G ? tid : 0) * 8 + (m < n_in ? m : 0)) * DECODE_PS;
      pm[m] = ld_coh<true>(pp); ps[m] = ld_coh<true>(pp + 1);
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) { stat[m * 512 + tid] = tid < G ? pm[m] : -__builtin_inff(); stat[m * 512 + 256 + tid] = tid < G ? ps[m] : 0.f; }
  }
  __syncthreads();
  {
    // block max / sum by wave shuffles + the four waves' results through LDS (fixed order: reproducible)
    const int lane = tid & 63, wave = tid >> 6;
    float wm[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) wm[m] = wave_max(stat[m * 512 + tid]);
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < 8; ++m) red_v[wave * 8 + m] = wm[m];
    }
    __syncthreads();
    if (tid < 8) bM[tid] = fmaxf(fmaxf(red_v[tid], red_v[8 + tid]), fmaxf(red_v[16 + tid], red_v[24 + tid]));
    __syncthreads();
    float ws[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float sg = stat[m * 512 + 256 + tid];
      ws[m] = wave_sum(sg > 0.f ? sg * expf(stat[m * 512 + tid] - bM[m]) : 0.f);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < 8; ++m) red_v[wave * 8 + m] = ws[m];
    }
    __syncthreads();
  }
  if (tid < 8) {
    const int m = tid;
    if (m < n_in) {
      bS[m] = ((red_v[m] + red_v[8 + m]) + red_v[16 + m]) + red_v[24 + m];
      const bool st = first ? false : a.stopped[m] != 0;
      o_st[m] = st ? 1 : 0;
      o_sc[m] = first ? 0.f : a.scores[m];
      o_len[m] = first ? 1.f : a.seq_len[m] + (st ? 0.f : 1.f);    // seq_lengths[~is_stopped] += 1 (not in the first selection)
    }
  }
  __syncthreads();
  const int C = n_in * G * k;
  for (int c0 = tid; c0 < C; c0 += 2304) {                          // candidates: nine per thread in flight
    float zz[9]; int tk[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int c = c0 + 256 * u < C ? c0 + 256 * u : C - 1;
      const int r = c % k, g = (c / k) % G, m = c / (k * G);
      const float* pp = a.part + ((long)g * 8 + m) * DECODE_PS;
      zz[u] = ld_coh<true>(pp + 2 + 2 * r);
      tk[u] = ld_coh<true>((const int*)pp + 3 + 2 * r);
    }
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int c = c0 + 256 * u;
      if (c >= C) continue;
      const int r = c % k, g = (c / k) % G, m = c / (k * G);
      const float z = zz[u];
      const int tok = tk[u];
      float avg = -__builtin_inff();
      int flat = 0x7fffffff;
      if (o_st[m]) {                                                // logits[is_stopped] = -inf; logits[is_stopped, 0] = 0
        if (g == 0 && r == 0) { avg = (o_sc[m] + 0.f) / o_len[m]; flat = m * a.V; }
      } else if (z > -__builtin_inff() && tok >= 0 && tok < a.V) {
        const float pr = expf(z - bM[m]) / bS[m];                   // softmax(-1) ...
        const float lp = logf(pr);                                  // ... .log()
        avg = (o_sc[m] + lp) / o_len[m];
        flat = m * a.V + tok;
      }
      cav[c] = avg; cfl[c] = flat;
    }
  }
  __syncthreads();
  for (int r = 0; r < k; ++r) {                                     // top-k of the flattened [beams x V] averages, best first
    float bv = -__builtin_inff(); int bc = -1, bf = 0x7fffffff;
    for (int c = tid; c < C; c += 256) {
      const float v = cav[c]; const int f = cfl[c];
      if (f != 0x7fffffff && (bc < 0 || v > bv || (v == bv && f < bf))) { bv = v; bc = c; bf = f; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                              // wave arg-max: larger average, then the lower flat index
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64), of = __shfl_xor(bf, o, 64);
      if (oc >= 0 && (bc < 0 || ov > bv || (ov == bv && of < bf))) { bv = ov; bc = oc; bf = of; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bc; red_i[4 + (tid >> 6)] = bf; }
    __syncthreads();
    if (tid == 0) {
      float v0 = -__builtin_inff(); int c0 = -1, f0 = 0x7fffffff;
      for (int t = 0; t < 4; ++t) {
        const int cc = red_i[t];
        if (cc < 0) continue;
        const float v = red_v[t]; const int f = red_i[4 + t];
        if (c0 < 0 || v > v0 || (v == v0 && f < f0)) { v0 = v; c0 = cc; f0 = f; }
      }
      w_avg[r] = v0; w_flat[r] = c0 >= 0 ? f0 : 0;
      if (c0 >= 0) cfl[c0] = 0x7fffffff;
    }
    __syncthreads();
  }
  // bookkeeping: everything below reads the OLD beam state from LDS / registers before it writes the new one
  int src[8], tok[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int f = i < k ? w_flat[i] : 0;
    src[i] = f / a.V; tok[i] = f % a.V;
    if (src[i] >= n_in) src[i] = n_in - 1;
  }
  // every load of the bookkeeping goes out first (token rows, slot-table rows, embedding rows: unconditional, clamped
  // addresses), then the stores: issued phase by phase this was ~8 dependent memory round trips
  const int next_pos = first ? a.pos0 : cur_pos + 1;
  const bool has_next = next_pos < a.max_len;
  int told[MCAP], sold[MCAP];
  float e[MCAP][4], pe[4];
  {
    const int j = tid < ntok ? tid : 0;
#pragma unroll
    for (int m = 0; m < MCAP; ++m) told[m] = a.tokens[(long)(m < n_in ? m : 0) * a.ld_tokens + j];
    const int t = tid <= cur_pos ? tid : 0;
#pragma unroll
    for (int m = 0; m < MCAP; ++m) sold[m] = ld_coh<true>(a.slot_of + (long)(t < 0 ? 0 : t) * 8 + m);
    const int np = has_next ? next_pos : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int d = tid + 256 * u < a.D ? tid + 256 * u : 0;
      pe[u] = a.wpe32[(long)np * a.D + d];
#pragma unroll
      for (int i = 0; i < MCAP; ++i) e[i][u] = a.wte32[(long)tok[i < nb ? i : 0] * a.D + d];
    }
  }
  if (tid < ntok) {                                                 // tokens = cat(tokens[next_tokens_source], next_tokens)
#pragma unroll
    for (int i = 0; i < MCAP; ++i) {
      int v = told[0];
#pragma unroll
      for (int m = 1; m < MCAP; ++m) v = src[i] == m ? told[m] : v;          // (select chain: no dynamically indexed register array)
      if (i < nb) a.tokens[(long)i * a.ld_tokens + tid] = v;
    }
  }
  if (!first && tid <= cur_pos) {                                   // cache reorder = permute the slot table
#pragma unroll
    for (int i = 0; i < MCAP; ++i) {
      int v = sold[0];
#pragma unroll
      for (int m = 1; m < MCAP; ++m) v = src[i] == m ? sold[m] : v;
      if (i < nb) st_coh<true>(a.slot_of + (long)tid * 8 + i, v);
    }
  }
  if (has_next) {
    if (tid < nb) st_coh<true>(a.slot_of + (long)next_pos * 8 + tid, tid);        // the next step appends beam b's row to slot b
#pragma unroll
    for (int i = 0; i < MCAP; ++i)                                  // next input: wte[token] + wpe[position] (D <= 1024: 4 per thread)
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i < nb && tid + 256 * u < a.D) st_coh<true>(a.x + (long)i * a.D + tid + 256 * u, e[i][u] + pe[u]);
  }
  for (int j = tid + 256; j < ntok; j += 256) {                     // (prompts longer than 256 tokens)
    int old[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) old[m] = m < n_in ? a.tokens[(long)m * a.ld_tokens + j] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) if (i < nb) a.tokens[(long)i * a.ld_tokens + j] = old[src[i]];
  }
  if (!first) {
    for (int t = tid + 256; t <= cur_pos; t += 256) {               // (positions past 256)
      int old[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) old[m] = ld_coh<true>(a.slot_of + (long)t * 8 + m);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        int v = old[0];
#pragma unroll
        for (int m = 1; m < 8; ++m) v = src[i] == m ? old[m] : v;
        if (i < nb) st_coh<true>(a.slot_of + (long)t * 8 + i, v);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    bool all = true;
    for (int i = 0; i < nb; ++i) {
      const float len = o_len[src[i]];
      const int st = (o_st[src[i]] != 0) || tok[i] == a.stop_token;
      if (ntok < a.ld_tokens) a.tokens[(long)i * a.ld_tokens + ntok] = tok[i];
      a.seq_len[i] = len;
      a.scores[i] = w_avg[i] * len;                                 // scores = scores_sum_average * seq_lengths
      a.stopped[i] = st;
      all = all && st;
    }
    a.state[4] = ntok + 1;
    if (all && !a.state[2]) { a.state[3] = it + 1; __hip_atomic_store(a.state + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  }
  __syncthreads();
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// what both entry points require of the step descriptor (the row count is checked by each)
static inline bool persist_desc_ok(const cclip_decode_desc& s) {
  if (!s.blocks || !s.x || !s.kcache || !s.vcache || !s.scratch16) return false;
  if (s.n_layer <= 0 || s.n_layer > DECODE_MAXL || s.linear_layout) return false;
  if (s.width <= 0 || (s.width & 63) || s.width > 1024 || s.width != s.heads * 64 || s.hidden <= 0 || (s.hidden & 31) || s.pos < 0) return false;
  if (s.act != CCLIP_ACT_NONE && s.act != CCLIP_ACT_GELU_NEW) return false;
  return s.lnf_w && s.lnf_b && s.wte16 && s.vocab > 0 && !(s.ld_seq & 7) && !(s.ld_layer & 7);
}

// CUs of the current device (cached); 0: the runtime would not say
static inline int persist_cu_count() {
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    n_cu = prop.multiProcessorCount;
  }
  return n_cu;
}

// Grid G and vocabulary rows per workgroup slice R.  At most one workgroup per CU (every workgroup resident: the hand-overs can
// fill), independent of the number of rows.  The projection phases have 24-96 column blocks, so more workgroups than that only
// add pollers at the step boundaries: 96, or as many as the vocabulary slices need (measured on GPT-2-small, V = 21128, one
// caption: 0.685 ms / step with 96 workgroups, 0.727 with 256).  false: vocabulary too large for one slice per workgroup.
static inline bool persist_grid(int vocab, int grid_cap, int n_cu, int* G_out, int* R_out) {
  int G = (vocab + 223) / 224; if (G < 96) G = 96;
  if (G > 256) G = 256;
  if (G > n_cu) G = n_cu;
  if (grid_cap > 0 && grid_cap < G) G = grid_cap;
  int R = (vocab + G - 1) / G; R = (R + 31) / 32 * 32;
  *G_out = G; *R_out = R;
  return R <= DECODE_MAXR;
}

// launch Kernel(a) on G workgroups of 256 threads with lds_bytes of dynamic LDS; the kernel's dynamic-LDS limit is raised only
// when it has to grow (one high-water mark per kernel instantiation)
template <auto Kernel, typename Args>
static int launch_persist(int G, size_t lds_bytes, hipStream_t stream, const Args& a) {
  static size_t attr = 0;
  if (lds_bytes > attr) {
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return CCLIP_ERR_LAUNCH;
    attr = lds_bytes;
  }
  hipLaunchKernelGGL(Kernel, dim3(G), dim3(256), lds_bytes, stream, a);
  return cclip_launch_status();
}

}  // namespace CCLIP_NS
