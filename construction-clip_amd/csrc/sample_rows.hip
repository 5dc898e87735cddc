// Row sampling for gfx950: one launch draws one token per row of an fp32 logits matrix [n, V] (row stride ld >= V) under a
// temperature, a top-k and a nucleus (top-p) filter.  It replaces softmax -> sort -> cumsum -> mask -> renormalise ->
// multinomial of a host-side sampler by one kernel; the row is read a fixed six times (84 KB at V = 21128: it sits in L2).
//
// Semantics (tests/sample_ref.py restates this text in float64).  For a row x[0 .. V-1] that is not done:
//   p        = softmax(x * inv_temperature).
//   order    : the tokens by (logit descending, id ascending), comparing the fp32 logits themselves (-0 == +0).
//   top-k    : keeps the first k tokens of that order (top_k == 0 or top_k >= V: all of them).
//   top-p    : among those, a token is kept if and only if the mass of the tokens STRICTLY AHEAD of it is <= top_p (the
//              reference's filter: sort, cumsum, `> top_p`, shift right by one, first never removed).  top_p == 1: off.
//   n_kept   = the size of the kept set (a prefix of the order);  kept_mass = Z = the sum of p over it.
//   draw     : walk the kept tokens in ascending id order; the token is the first whose running kept mass exceeds u * Z
//              (u is clamped into [0, 1 - 2^-24]).
//   logprob  = log p[token], of the full temperature-scaled softmax, not the renormalised one.
//   done     : a row with done[r] != 0 emits token 0, logprob 0, n_kept 0, kept_mass 0 and leaves done[r] alone; otherwise
//              done[r] becomes 1 when the token equals stop_token.
//   -inf logits are legal: p is 0 and such a token is never drawn while a finite logit exists.  A row with a NaN, a +inf or no
//   finite logit is UNDEFINED: the kernel stays inside its buffers and emits some token in [0, V), nothing more is promised.
//
// Masses are integers.  With m = max x and d_i = (x_i - m) * inv_temperature, e_i = exp(d_i) in (0, 1] and the mass of token i
// is q_i = trunc(e_i * 2^40), at least 1 where e_i > 0 (so "p > 0" and "mass > 0" are the same tokens).  Every mass in the
// text above is a sum of q_i in a 64-bit integer (Q = sum of all q_i < 2^57), p_i = q_i / Q.  Integer addition is associative:
// the histograms below are filled with LDS integer atomics and still come out the same whatever order the lanes arrive in.
// There is no floating-point sum and no floating-point atomic anywhere in the kernel, so two launches agree bit for bit, and
// a row's outputs do not depend on n or on where the row sits.  The quantisation costs at most one unit per token:
// V * 2^-40 <= 6e-8 of the largest term on any mass; fp32 exp adds a relative 1e-6 per term.
//
// Selection is a radix select on the 48-bit key (monotone image of the logit bits << 16) | (65535 - id), whose descending
// order IS the order above.  Four levels of 12 bits; at each level the tokens whose key matches the digits found so far add
// (1, q_i) to the (count, mass) of their bin, and one scan of the 4096 bins from the top finds the bin holding the LAST kept
// token: the first bin at whose end the running count reaches min(k, V) or the running mass exceeds top_p * Q.  (The token at
// which the inclusive mass first exceeds top_p * Q is kept - the mass ahead of it does not exceed it - and the next is not.)
// After the fourth level the bin holds that one token; its key T, n_kept and Z are known.  The draw is the same machinery in
// id order: kept tokens (key >= T) add q_i to the mass of their 16-id segment, one ascending scan finds the segment in which
// the running mass passes floor(u * Z), one thread walks its 16 tokens.
//
// One 256-thread work-group per row; passes over the row: max, four levels, draw.  48 KB of LDS, no global scratch, no
// workspace, every loop bound known at launch.
#include "score_key.h"
#include "../../include/cclip_hip.h"

#define SR_BINS 4096                              // bins of a radix level (12 bits) = segments of the draw
#define SR_PER 16                                 // bins a thread scans (SR_BINS / 256) = ids per segment
#define SR_MAX_V 65536                            // ids fit the low 16 bits of the key; V / SR_PER <= SR_BINS

namespace CCLIP_NS {

typedef unsigned long long u64;

struct SrShared {
  u64 mass[SR_BINS];
  unsigned cnt[SR_BINS];
  u64 wave_m[4];
  unsigned wave_c[4];
  float wave_x[4];
  // what a scan found: the bin, the (count, mass) ahead of it and the bin's own mass
  int bin;
  unsigned cnt_excl;
  u64 mass_excl, bin_mass;
};

__device__ __forceinline__ u64 sr_key(float x, int id) { return ((u64)mono_bits(x) << 16) | (unsigned)(0xffff - id); }

__device__ __forceinline__ u64 sr_mass(float x, float xmax, float inv_t) {
  const float e = __expf((x - xmax) * inv_t);
  const u64 q = (u64)(e * 0x1p40f);               // e <= 1; NaN and 0 give 0
  return e > 0.0f && q == 0 ? 1ull : q;
}

// f(x, i) for every element of the row, the elements tid, tid + 256, ..: SR_LOADS loads are issued before the first is used
// (one wave per SIMD: nothing else hides a load's latency).  Beyond the row the index is clamped - loaded, not used.
#define SR_LOADS 16
template <class F>
__device__ __forceinline__ void sr_for_row(const float* __restrict__ row, int V, F f) {
  for (int i0 = threadIdx.x; i0 < V; i0 += 256 * SR_LOADS) {
    float x[SR_LOADS];
#pragma unroll
    for (int j = 0; j < SR_LOADS; ++j) x[j] = row[min(i0 + 256 * j, V - 1)];
#pragma unroll
    for (int j = 0; j < SR_LOADS; ++j)
      if (i0 + 256 * j < V) f(x[j], i0 + 256 * j);
  }
}

// One scan over the 4096 (cnt, mass) bins, thread t taking the 16 bins at scan positions 16 t .. 16 t + 15 (descending: position
// p is bin 4095 - p).  Finds the first bin at whose end cnt_base + count >= kk or mass_base + mass > limit and leaves it, with
// the running values ahead of it, in `s`; where no bin does, `s` says bin 0 with the bases.  Clears every bin behind itself.
__device__ __forceinline__ void sr_scan(SrShared& s, bool descending, unsigned cnt_base, u64 mass_base, unsigned kk, u64 limit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { s.bin = 0; s.cnt_excl = cnt_base; s.mass_excl = mass_base; s.bin_mass = 0; }
  unsigned c = 0;
  u64 m = 0;
#pragma unroll
  for (int j = 0; j < SR_PER; ++j) {
    const int pos = SR_PER * tid + j, b = descending ? SR_BINS - 1 - pos : pos;
    c += s.cnt[b];
    m += s.mass[b];
  }
  unsigned ci = c;                                // inclusive scan over the wave, then the waves ahead
  u64 mi = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned c2 = __shfl_up(ci, o, 64);
    const u64 m2 = __shfl_up(mi, o, 64);
    if (lane >= o) { ci += c2; mi += m2; }
  }
  if (lane == 63) { s.wave_c[wave] = ci; s.wave_m[wave] = mi; }
  __syncthreads();
  unsigned cc = cnt_base + ci - c;
  u64 mm = mass_base + mi - m;
  for (int w = 0; w < wave; ++w) { cc += s.wave_c[w]; mm += s.wave_m[w]; }
  bool before = cc >= kk || mm > limit;
#pragma unroll
  for (int j = 0; j < SR_PER; ++j) {
    const int pos = SR_PER * tid + j, b = descending ? SR_BINS - 1 - pos : pos;
    const unsigned cb = s.cnt[b];
    const u64 mb = s.mass[b];
    const bool after = cc + cb >= kk || mm + mb > limit;
    if (!before && after) { s.bin = b; s.cnt_excl = cc; s.mass_excl = mm; s.bin_mass = mb; }   // one thread, one bin
    cc += cb; mm += mb; before = after;
    s.cnt[b] = 0; s.mass[b] = 0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ logits, long ld, int V, float inv_t, int top_k,
                                                          float top_p, const float* __restrict__ u, int stop_token,
                                                          int* __restrict__ done, int* __restrict__ token,
                                                          float* __restrict__ logprob, int* __restrict__ n_kept,
                                                          float* __restrict__ kept_mass) {
  __shared__ SrShared s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long r = blockIdx.x;
  if (done[r] != 0) {                             // (uniform over the work-group)
    if (tid == 0) { token[r] = 0; logprob[r] = 0.0f; n_kept[r] = 0; kept_mass[r] = 0.0f; }
    return;
  }
  const float* row = logits + r * ld;
  for (int b = tid; b < SR_BINS; b += 256) { s.cnt[b] = 0; s.mass[b] = 0; }

  // pass 1: the row's maximum (a maximum does not depend on the order it is taken in; NaN is skipped)
  float xmax = -__builtin_inff();
  sr_for_row(row, V, [&](float x, int) { xmax = fmaxf(xmax, x); });
  xmax = wave_max(xmax);
  if (lane == 0) s.wave_x[wave] = xmax;
  __syncthreads();
  xmax = fmaxf(fmaxf(s.wave_x[0], s.wave_x[1]), fmaxf(s.wave_x[2], s.wave_x[3]));

  // passes 2-5: radix select of the last kept token
  const unsigned kk = top_k <= 0 || top_k > V ? (unsigned)V : (unsigned)top_k;
  u64 prefix = 0, mass_base = 0, limit = ~0ull, Q = 0;
  unsigned cnt_base = 0;
  for (int level = 0; level < 4; ++level) {
    const int shift = 36 - 12 * level;
    sr_for_row(row, V, [&](float x, int i) {
      const u64 key = sr_key(x, i);
      if ((key >> (shift + 12)) == prefix) {
        const int b = (int)(key >> shift) & (SR_BINS - 1);
        atomicAdd(&s.cnt[b], 1u);
        const u64 q = sr_mass(x, xmax, inv_t);
        if (q) atomicAdd(&s.mass[b], q);
      }
    });
    __syncthreads();
    if (level == 0) {                             // Q first: the nucleus limit is a share of it
      u64 m = 0;
      for (int b = tid; b < SR_BINS; b += 256) m += s.mass[b];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
      if (lane == 0) s.wave_m[wave] = m;
      __syncthreads();
      Q = s.wave_m[0] + s.wave_m[1] + s.wave_m[2] + s.wave_m[3];
      limit = top_p >= 1.0f ? ~0ull : (u64)((double)top_p * (double)Q);
      __syncthreads();                            // (wave_m is written again inside the scan)
    }
    sr_scan(s, true, cnt_base, mass_base, kk, limit);
    prefix = (prefix << 12) | (unsigned)s.bin;
    cnt_base = s.cnt_excl;
    mass_base = s.mass_excl;
    if (level == 3) mass_base += s.bin_mass;      // the bin is the last kept token itself
    __syncthreads();                              // everyone has read `s` before the next scan resets it
  }
  const u64 T = prefix, Z = mass_base;
  const unsigned kept = cnt_base + 1;

  // pass 6: the draw, in id order
  const float uu = fminf(fmaxf(u[r], 0.0f), 0x1.fffffep-1f);
  u64 tq = (u64)((double)uu * (double)Z);
  if (Z && tq >= Z) tq = Z - 1;
  sr_for_row(row, V, [&](float x, int i) {
    if (sr_key(x, i) >= T) {
      const u64 q = sr_mass(x, xmax, inv_t);
      if (q) atomicAdd(&s.mass[i / SR_PER], q);
    }
  });
  __syncthreads();
  sr_scan(s, false, 0u, 0ull, ~0u, tq);
  if (tid == 0) {
    u64 run = s.mass_excl;
    const int i0 = s.bin * SR_PER, i1 = min(V, i0 + SR_PER);
    int tok = min(0xffff - (int)(T & 0xffff), V - 1);   // a row without mass (undefined input): the last token of the kept order
    for (int i = i0; i < i1; ++i) {
      const float x = row[i];
      if (sr_key(x, i) < T) continue;
      run += sr_mass(x, xmax, inv_t);
      if (run > tq) { tok = i; break; }
    }
    const float d = (row[tok] - xmax) * inv_t;
    const double logQ = log((double)Q) - 40.0 * 0.693147180559945309417;
    token[r] = tok;
    logprob[r] = (float)((double)d - logQ);
    n_kept[r] = (int)kept;
    kept_mass[r] = (float)((double)Z / (double)Q);
    if (tok == stop_token) done[r] = 1;
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int cclip_sample_rows(const float* logits, int64_t ld, int32_t n, int32_t V, float inv_temperature, int32_t top_k,
                                 float top_p, const float* u, int32_t stop_token, int32_t* done, int32_t* token, float* logprob,
                                 int32_t* n_kept, float* kept_mass, hipStream_t stream) {
  if (!logits || !u || !done || !token || !logprob || !n_kept || !kept_mass) return CCLIP_ERR_ARG;
  if (n <= 0 || V < 1 || V > SR_MAX_V || ld < V) return CCLIP_ERR_ARG;
  if (top_k < 0 || !(top_p > 0.0f && top_p <= 1.0f) || !(inv_temperature > 0.0f) || inv_temperature == __builtin_inff())
    return CCLIP_ERR_ARG;
  static_assert(SR_BINS == 256 * SR_PER && SR_MAX_V <= SR_BINS * SR_PER, "a thread scans SR_PER bins; a segment holds SR_PER ids");
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)n), dim3(256), 0, stream, logits, (long)ld, V, inv_temperature, top_k, top_p,
                     u, stop_token, done, token, logprob, n_kept, kept_mass);
  return cclip_launch_status();
}
