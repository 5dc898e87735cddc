// What the fp32 one-wave-per-row kernels share (loss.hip, class_loss.hip, sigmoid_loss.hip, distill_loss.hip; embed.hip for the
// grid alone): the wave reductions of a row's running (max, sum, argmax), the online softmax column step, the four-columns-per-
// trip sweep of a row and its companion vector, lane 0's pred / hit epilogue, and on the host the grid, the refusals and the
// launch of a four-rows-per-block grid-stride kernel.
#pragma once
#include "cclip_common.h"

namespace CCLIP_NS {

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// combine the lanes' (max, first index of it) of one row; ties -> smallest index (torch.argmax returns the first max)
__device__ __forceinline__ void wave_argmax(float& m, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const int a2 = __shfl_xor(arg, o, 64);
    if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
  }
}

// combine the lanes' online softmax state (m, s = sum of exp(x - m), arg) of one row; ties -> smallest index
__device__ __forceinline__ void wave_softmax_argmax(float& m, float& s, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const int a2 = __shfl_xor(arg, o, 64);
    const float mn = fmaxf(m, m2);
    s = s * (m == mn ? 1.f : __expf(m - mn)) + s2 * (m2 == mn ? 1.f : __expf(m2 - mn));
    if (m2 > m || (m2 == m && a2 < arg)) arg = a2;
    m = mn;
  }
}

// one column (value v, index c) of a lane's online softmax state: m = running max, s = sum of exp(x - m), arg = first index of
// m; start from m = -inf, s = 0, arg = INT_MAX.  SKIP_NEG_INF keeps v == -inf out of the sum: it adds exp(-inf) = 0 whatever m
// is, but while m is still -inf the unguarded exp(-inf - -inf) is NaN.  kl_rows has the guard (a teacher may mask cells with
// -inf); xent_rows and xent_rows_classes do not, and a lane of theirs whose first column is -inf has a NaN sum.
template <bool SKIP_NEG_INF>
__device__ __forceinline__ void online_softmax_step(float v, int c, float& m, float& s, int& arg) {
  if (v > m) { s = s * __expf(m - v) + 1.f; m = v; arg = c; }
  else if (!SKIP_NEG_INF || !(v == -__builtin_inff())) s += __expf(v - m);
}

// One lane's sweep of a row and its companion vector (a class per column, or a second row): f(row[c], aux[c], c) for
// c = lane, lane + 64, ... in that order.  Four columns per trip, all eight loads issued before the first use: at one wave per
// SIMD (R = 1024 is four waves per CU) nothing else hides a load's latency, and a companion element fetched only after its
// logit had arrived cost a second one.  A one-column tail follows.  aux is read through L2 with row's coalesced index.
template <typename AUX, typename F>
__device__ __forceinline__ void sweep_row4(const float* row, const AUX* aux, int lane, int C, F&& f) {
  int c = lane;
  for (; c + 192 < C; c += 256) {
    const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
    const AUX a0 = aux[c], a1 = aux[c + 64], a2 = aux[c + 128], a3 = aux[c + 192];
    f(v0, a0, c); f(v1, a1, c + 64); f(v2, a2, c + 128); f(v3, a3, c + 192);
  }
  for (; c < C; c += 64) f(row[c], aux[c], c);
}

// The same sweep where f returns the cell's gradient, stored to drow[c] when STORE.  drow may be row (clip/loss.py overwrites
// the logits with their gradient in place), so neither the kernels' `logits` nor their `dlogits` carries __restrict__: every
// element is read by the lane that later writes it, before that store, and a trip's four stores follow its four cells.  What a
// kernel needs of the whole row (its softmax statistics, the positives' sum, a label's logit) it takes before this sweep.
template <bool STORE, typename AUX, typename F>
__device__ __forceinline__ void sweep_row4_store(const float* row, const AUX* aux, float* drow, int lane, int C, F&& f) {
  int c = lane;
  for (; c + 192 < C; c += 256) {
    const float v0 = row[c], v1 = row[c + 64], v2 = row[c + 128], v3 = row[c + 192];
    const AUX a0 = aux[c], a1 = aux[c + 64], a2 = aux[c + 128], a3 = aux[c + 192];
    const float d0 = f(v0, a0, c), d1 = f(v1, a1, c + 64), d2 = f(v2, a2, c + 128), d3 = f(v3, a3, c + 192);
    if (STORE) { drow[c] = d0; drow[c + 64] = d1; drow[c + 128] = d2; drow[c + 192] = d3; }
  }
  for (; c < C; c += 64) {
    const float d = f(row[c], aux[c], c);
    if (STORE) drow[c] = d;
  }
}

// row r's outputs after the wave's argmax, for lane 0 to call: pred = arg, and hit = 1 when the row has a maximum and match()
// holds for it, else 0.  arg >= C is a row without a maximum (all NaN); match() is not called for it, so it may index by arg.
// Give match its values by copy ([=]): with col_class captured by reference the compiler formed the sweep's addresses anew in
// every trip (two 64-bit adds in front of the loads), which cost xent_rows_classes 1 - 1.5 % at C = 8192
// (profiles/row_loss_refactor_ab.txt).
template <typename MATCH>
__device__ __forceinline__ void store_pred_hit(int r, int arg, int C, int* pred, float* hit, MATCH&& match) {
  if (pred) pred[r] = arg;
  if (hit) hit[r] = (arg < C && match()) ? 1.f : 0.f;
}

}  // namespace CCLIP_NS

// blocks of a launch in which each of a block's four waves strides over the rows
static inline int grid_rows4(int rows) { int g = (rows + 3) / 4; return g > 4096 ? 4096 : (g < 1 ? 1 : g); }

// what every class / teacher row loss refuses: no logits, an empty shape, a row stride shorter than the row
static inline bool row_loss_shape_ok(const void* logits, int R, int C, long ld, const void* dlogits, long ldd) {
  return logits && R > 0 && C > 0 && ld >= C && !(dlogits && ldd < C);
}

// launch such a kernel (256 threads, no LDS) over `rows` rows; the status of the launch
template <typename... P, typename... A>
static inline int launch_rows4(void (*kernel)(P...), int rows, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_rows4(rows)), dim3(256), 0, stream, args...);
  return cclip_launch_status();
}
