// Agreement of two label maps: pred and gt uint8 [B][H][W] -> the confusion counts behind mean IoU and the boundary-band counts
// behind boundary IoU (Cheng et al., "Boundary IoU: Improving Object-Centric Image Segmentation Evaluation", CVPR 2021), stated
// from the paper's definition (include/cclip_hip.h holds the contract; no other implementation was compared).  Integers only:
// every output is a sum of ones, so two calls give equal bytes whatever order the atomics land in.
//
//   confusion [R][C][C+1]  gt == g < C against pred == p (column C: pred == 255, "none"); gt == 255 is ignored everywhere
//   bad       [R][2]       gt in [C, 254]; gt valid and pred in [C, 254] - such pixels enter no other count
//   bands     [R][C][3]    |G_c|, |P_c|, |G_c n P_c| with the band half-width d (only for d > 0)
//
// A pixel is in the band of a map when its (2d+1)^2 window leaves the image or holds a byte other than its own.
//
// Tiles.  A work-group of 1024 threads owns a 64 x 64 tile of one image; a thread owns four consecutive pixels of a row (the
// ownership of label_pixels.h).  With d > 0 both maps are staged as bytes in LDS with a halo of d: (64 + 2d)^2 <= 128 x 128
// cells a map.  A halo cell holds the value at its CLAMPED coordinates (dense_refine.hip's idiom), so no inner loop has a bounds
// test; the image border is arithmetic: a pixel closer than d to an edge is in the band of both maps, whatever its window holds.
// "All equal in the window" is separable.  The row pass writes, per staged row and tile column, one dword that packs for each
// map the centre byte and a bit "the row window [x - d, x + d] holds this byte only"; the column pass asks whether the 2d + 1
// dwords above and below a pixel all equal the pixel's own dword with the bit set (one compare per map and row; the dword is
// the minimum / maximum pair of the row window in a cheaper form: min == max == centre, or "no").
//
// Counts.  Each thread first merges equal keys among its four pixels.  While C (C + 1) <= LA_HIST_CELLS the confusion counts go
// into an LDS histogram by 32-bit LDS atomics (a tile holds 4096 pixels: no overflow) and the group flushes the non-zero cells
// with 64-bit global atomics; above that the lanes of a wave that hold the same key are combined by shuffles and one lane
// issues the global atomic (lc_stats_kernel's combine): a photo that is all one class sends one atomic per wave, not per pixel.
// The 3 C band counters and the two bad counters are always in LDS.  Global atomics are relaxed, agent scope, integer.
// accumulate == 0 zeroes the outputs in a launch of its own first; no kernel waits for another work-group.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#define LA_TILE 64                                          // tile side in pixels
#define LA_QUAD 4                                           // consecutive pixels per thread
#define LA_THREADS (LA_TILE * LA_TILE / LA_QUAD)            // 1024
#define LA_MAX_BAND CCLIP_AGREEMENT_MAX_BAND                // 32
#define LA_SIDE (LA_TILE + 2 * LA_MAX_BAND)                 // 128: the largest staged side
#define LA_HIST_CELLS CCLIP_AGREEMENT_HIST_CELLS            // confusion cells kept in LDS: C <= 44
#define LA_MAX_C 255
#define LA_ROUNDS 4                                         // keys combined per wave before the rest go out lane by lane
#define LA_NONE 255u

struct la_args {
  const uint8_t* pred; const uint8_t* gt;
  int B, H, W, C, d, per_image;
  int tiles_x, tiles_y;
  unsigned long long* confusion; unsigned long long* bad; unsigned long long* bands;
  long n_conf, n_bad, n_bands;                              // cells of each output
};

__device__ __forceinline__ void la_global_add(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int la_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void la_zero_kernel(const la_args a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_conf) a.confusion[i] = 0ull;
  if (i < a.n_bad) a.bad[i] = 0ull;
  if (i < a.n_bands) a.bands[i] = 0ull;
}

// the lanes of the wave that hold the same key, combined; all 64 lanes take part in every shuffle (cnt == 0: nothing to add)
__device__ __forceinline__ void la_wave_add(unsigned long long* dst, int key, unsigned cnt, int lane) {
  bool open = cnt > 0u;
  for (int round = 0; round < LA_ROUNDS; ++round) {         // a fixed number of rounds
    const unsigned long long m = __ballot(open);
    if (m == 0ull) break;                                   // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const int k = __shfl(key, lead, 64);
    const bool in = open && key == k;
    unsigned c = in ? cnt : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == lead) la_global_add(dst + k, c);
    if (in) open = false;
  }
  if (open) la_global_add(dst + key, cnt);                  // more keys in the wave than rounds: these go out on their own
}

template <bool BAND, bool LDS_HIST>
__global__ __launch_bounds__(LA_THREADS) void label_agreement_kernel(const la_args a) {
  __shared__ uint8_t sg[BAND ? LA_SIDE * LA_SIDE : 4];      // gt, staged with its halo
  __shared__ uint8_t sp[BAND ? LA_SIDE * LA_SIDE : 4];      // pred
  __shared__ __attribute__((aligned(16))) unsigned rowres[BAND ? LA_SIDE * LA_TILE : 1];   // per staged row and tile column: gt code | pred code << 16
  __shared__ unsigned hist[LDS_HIST ? LA_HIST_CELLS : 1];
  __shared__ unsigned bandc[BAND ? 3 * LA_MAX_C : 1];
  __shared__ unsigned badc[2];

  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned per = (unsigned)(a.tiles_x * a.tiles_y);   // <= 256 * 256
  const int b = (int)(blockIdx.x / per);
  const int rt = (int)(blockIdx.x - (unsigned)b * per);
  const int ty = rt / a.tiles_x;
  const int y0 = ty * LA_TILE, x0 = (rt - ty * a.tiles_x) * LA_TILE;
  const int C = a.C, d = a.d, H = a.H, W = a.W;
  const int cells = C * (C + 1);
  const long plane = (long)H * W;
  const uint8_t* gimg = a.gt + b * plane;
  const uint8_t* pimg = a.pred + b * plane;

  if (LDS_HIST)
    for (int i = tid; i < cells; i += LA_THREADS) hist[i] = 0u;
  if (BAND)
    for (int i = tid; i < 3 * C; i += LA_THREADS) bandc[i] = 0u;
  if (tid < 2) badc[tid] = 0u;

  const int ly = tid >> 4, lx0 = (tid & 15) * LA_QUAD;
  const int y = y0 + ly, x = x0 + lx0;
  const int live = y < H ? (W - x < LA_QUAD ? (W - x < 0 ? 0 : W - x) : LA_QUAD) : 0;   // how many of the four lie in the image
  unsigned g[LA_QUAD], p[LA_QUAD];
  bool ing[LA_QUAD], inp[LA_QUAD];

  if (BAND) {
    const int side = LA_TILE + 2 * d;
    for (int i = tid; i < side * side; i += LA_THREADS) {
      const int sy = i / side, sx = i - sy * side;
      const long at = (long)la_clamp(y0 - d + sy, H - 1) * W + la_clamp(x0 - d + sx, W - 1);
      sg[i] = gimg[at]; sp[i] = pimg[at];
    }
    __syncthreads();
    // row pass: cell (r, cx) looks at staged columns cx .. cx + 2d of staged row r; its centre is column cx + d
    for (int i = tid; i < side * LA_TILE; i += LA_THREADS) {
      const int r = i >> 6, cx = i & (LA_TILE - 1);
      const uint8_t* rg = sg + r * side + cx;
      const uint8_t* rp = sp + r * side + cx;
      const unsigned cg = rg[d], cp = rp[d];
      bool eg = true, ep = true;
      for (int k = 0; k <= 2 * d; ++k) { eg &= rg[k] == cg; ep &= rp[k] == cp; }
      rowres[i] = (cg | (eg ? 256u : 0u)) | ((cp | (ep ? 256u : 0u)) << 16);
    }
    __syncthreads();
    // column pass: staged rows ly .. ly + 2d of the thread's four columns; its own row is ly + d
    const unsigned* col = rowres + ly * LA_TILE + lx0;
    const uint4 own = *(const uint4*)(col + d * LA_TILE);
    const unsigned o[LA_QUAD] = {own.x, own.y, own.z, own.w};
    bool flatg[LA_QUAD], flatp[LA_QUAD];
#pragma unroll
    for (int k = 0; k < LA_QUAD; ++k) {
      g[k] = o[k] & 255u; p[k] = (o[k] >> 16) & 255u;
      flatg[k] = true; flatp[k] = true;
    }
    for (int r = 0; r <= 2 * d; ++r) {
      const uint4 v4 = *(const uint4*)(col + r * LA_TILE);
      const unsigned v[LA_QUAD] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int k = 0; k < LA_QUAD; ++k) {
        flatg[k] &= (v[k] & 0xffffu) == (g[k] | 256u);
        flatp[k] &= (v[k] >> 16) == (p[k] | 256u);
      }
    }
    const bool edge_y = y < d || y + d > H - 1;
#pragma unroll
    for (int k = 0; k < LA_QUAD; ++k) {
      const bool edge = edge_y || x + k < d || x + k + d > W - 1;      // the window leaves the image
      ing[k] = edge || !flatg[k];
      inp[k] = edge || !flatp[k];
    }
  } else {
    __syncthreads();                                        // the counters are zero
    const uint8_t* gp = gimg + (long)y * W + x;
    const uint8_t* pp = pimg + (long)y * W + x;
#pragma unroll
    for (int k = 0; k < LA_QUAD; ++k) {
      g[k] = k < live ? gp[k] : LA_NONE; p[k] = k < live ? pp[k] : LA_NONE;
      ing[k] = false; inp[k] = false;
    }
  }

  // the four pixels' keys, equal neighbours merged: key < 0 means "enters no confusion cell"
  int key[LA_QUAD];
  unsigned cnt[LA_QUAD];
  unsigned bad_g = 0u, bad_p = 0u;
#pragma unroll
  for (int k = 0; k < LA_QUAD; ++k) {
    key[k] = -1; cnt[k] = 0u;
    if (k >= live || g[k] == LA_NONE) continue;
    if (g[k] >= (unsigned)C) { ++bad_g; continue; }
    if (p[k] >= (unsigned)C && p[k] != LA_NONE) { ++bad_p; continue; }
    const int pc = p[k] == LA_NONE ? C : (int)p[k];
    key[k] = (int)g[k] * (C + 1) + pc; cnt[k] = 1u;
    if (BAND) {
      if (ing[k]) atomicAdd(bandc + 3 * g[k], 1u);
      if (pc < C && inp[k]) atomicAdd(bandc + 3 * pc + 1, 1u);
      if (pc == (int)g[k] && ing[k] && inp[k]) atomicAdd(bandc + 3 * pc + 2, 1u);
    }
  }
#pragma unroll
  for (int k = 1; k < LA_QUAD; ++k)                         // a run of equal keys ends up in its last pixel
    if (key[k] >= 0 && key[k] == key[k - 1]) { cnt[k] += cnt[k - 1]; cnt[k - 1] = 0u; }
  if (bad_g) atomicAdd(badc + 0, bad_g);
  if (bad_p) atomicAdd(badc + 1, bad_p);

  const int rr = a.per_image ? b : 0;
  unsigned long long* conf = a.confusion + (long)rr * cells;
  if (LDS_HIST) {
#pragma unroll
    for (int k = 0; k < LA_QUAD; ++k)
      if (cnt[k]) atomicAdd(hist + key[k], cnt[k]);
  } else {
#pragma unroll
    for (int k = 0; k < LA_QUAD; ++k) la_wave_add(conf, key[k] < 0 ? 0 : key[k], cnt[k], lane);
  }
  __syncthreads();

  if (LDS_HIST) {
    for (int i = tid; i < cells; i += LA_THREADS) {
      const unsigned v = hist[i];
      if (v) la_global_add(conf + i, v);
    }
  }
  if (BAND) {
    unsigned long long* bands = a.bands + (long)rr * 3 * C;
    for (int i = tid; i < 3 * C; i += LA_THREADS) {
      const unsigned v = bandc[i];
      if (v) la_global_add(bands + i, v);
    }
  }
  if (tid < 2 && badc[tid]) la_global_add(a.bad + 2 * rr + tid, badc[tid]);
}

static bool la_overlap(const void* p, uint64_t np, const void* q, uint64_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + nq && b < a + np;
}

extern "C" int cclip_label_agreement(const uint8_t* pred, const uint8_t* gt, int32_t B, int32_t H, int32_t W, int32_t C, int32_t band,
                                     int32_t per_image, int32_t accumulate, int64_t* confusion, int64_t* bad, int64_t* bands,
                                     hipStream_t stream) {
  if (!pred || !gt || !confusion || !bad) return CCLIP_ERR_ARG;
  if (C < 1 || C > LA_MAX_C || band < 0 || band > LA_MAX_BAND || (band > 0) != (bands != nullptr)) return CCLIP_ERR_ARG;
  if ((per_image != 0 && per_image != 1) || (accumulate != 0 && accumulate != 1)) return CCLIP_ERR_ARG;
  if (B < 1 || H < 1 || H > CCLIP_OVERLAY_MAX_SIDE || W < 1 || W > CCLIP_OVERLAY_MAX_SIDE || (int64_t)B * H * W > 0x7fffffffLL)
    return CCLIP_ERR_ARG;
  if (((uintptr_t)confusion | (uintptr_t)bad | (uintptr_t)bands) & 7) return CCLIP_ERR_ARG;
  la_args a;
  const int64_t R = per_image ? B : 1;
  a.n_conf = R * C * (C + 1); a.n_bad = R * 2; a.n_bands = bands ? R * C * 3 : 0;
  const uint64_t npix = (uint64_t)B * H * W;
  const void* ptr[5] = {pred, gt, confusion, bad, bands};
  const uint64_t len[5] = {npix, npix, (uint64_t)a.n_conf * 8, (uint64_t)a.n_bad * 8, (uint64_t)a.n_bands * 8};
  for (int i = 2; i < 5; ++i)                               // an output against the inputs and the outputs before it
    for (int j = 0; j < i; ++j)
      if (la_overlap(ptr[i], len[i], ptr[j], len[j])) return CCLIP_ERR_ARG;
  a.pred = pred; a.gt = gt; a.B = B; a.H = H; a.W = W; a.C = C; a.d = band; a.per_image = per_image;
  a.confusion = (unsigned long long*)confusion; a.bad = (unsigned long long*)bad; a.bands = (unsigned long long*)bands;
  a.tiles_x = (W + LA_TILE - 1) / LA_TILE;
  a.tiles_y = (H + LA_TILE - 1) / LA_TILE;
  if (!accumulate) {
    const long most = a.n_conf > a.n_bands ? a.n_conf : a.n_bands;       // n_conf >= 2 >= n_bad / R
    hipLaunchKernelGGL(la_zero_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, stream, a);
  }
  const dim3 grid((unsigned)B * (unsigned)(a.tiles_x * a.tiles_y)), block(LA_THREADS);   // <= B H W <= 2^31 - 1
  const bool lds_hist = C * (C + 1) <= LA_HIST_CELLS;
  if (band > 0) {
    if (lds_hist) hipLaunchKernelGGL((label_agreement_kernel<true, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((label_agreement_kernel<true, false>), grid, block, 0, stream, a);
  } else {
    if (lds_hist) hipLaunchKernelGGL((label_agreement_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((label_agreement_kernel<false, false>), grid, block, 0, stream, a);
  }
  return cclip_launch_status();
}
