// Connected components of dense label maps: labels uint8 [B][H][W] (255 = none) -> per pixel the component's first pixel (root),
// a dense component number (ids), the number of components (count) and, in a second call, per-component statistics.  Integers
// only; every output is a canonical form, so two calls give equal bytes whatever order the atomics land in.
//
// Two pixels are joined when they lie in the same image, carry the same label other than 255 and are 4-neighbours (or
// 8-neighbours); nothing joins across images, nothing wraps from the end of a row to the start of the next.  With the flat index
// p = (b H + y) W + x, root[p] is the smallest flat index of p's component, ids[p] the rank of root[p] among all roots.
//
// Label equivalence by union-find with "the smaller index wins" (Komura 2015; Playne & Hawick 2018).  A parent never exceeds its
// child, so every walk towards a root moves to strictly smaller indices and a root is its component's first pixel.  What must
// be ordered is ordered by a launch boundary; no kernel waits for another work-group:
//   1 lc_tile_kernel    one 32 x 32 tile per work-group, labelled in LDS (LDS atomicMin); parent[p] = the flat index of the
//                       first pixel of p's component WITHIN the tile.  The parents live in `ids` until launch 5.
//   2 lc_border_kernel  the links that cross a tile border, united by atomicMin on the parents; every other access to the
//                       parents in this launch is an agent-scope load (work-groups on other XCDs have L2s of their own).
//   3 lc_root_kernel    every pixel walks to its root and writes it into `root`, an array of its own: nothing this launch reads
//                       is written by it.  Also counts the roots (root[p] == p) per group of 1024 flat pixels.
//   4 lc_scan_kernel    ONE work-group turns the group counts into exclusive offsets and stores the total in `count`.
//   5 lc_number_kernel  ids[p] = offset + rank inside the group for the roots, -1 for "none".
//   6 lc_spread_kernel  ids[p] = ids[root[p]] for every other pixel (reads root positions only, writes the others only).
// Which links a pixel owes (lc_links) is one rule for launches 1 and 2: launch 1 makes those whose far end lies in the tile,
// launch 2 the rest.
//
// Statistics (a second entry point, after the host has read `count`): lc_stats_init_kernel sets the n records up, and
// lc_stats_kernel adds every pixel in.  A thread first sums its own 16 pixels while the id stays the same, then the lanes of a
// wave that hold the same id are combined by shuffles and ONE lane issues the atomics (a photo that is all one class sends one
// set of atomics per 4096 pixels, not per pixel).  area / box / qsum are integer sums, minima and maxima: order-independent.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#pragma clang fp contract(off)                              // lc_q is the header's formula, one rounding per operation

#define LC_TILE 32                                         // tile side in pixels
#define LC_THREADS 256                                      // threads per work-group of the tile and the flat kernels
#define LC_QUAD 4                                           // consecutive pixels per thread
#define LC_GROUP CCLIP_COMPONENTS_GROUP                     // flat pixels per work-group of launches 3, 5, 6: LC_THREADS * LC_QUAD
#define LC_HALO_W (LC_TILE + 2)                             // tile row with its left and right neighbour column
#define LC_BORDER_THREADS 128                               // launch 2: 32 top-row, 31 left-column, 31 right-column pixels per tile
#define LC_SCAN_THREADS 1024
#define LC_STATS_QUADS 4                                    // quads per thread of the statistics kernel: 4096 pixels per group
#define LC_STATS_ROUNDS 4                                   // ids combined per wave before the rest go out lane by lane
#define LC_NONE 255

static_assert(LC_GROUP == LC_THREADS * LC_QUAD, "the header's group size is the flat kernels' geometry");

struct lc_args {
  const uint8_t* labels; int B, H, W, conn;
  int* root; int* parent;                                   // parent == ids
  int* count; int* groups; int ngroups;
  long npix; int tiles_x, tiles_y;
};

// the backward neighbours (left, up, up-left, up-right) a pixel must be united with, given which of them share its label.
// Links that the others already imply are left out: with left and up-left in the component, up is joined through them
// (induction along the row: every pixel ends up joined to an equal pixel above it); up-left follows from up or from left,
// up-right from up.  Left is never left out.
#define LC_L 1
#define LC_U 2
#define LC_UL 4
#define LC_UR 8
__device__ __forceinline__ int lc_links(bool sl, bool su, bool sul, bool sur, bool eight) {
  int m = sl ? LC_L : 0;
  if (su && !(sl && sul)) m |= LC_U;
  if (eight && sul && !su && !sl) m |= LC_UL;
  if (eight && sur && !su) m |= LC_UR;
  return m;
}

// ---- launch 1: a tile in LDS -------------------------------------------------------------------
__device__ __forceinline__ int lc_lds_load(int* par, int i) {
  return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lc_lds_find(int* par, int i) {
  // ends: a step is taken only to a strictly smaller index, and indices are >= 0
  for (;;) {
    const int n = lc_lds_load(par, i);
    if ((unsigned)n >= (unsigned)i) return i;
    i = n;
  }
}

__device__ __forceinline__ void lc_lds_union(int* par, int a, int b) {
  a = lc_lds_find(par, a);
  b = lc_lds_find(par, b);
  // ends: each round replaces the larger of (a, b) by a strictly smaller index (b < a, or what the atomic returned, < a)
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);                  // par[a] <= a always: old <= a
    if (old >= a) break;                                    // a was a root and now hangs under b
    a = old;                                                // a had a parent already: unite that one with b
  }
}

__global__ __launch_bounds__(LC_THREADS) void lc_tile_kernel(const lc_args a) {
  __shared__ uint8_t lab[(LC_TILE + 1) * LC_HALO_W];        // rows -1 .. 31, columns -1 .. 32 of the tile
  __shared__ int par[LC_TILE * LC_TILE];
  const int tid = threadIdx.x;
  const long t = blockIdx.x;
  const int tx = (int)(t % a.tiles_x), ty = (int)((t / a.tiles_x) % a.tiles_y), b = (int)(t / ((long)a.tiles_x * a.tiles_y));
  const int x0 = tx * LC_TILE, y0 = ty * LC_TILE;
  const uint8_t* img = a.labels + (long)b * a.H * a.W;

  for (int i = tid; i < (LC_TILE + 1) * LC_HALO_W; i += LC_THREADS) {
    const int y = y0 + i / LC_HALO_W - 1, x = x0 + i % LC_HALO_W - 1;
    lab[i] = (x >= 0 && x < a.W && y >= 0 && y < a.H) ? img[(long)y * a.W + x] : (uint8_t)LC_NONE;
  }
  __syncthreads();

  const int ly = tid >> 3, lx0 = (tid & 7) * LC_QUAD;
  const uint8_t* row = lab + (ly + 1) * LC_HALO_W + lx0 + 1;   // row[k]: the thread's pixel k; row[k - LC_HALO_W]: above it
  int links[LC_QUAD];
  int first = 0;                                            // where the run that pixel k lies in begins inside the quad
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const unsigned c = row[k];
    const bool live = c != LC_NONE;
    const bool sl = live && row[k - 1] == c, su = live && row[k - LC_HALO_W] == c;
    const bool sul = live && row[k - LC_HALO_W - 1] == c, sur = live && row[k - LC_HALO_W + 1] == c;
    links[k] = lc_links(sl, su, sul, sur, a.conn == 8);
    if (k == 0 || !sl) first = k;                           // the left link inside a quad is made here, in registers
    else links[k] &= ~LC_L;
    par[ly * LC_TILE + lx0 + k] = ly * LC_TILE + lx0 + first;
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const int lx = lx0 + k, i = ly * LC_TILE + lx;
    const int m = links[k];
    if ((m & LC_L) && lx > 0) lc_lds_union(par, i, i - 1);
    if ((m & LC_U) && ly > 0) lc_lds_union(par, i, i - LC_TILE);
    if ((m & LC_UL) && ly > 0 && lx > 0) lc_lds_union(par, i, i - LC_TILE - 1);
    if ((m & LC_UR) && ly > 0 && lx < LC_TILE - 1) lc_lds_union(par, i, i - LC_TILE + 1);
  }
  __syncthreads();

  const int y = y0 + ly;
  if (y >= a.H) return;
  const long rowbase = ((long)b * a.H + y) * a.W;
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const int x = x0 + lx0 + k;
    if (x >= a.W) break;
    int v = -1;
    if (row[k] != LC_NONE) {
      const int r = lc_lds_find(par, ly * LC_TILE + lx0 + k);     // no LDS write after the barrier above
      v = (int)(((long)b * a.H + y0 + (r >> 5)) * a.W + x0 + (r & (LC_TILE - 1)));
    }
    a.parent[rowbase + x] = v;
  }
}

// ---- launch 2: links across tile borders -------------------------------------------------------
__device__ __forceinline__ int lc_par_load(const int* par, long i) {
  return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int lc_find(const int* par, int i) {
  // ends: a step is taken only to a strictly smaller index, and indices are >= 0
  for (;;) {
    const int n = lc_par_load(par, i);
    if ((unsigned)n >= (unsigned)i) return i;
    i = n;
  }
}

__device__ __forceinline__ void lc_union(int* par, int a, int b) {
  a = lc_find(par, a);
  b = lc_find(par, b);
  // ends: each round replaces the larger of (a, b) by a strictly smaller index (b < a, or what the atomic returned, < a)
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);                  // agent scope; par[a] <= a always: old <= a
    if (old >= a) break;
    a = old;
  }
}

__global__ __launch_bounds__(LC_BORDER_THREADS) void lc_border_kernel(const lc_args a) {
  const int tid = threadIdx.x;
  const long t = blockIdx.x;
  const int tx = (int)(t % a.tiles_x), ty = (int)((t / a.tiles_x) % a.tiles_y), b = (int)(t / ((long)a.tiles_x * a.tiles_y));
  // the tile's top row (threads 0 .. 31), left column below it (32 .. 62), right column below it (64 .. 94, 8-neighbours only)
  int lx, ly;
  if (tid < LC_TILE) { lx = tid; ly = 0; }
  else if (tid < 2 * LC_TILE - 1) { lx = 0; ly = tid - LC_TILE + 1; }
  else if (tid >= 2 * LC_TILE && tid < 3 * LC_TILE - 1 && a.conn == 8) { lx = LC_TILE - 1; ly = tid - 2 * LC_TILE + 1; }
  else return;
  const int x = tx * LC_TILE + lx, y = ty * LC_TILE + ly;
  if (x >= a.W || y >= a.H) return;
  const uint8_t* img = a.labels + (long)b * a.H * a.W;
  const long at = (long)y * a.W + x;
  const unsigned c = img[at];
  if (c == LC_NONE) return;
  const bool hl = x > 0, hu = y > 0, hr = x < a.W - 1;
  const bool sl = hl && img[at - 1] == c, su = hu && img[at - a.W] == c;
  const bool sul = hl && hu && img[at - a.W - 1] == c, sur = hu && hr && img[at - a.W + 1] == c;
  const int m = lc_links(sl, su, sul, sur, a.conn == 8);
  const int p = (int)((long)b * a.H * a.W + at);            // < 2^31 by the entry point's check
  // the far end lies in another tile: left of column 0, above row 0, right of column 31
  if ((m & LC_L) && lx == 0) lc_union(a.parent, p, p - 1);
  if ((m & LC_U) && ly == 0) lc_union(a.parent, p, p - a.W);
  if ((m & LC_UL) && (ly == 0 || lx == 0)) lc_union(a.parent, p, p - a.W - 1);
  if ((m & LC_UR) && (ly == 0 || lx == LC_TILE - 1)) lc_union(a.parent, p, p - a.W + 1);
}

// ---- launches 3 to 6: roots and their numbering --------------------------------------------------
__device__ __forceinline__ int lc_wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(LC_THREADS) void lc_root_kernel(const lc_args a) {
  __shared__ int wcnt[LC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = ((long)blockIdx.x * LC_THREADS + tid) * LC_QUAD;
  int roots = 0;
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const long p = p0 + k;
    if (p >= a.npix) break;
    int r = a.parent[p];
    if (r >= 0) {
      // ends: a step is taken only to a strictly smaller index.  Plain loads: the parents are not written in this launch
      for (;;) {
        const int n = a.parent[r];
        if ((unsigned)n >= (unsigned)r) break;
        r = n;
      }
      roots += r == (int)p;
    }
    a.root[p] = r;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o, 64);
  if (lane == 0) wcnt[wave] = roots;
  __syncthreads();
  if (tid == 0) a.groups[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(LC_SCAN_THREADS) void lc_scan_kernel(const lc_args a) {
  __shared__ int wsum[LC_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < a.ngroups; base += LC_SCAN_THREADS) {   // block-uniform bounds: every thread reaches the barriers
    const int i = base + tid;
    const int v = i < a.ngroups ? a.groups[i] : 0;
    const int incl = lc_wave_incl_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < LC_SCAN_THREADS / 64; ++w) {
      const int s = wsum[w];
      if (w < wave) before += s;
      total += s;
    }
    if (i < a.ngroups) a.groups[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();                                        // wsum is rewritten by the next round
  }
  if (tid == 0) a.count[0] = carry;
}

__global__ __launch_bounds__(LC_THREADS) void lc_number_kernel(const lc_args a) {
  __shared__ int wsum[LC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = ((long)blockIdx.x * LC_THREADS + tid) * LC_QUAD;
  int r[LC_QUAD];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const long p = p0 + k;
    r[k] = p < a.npix ? a.root[p] : -1;
    mine += p < a.npix && r[k] == (int)p;
  }
  const int incl = lc_wave_incl_scan(mine, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int id = a.groups[blockIdx.x] + incl - mine;
#pragma unroll
  for (int w = 0; w < LC_THREADS / 64; ++w)
    if (w < wave) id += wsum[w];
  int* ids = a.parent;                                      // the parents are done with: launch 3 was their last reader
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const long p = p0 + k;
    if (p >= a.npix) break;
    if (r[k] == (int)p) ids[p] = id++;
    else if (r[k] < 0) ids[p] = -1;
  }
}

__global__ __launch_bounds__(LC_THREADS) void lc_spread_kernel(const lc_args a) {
  const long p0 = ((long)blockIdx.x * LC_THREADS + threadIdx.x) * LC_QUAD;
  int* ids = a.parent;
#pragma unroll
  for (int k = 0; k < LC_QUAD; ++k) {
    const long p = p0 + k;
    if (p >= a.npix) break;
    const int r = a.root[p];
    if (r >= 0 && r != (int)p) ids[p] = ids[r];             // reads root positions, which this launch does not write
  }
}

static bool lc_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && H <= CCLIP_OVERLAY_MAX_SIDE && W >= 1 && W <= CCLIP_OVERLAY_MAX_SIDE &&
         (int64_t)B * H * W <= 0x7fffffffLL;
}

extern "C" int cclip_label_components(const uint8_t* labels, int32_t B, int32_t H, int32_t W, int32_t connectivity, int32_t* root,
                                      int32_t* ids, int32_t* count, int32_t* workspace, int64_t workspace_ints,
                                      hipStream_t stream) {
  if (!labels || !root || !ids || !count || !workspace || !lc_shape_ok(B, H, W) || (connectivity != 4 && connectivity != 8))
    return CCLIP_ERR_ARG;
  if (((uintptr_t)root | (uintptr_t)ids | (uintptr_t)count | (uintptr_t)workspace) & 3) return CCLIP_ERR_ARG;
  lc_args a;
  a.labels = labels; a.B = B; a.H = H; a.W = W; a.conn = connectivity;
  a.root = root; a.parent = ids; a.count = count; a.groups = workspace;
  a.npix = (long)B * H * W;
  a.ngroups = (int)((a.npix + LC_GROUP - 1) / LC_GROUP);
  if (workspace_ints < a.ngroups) return CCLIP_ERR_ARG;
  a.tiles_x = (W + LC_TILE - 1) / LC_TILE;
  a.tiles_y = (H + LC_TILE - 1) / LC_TILE;
  const int64_t tiles = (int64_t)B * a.tiles_x * a.tiles_y;   // <= B H W
  hipLaunchKernelGGL(lc_tile_kernel, dim3((unsigned)tiles), dim3(LC_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_border_kernel, dim3((unsigned)tiles), dim3(LC_BORDER_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_root_kernel, dim3((unsigned)a.ngroups), dim3(LC_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_scan_kernel, dim3(1), dim3(LC_SCAN_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_number_kernel, dim3((unsigned)a.ngroups), dim3(LC_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_spread_kernel, dim3((unsigned)a.ngroups), dim3(LC_THREADS), 0, stream, a);
  return cclip_launch_status();
}

// ---- statistics ----------------------------------------------------------------------------------
struct lc_stats_args {
  const uint8_t* labels; const float* conf; const int* root; const int* ids;
  int H, W, n; long npix;
  uint8_t* label; int* image; int* first; int* area; int* box; unsigned long long* qsum;
};

struct lc_acc { int id, area, x0, y0, x1, y1; unsigned long long q; };

// q(v) = (v >= 0) ? min(65536, (uint32)(v * 65536.0f + 0.5f)) : 0; NaN gives 0 (the comparison is false)
__device__ __forceinline__ unsigned lc_q(float v) {
  if (!(v >= 0.0f)) return 0u;
  if (v >= 1.0f) return 65536u;                             // also keeps the conversion below inside uint32 for huge v and inf
  const unsigned u = (unsigned)(v * 65536.0f + 0.5f);
  return u < 65536u ? u : 65536u;
}

__device__ __forceinline__ void lc_flush(const lc_stats_args& a, const lc_acc& s) {
  atomicAdd(a.area + s.id, s.area);
  int* bx = a.box + 4 * (long)s.id;
  atomicMin(bx + 0, s.x0); atomicMin(bx + 1, s.y0);
  atomicMax(bx + 2, s.x1); atomicMax(bx + 3, s.y1);
  if (a.qsum) atomicAdd(a.qsum + s.id, s.q);
}

__global__ __launch_bounds__(LC_THREADS) void lc_stats_init_kernel(const lc_stats_args a) {
  const int i = blockIdx.x * LC_THREADS + threadIdx.x;
  if (i >= a.n) return;
  a.area[i] = 0;
  a.box[4 * (long)i + 0] = a.W; a.box[4 * (long)i + 1] = a.H;
  a.box[4 * (long)i + 2] = 0;   a.box[4 * (long)i + 3] = 0;
  if (a.qsum) a.qsum[i] = 0ull;
}

__global__ __launch_bounds__(LC_THREADS) void lc_stats_kernel(const lc_stats_args a) {
  const int tid = threadIdx.x, lane = tid & 63;
  lc_acc s;
  s.id = -1; s.area = 0; s.x0 = a.W; s.y0 = a.H; s.x1 = 0; s.y1 = 0; s.q = 0ull;
#pragma unroll
  for (int j = 0; j < LC_STATS_QUADS; ++j) {
    const long p0 = (((long)blockIdx.x * LC_STATS_QUADS + j) * LC_THREADS + tid) * LC_QUAD;
#pragma unroll
    for (int k = 0; k < LC_QUAD; ++k) {
      const long p = p0 + k;
      if (p >= a.npix) break;
      const int id = a.ids[p];
      if ((unsigned)id >= (unsigned)a.n) continue;          // "none", or a count that is not this labelling's
      const int row = (int)(p / a.W), x = (int)(p - (long)row * a.W), y = row % a.H;
      if (a.root[p] == (int)p) {                            // the component's first pixel writes what is not a sum
        a.label[id] = a.labels[p]; a.image[id] = row / a.H; a.first[id] = (int)p;
      }
      if (id != s.id) {
        if (s.id >= 0) lc_flush(a, s);
        s.id = id; s.area = 0; s.x0 = a.W; s.y0 = a.H; s.x1 = 0; s.y1 = 0; s.q = 0ull;
      }
      s.area += 1;
      s.x0 = min(s.x0, x); s.y0 = min(s.y0, y); s.x1 = max(s.x1, x + 1); s.y1 = max(s.y1, y + 1);
      if (a.conf) s.q += lc_q(a.conf[p]);
    }
  }
  // the lanes of the wave that hold the same id, combined; all 64 lanes take part in every shuffle
  bool open = s.id >= 0;
  for (int round = 0; round < LC_STATS_ROUNDS; ++round) {   // a fixed number of rounds
    const unsigned long long m = __ballot(open);
    if (m == 0ull) break;                                   // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const int id = __shfl(s.id, lead, 64);
    const bool in = open && s.id == id;
    int ar = in ? s.area : 0, x0 = in ? s.x0 : a.W, y0 = in ? s.y0 : a.H, x1 = in ? s.x1 : 0, y1 = in ? s.y1 : 0;
    unsigned qlo = in ? (unsigned)s.q : 0u, qhi = in ? (unsigned)(s.q >> 32) : 0u;
    unsigned long long q = ((unsigned long long)qhi << 32) | qlo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ar += __shfl_xor(ar, o, 64);
      x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
      x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
      const unsigned lo = __shfl_xor((unsigned)q, o, 64), hi = __shfl_xor((unsigned)(q >> 32), o, 64);
      q += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == lead) {
      lc_acc w;
      w.id = id; w.area = ar; w.x0 = x0; w.y0 = y0; w.x1 = x1; w.y1 = y1; w.q = q;
      lc_flush(a, w);
    }
    if (in) open = false;
  }
  if (open) lc_flush(a, s);                                 // more ids in the wave than rounds: these go out on their own
}

extern "C" int cclip_component_stats(const uint8_t* labels, const float* conf, const int32_t* root, const int32_t* ids, int32_t B,
                                     int32_t H, int32_t W, int32_t n, uint8_t* label, int32_t* image, int32_t* first,
                                     int32_t* area, int32_t* box, uint64_t* qsum, hipStream_t stream) {
  if (!labels || !root || !ids || !lc_shape_ok(B, H, W) || n < 0 || (int64_t)n > (int64_t)B * H * W) return CCLIP_ERR_ARG;
  if ((conf != nullptr) != (qsum != nullptr)) return CCLIP_ERR_ARG;
  if (((uintptr_t)root | (uintptr_t)ids | (uintptr_t)conf) & 3) return CCLIP_ERR_ARG;
  if (n == 0) return CCLIP_OK;                              // nothing to describe, nothing launched
  if (!label || !image || !first || !area || !box) return CCLIP_ERR_ARG;
  if ((((uintptr_t)image | (uintptr_t)first | (uintptr_t)area | (uintptr_t)box) & 3) || ((uintptr_t)qsum & 7)) return CCLIP_ERR_ARG;
  lc_stats_args a;
  a.labels = labels; a.conf = conf; a.root = root; a.ids = ids; a.H = H; a.W = W; a.n = n; a.npix = (long)B * H * W;
  a.label = label; a.image = image; a.first = first; a.area = area; a.box = box; a.qsum = (unsigned long long*)qsum;
  const long per_group = (long)LC_STATS_QUADS * LC_GROUP;
  const long groups = (a.npix + per_group - 1) / per_group;
  hipLaunchKernelGGL(lc_stats_init_kernel, dim3((unsigned)((n + LC_THREADS - 1) / LC_THREADS)), dim3(LC_THREADS), 0, stream, a);
  hipLaunchKernelGGL(lc_stats_kernel, dim3((unsigned)groups), dim3(LC_THREADS), 0, stream, a);
  return cclip_launch_status();
}
