// Few-shot class prototypes for the dense path: masked average pooling of per-patch features under annotated masks (the prototype
// form of few-shot segmentation).  feat fp32 [K g g][E] (encode_image_dense viewed flat), masks uint8 [B][H][W], boxes int32
// [K][4] and image int32 [K] on the device -> sums [C][E], weight [C], patches [C], pixels [C], bad [1].  include/cclip_hip.h holds
// the contract; this file is how it is met.
//
// Cells.  Pixel u of a side of w pixels lies in cell ((2 u + 1) g) / (2 w).  Cell j therefore owns u in [lo(j), lo(j + 1)) with
// lo(j) = ceil(2 w j / g) / 2 (integer division): the smallest u with (2 u + 1) g >= 2 w j.  2 w j <= 2^29: plain int.
//
// Slabs.  The K g g cells are cut into slabs of CCLIP_PROTOTYPES_SLAB consecutive cells: a function of K and g alone.  A
// work-group of 256 threads takes one slab at a time and walks its cells in ascending order; for each cell
//   1. all threads read the cell's pixels that lie inside the picture, in row segments of DP_SEG bytes; a thread merges runs of
//      equal bytes in registers and adds each run to an LDS histogram with a 32-bit integer atomic (area <= 2^28: no overflow);
//   2. thread c owns class c for the whole slab: it takes count_c from the histogram (and clears the cell), keeps pixels, patches
//      and the weight sum of its class in registers, decides whether the cell contributes and leaves w = count / area in LDS; a
//      ballot per wave records which classes contribute (thread 255 owns the "bad" counter: C <= 255);
//   3. if any class contributes, every wave forms the row's sum of squares on its own (dense_class_probs's order: the lane's
//      float4s ascending, then the xor butterfly) - four equal copies, no barrier - and thread t adds w * f^_t, one float4, to row
//      c of the slab's own [C][E] partial in the workspace.  One owner per element and plain stores: the first contribution of a
//      class in a slab is stored, later ones are read back, added and stored by the same thread.
// At the end of a slab thread c writes the slab's weight sum and patch count of its class (always: they tell the second kernel
// which partial rows hold anything, so nothing is zero-filled and untouched rows are never read) and adds its integer counts to
// the outputs with 64-bit global atomics.  dp_combine_kernel then sums the slabs in ascending order, one work-group per class,
// and sets or adds to sums and weight.  No float atomics and nothing depends on the launch geometry: two calls give equal bytes.
//
// Safety.  boxes and image are never trusted: a window is used only when 1 <= side <= CCLIP_OVERLAY_MAX_SIDE (formed in 64 bits)
// and 0 <= image < B, every pixel coordinate is clipped to [0, W) x [0, H) before it becomes an address, and feature rows are
// indexed by the cell number alone.
#include "cclip_common.h"
#include "../../include/cclip_hip.h"

#define DP_THREADS 256
#define DP_SLAB CCLIP_PROTOTYPES_SLAB
#define DP_SEG 8                                            // bytes of one row segment
#define DP_MAX_C 255
#define DP_BAD 256                                          // histogram slot of mask values in [C, 254]
#define DP_MAX_GRID (1 << 20)

struct dp_args {
  const float* feat; long ldf;
  const uint8_t* masks; const int* boxes; const int* image;
  int K, g, C, E, B, H, W, min_share8, accumulate;
  long cells, slabs;                                        // K g g and ceil(cells / DP_SLAB)
  float* sums; float* weight;
  unsigned long long* patches; unsigned long long* pixels; unsigned long long* bad;
  float* ws_sums; float* ws_weight; int* ws_count;          // [slabs][C][E], [slabs][C], [slabs][C]
};

__device__ __forceinline__ void dp_global_add(unsigned long long* p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int dp_lo(int side, int j, int g) { return (int)((2L * side * j + g - 1) / g) >> 1; }

__global__ __launch_bounds__(256) void dp_zero_kernel(const dp_args a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.C) { a.patches[i] = 0ull; a.pixels[i] = 0ull; }
  if (i == 0) a.bad[0] = 0ull;
}

__global__ __launch_bounds__(DP_THREADS) void dense_prototypes_kernel(const dp_args a) {
  __shared__ unsigned hist[DP_BAD + 1];
  __shared__ float wts[DP_THREADS];
  __shared__ unsigned char firsts[DP_THREADS];
  __shared__ unsigned long long masks4[DP_THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, g = a.g, E4 = a.E >> 2, H = a.H, W = a.W;
  const long gg = (long)g * g;

  for (int i = tid; i <= DP_BAD; i += DP_THREADS) hist[i] = 0u;
  __syncthreads();

  for (long slab = blockIdx.x; slab < a.slabs; slab += gridDim.x) {
    const long p0 = slab * DP_SLAB;
    const long p1 = p0 + DP_SLAB < a.cells ? p0 + DP_SLAB : a.cells;
    unsigned long long npix = 0ull;                         // thread c < C: class c; thread 255: the bad pixels
    int npatch = 0;
    float wsum = 0.0f;
    float4* part = (float4*)(a.ws_sums + slab * C * (long)a.E);

    for (long p = p0; p < p1; ++p) {
      const int k = (int)(p / gg);
      const int cell = (int)(p - k * gg);
      const int ci = cell / g, cj = cell - ci * g;
      const int* bp = a.boxes + 4L * k;                     // boxes need only be 4-byte aligned
      const int4 box = make_int4(bp[0], bp[1], bp[2], bp[3]);
      const long bw = (long)box.z - box.x, bh = (long)box.w - box.y;
      const int b = a.image ? a.image[k] : 0;
      if (bw < 1 || bw > CCLIP_OVERLAY_MAX_SIDE || bh < 1 || bh > CCLIP_OVERLAY_MAX_SIDE || b < 0 || b >= a.B) continue;   // group-uniform
      const int ux0 = dp_lo((int)bw, cj, g), ux1 = dp_lo((int)bw, cj + 1, g);
      const int uy0 = dp_lo((int)bh, ci, g), uy1 = dp_lo((int)bh, ci + 1, g);
      const int area = (ux1 - ux0) * (uy1 - uy0);           // <= 2^28
      if (area == 0) continue;
      // the cell's pixels inside the picture: [X0, X1) x [Y0, Y1)
      long X0 = (long)box.x + ux0, X1 = (long)box.x + ux1, Y0 = (long)box.y + uy0, Y1 = (long)box.y + uy1;
      X0 = X0 < 0 ? 0 : X0; X1 = X1 > W ? W : X1; Y0 = Y0 < 0 ? 0 : Y0; Y1 = Y1 > H ? H : Y1;
      const int cw = X1 > X0 ? (int)(X1 - X0) : 0, ch = Y1 > Y0 ? (int)(Y1 - Y0) : 0;
      if (cw > 0 && ch > 0) {
        const uint8_t* img = a.masks + ((long)b * H + Y0) * W + X0;
        const int nseg = (cw + DP_SEG - 1) / DP_SEG;
        const int total = nseg * ch;                        // <= 2^11 * 2^14
        unsigned cur = 255u, cnt = 0u;                      // the open run; 255 is never counted
        for (int s = tid; s < total; s += DP_THREADS) {
          const int r = s / nseg, x = (s - r * nseg) * DP_SEG;
          const uint8_t* row = img + (long)r * W + x;
          const int n = cw - x < DP_SEG ? cw - x : DP_SEG;
          for (int q = 0; q < n; ++q) {
            const unsigned v = row[q];
            if (v == cur) { ++cnt; continue; }
            if (cur != 255u) atomicAdd(hist + (cur < (unsigned)C ? cur : DP_BAD), cnt);
            cur = v; cnt = 1u;
          }
        }
        if (cur != 255u && cnt) atomicAdd(hist + (cur < (unsigned)C ? cur : DP_BAD), cnt);
      }
      __syncthreads();                                      // A: the histogram is complete

      bool give = false;
      if (tid < C) {
        const unsigned n = hist[tid];
        if (n) {
          hist[tid] = 0u;
          npix += n;
          give = 256ull * n >= (unsigned long long)a.min_share8 * (unsigned long long)area;
          if (give) {
            const float w = (float)n / (float)area;
            wts[tid] = w;
            firsts[tid] = npatch == 0;
            wsum += w;
            ++npatch;
          }
        }
      } else if (tid == DP_THREADS - 1) {
        npix += hist[DP_BAD];
        hist[DP_BAD] = 0u;
      }
      const unsigned long long m = __ballot(give);
      if (lane == 0) masks4[wave] = m;
      __syncthreads();                                      // B: weights and masks are in LDS

      unsigned long long mk[DP_THREADS / 64];
#pragma unroll
      for (int q = 0; q < DP_THREADS / 64; ++q) mk[q] = masks4[q];
      if ((mk[0] | mk[1] | mk[2] | mk[3]) == 0ull) continue;               // group-uniform

      // every wave normalises the whole row for itself; thread t keeps float4 t
      const float4* frow = (const float4*)(a.feat + p * a.ldf);
      float ss = 0.0f;
      float4 own = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        const float4 f = i < E4 ? frow[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        ss = __builtin_fmaf(f.x, f.x, ss); ss = __builtin_fmaf(f.y, f.y, ss);
        ss = __builtin_fmaf(f.z, f.z, ss); ss = __builtin_fmaf(f.w, f.w, ss);
        if (q == wave) own = f;
      }
      ss = wave_sum(ss);
      const float inv = ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f;
      own.x *= inv; own.y *= inv; own.z *= inv; own.w *= inv;
      if (tid < E4) {
#pragma unroll
        for (int q = 0; q < DP_THREADS / 64; ++q) {
          unsigned long long rest = mk[q];
          while (rest) {                                    // group-uniform
            const int c = 64 * q + __ffsll((long long)rest) - 1;
            rest &= rest - 1ull;
            const float w = wts[c];
            float4* dst = part + (long)c * E4 + tid;
            float4 acc = make_float4(w * own.x, w * own.y, w * own.z, w * own.w);
            if (!firsts[c]) { const float4 old = *dst; acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w; }
            *dst = acc;
          }
        }
      }
      // the next cell writes wts / firsts / masks4 only after its barrier A, which every thread reaches after this point
    }

    if (tid < C) {
      a.ws_weight[slab * C + tid] = wsum;
      a.ws_count[slab * C + tid] = npatch;
      if (npix) dp_global_add(a.pixels + tid, npix);
      if (npatch) dp_global_add(a.patches + tid, (unsigned long long)npatch);
    } else if (tid == DP_THREADS - 1 && npix) {
      dp_global_add(a.bad, npix);
    }
  }
}

// one work-group per class: the slabs that hold something for it, in ascending order
__global__ __launch_bounds__(DP_THREADS) void dp_combine_kernel(const dp_args a) {
  const int c = blockIdx.x, tid = threadIdx.x, C = a.C, E4 = a.E >> 2;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float wacc = 0.0f;
  for (long s = 0; s < a.slabs; ++s) {
    if (a.ws_count[s * C + c] == 0) continue;               // group-uniform
    if (tid < E4) {
      const float4 v = ((const float4*)(a.ws_sums + (s * C + c) * (long)a.E))[tid];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    wacc += a.ws_weight[s * C + c];
  }
  if (tid < E4) {
    float* out = a.sums + (long)c * a.E + 4 * tid;          // sums need only be 4-byte aligned
    if (a.accumulate) { out[0] += acc.x; out[1] += acc.y; out[2] += acc.z; out[3] += acc.w; }
    else { out[0] = acc.x; out[1] = acc.y; out[2] = acc.z; out[3] = acc.w; }
  }
  if (tid == 0) a.weight[c] = a.accumulate ? a.weight[c] + wacc : wacc;
}

static bool dp_overlap(const void* p, uint64_t np, const void* q, uint64_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + nq && b < a + np;
}

extern "C" int64_t cclip_dense_prototypes_workspace(int32_t K, int32_t g, int32_t C, int32_t E) {
  if (K < 1 || g < 1 || C < 1 || E < 1) return 0;
  const int64_t cells = (int64_t)K * g * g;
  return (cells + DP_SLAB - 1) / DP_SLAB * C * ((int64_t)E + 2) * 4;
}

extern "C" int cclip_dense_prototypes(const float* feat, int64_t ldf, const uint8_t* masks, const int32_t* boxes, const int32_t* image,
                                      int32_t K, int32_t g, int32_t C, int32_t E, int32_t B, int32_t H, int32_t W, int32_t min_share8,
                                      int32_t accumulate, float* sums, float* weight, int64_t* patches, int64_t* pixels, int64_t* bad,
                                      void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!feat || !masks || !boxes || !sums || !weight || !patches || !pixels || !bad || !workspace) return CCLIP_ERR_ARG;
  if (K < 1 || K > 65535 || C < 1 || C > DP_MAX_C) return CCLIP_ERR_ARG;
  if (g < 1 || g > CCLIP_OVERLAY_MAX_SIDE || H < 1 || H > CCLIP_OVERLAY_MAX_SIDE || W < 1 || W > CCLIP_OVERLAY_MAX_SIDE) return CCLIP_ERR_ARG;
  if (B < 1 || (int64_t)B * H * W > 0x7fffffffLL) return CCLIP_ERR_ARG;
  if (E < 4 || E > 1024 || (E & 3) || ldf < E || (ldf & 3)) return CCLIP_ERR_ARG;
  if (min_share8 < 0 || min_share8 > 256 || (accumulate != 0 && accumulate != 1)) return CCLIP_ERR_ARG;
  if (((uintptr_t)feat | (uintptr_t)workspace) & 15) return CCLIP_ERR_ARG;
  if (((uintptr_t)sums | (uintptr_t)weight | (uintptr_t)boxes | (uintptr_t)image) & 3) return CCLIP_ERR_ARG;
  if (((uintptr_t)patches | (uintptr_t)pixels | (uintptr_t)bad) & 7) return CCLIP_ERR_ARG;
  const int64_t need = cclip_dense_prototypes_workspace(K, g, C, E);
  if (workspace_bytes < need) return CCLIP_ERR_ARG;

  dp_args a;
  a.cells = (int64_t)K * g * g;
  a.slabs = (a.cells + DP_SLAB - 1) / DP_SLAB;
  if ((unsigned __int128)a.cells * (uint64_t)ldf > ((unsigned __int128)1 << 62)) return CCLIP_ERR_ARG;   // feat indices stay inside 64 bits
  // an output (the workspace among them) against the inputs and the outputs before it; a length that does not fit is capped
  const unsigned __int128 fl = ((unsigned __int128)(a.cells - 1) * (uint64_t)ldf + (uint64_t)E) * 4u;     // < 2^64 after the check above
  const uint64_t cap = ~(uint64_t)0 - (uintptr_t)feat;
  const void* ptr[10] = {feat, masks, boxes, image, sums, weight, patches, pixels, bad, workspace};
  const uint64_t len[10] = {fl > cap ? cap : (uint64_t)fl, (uint64_t)B * H * W, (uint64_t)K * 16, (uint64_t)K * 4, (uint64_t)C * E * 4,
                            (uint64_t)C * 4, (uint64_t)C * 8, (uint64_t)C * 8, 8, (uint64_t)need};
  for (int i = 4; i < 10; ++i)
    for (int j = 0; j < i; ++j)
      if (ptr[j] && dp_overlap(ptr[i], len[i], ptr[j], len[j])) return CCLIP_ERR_ARG;

  a.feat = feat; a.ldf = ldf; a.masks = masks; a.boxes = boxes; a.image = image;
  a.K = K; a.g = g; a.C = C; a.E = E; a.B = B; a.H = H; a.W = W; a.min_share8 = min_share8; a.accumulate = accumulate;
  a.sums = sums; a.weight = weight;
  a.patches = (unsigned long long*)patches; a.pixels = (unsigned long long*)pixels; a.bad = (unsigned long long*)bad;
  a.ws_sums = (float*)workspace;
  a.ws_weight = a.ws_sums + a.slabs * C * (int64_t)E;
  a.ws_count = (int*)(a.ws_weight + a.slabs * C);
  if (!accumulate) hipLaunchKernelGGL(dp_zero_kernel, dim3(1), dim3(256), 0, stream, a);
  const unsigned grid = (unsigned)(a.slabs < DP_MAX_GRID ? a.slabs : DP_MAX_GRID);
  hipLaunchKernelGGL(dense_prototypes_kernel, dim3(grid), dim3(DP_THREADS), 0, stream, a);
  hipLaunchKernelGGL(dp_combine_kernel, dim3((unsigned)C), dim3(DP_THREADS), 0, stream, a);
  return cclip_launch_status();
}
