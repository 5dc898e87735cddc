// Batched persistent KV-cached beam search: n_cap captions x beams rows (<= 64) in ONE launch
// (cclip_gpt2_beam_search_batch in include/cclip_hip.h).
//
// The one-caption kernel (decode_persist.hip) pays, for every caption, one read of the ~200 MB of GPT-2 + lm_head weights per
// step and a chain of ~62 phase hand-overs per step.  Both are the same for every caption, so here they are shared: the step
// structure is that kernel's (per layer P1 LN + qkv, P2 attention, P3 out-proj + residual, P4 LN + fc + act, P5 proj +
// residual; then LN_f + lm_head slices and the selection), with
//   - projections on v_mfma_f32_16x16x32: a 32-column block streams its Conv1D weight panel ONCE per step (768-row K chunks,
//     transposed into LDS on the way in) and every row multiplies against it; the rows (LayerNorm'd and rounded to the operand
//     type as skinny_block does) are staged in LDS as 16-bit values.  Wave w owns the 32-wide K steps w, w+4, ... and the four
//     waves' partial sums are added in wave order, so an output element's summation order depends neither on the number of
//     rows nor on the row's position: a caption's results do not depend on the batch it is decoded in.
//   - attention: one wave per (row, head), attn_task against the caption's own slot table slot_of[cap][t][beam] (caption c
//     owns cache slots c*beams .. c*beams+beams-1, its prefix in slot c*beams);
//   - lm_head: each workgroup's vocabulary slice x all rows on MFMA (the slice is read once), then per-(workgroup, row)
//     (max, sum-exp, top-k) partials (select_partials);
//   - selection: caption c is merged by workgroup c mod G with the one-caption kernel's select_merge; a caption
//     that has stopped is not merged again, so its tokens / lengths / scores are those of the one-caption loop's break.
// Hand-overs, bounded spins, the error flag that drains the grid, one workgroup per CU and the re-initialised state words are
// those of decode_persist.hip; what the two kernels share is in decode_persist_impl.h.
#include "decode_persist_impl.h"

namespace CCLIP_NS {

#define BB_MAXROWS 64       // captions x beams per launch
#define BB_KC 768           // K chunk of a projection block
#define BB_LDA (BB_KC + 8)  // LDS row stride of the staged rows / transposed weights (16-bit elements)

struct BatchArgs {
  int n_layer, nb, n_cap, rows, D, H, Hd, act, V, pos0, n_steps, stop_token, ld_tokens, max_len, rows_per_wg;
  float temperature;
  cclip_block_ptrs blocks[DECODE_MAXL];
  float* x;
  bf16* kc; bf16* vc; long ld_layer, ld_seq;
  bf16* scratch;
  const float* lnf_w; const float* lnf_b; const bf16* wte16;
  const float* first_logits;  // [n_cap][V]
  const float* wte32; const float* wpe32;
  int* slot_of;               // [n_cap][max_len][8]
  int* tokens; float* scores; float* seq_len; int* stopped;   // rows c * nb + b
  int* state;                 // [0] hand-over counter, [1] error, [2] captions stopped
  int* cap_state;             // [n_cap][8]: [2] stopped, [3] selections made by then, [4] token columns
  float* part;                // [n_cap][G][8][DECODE_PS]
};

// ---- one 32-column block of a projection for all M rows, on MFMA ------------------------------------------------------------
// LDS: As [64][BB_LDA] 16-bit rows of the K chunk, Ws [32][BB_LDA] the chunk's weights transposed (column n's K run is
// contiguous: one 16-byte read per B fragment), then [64] mean + [64] rstd; the reduction reuses As as fp32 [4][64][33].
// The chunk's weights are loaded into registers before the wait for the previous phase (they do not depend on it) and the
// next chunk's are in flight while this one multiplies.  Epilogue forms as skinny_block's.
template <int ACT>
__device__ __forceinline__ void mma_block(const GemmArgs& p, const int n0, float* lds, PhaseSync* ps) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int M = p.M, K = p.K, RT = (M + 15) >> 4;
  bf16* As = (bf16*)lds;
  bf16* Ws = As + BB_MAXROWS * BB_LDA;
  float* stt = (float*)(Ws + 32 * BB_LDA);
  const int wj = tid & 3;                            // weight piece i = tid + 256 u: chunk row (tid >> 2) + 64 u, columns 8 wj..
  const int ncol = n0 + 8 * wj;
  const bool live = ncol < p.N;                      // N % 8 == 0
  const bf16* wpc = p.B + (live ? ncol : 0);
  bf16x8 w[12];
  auto wload = [&](int kb) {
#pragma unroll
    for (int u = 0; u < 12; ++u) {
      const int k = kb + (tid >> 2) + 64 * u;
      w[u] = *(const bf16x8*)(wpc + (long)(k < K ? k : K - 1) * p.ldb);
    }
  };
  wload(0);
  ps->wait();
  if (p.ln_x) {                                      // LayerNorm statistics (K <= 1024: one read of the row), as skinny_block
    for (int m = wave; m < M; m += 4) {
      const float* xr = p.ln_x + (long)m * p.ln_ldx;
      float xv[16], mean, rstd;
      ln_row_stats<true>(xr, K, xv, mean, rstd);
      if (lane == 0) { stt[m] = mean; stt[64 + m] = rstd; }
    }
  }
  f32x4 acc[4][2];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < K; kb += BB_KC) {
    const int kc = K - kb < BB_KC ? K - kb : BB_KC;  // a multiple of 32
    __syncthreads();                                 // the previous chunk's fragments are read; statistics are visible
#pragma unroll
    for (int u = 0; u < 12; ++u) {
      const int kl = (tid >> 2) + 64 * u;
      const bool on = live && kb + kl < K;
#pragma unroll
      for (int e = 0; e < 8; ++e) Ws[(8 * wj + e) * BB_LDA + kl] = on ? w[u][e] : (bf16)0.f;
    }
    if (kb + BB_KC < K) wload(kb + BB_KC);
    const int RP = RT * 16;
    if (p.ln_x) {                                    // A = LayerNorm(x) rounded to the operand type, 4 columns per piece
      const int q4 = kc >> 2, n4 = RP * q4;
      for (int i0 = tid; i0 < n4; i0 += 2048) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 256 * u < n4 ? i0 + 256 * u : n4 - 1;
          const int m = i / q4, q = i - m * q4;
          v[u] = ld_coh<true>((const f32x4*)(p.ln_x + (long)(m < M ? m : M - 1) * p.ln_ldx + kb + 4 * q));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 256 * u;
          if (i < n4) {
            const int m = i / q4, q = i - m * q4;
            const float mean = stt[m < M ? m : 0], rstd = stt[64 + (m < M ? m : 0)];
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int k = kb + 4 * q + e;
              o[e] = m < M ? (bf16)((v[u][e] - mean) * rstd * p.ln_gamma[k] + p.ln_beta[k]) : (bf16)0.f;
            }
            *(bf16x4*)(As + m * BB_LDA + 4 * q) = o;
          }
        }
      }
    } else {                                         // A rows as they are (16-bit), 8 columns per piece
      const int q8 = kc >> 3, n8 = RP * q8;
      for (int i0 = tid; i0 < n8; i0 += 2048) {
        bf16x8 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 256 * u < n8 ? i0 + 256 * u : n8 - 1;
          const int m = i / q8, q = i - m * q8;
          v[u] = ld_coh<true>((const bf16x8*)(p.A + (long)(m < M ? m : M - 1) * p.lda + kb + 8 * q));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + 256 * u;
          if (i < n8) {
            const int m = i / q8, q = i - m * q8;
            bf16x8 o = v[u];
            if (m >= M) {
#pragma unroll
              for (int e = 0; e < 8; ++e) o[e] = (bf16)0.f;
            }
            *(bf16x8*)(As + m * BB_LDA + 8 * q) = o;
          }
        }
      }
    }
    __syncthreads();
    const int nk = kc >> 5;
    for (int kk = wave; kk < nk; kk += 4) {          // this wave's K steps, ascending: a fixed order for every element
      const bf16x8 b0 = *(const bf16x8*)(Ws + li * BB_LDA + 32 * kk + 8 * g);
      const bf16x8 b1 = *(const bf16x8*)(Ws + (16 + li) * BB_LDA + 32 * kk + 8 * g);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        if (rt < RT) {
          const bf16x8 af = *(const bf16x8*)(As + (16 * rt + li) * BB_LDA + 32 * kk + 8 * g);
          acc[rt][0] = CCLIP_MFMA_16x16x32(af, b0, acc[rt][0]);
          acc[rt][1] = CCLIP_MFMA_16x16x32(af, b1, acc[rt][1]);
        }
      }
    }
  }
  __syncthreads();
  float* red = lds;                                  // [4 waves][64 rows][33]
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
    if (rt < RT)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 64 + 16 * rt + 4 * g + r) * 33 + 16 * ct + li] = acc[rt][ct][r];
  __syncthreads();
  for (int i = tid; i < M * 32; i += 256) {
    const int m = i >> 5, c = i & 31, n = n0 + c;
    if (n >= p.N) continue;
    const float s = ((red[m * 33 + c] + red[(64 + m) * 33 + c]) + red[(128 + m) * 33 + c]) + red[(192 + m) * 33 + c];
    float v = s * p.alpha + (p.bias ? p.bias[n] : 0.f);
    if (p.out_pre) st_coh<true>(p.out_pre + (long)m * p.ldc + n, (bf16)v);
    v = act_apply<ACT>(v, 0.f);
    if (p.residual) v += ld_coh<true>(p.residual + (long)m * p.ldr + n);
    if (p.out_f32) st_coh<true>(p.out_f32 + (long)m * p.ldc + n, v);
    if (p.out_bf16) st_coh<true>(p.out_bf16 + (long)m * p.ldc + n, (bf16)v);
    if (p.kv_k && n >= p.kv_width) {                 // packed q|k|v projection: k and v rows also go to the cache
      if (n < 2 * p.kv_width) st_coh<true>(p.kv_k + (long)m * p.kv_ld_seq + n - p.kv_width, (bf16)v);
      else st_coh<true>(p.kv_v + (long)m * p.kv_ld_seq + n - 2 * p.kv_width, (bf16)v);
    }
  }
}

template <int ACT>
__device__ __forceinline__ void proj_phase(const GemmArgs& p, int nblk, int G, float* lds, PhaseSync* ps) {
  for (int cb = blockIdx.x; cb < nblk; cb += G) mma_block<ACT>(p, cb * 32, lds, ps);
}

// ---- LN_f + tied lm_head over the slice [r0, r0 + nr) for every row, on MFMA; logits to sl = lds as [rows][DECODE_MAXR] --------
// xs: LN_f(x) rounded to the operand type, 16-bit [RT*16][D+8] (rows past `rows` zero).  Wave w owns vocabulary tiles w, w+4,
// .. (<= 4) for every row tile: the slice's wte rows are read once, whatever the number of rows.
__device__ __forceinline__ void head_phase(const BatchArgs& a, float* lds, int r0, int nr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int D = a.D, R = a.rows, RT = (R + 15) >> 4, ldx = D + 8;
  bf16* xs = (bf16*)lds;
  for (int m = wave; m < R; m += 4) {
    const float* xr = a.x + (long)m * D;
    float xv[16], mean, rstd;
    ln_row_stats<true>(xr, D, xv, mean, rstd);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kk = lane + 64 * u;
      if (kk < D) xs[m * ldx + kk] = (bf16)((xv[u] - mean) * rstd * a.lnf_w[kk] + a.lnf_b[kk]);
    }
  }
  for (int i = tid; i < (RT * 16 - R) * D; i += 256) xs[(R + i / D) * ldx + i % D] = (bf16)0.f;
  __syncthreads();
  const int nvt = (nr + 15) >> 4;                    // 16-row vocabulary tiles of the slice (<= 16)
  f32x4 acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[j][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (nr > 0) {
    const bf16* wr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 16 * (wave + 4 * j) + li;
      wr[j] = a.wte16 + (long)(r0 + (row < nr ? row : nr - 1)) * D + 8 * g;
    }
    const int nk = D >> 5;
    for (int k0 = 0; k0 < nk; k0 += 4) {             // four K steps of the four tiles in flight together
      bf16x8 bw[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) bw[s][j] = *(const bf16x8*)(wr[j] + 32 * (k0 + s < nk ? k0 + s : nk - 1));
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (k0 + s >= nk) break;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          if (rt >= RT) break;
          const bf16x8 af = *(const bf16x8*)(xs + (16 * rt + li) * ldx + 32 * (k0 + s) + 8 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (wave + 4 * j < nvt) acc[j][rt] = CCLIP_MFMA_16x16x32(af, bw[s][j], acc[j][rt]);
        }
      }
    }
  }
  __syncthreads();                                   // xs is read: the logits take its place
  float* sl = lds;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + 4 * g + r, v = 16 * (wave + 4 * j) + li;
        if (rt < RT && row < R && v < nr) sl[row * DECODE_MAXR + v] = acc[j][rt][r];
      }
  __syncthreads();
}

template <int MCAP>
__global__ __launch_bounds__(256) void gpt2_beam_batch_persist_kernel(const BatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int G = gridDim.x, D = a.D, Hd = a.Hd, nb = a.nb, R = a.rows;
  PhaseSync ps{a.state, a.state + 1, 0, false};
  auto nprod = [&](int nblk) { return nblk < G ? nblk : G; };
  const long ldrow = 5L * D + Hd;
  bf16* qkv = a.scratch + D;
  bf16* att = a.scratch + 4L * D;
  bf16* hid = a.scratch + 5L * D;
  const float T = a.temperature > 0.f ? a.temperature : 1.0f;
  const int VR = a.rows_per_wg;
  const int r0 = blockIdx.x * VR;
  const int nr = r0 >= a.V ? 0 : (a.V - r0 < VR ? a.V - r0 : VR);
  // the selections of every caption that has not stopped: caption c by workgroup c mod G
  auto select_all = [&](int n_in, bool first, int it, int cur_pos) {
    if (blockIdx.x < a.n_cap) {
      ps.wait();
      for (int c = blockIdx.x; c < a.n_cap; c += G) {
        int* cs = a.cap_state + 8 * c;
        if (__hip_atomic_load(cs + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;    // written by this workgroup only
        CapView v;
        v.nb = nb; v.V = a.V; v.D = D; v.pos0 = a.pos0; v.max_len = a.max_len; v.ld_tokens = a.ld_tokens; v.stop_token = a.stop_token;
        v.wte32 = a.wte32; v.wpe32 = a.wpe32;
        v.x = a.x + (long)c * nb * D; v.slot_of = a.slot_of + (long)c * a.max_len * 8; v.tokens = a.tokens + (long)c * nb * a.ld_tokens;
        v.scores = a.scores + c * nb; v.seq_len = a.seq_len + c * nb; v.stopped = a.stopped + c * nb; v.state = cs;
        v.part = a.part + (long)c * G * 8 * DECODE_PS;
        select_merge<MCAP>(v, n_in, first, it, cur_pos, G, it, lds);
        if (tid == 0 && __hip_atomic_load(cs + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          __hip_atomic_fetch_add(a.state + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    ps.arrive(nprod(a.n_cap), blockIdx.x < a.n_cap);
  };
  int it = 0;
  {
    // the prefill's last-position logits of every caption: selections with one input beam (test.py:396-405)
    for (int i = tid; i < a.n_cap * VR; i += 256) {
      const int c = i / VR, j = i - c * VR;
      if (j < nr) lds[c * DECODE_MAXR + j] = a.first_logits[(long)c * a.V + r0 + j];
    }
    __syncthreads();
    select_partials(a.part, nb, lds, a.n_cap, true, r0, nr, T, G);
    ps.arrive(G, true);
    select_all(1, true, it, a.pos0 - 1);
    ++it;
  }
  for (int s = 0; s < a.n_steps; ++s, ++it) {
    ps.wait();                                                      // the selections: next input rows, slot tables, stop flags
    if (__hip_atomic_load(a.state + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.n_cap) break;   // every caption stopped
    const int pos = a.pos0 + s;
    if (pos >= a.max_len) break;
    GemmArgs p;
    p.alpha = 1.0f; p.aux = nullptr; p.ldaux = 0; p.out_pre = nullptr; p.split_ws = nullptr; p.ktiles_per_split = 0; p.M = R;
    for (int l = 0; l < a.n_layer; ++l) {
      const cclip_block_ptrs& w = a.blocks[l];
      bf16* kc = a.kc + (long)l * a.ld_layer;
      bf16* vc = a.vc + (long)l * a.ld_layer;
      // P1: LayerNorm + qkv projection, k / v appended at `pos` of each row's own slot
      p.A = nullptr; p.lda = 0; p.B = (const bf16*)w.w_qkv; p.ldb = 3 * D; p.N = 3 * D; p.K = D; p.bias = w.b_qkv; p.act = 0;
      p.residual = nullptr; p.ldr = 0; p.out_f32 = nullptr; p.out_bf16 = qkv; p.ldc = ldrow;
      p.ln_x = a.x; p.ln_ldx = D; p.ln_gamma = w.ln1_w; p.ln_beta = w.ln1_b;
      p.kv_k = kc + (long)pos * D; p.kv_v = vc + (long)pos * D; p.kv_ld_seq = a.ld_seq; p.kv_width = D;
      {
        const int nblk = (3 * D + 31) / 32;
        proj_phase<CCLIP_ACT_NONE>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P2: attention of the new token against positions [0, pos], one wave per (row, head)
      const int ntask = R * a.H, ntask4 = (ntask + 3) / 4;
      if (blockIdx.x < ntask4) ps.wait();
      for (int t0 = blockIdx.x * 4; t0 < ntask; t0 += G * 4) {
        const int t = t0 + wave;
        const bool valid = t < ntask;
        const int tt = valid ? t : ntask - 1;
        const int row = tt / a.H, c = row / nb;
        float* wl = lds + wave * (128 + a.max_len + 64);
        attn_task(a.slot_of + (long)c * a.max_len * 8, c * nb, nb, a.ld_seq, D, qkv, ldrow, kc, vc, att, ldrow, row, row - c * nb, tt % a.H,
                  pos + 1, valid, wl, (int*)(wl + 128), wl + 128 + a.max_len);
      }
      ps.arrive(nprod(ntask4), blockIdx.x < ntask4);
      // P3: out-proj + residual (x += ...)
      p.ln_x = nullptr; p.kv_k = nullptr; p.kv_v = nullptr; p.kv_width = 0;
      p.A = att; p.lda = ldrow; p.B = (const bf16*)w.w_o; p.ldb = D; p.N = D; p.K = D; p.bias = w.b_o;
      p.residual = a.x; p.ldr = D; p.out_f32 = a.x; p.out_bf16 = nullptr; p.ldc = D;
      {
        const int nblk = (D + 31) / 32;
        proj_phase<CCLIP_ACT_NONE>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P4: LayerNorm + fc + activation
      p.A = nullptr; p.lda = 0; p.B = (const bf16*)w.w_fc; p.ldb = Hd; p.N = Hd; p.K = D; p.bias = w.b_fc;
      p.residual = nullptr; p.ldr = 0; p.out_f32 = nullptr; p.out_bf16 = hid; p.ldc = ldrow;
      p.ln_x = a.x; p.ln_ldx = D; p.ln_gamma = w.ln2_w; p.ln_beta = w.ln2_b;
      {
        const int nblk = (Hd + 31) / 32;
        if (a.act == CCLIP_ACT_GELU_NEW) proj_phase<CCLIP_ACT_GELU_NEW>(p, nblk, G, lds, &ps);
        else proj_phase<CCLIP_ACT_NONE>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P5: proj + residual
      p.ln_x = nullptr;
      p.A = hid; p.lda = ldrow; p.B = (const bf16*)w.w_proj; p.ldb = D; p.N = D; p.K = Hd; p.bias = w.b_proj;
      p.residual = a.x; p.ldr = D; p.out_f32 = a.x; p.out_bf16 = nullptr; p.ldc = D;
      {
        const int nblk = (D + 31) / 32;
        proj_phase<CCLIP_ACT_NONE>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
    }
    // LN_f + tied lm_head over this workgroup's vocabulary slice, the slice's partials, then the selections
    ps.wait();
    head_phase(a, lds, r0, nr);
    select_partials(a.part, nb, lds, R, false, r0, nr, T, G);
    ps.arrive(G, true);
    select_all(nb, false, it, pos);
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_gpt2_beam_search_batch)(const cclip_beam_batch_desc* d, hipStream_t stream) {
  if (!d || !persist_desc_ok(d->step)) return CCLIP_ERR_ARG;
  const cclip_decode_desc& s = d->step;
  if (d->n_cap <= 0 || d->beams <= 0 || d->beams > 8 || (long)d->n_cap * d->beams > BB_MAXROWS || s.n_seq != d->n_cap * d->beams)
    return CCLIP_ERR_ARG;
  if (!d->first_logits || !d->wte_f32 || !d->wpe_f32 || !d->slot_of || !d->tokens || !d->scores || !d->seq_lengths || !d->is_stopped ||
      !d->state || !d->cap_state || !d->select_ws)
    return CCLIP_ERR_ARG;
  if (d->n_steps < 0 || d->max_len <= s.pos || d->max_len > 2048 || d->ld_tokens < d->n_steps + 1 || s.ld_seq < (long)d->max_len * s.width)
    return CCLIP_ERR_ARG;
  const int n_cu = persist_cu_count();
  if (n_cu == 0) return CCLIP_ERR_LAUNCH;
  int G, VR;
  if (!persist_grid(s.vocab, d->grid_cap, n_cu, &G, &VR)) return CCLIP_ERR_ARG;
  const int rows = s.n_seq, nb = d->beams;
  const int mcap = nb <= 4 ? 4 : 8;
  // LDS: projection block (rows + transposed weights + statistics), attention rows, lm_head rows / slice logits, selection
  size_t by = (size_t)(BB_MAXROWS + 32) * BB_LDA * 2 + 128 * 4;
  const size_t att = (size_t)4 * (128 + d->max_len + 64) * 4; if (att > by) by = att;
  const size_t head = (size_t)((rows + 15) / 16 * 16) * (s.width + 8) * 2; if (head > by) by = head;
  const size_t slc = (size_t)(rows > d->n_cap ? rows : d->n_cap) * DECODE_MAXR * 4; if (slc > by) by = slc;
  const size_t sel = (64 + 512 + 4096 + 2 * (size_t)nb * G * nb) * 4; if (sel > by) by = sel;
  if (by > 150 * 1024) return CCLIP_ERR_ARG;
  BatchArgs a;
  a.n_layer = s.n_layer; a.nb = nb; a.n_cap = d->n_cap; a.rows = rows; a.D = s.width; a.H = s.heads; a.Hd = s.hidden; a.act = s.act;
  a.V = s.vocab; a.pos0 = s.pos; a.n_steps = d->n_steps; a.stop_token = d->stop_token; a.ld_tokens = d->ld_tokens; a.max_len = d->max_len;
  a.rows_per_wg = VR; a.temperature = d->temperature;
  for (int l = 0; l < s.n_layer; ++l) a.blocks[l] = s.blocks[l];
  a.x = s.x; a.kc = (bf16*)s.kcache; a.vc = (bf16*)s.vcache; a.ld_layer = s.ld_layer; a.ld_seq = s.ld_seq; a.scratch = (bf16*)s.scratch16;
  a.lnf_w = s.lnf_w; a.lnf_b = s.lnf_b; a.wte16 = (const bf16*)s.wte16;
  a.first_logits = d->first_logits; a.wte32 = d->wte_f32; a.wpe32 = d->wpe_f32;
  a.slot_of = d->slot_of; a.tokens = d->tokens; a.scores = d->scores; a.seq_len = d->seq_lengths; a.stopped = d->is_stopped;
  a.state = d->state; a.cap_state = d->cap_state; a.part = d->select_ws;
  if (hipMemsetAsync(d->state, 0, 8 * sizeof(int), stream) != hipSuccess) return CCLIP_ERR_LAUNCH;
  if (hipMemsetAsync(d->cap_state, 0, (size_t)8 * d->n_cap * sizeof(int), stream) != hipSuccess) return CCLIP_ERR_LAUNCH;
  return mcap == 4 ? launch_persist<gpt2_beam_batch_persist_kernel<4>>(G, by, stream, a)
                   : launch_persist<gpt2_beam_batch_persist_kernel<8>>(G, by, stream, a);
}