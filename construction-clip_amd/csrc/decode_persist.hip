// Persistent KV-cached beam-search decoder (see cclip_gpt2_beam_search in include/cclip_hip.h).
//
// The reference's generate_beam (CLIP_prefix_caption test.py:353-441, application.py:152-229) runs, per new
// token, the whole GPT-2 on the growing sequence and then ~15 small torch ops on the [beams, V] logits.  With a KV cache the
// step's arithmetic is a chain of GEMVs over 170 MB of weights (40 us of HBM time) - what is left is overhead: the
// launch-by-launch form of this repo (cclip_gpt2_decode_step: 62 dependent 5-13 us launches, then the selection ops and a
// cache gather from Python) takes 1.14 ms per step.  Here ONE kernel of one workgroup per CU runs every step of a caption:
//
//   per layer   P1  LayerNorm + qkv GEMV, k / v rows appended to the cache        (3D/32 column blocks)
//               P2  decode attention, one wave per (beam, head)
//               P3  out-proj GEMV + residual                                      (D/32 blocks)
//               P4  LayerNorm + fc GEMV + activation                              (hidden/32 blocks)
//               P5  proj GEMV + residual                                          (D/32 blocks)
//   then        LN_f + tied lm_head GEMV over a contiguous vocabulary slice per workgroup, which also leaves the slice's
//               per-beam (max, sum-exp, top-k) partials, and
//               the selection (workgroup 0): temperature / log-softmax / stopped-beam rule / length-normalised top-k, token
//               append, beam reorder, next input embedding - the arithmetic of test.py:395-428, restated.
//
// Phases are separated by a grid barrier (one atomic counter); the small buffers one phase hands to the next are written with
// write-through (sc1) stores and read with sc1 loads, which are coherent across the XCDs' L2s without cache-wide fences.  Beam
// reorder never copies the cache: `slot_of[t][b]` names the cache slot that holds beam b's key / value of position t, and
// reordering permutes that table.  A stopped caption ends the kernel (flag checked after a barrier, so every workgroup takes
// the same exit); a barrier that does not fill within ~1 s sets an error flag and is never waited on again, so the grid always
// drains.  The hand-over, the attention task, the selection and the host helpers are shared with the batched kernel
// (decode_persist_impl.h).
#include "decode_persist_impl.h"

namespace CCLIP_NS {

struct BeamArgs {
  int n_layer, nb, D, H, Hd, act, V, pos0, n_steps, first, stop_token, ld_tokens, max_len, rows_per_wg;
  float temperature;
  cclip_block_ptrs blocks[DECODE_MAXL];
  float* x;
  bf16* kc; bf16* vc; long ld_layer, ld_seq;
  bf16* scratch;
  const float* lnf_w; const float* lnf_b; const bf16* wte16;
  float* logits; long ld_logits; const float* first_logits;
  const float* wte32; const float* wpe32;
  int* slot_of; int* tokens; float* scores; float* seq_len; int* stopped;
  int* state;                 // [0] barrier counter, [1] error, [2] done, [3] selections made when every beam had stopped, [4] tokens per beam
  float* part;
};

// LN_f + tied lm_head over the vocabulary slice [r0, r0 + nr): xs = LN_f(x) rounded to the operand type, fp32 [nb][D] at lds;
// the slice's logits go to sl = lds + MCAP*D as [nb][DECODE_MAXR] (and to a.logits when given)
template <int MCAP>
__device__ __forceinline__ void head_phase(const BeamArgs& a, float* lds, int r0, int nr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, nb = a.nb;
  {
    float* xs = lds;
    float* sl = lds + MCAP * D;
    for (int m = wave; m < nb; m += 4) {                              // (D <= 1024 checked by the launcher: one read of the row)
      const float* xr = a.x + (long)m * D;
      float xv[16], mean, rstd;
      ln_row_stats<true>(xr, D, xv, mean, rstd);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int kk = lane + 64 * u;
        if (kk < D) xs[m * D + kk] = (float)(bf16)((xv[u] - mean) * rstd * a.lnf_w[kk] + a.lnf_b[kk]);
      }
    }
    __syncthreads();
    {
      // lane (r = lane >> 4, c = lane & 15): vocabulary row r of the wave's 4, 16-byte chunks c, c + 16, ... (D <= 1024: up to
      // 4 per lane per half); 48 rows of the slice per trip with every load of the trip in flight (8 x 16 bytes per lane
      // per half-row pass): the slice is weight-read latency, not bandwidth
      const int rr = lane >> 4, c16 = lane & 15;
      const int nch = D >> 3;                                       // 16-byte chunks per row
      for (int g0 = 0; g0 < nr; g0 += 48) {
        float acc[3][MCAP];
#pragma unroll
        for (int h = 0; h < 3; ++h)
#pragma unroll
          for (int m = 0; m < MCAP; ++m) acc[h][m] = 0.f;
        bf16x8 wv[3][8];
#pragma unroll
        for (int h = 0; h < 3; ++h) {
          const int row = g0 + 16 * h + 4 * wave + rr;
          const bf16* wr = a.wte16 + (long)(r0 + (row < nr ? row : nr - 1)) * D;
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int ch = c16 + 16 * u;
            wv[h][u] = *(const bf16x8*)(wr + 8 * (ch < nch ? ch : nch - 1));
          }
        }
#pragma unroll
        for (int h = 0; h < 3; ++h)
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int ch = c16 + 16 * u;
            if (ch < nch) {
#pragma unroll
              for (int m = 0; m < MCAP; ++m) {
                if (m < nb) {
                  const float* xm = xs + m * D + 8 * ch;
#pragma unroll
                  for (int j = 0; j < 8; ++j) acc[h][m] += xm[j] * (float)wv[h][u][j];
                }
              }
            }
          }
#pragma unroll
        for (int h = 0; h < 3; ++h) {
          const int row = g0 + 16 * h + 4 * wave + rr;
#pragma unroll
          for (int m = 0; m < MCAP; ++m) {
            float v = acc[h][m];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            if (c16 == 0 && m < nb && row < nr) {
              sl[m * DECODE_MAXR + row] = v;
              if (a.logits) a.logits[(long)m * a.ld_logits + r0 + row] = v;
            }
          }
        }
      }
    }
  }
}

// one projection phase: this workgroup's column blocks
template <int MCAP, int ACT, int U>
__device__ __forceinline__ void proj_phase(const GemmArgs& p, int nblk, int G, float* lds, PhaseSync* ps) {
  auto pw = [&]() { ps->wait(); };           // (waiting twice for the same total is free: the second call returns at once)
  for (int cb = blockIdx.x; cb < nblk; cb += G) skinny_block<MCAP, ACT, U, true>(p, cb * 32, lds, pw);
}

template <int MCAP>
__global__ __launch_bounds__(256) void gpt2_beam_persist_kernel(const BeamArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = gridDim.x, D = a.D, Hd = a.Hd, nb = a.nb;
  PhaseSync ps{a.state, a.state + 1, 0, false};
  auto nprod = [&](int nblk) { return nblk < G ? nblk : G; };
  const long ldrow = 5L * D + Hd;
  bf16* qkv = a.scratch + D;
  bf16* att = a.scratch + 4L * D;
  bf16* hid = a.scratch + 5L * D;
  const float T = a.temperature > 0.f ? a.temperature : 1.0f;
  const int R = a.rows_per_wg;
  const int r0 = blockIdx.x * R;
  const int nr = r0 >= a.V ? 0 : (a.V - r0 < R ? a.V - r0 : R);
  CapView cv;                                                      // the one caption: rows 0.., the whole slot table and partials
  cv.nb = nb; cv.V = a.V; cv.D = D; cv.pos0 = a.pos0; cv.max_len = a.max_len; cv.ld_tokens = a.ld_tokens; cv.stop_token = a.stop_token;
  cv.wte32 = a.wte32; cv.wpe32 = a.wpe32;
  cv.x = a.x; cv.slot_of = a.slot_of; cv.tokens = a.tokens; cv.scores = a.scores; cv.seq_len = a.seq_len; cv.stopped = a.stopped;
  cv.state = a.state; cv.part = a.part;
  int it = 0;
  const int ntok0 = a.state[4];                                    // token columns present at launch; one more per selection
  if (a.first) {
    // the prefill's last-position logits: selection with one input beam (test.py:396-405)
    for (int j = tid; j < nr; j += 256) lds[j] = a.first_logits[r0 + j];
    __syncthreads();
    select_partials(a.part, nb, lds, 1, true, r0, nr, T, G);
    ps.arrive(G, true);
    if (blockIdx.x == 0) { ps.wait(); select_merge<MCAP>(cv, 1, true, it, a.pos0 - 1, G, ntok0 + it, lds); }
    ps.arrive(1, blockIdx.x == 0);
    ++it;
  }
  for (int s = 0; s < a.n_steps; ++s, ++it) {
    ps.wait();                                                      // the selection: next input rows, slot table, the stop flag
    if (__hip_atomic_load(a.state + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;     // every beam has stopped
    const int pos = a.pos0 + s;
    if (pos >= a.max_len) break;
    GemmArgs p;
    p.alpha = 1.0f; p.aux = nullptr; p.ldaux = 0; p.out_pre = nullptr; p.split_ws = nullptr; p.ktiles_per_split = 0; p.M = nb;
    for (int l = 0; l < a.n_layer; ++l) {
      const cclip_block_ptrs& w = a.blocks[l];
      bf16* kc = a.kc + (long)l * a.ld_layer;
      bf16* vc = a.vc + (long)l * a.ld_layer;
      // P1: LayerNorm + qkv projection, k / v appended at `pos` of each beam's own slot
      p.A = nullptr; p.lda = 0; p.B = (const bf16*)w.w_qkv; p.ldb = 3 * D; p.N = 3 * D; p.K = D; p.bias = w.b_qkv; p.act = 0;
      p.residual = nullptr; p.ldr = 0; p.out_f32 = nullptr; p.out_bf16 = qkv; p.ldc = ldrow;
      p.ln_x = a.x; p.ln_ldx = D; p.ln_gamma = w.ln1_w; p.ln_beta = w.ln1_b;
      p.kv_k = kc + (long)pos * D; p.kv_v = vc + (long)pos * D; p.kv_ld_seq = a.ld_seq; p.kv_width = D;
      {
        const int nblk = (3 * D + 31) / 32;
        proj_phase<MCAP, CCLIP_ACT_NONE, 12>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P2: attention of the new token against positions [0, pos]
      const int ntask4 = (nb * a.H + 3) / 4;
      if (blockIdx.x < ntask4) ps.wait();
      for (int t0 = blockIdx.x * 4; t0 < nb * a.H; t0 += G * 4) {
        const int t = t0 + wave;
        const bool valid = t < nb * a.H;
        const int tt = valid ? t : nb * a.H - 1;
        float* wl = lds + wave * (128 + a.max_len + 64);           // per wave: 128 probabilities, max_len row offsets, 64 q
        attn_task(a.slot_of, 0, nb, a.ld_seq, D, qkv, ldrow, kc, vc, att, ldrow, tt / a.H, tt / a.H, tt % a.H, pos + 1, valid, wl, (int*)(wl + 128),
                  wl + 128 + a.max_len);
      }
      ps.arrive(nprod(ntask4), blockIdx.x < ntask4);
      // P3: out-proj + residual (x += ...)
      p.ln_x = nullptr; p.kv_k = nullptr; p.kv_v = nullptr; p.kv_width = 0;
      p.A = att; p.lda = ldrow; p.B = (const bf16*)w.w_o; p.ldb = D; p.N = D; p.K = D; p.bias = w.b_o;
      p.residual = a.x; p.ldr = D; p.out_f32 = a.x; p.out_bf16 = nullptr; p.ldc = D;
      {
        const int nblk = (D + 31) / 32;
        proj_phase<MCAP, CCLIP_ACT_NONE, 12>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P4: LayerNorm + fc + activation
      p.A = nullptr; p.lda = 0; p.B = (const bf16*)w.w_fc; p.ldb = Hd; p.N = Hd; p.K = D; p.bias = w.b_fc;
      p.residual = nullptr; p.ldr = 0; p.out_f32 = nullptr; p.out_bf16 = hid; p.ldc = ldrow;
      p.ln_x = a.x; p.ln_ldx = D; p.ln_gamma = w.ln2_w; p.ln_beta = w.ln2_b;
      {
        const int nblk = (Hd + 31) / 32;
        if (a.act == CCLIP_ACT_GELU_NEW) proj_phase<MCAP, CCLIP_ACT_GELU_NEW, 12>(p, nblk, G, lds, &ps);
        else proj_phase<MCAP, CCLIP_ACT_NONE, 12>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
      // P5: proj + residual
      p.ln_x = nullptr;
      p.A = hid; p.lda = ldrow; p.B = (const bf16*)w.w_proj; p.ldb = D; p.N = D; p.K = Hd; p.bias = w.b_proj;
      p.residual = a.x; p.ldr = D; p.out_f32 = a.x; p.out_bf16 = nullptr; p.ldc = D;
      {
        const int nblk = (D + 31) / 32;
        proj_phase<MCAP, CCLIP_ACT_NONE, 16>(p, nblk, G, lds, &ps);
        ps.arrive(nprod(nblk), blockIdx.x < nblk);
      }
    }
    // LN_f + tied lm_head over this workgroup's vocabulary slice [r0, r0 + nr), then the slice's selection partials.
    // xs: LN_f(x) rounded to the operand type, fp32 [nb][D]; sl: the slice's logits [nb][DECODE_MAXR]
    ps.wait();
    float* sl = lds + MCAP * D;
    head_phase<MCAP>(a, lds, r0, nr);
    __syncthreads();
    select_partials(a.part, nb, sl, nb, false, r0, nr, T, G);
    ps.arrive(G, true);
    if (blockIdx.x == 0) { ps.wait(); select_merge<MCAP>(cv, nb, false, it, pos, G, ntok0 + it, lds); }
    ps.arrive(1, blockIdx.x == 0);
  }
}

}  // namespace CCLIP_NS
using namespace CCLIP_NS;

extern "C" int CCLIP_FN(cclip_gpt2_beam_search)(const cclip_beam_desc* d, hipStream_t stream) {
  if (!d || !persist_desc_ok(d->step)) return CCLIP_ERR_ARG;
  const cclip_decode_desc& s = d->step;
  if (s.n_seq <= 0 || s.n_seq > 8) return CCLIP_ERR_ARG;
  if (s.logits && (s.ld_logits < s.vocab)) return CCLIP_ERR_ARG;
  if (!d->wte_f32 || !d->wpe_f32 || !d->slot_of || !d->tokens || !d->scores || !d->seq_lengths || !d->is_stopped || !d->state || !d->select_ws)
    return CCLIP_ERR_ARG;
  if (d->n_steps < 0 || d->max_len <= 0 || d->max_len > 2048 || d->ld_tokens <= 0 || (d->first && !d->first_logits)) return CCLIP_ERR_ARG;
  if (!d->first && d->n_steps == 0) return CCLIP_OK;
  const int n_cu = persist_cu_count();
  if (n_cu == 0) return CCLIP_ERR_LAUNCH;
  int G, R;
  if (!persist_grid(s.vocab, d->grid_cap, n_cu, &G, &R)) return CCLIP_ERR_ARG;
  const int mcap = s.n_seq <= 4 ? 4 : 8;
  // LDS: GEMV A rows / reduction, attention rows, lm_head rows + slice, selection candidates
  size_t fl = (size_t)s.n_seq * s.hidden;
  const size_t red = (size_t)256 * mcap * 8; if (red > fl) fl = red;
  const size_t att = (size_t)4 * (128 + d->max_len + 64); if (att > fl) fl = att;
  const size_t head = (size_t)mcap * s.width + (size_t)s.n_seq * DECODE_MAXR; if (head > fl) fl = head;
  const size_t sel = 64 + 512 + 4096 + 2 * (size_t)s.n_seq * G * s.n_seq; if (sel > fl) fl = sel;
  const size_t lds = fl * sizeof(float);
  if (lds > 150 * 1024) return CCLIP_ERR_ARG;
  BeamArgs a;
  a.n_layer = s.n_layer; a.nb = s.n_seq; a.D = s.width; a.H = s.heads; a.Hd = s.hidden; a.act = s.act; a.V = s.vocab; a.pos0 = s.pos;
  a.n_steps = d->n_steps; a.first = d->first ? 1 : 0; a.stop_token = d->stop_token; a.ld_tokens = d->ld_tokens; a.max_len = d->max_len;
  a.rows_per_wg = R; a.temperature = d->temperature;
  for (int l = 0; l < s.n_layer; ++l) a.blocks[l] = s.blocks[l];
  a.x = s.x; a.kc = (bf16*)s.kcache; a.vc = (bf16*)s.vcache; a.ld_layer = s.ld_layer; a.ld_seq = s.ld_seq; a.scratch = (bf16*)s.scratch16;
  a.lnf_w = s.lnf_w; a.lnf_b = s.lnf_b; a.wte16 = (const bf16*)s.wte16; a.logits = s.logits; a.ld_logits = s.ld_logits;
  a.first_logits = d->first_logits; a.wte32 = d->wte_f32; a.wpe32 = d->wpe_f32;
  a.slot_of = d->slot_of; a.tokens = d->tokens; a.scores = d->scores; a.seq_len = d->seq_lengths; a.stopped = d->is_stopped;
  a.state = d->state; a.part = d->select_ws;
  if (hipMemsetAsync(d->state, 0, 2 * sizeof(int), stream) != hipSuccess) return CCLIP_ERR_LAUNCH;   // barrier counter, error flag
  return mcap == 4 ? launch_persist<gpt2_beam_persist_kernel<4>>(G, lds, stream, a) : launch_persist<gpt2_beam_persist_kernel<8>>(G, lds, stream, a);
}